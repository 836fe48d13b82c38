#!/usr/bin/env python3
"""What the hit-list rules of a split-index merge (merge_hits, map.c:520-531: sort, parents, secondaries, SAM primary) cost on the device, in
hits_merge_kernel's launch classes, and on the host threads running the same rules.

    python tools/split_merge_bench.py [--segments 5000] [--parts 8] [--per-part 50] [--repeat 3] [--threads 16] [--commit ID] [--out profiles/split_merge_bench.json]

The workload is synthetic hit lists shaped like long reads mapped with -N 50 against an index in --parts parts: per read segment every part adds
1 .. --per-part aligned hits (a strong one and a tail of weaker ones) over a read of 2-20 kb; one list in 50 repeats a hit of one part in another
(equal score and hash, the same sequence at the same place of two parts), one in 500 has more hits than the wide class holds.  Timed, after a
warm-up call each: mm2amd_hits_merge_batch --repeat times with the profiler off (the call's wall time: upload, both launches, download, the host
class) and --repeat times with it on (the events' milliseconds per class); mm2amd_hits_merge_host_batch on --threads threads (wall and
core-seconds).  The two results are compared hit by hit.  A second workload, "short", gives the narrow class its number: four times as many segments
against two parts with 1 .. 20 hits each (no list above 40 hits, none above the wide cap).  --commit names the tree in the JSON where there is no git
checkout to ask.  A third part, "merge_pass", times the merge pass itself on the temp files of a real first pass (see measure_merge): with the kernel, with the host's
routines, and the reference's own serial mm_split_merge through oracle/_ref/libminimap2_ref.so in a child process.  One JSON object, printed and written to --out."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make_lists(np, mm, rng, n_seg, parts, per_part, wide_cap, big_share=0.002):
    counts = rng.integers(1, per_part + 1, (n_seg, parts)).sum(axis=1)
    big = rng.random(n_seg) < big_share
    counts[big] = wide_cap + rng.integers(1, 200, int(big.sum()))
    off = np.zeros(n_seg + 1, dtype=np.uint64)
    off[1:] = np.cumsum(counts, dtype=np.uint64)
    total = int(off[-1])
    seg_of = np.repeat(np.arange(n_seg), counts)
    qlen = rng.integers(2000, 20001, n_seg)[seg_of]
    ln = np.maximum(200, (qlen * rng.random(total) ** 2).astype(np.int64))
    qs = ((qlen - ln) * rng.random(total)).astype(np.int64)
    h = np.zeros(total, dtype=mm.HM_HIT_DTYPE)
    h["qs"], h["qe"] = qs, qs + ln
    h["rs"] = rng.integers(0, 1 << 24, total)
    h["re"] = h["rs"] + ln
    h["rid"] = rng.integers(0, parts * 40, total)
    h["dp_max"] = (ln * (0.4 + 1.2 * rng.random(total))).astype(np.int64)
    h["score"] = (h["dp_max"] * 0.6).astype(np.int64)
    h["cnt"] = np.maximum(3, ln // 60)
    h["hash"] = rng.integers(0, 1 << 32, total, dtype=np.uint64).astype(np.uint32)
    h["flags"] = mm.HM_ALIGNED | (rng.random(total) < 0.5).astype(np.uint32) * mm.HM_REV
    for s in np.nonzero(rng.random(n_seg) < 0.02)[0]:  # the same hit from two parts
        a = int(off[s])
        if counts[s] >= 2:
            rid = int(h["rid"][a + 1])
            h[a + 1] = h[a]
            h["rid"][a + 1] = rid
    return off, h


def measure(np, mm, L, a, rng, n_seg, parts, per_part, best_n, big_share, have_gpu):
    lim = mm.hits_merge_limits()
    off, hits = make_lists(np, mm, rng, n_seg, parts, per_part, lim["wide_cap"], big_share)
    n, total = n_seg, int(off[-1])
    opt = mm.hm_opt(best_n=best_n, pri_ratio=0.8)
    res = {"segments": n, "hits": total, "parts": parts, "per_part": per_part, "best_n": best_n}
    hout, hseg = np.zeros(total, dtype=mm.HM_OUT_DTYPE), np.zeros((n, 2), dtype=np.int32)
    cs = C.c_double(0)
    hms, hcs = [], []
    for it in range(a.repeat + 1):  # one warm-up: the pool's threads start in it
        t0 = time.perf_counter()
        mm._check(L.mm2amd_hits_merge_host_batch(n, off.ctypes.data, hits.ctypes.data, C.byref(opt), a.threads, hout.ctypes.data, hseg.ctypes.data, C.byref(cs)))
        if it:
            hms.append((time.perf_counter() - t0) * 1e3), hcs.append(cs.value)
    res["host"] = {"threads": a.threads, "ms": hms, "core_seconds": hcs, "hits_per_s": [total / m * 1e3 for m in hms], "kept": int(hseg[:, 0].sum())}
    if not have_gpu:
        res["device"] = None
        return res
    dout, dseg = np.zeros(total, dtype=mm.HM_OUT_DTYPE), np.zeros((n, 2), dtype=np.int32)
    call = lambda: mm._check(L.mm2amd_hits_merge_batch(n, off.ctypes.data, hits.ctypes.data, C.byref(opt), dout.ctypes.data, dseg.ctypes.data))  # noqa: E731
    call()
    wall, narrow, wide = [], [], []
    for _ in range(a.repeat):
        t0 = time.perf_counter()
        call()
        wall.append((time.perf_counter() - t0) * 1e3)
    for _ in range(a.repeat):
        mm.profile_enable(True)
        call()
        prof = mm.profile_get()
        mm.profile_enable(False)
        narrow.append(prof.get("hits_merge_kernel[narrow]", {"ms": 0.0})["ms"])
        wide.append(prof.get("hits_merge_kernel[wide]", {"ms": 0.0})["ms"])
    assert np.array_equal(dseg[:, 0], hseg[:, 0]) and all(np.array_equal(dout[f], hout[f]) for f in ("pos", "id", "parent", "subsc", "n_sub", "dp_max2", "flags")), \
        "the device's lists and the host's differ"
    cnt = np.diff(off.astype(np.int64))
    classes = (("narrow", mm.HM_PATH_NARROW), ("wide", mm.HM_PATH_WIDE), ("host", mm.HM_PATH_HOST))
    share = {k: float((dseg[:, 1] == v).mean()) for k, v in classes}
    hit_share = {k: float(cnt[dseg[:, 1] == v].sum()) / total for k, v in classes}
    res["device"] = {"call_ms": wall, "narrow_ms": narrow, "wide_ms": wide, "kernel_ms": [x + y for x, y in zip(narrow, wide)], "segment_share": share, "hit_share": hit_share,
                     "call_hits_per_s": [total / m * 1e3 for m in wall]}
    res["device_call_over_host"] = [min(wall) / max(hms), max(wall) / min(hms)]
    print("[split_merge_bench] %d segments, %d hits: device call %.1f ms (kernels %.1f + %.1f ms), host on %d threads %.1f ms" %
          (n, total, min(wall), min(narrow), min(wide), a.threads, min(hms)), file=sys.stderr, flush=True)
    return res


_REF_CHILD = r"""
import ctypes as C, sys, time
sys.path.insert(0, sys.argv[1])
import minimap2_amd as mm
R = C.CDLL(sys.argv[2])
io, mo = mm.IdxOpt(), mm.MapOpt()
R.mm_set_opt(None, C.byref(io), C.byref(mo))
R.mm_set_opt(b"map-ont", C.byref(io), C.byref(mo))
mo.flag |= mm.F_CIGAR | mm.F_OUT_SAM
mo.best_n = 50
keep = sys.argv[3].encode()
mo.split_prefix = keep
fn = (C.c_char_p * 1)(sys.argv[5].encode())
R.mm_split_merge.argtypes = [C.c_int, C.POINTER(C.c_char_p), C.c_void_p, C.c_int]
t0 = time.perf_counter()
rc = R.mm_split_merge(1, fn, C.byref(mo), int(sys.argv[4]))
C.CDLL(None).fflush(None)
sys.stderr.write("%.3f\n" % ((time.perf_counter() - t0) * 1e3))
sys.exit(0 if rc == 0 else 3)
"""


def measure_merge(np, mm, a, rng):
    """the merge pass itself on temp files: a synthetic reference in eight parts (eight 40 kb contigs that share four 5 kb repeat families at 3 % divergence),
    --merge-reads long reads with -N 50, mapped once; then the merge phase alone (SplitMerger.merge over the read file, formatting left out) with the kernel, with
    the host's routines, and the reference's mm_split_merge in a child process (its time includes reading the reads and writing SAM to /dev/null)"""
    import shutil
    import tempfile
    ref_bin, ref_so = os.path.join(ROOT, "oracle", "_ref", "minimap2_ref"), os.path.join(ROOT, "oracle", "_ref", "libminimap2_ref.so")
    if not (os.path.exists(ref_bin) and os.path.exists(ref_so)):
        return {"note": "not measured: oracle/_ref is absent"}
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    fams = [rng.integers(0, 4, 5000, dtype=np.uint8) for _ in range(4)]
    contigs = []
    for c in range(8):
        s = rng.integers(0, 4, 40000, dtype=np.uint8)
        for k, f in enumerate(fams):
            g = f.copy()
            hit = rng.random(len(g)) < 0.03
            g[hit] = rng.integers(0, 4, int(hit.sum()), dtype=np.uint8)
            s[2000 + k * 9000:2000 + k * 9000 + 5000] = g
        contigs.append(s)
    reads = []
    for i in range(a.merge_reads):
        s = contigs[int(rng.integers(0, 8))]
        ln = int(rng.integers(1000, 5000))
        st = int(rng.integers(0, len(s) - ln))
        r = s[st:st + ln].copy()
        hit = rng.random(ln) < 0.08
        r[hit] = rng.integers(0, 4, int(hit.sum()), dtype=np.uint8)
        reads.append(acgt[r].tobytes())
    tmp = tempfile.mkdtemp(prefix="split_merge_bench")
    try:
        fa, fq, mmi, pre = (os.path.join(tmp, x) for x in ("ref.fa", "reads.fq", "ref.mmi", "pre"))
        with open(fa, "wb") as f:
            for c, s in enumerate(contigs):
                f.write(b">ctg%d\n" % c + acgt[s].tobytes() + b"\n")
        with open(fq, "wb") as f:
            for i, r in enumerate(reads):
                f.write(b"@r%d\n" % i + r + b"\n+\n" + b"I" * len(r) + b"\n")
        subprocess.run([ref_bin, "-x", "map-ont", "-I", "30k", "-d", mmi, fa], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        with open(os.devnull, "wb") as null:
            n_parts = mm.map_split(mmi, fq, pre, null, preset="map-ont", sam=True, keep_tmp=True, opt_overrides={"best_n": 50})
        io, mo = mm.IdxOpt(), mm.MapOpt()
        mm.lib().mm2amd_set_opt(None, C.byref(io), C.byref(mo))
        mm.lib().mm2amd_set_opt(b"map-ont", C.byref(io), C.byref(mo))
        mo.flag |= mm.F_CIGAR | mm.F_OUT_SAM
        mo.best_n = 50
        res = {"parts": n_parts, "reads": len(reads), "bases": sum(len(r) for r in reads), "tmp_bytes": sum(os.path.getsize("%s.%.4d.tmp" % (pre, j)) for j in range(n_parts))}
        for route, v in (("device", "1"), ("host", "0")):
            os.environ["MM2AMD_DEVICE_MERGE"] = v
            ms, hits = [], 0
            for it in range(a.repeat + 1):
                mg = mm.SplitMerger(pre, n_parts, mo)
                t, hits = 0.0, 0
                for b in mm.FastxReader(fq):
                    t0 = time.perf_counter()
                    n_reg, reg, rep_len, _ = mg.merge(b)
                    t += time.perf_counter() - t0
                    hits += sum(n_reg[i] for i in range(len(b.items)))
                    mm.lib().mm2amd_free_regs(len(n_reg), n_reg, reg)
                mg.close(remove_tmp=False)
                if it:
                    ms.append(t * 1e3)
            res[route] = {"merge_ms": ms, "records_out": hits}
        os.environ.pop("MM2AMD_DEVICE_MERGE", None)
        rms = []
        for _ in range(a.repeat):
            cp = os.path.join(tmp, "cp")
            for j in range(n_parts):
                shutil.copy("%s.%.4d.tmp" % (pre, j), "%s.%.4d.tmp" % (cp, j))
            r = subprocess.run([sys.executable, "-c", _REF_CHILD, ROOT, ref_so, cp, str(n_parts), fq], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE)
            rms.append(float(r.stderr.decode().split()[-1]))
        res["reference_mm_split_merge"] = {"ms": rms, "note": "the whole call in a child process: reads parsed, hits merged on one thread, SAM written to /dev/null"}
        print("[split_merge_bench] merge of %d parts, %d reads: device route %.1f ms, host route %.1f ms, mm_split_merge %.1f ms" %
              (n_parts, len(reads), min(res["device"]["merge_ms"]), min(res["host"]["merge_ms"]), min(rms)), file=sys.stderr, flush=True)
        return res
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def main(argv=None):
    import numpy as np
    import minimap2_amd as mm
    ap = argparse.ArgumentParser()
    ap.add_argument("--segments", type=int, default=5000)
    ap.add_argument("--parts", type=int, default=8)
    ap.add_argument("--per-part", type=int, default=50)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--commit", default=None)
    ap.add_argument("--merge-reads", type=int, default=2000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "split_merge_bench.json"))
    a = ap.parse_args(argv)
    L = mm.lib()
    have_gpu = L.mm2amd_device_count() >= 1
    rng = np.random.default_rng(11)
    res = {"backend": L.mm2amd_backend_name().decode(), "limits": mm.hits_merge_limits(), "repeat": a.repeat, "host_threads": a.threads, "commit": a.commit,
           }
    if res["commit"] is None:
        try:
            res["commit"] = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], stderr=subprocess.DEVNULL).decode().strip()
        except Exception:  # noqa: BLE001
            pass
    res["long_n50"] = measure(np, mm, L, a, rng, a.segments, a.parts, a.per_part, 50, 0.002, have_gpu)  # -N 50 against --parts parts
    res["short"] = measure(np, mm, L, a, rng, 4 * a.segments, 2, 20, 5, 0.0, have_gpu)  # the narrow class: two parts, the default -N
    if have_gpu:
        res["merge_pass"] = measure_merge(np, mm, a, rng)
    if not have_gpu:
        res["note"] = "no GPU in this session: the device route is unmeasured"
    print(json.dumps(res, sort_keys=True))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(res, sort_keys=True, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
