#!/usr/bin/env python3
"""What pairing the two mates (mm_pair + mm_set_pe_thru, pe.c:50-68, :81-182) costs on the device, in pair_kernel's launch classes, and on the host
threads running the same rules.

    python tools/pair_bench.py [--fragments 1000000] [--repeat 3] [--threads 16] [--commit ID] [--out profiles/pair_bench.json]

Two synthetic workloads.  "sr": --fragments fragments shaped like the sr preset's default output, one to three hits per mate -- the true placement of
both mates a few hundred bases apart in proper orientation, the others elsewhere, secondaries of the first hit.  "n20": a tenth as many fragments with
-N 20-like lists, 15-27 hits per mate spread over a tandem repeat so that most ends reach most others; a quarter of these fragments carry two ends
with equal keys.  Timed, after a warm-up call each: mm2amd_pair_batch --repeat times with the profiler off (the call's wall time: classification,
upload, the launches, download, the host class) and --repeat times with it on (the events' milliseconds per class, and around the call's copies each
way, which go from and to the caller's pageable arrays); mm2amd_pair_host_batch on --threads threads (wall and core-seconds).  The two answers are compared hit by hit and fragment by fragment: the tool fails if they differ.  --commit names the tree in the
JSON where there is no git checkout to ask.  One JSON object, printed and written to --out."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make_fragments(np, mm, rng, n_frag, lo, hi, tandem, tie_share):
    """per mate lo .. hi hits; tandem: the hits of both mates sit `tandem` bases apart around the fragment's place instead of anywhere"""
    n0, n1 = rng.integers(lo, hi + 1, n_frag), rng.integers(lo, hi + 1, n_frag)
    cnt = n0 + n1
    hit0 = np.zeros(n_frag, dtype=np.uint64)
    hit0[1:] = np.cumsum(cnt[:-1], dtype=np.uint64)
    total = int(cnt.sum())
    fr = np.zeros(n_frag, dtype=mm.PE_FRAG_DTYPE)
    fr["hit0"], fr["n"][:, 0], fr["n"][:, 1], fr["qlen"], fr["max_gap_ref"] = hit0, n0, n1, 150, 800
    f_of = np.repeat(np.arange(n_frag), cnt)
    pos = np.arange(total) - hit0.astype(np.int64)[f_of]       # place in the fragment
    seg = (pos >= n0[f_of]).astype(np.int64)
    k = pos - seg * n0[f_of]                                    # place in the segment
    strand = rng.integers(0, 2, n_frag)[f_of]
    place = rng.integers(1000, 1 << 27, n_frag)[f_of]
    h = np.zeros(total, dtype=mm.PE_HIT_DTYPE)
    opens = seg == strand                                       # (the key's lowest bit is seg ^ rev, and rev == strand here)
    if tandem:
        h["rs"] = place + k * tandem + np.where(opens, 0, 300)
        h["rid"] = rng.integers(0, 24, n_frag)[f_of]
        h["flags"] = strand.astype(np.uint32) * mm.PE_REV
    else:
        first = k == 0
        h["rs"] = np.where(first, place + np.where(opens, 0, 300), rng.integers(1000, 1 << 27, total))
        h["rid"] = np.where(first, rng.integers(0, 24, n_frag)[f_of], rng.integers(0, 24, total))
        h["flags"] = np.where(first, strand, rng.integers(0, 2, total)).astype(np.uint32) * mm.PE_REV
    h["re"] = h["rs"] + 150 - rng.integers(0, 3, total)
    h["qs"], h["qe"] = 0, 150
    h["dp_max"] = np.where(k == 0, 300, 300 - rng.integers(0, 60, total)) - rng.integers(0, 12, total)
    h["hash"] = rng.integers(0, 1 << 32, total, dtype=np.uint64).astype(np.uint32)
    h["id"], h["parent"] = k, 0
    h["mapq"] = np.where(k == 0, rng.integers(0, 61, total), 0)
    h["flags"] |= (k == 0).astype(np.uint32) * mm.PE_SAM_PRI
    tied = np.nonzero((rng.random(n_frag) < tie_share) & (n0 >= 2))[0]
    a = hit0[tied].astype(np.int64)
    for f in ("rs", "rid"):
        h[f][a + 1] = h[f][a]
    h["flags"][a + 1] = (h["flags"][a + 1] & ~np.uint32(mm.PE_REV)) | (h["flags"][a] & mm.PE_REV)
    return fr, h, len(tied)


def measure(np, mm, L, a, rng, n_frag, lo, hi, tandem, tie_share, have_gpu):
    fr, hits, n_tied = make_fragments(np, mm, rng, n_frag, lo, hi, tandem, tie_share)
    n, total = n_frag, len(hits)
    opt = mm.PeOpt(33, 8, 2, 0)
    res = {"fragments": n, "hits": total, "hits_per_mate": [lo, hi], "fragments_with_equal_keys": n_tied}
    hout, hres = np.zeros(total, dtype=mm.PE_OUT_DTYPE), np.zeros(n, dtype=mm.PE_RES_DTYPE)
    cs = C.c_double(0)
    hms, hcs = [], []
    for it in range(a.repeat + 1):  # one warm-up: the pool's threads start in it
        t0 = time.perf_counter()
        mm._check(L.mm2amd_pair_host_batch(n, fr.ctypes.data, hits.ctypes.data, C.byref(opt), a.threads, hout.ctypes.data, hres.ctypes.data, C.byref(cs)))
        if it:
            hms.append((time.perf_counter() - t0) * 1e3), hcs.append(cs.value)
    res["host"] = {"threads": a.threads, "ms": hms, "core_seconds": hcs, "fragments_per_s": [n / m * 1e3 for m in hms], "paired": int((hres["best"][:, 0] >= 0).sum()),
                   "candidates": int(hres["n_pairs"].sum())}
    if not have_gpu:
        res["device"] = None
        return res
    dout, dres = np.zeros(total, dtype=mm.PE_OUT_DTYPE), np.zeros(n, dtype=mm.PE_RES_DTYPE)
    call = lambda: mm._check(L.mm2amd_pair_batch(n, fr.ctypes.data, hits.ctypes.data, C.byref(opt), dout.ctypes.data, dres.ctypes.data))  # noqa: E731
    call()
    wall, narrow, wide, up, down = [], [], [], [], []
    for _ in range(a.repeat):
        t0 = time.perf_counter()
        call()
        wall.append((time.perf_counter() - t0) * 1e3)
    for _ in range(a.repeat):
        mm.profile_enable(True)
        call()
        prof = mm.profile_get()
        mm.profile_enable(False)
        narrow.append(prof.get("pair_kernel[narrow]", {"ms": 0.0})["ms"])
        wide.append(prof.get("pair_kernel[wide]", {"ms": 0.0})["ms"])
        up.append(prof.get("pair_copy[up]", {"ms": 0.0})["ms"]), down.append(prof.get("pair_copy[down]", {"ms": 0.0})["ms"])
        bytes_up, bytes_down = prof.get("pair_copy[up]", {}).get("alg_bytes", 0), prof.get("pair_copy[down]", {}).get("alg_bytes", 0)
    assert all(np.array_equal(dout[f], hout[f]) for f in ("parent", "mapq", "flags")) and all(np.array_equal(dres[f], hres[f]) for f in ("status", "n_pairs", "best")), \
        "the device's answers and the host twin's differ"
    classes = (("narrow", mm.PE_PATH_NARROW), ("wide", mm.PE_PATH_WIDE), ("host", mm.PE_PATH_HOST))
    res["device"] = {"call_ms": wall, "narrow_ms": narrow, "wide_ms": wide, "kernel_ms": [x + y for x, y in zip(narrow, wide)],
                     "fragment_share": {k: float((dres["path"] == v).mean()) for k, v in classes}, "call_fragments_per_s": [n / m * 1e3 for m in wall],
                     "copies": {"up_ms": up, "down_ms": down, "up_bytes": int(bytes_up), "down_bytes": int(bytes_down)}}
    res["device_call_over_host"] = [min(wall) / max(hms), max(wall) / min(hms)]
    print("[pair_bench] %d fragments, %d hits: device call %.1f ms (kernels %.2f + %.2f ms), host on %d threads %.1f ms" %
          (n, total, min(wall), min(narrow), min(wide), a.threads, min(hms)), file=sys.stderr, flush=True)
    return res


def main(argv=None):
    import numpy as np
    import minimap2_amd as mm
    ap = argparse.ArgumentParser()
    ap.add_argument("--fragments", type=int, default=1000000)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--commit", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pair_bench.json"))
    a = ap.parse_args(argv)
    L = mm.lib()
    have_gpu = L.mm2amd_device_count() >= 1
    rng = np.random.default_rng(17)
    res = {"backend": L.mm2amd_backend_name().decode(), "limits": mm.pair_limits(), "repeat": a.repeat, "host_threads": a.threads, "commit": a.commit}
    if res["commit"] is None:
        try:
            res["commit"] = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], stderr=subprocess.DEVNULL).decode().strip()
        except Exception:  # noqa: BLE001
            pass
    res["sr"] = measure(np, mm, L, a, rng, a.fragments, 1, 3, 0, 0.0, have_gpu)
    res["n20"] = measure(np, mm, L, a, rng, max(a.fragments // 10, 1), 15, 27, 40, 0.25, have_gpu)
    if not have_gpu:
        res["note"] = "no GPU in this session: the device route is unmeasured"
    print(json.dumps(res, sort_keys=True))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(res, sort_keys=True, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
