#!/usr/bin/env python3
"""What reading FASTA / FASTQ costs: the reference's reader, the host's parser and the device path on the same text.

    python tools/fastx_bench.py [--mb 200] [--repeat 3] [--kinds fastq10k,fastq150,fasta60] [--out profiles/fastx_bench.json]

Three generated inputs of about --mb megabytes of text each: four-line FASTQ of 10 kb reads, four-line FASTQ of 150-base reads, FASTA in 60-column
lines (records of 600 kb).  Per input, best of --repeat after a warm-up, with the file in the page cache:
  reference   mm_bseq_read3 of oracle/_ref/libminimap2_ref.so on one thread, one call over the whole file, qualities kept (its records are not
              freed: the time of 4 million free() calls through ctypes would be the benchmark's, not the reader's);
  file_read   reading the file into memory, which the two parsers below need first and the reference's figure includes;
  host        mm2amd_fastx_parse_host over the text, into a table and a pool allocated and touched before;
  device      mm2amd_fastx_parse likewise: the call's wall time with the profiler off, then with it on the split into upload, device work up to
              the sizes (lines, classify, the sums), the copy kernels, download, the host's table (mm2amd_fastx_last_times) and the events'
              milliseconds per kernel (mm2amd_profile_get).
The records of the three are compared.  One JSON object, printed and written to --out."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make_text(np, rng, kind, mb):
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    if kind == "fasta60":
        n_lines, n_rec = 10000, max(1, mb * 1000000 // (10000 * 61))
        out = []
        for r in range(n_rec):
            body = np.empty((n_lines, 61), dtype=np.uint8)
            body[:, :60] = acgt[rng.integers(0, 4, (n_lines, 60), dtype=np.uint8)]
            body[:, 60] = 10
            out.append(b">contig%d len=%d\n" % (r, 60 * n_lines) + body.tobytes())
        return b"".join(out)
    ln = 10000 if kind == "fastq10k" else 150
    n = max(1, mb * 1000000 // (2 * ln + 16))
    rec = np.empty((n, 2 * ln + 16), dtype=np.uint8)  # @r%09d \n seq \n + \n qual \n
    rec[:, 0], rec[:, 1] = ord("@"), ord("r")
    idx = np.arange(n)
    for d in range(9):
        rec[:, 10 - d] = 48 + (idx // 10 ** d) % 10
    rec[:, 11] = 10
    rec[:, 12:12 + ln] = acgt[rng.integers(0, 4, (n, ln), dtype=np.uint8)]
    rec[:, 12 + ln], rec[:, 13 + ln], rec[:, 14 + ln] = 10, ord("+"), 10
    rec[:, 15 + ln:15 + 2 * ln] = rng.integers(35, 75, (n, ln), dtype=np.uint8)
    rec[:, 15 + 2 * ln] = 10
    return rec.tobytes()


def main(argv=None):
    import numpy as np
    import minimap2_amd as mm
    ap = argparse.ArgumentParser()
    ap.add_argument("--mb", type=int, default=200)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--kinds", default="fastq10k,fastq150,fasta60")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fastx_bench.json"))
    a = ap.parse_args(argv)
    L = mm.lib()
    if L.mm2amd_device_count() < 1:
        raise SystemExit("fastx_bench needs a GPU: " + L.mm2amd_last_error().decode())
    ref_so = os.path.join(ROOT, "oracle", "_ref", "libminimap2_ref.so")
    R = C.CDLL(ref_so) if os.path.exists(ref_so) else None
    if R is not None:
        R.mm_bseq_open.restype, R.mm_bseq_open.argtypes = C.c_void_p, [C.c_char_p]
        R.mm_bseq_close.argtypes = [C.c_void_p]
        R.mm_bseq_read3.restype = C.POINTER(mm.Bseq1)
        R.mm_bseq_read3.argtypes = [C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)]
    rng = np.random.default_rng(7)
    res = {"backend": L.mm2amd_backend_name().decode(), "limits": mm.fastx_limits(), "mb": a.mb, "repeat": a.repeat, "inputs": {}}
    try:
        res["commit"] = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], stderr=subprocess.DEVNULL).decode().strip()
    except Exception:  # noqa: BLE001
        res["commit"] = None
    n, pl, used, path = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0), C.c_int(0)
    for kind in a.kinds.split(","):
        data = make_text(np, rng, kind, a.mb)
        with tempfile.NamedTemporaryFile(suffix=".fx", delete=False) as f:
            f.write(data)
        try:
            one = {"text_bytes": len(data)}
            t_read = []
            for _ in range(a.repeat + 1):
                t0 = time.perf_counter()
                with open(f.name, "rb") as g:
                    text_b = g.read()
                t_read.append(time.perf_counter() - t0)
            one["file_read_ms"] = 1e3 * min(t_read[1:])
            text = np.frombuffer(text_b, dtype=np.uint8)
            ref_first = None
            if R is not None:
                t_ref = []
                for _ in range(a.repeat + 1):
                    fp = R.mm_bseq_open(os.fsencode(f.name))
                    k = C.c_int(0)
                    t0 = time.perf_counter()
                    arr = R.mm_bseq_read3(fp, 1 << 62, 1, 0, 0, C.byref(k))
                    t_ref.append(time.perf_counter() - t0)
                    one["records"] = k.value
                    ref_first = (arr[0].name, arr[0].seq[:50], arr[k.value - 1].name, arr[k.value - 1].l_seq, sum(arr[j].l_seq for j in range(0, k.value, max(1, k.value // 1000))))
                    R.mm_bseq_close(fp)
                one["reference_ms"] = 1e3 * min(t_ref[1:])
            # sizes, then buffers that are touched before the timed calls
            mm._check(L.mm2amd_fastx_parse_host(text.ctypes.data, text.size, 1, 1, None, 0, None, 0, C.byref(n), C.byref(pl), C.byref(used), C.byref(path)))
            recs, pool = np.zeros(n.value, dtype=mm._fastx_dtype()), np.zeros(pl.value, dtype=np.uint8)

            def run(call):
                t0 = time.perf_counter()
                mm._check(call(text.ctypes.data, text.size, 1, 1, recs.ctypes.data, len(recs), pool.ctypes.data, len(pool), C.byref(n), C.byref(pl), C.byref(used), C.byref(path)))
                return time.perf_counter() - t0
            t_host = [run(L.mm2amd_fastx_parse_host) for _ in range(a.repeat + 1)]
            one["host_ms"] = 1e3 * min(t_host[1:])
            host_recs, host_pool = recs.copy(), pool.copy()
            recs[:], pool[:] = 0, 0
            t_dev = [run(L.mm2amd_fastx_parse) for _ in range(a.repeat + 1)]
            one["device_ms"] = 1e3 * min(t_dev[1:])
            one["device_path"] = path.value
            one["device_equals_host"] = bool((recs == host_recs).all() and (pool == host_pool).all())
            if ref_first is not None:
                j = len(recs) - 1
                mine = (pool[int(recs[0]["name"]):int(recs[0]["name"]) + int(recs[0]["name_len"])].tobytes(), pool[int(recs[0]["seq"]):int(recs[0]["seq"]) + 50].tobytes().split(b"\0")[0],
                        pool[int(recs[j]["name"]):int(recs[j]["name"]) + int(recs[j]["name_len"])].tobytes(), int(recs[j]["l_seq"]),
                        int(recs["l_seq"][::max(1, len(recs) // 1000)].sum()))
                one["device_equals_reference_sample"] = bool(mine == ref_first and len(recs) == one["records"])
            mm.profile_enable(True)
            best = None
            for _ in range(a.repeat):
                mm.profile_enable(True)  # (resets the sums)
                t = run(L.mm2amd_fastx_parse)
                v = (C.c_double * 6)()
                L.mm2amd_fastx_last_times(v, 6)
                if best is None or t < best[0]:
                    best = (t, list(v), mm.profile_get())
            mm.profile_enable(False)
            one["device_profiled_ms"] = 1e3 * best[0]
            one["device_phases_ms"] = dict(zip(["upload", "lines_classify_sums", "copy_kernels", "download", "host_table", "host_parser"], [1e3 * x for x in best[1]]))
            one["kernels_ms"] = {k: v["ms"] for k, v in best[2].items() if k.startswith("fastx_")}
            for key in ("reference_ms", "host_ms", "device_ms"):
                if key in one:
                    one[key.replace("_ms", "_gb_s")] = len(data) / one[key] / 1e6
            res["inputs"][kind] = one
            print("[fastx_bench] %s: %s" % (kind, json.dumps(one)), file=sys.stderr, flush=True)
        finally:
            os.unlink(f.name)
    s = json.dumps(res, indent=1, sort_keys=True)
    print(s)
    with open(a.out, "w") as f:
        f.write(s + "\n")


if __name__ == "__main__":
    main()
