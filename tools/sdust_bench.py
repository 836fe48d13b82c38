#!/usr/bin/env python3
"""What SDUST masking (sdust(), W = 64) costs on the device, in sdust_kernel's two launch classes, and on the host threads that do it by default.

    python tools/sdust_bench.py [--reads 10000] [--len 10000] [--T 20] [--repeat 3] [--threads 16] [--out profiles/sdust_bench.json]

One batch of --reads x --len bases in three kinds:
  random        uniform random bases;
  repeats       random bases with four planted low-complexity stretches a read: homopolymers of 15-60 bases and tandem repeats of a 2-6-base unit
                over 30-150 bases, 2 % of their bases mutated;
  homopolymer   one base repeated: the worst case, every step inserts into a list of thousands of perfect intervals.
Per kind, after a sizing call that also warms up (the first call allocates): mm2amd_sdust_batch --repeat times with the profiler off for the call's
wall time, --repeat times more with it on for the events' milliseconds of sdust_kernel[narrow] and sdust_kernel[wide] (mm2amd_profile_get); then
mm2amd_sdust_host_batch (sdust_scan, what the `-T` path runs by default) on --threads host threads over the same reads, --repeat times after a
warm-up of its own, with its wall time and core-seconds, and the two results compared.  The host needs seconds per homopolymer read, so there it
scans the batch's first --host-homopolymers reads; the whole batch's figure is then an extrapolation and the JSON marks it.
One JSON object, printed and written to --out."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make_reads(np, rng, kind, n, ln):
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    if kind == "homopolymer":
        return [bytes(acgt[i & 3:(i & 3) + 1]) * ln for i in range(n)]
    codes = rng.integers(0, 4, (n, ln), dtype=np.uint8)
    if kind == "repeats":
        for r in range(n):
            for _ in range(4):
                if rng.integers(0, 2):
                    m, unit = int(rng.integers(15, 61)), rng.integers(0, 4, 1, dtype=np.uint8)
                else:
                    m, unit = int(rng.integers(30, 151)), rng.integers(0, 4, int(rng.integers(2, 7)), dtype=np.uint8)
                s = np.tile(unit, m // len(unit) + 1)[:m]
                hit = rng.random(m) < 0.02
                s[hit] = rng.integers(0, 4, int(hit.sum()), dtype=np.uint8)
                p = int(rng.integers(0, ln - m))
                codes[r, p:p + m] = s
    return [acgt[c].tobytes() for c in codes]


def main(argv=None):
    import numpy as np
    import minimap2_amd as mm
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10000)
    ap.add_argument("--len", type=int, default=10000)
    ap.add_argument("--T", type=int, default=20)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--host-homopolymers", type=int, default=32)
    ap.add_argument("--kinds", default="random,repeats,homopolymer")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sdust_bench.json"))
    a = ap.parse_args(argv)
    L = mm.lib()
    if L.mm2amd_device_count() < 1:
        raise SystemExit("sdust_bench needs a GPU: " + L.mm2amd_last_error().decode())
    rng = np.random.default_rng(7)
    res = {"backend": L.mm2amd_backend_name().decode(), "limits": mm.sdust_limits(), "T": a.T, "reads": a.reads, "len": a.len, "repeat": a.repeat, "host_threads": a.threads}
    try:
        res["commit"] = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], stderr=subprocess.DEVNULL).decode().strip()
    except Exception:  # noqa: BLE001
        res["commit"] = None
    for kind in a.kinds.split(","):
        reads = make_reads(np, rng, kind, a.reads, a.len)
        n, bases = len(reads), float(sum(len(r) for r in reads))
        arr, keep = mm._sdust_jobs(reads)
        out = (mm.SdustRes * n)()
        mm._check(L.mm2amd_sdust_batch(n, arr, a.T, out, None, 0))  # sizes the batch; the warm-up
        total = sum(r.n for r in out)
        pool = np.zeros(max(total, 1), dtype=np.uint64)
        wall, narrow, wide = [], [], []
        for _ in range(a.repeat):  # the call's wall time, with the profiler off
            t0 = time.perf_counter()
            mm._check(L.mm2amd_sdust_batch(n, arr, a.T, out, pool.ctypes.data, total))
            wall.append((time.perf_counter() - t0) * 1e3)
        for _ in range(a.repeat):  # the kernels' time from events, in calls of their own
            mm.profile_enable(True)
            mm._check(L.mm2amd_sdust_batch(n, arr, a.T, out, pool.ctypes.data, total))
            prof = mm.profile_get()
            mm.profile_enable(False)
            narrow.append(prof.get("sdust_kernel[narrow]", {"ms": 0.0})["ms"])
            wide.append(prof.get("sdust_kernel[wide]", {"ms": 0.0})["ms"])
        n_wide = sum(1 for r in out if r.path == mm.SDUST_PATH_WIDE)
        kern = [x + y for x, y in zip(narrow, wide)]
        dev = {"bases": bases, "regions": total, "wide_share": n_wide / float(n), "units": {k: v["units"] for k, v in prof.items() if k.startswith("sdust_kernel")},
               "call_ms": wall, "narrow_ms": narrow, "wide_ms": wide, "kernel_ms": kern,
               "kernel_gbases_per_s": [bases / k / 1e6 for k in kern], "call_gbases_per_s": [bases / w / 1e6 for w in wall]}
        # the host's routine over the same reads
        hn = min(n, a.host_homopolymers) if kind == "homopolymer" else n
        harr, hkeep = mm._sdust_jobs(reads[:hn])
        hout = (mm.SdustRes * hn)()
        htotal = sum(r.n for r in out[:hn])
        hpool = np.zeros(max(htotal, 1), dtype=np.uint64)
        cs = C.c_double(0)
        hms, hcs = [], []
        for it in range(a.repeat + 1):  # one warm-up (the pool's threads start in it), then as many scans as the kernel had calls
            t0 = time.perf_counter()
            mm._check(L.mm2amd_sdust_host_batch(hn, harr, a.T, a.threads, hout, hpool.ctypes.data, htotal, C.byref(cs)))
            if it:
                hms.append((time.perf_counter() - t0) * 1e3), hcs.append(cs.value)
        assert [r.n for r in hout] == [r.n for r in out[:hn]] and np.array_equal(hpool[:htotal], pool[:htotal]), "the device's regions and the host's differ"
        hbases = float(sum(len(r) for r in reads[:hn]))
        host = {"reads": hn, "bases": hbases, "threads": a.threads, "ms": hms, "core_seconds": hcs, "gbases_per_s": [hbases / m / 1e6 for m in hms],
                "core_seconds_per_gbase": [c / (hbases / 1e9) for c in hcs], "ms_for_the_whole_batch": [m * bases / hbases for m in hms], "extrapolated": hn < n,
                "note": "sdust_scan over the batch's first %d reads, the whole batch's time extrapolated: the host needs seconds per read here" % hn if hn < n else "sdust_scan over the same reads"}
        hall = min(hms) * bases / hbases
        res[kind] = {"device": dev, "host": host, "kernel_over_host": [min(kern) / (max(hms) * bases / hbases), max(kern) / hall]}  # (the range the repeats span)
        print("[sdust_bench] %s: kernel %.1f ms (wide share %.3f), call %.1f ms, host %.1f ms for the whole batch" % (kind, min(kern), dev["wide_share"], min(wall), hall), file=sys.stderr, flush=True)
        del reads, arr, keep, pool
    line = json.dumps(res, sort_keys=True)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(res, sort_keys=True, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
