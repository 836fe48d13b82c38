#!/usr/bin/env python3
"""What the local score with end coordinates (ksw_ll_i16) costs on the device, in its two launch classes, and on one CPU thread.

    python tools/ksw_ll_bench.py [--small 100000] [--mid 2000] [--repeat 3] [--out profiles/ksw_ll_bench.json]

Three workloads through mm2amd_ksw_ll_batch, each repeated after one warm-up call (the first call allocates):
  (a) --small jobs of about 55 x 55, the shape of mm_seed_ext_score (align.c:591-636);
  (b) --mid related jobs of about 1 500 x 1 500, the shape of the inversion test (align.c:84-101);
  (c) one related 5 000 x 5 000 job, through the workgroup class and, with MM2AMD_LL_NO_WG=1, through the wave class.
Per workload: the wall time of every call, the kernel's milliseconds and Gcells/s from mm2amd_profile_get, and -- where the compiled reference is
present (oracle/_ref) -- its ksw_ll_qinit + ksw_ll_i16 over the same jobs on one thread of the same machine, with the results compared.
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
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main(argv=None):
    import numpy as np
    import minimap2_amd as mm
    import ksw_ll_cases as X
    ap = argparse.ArgumentParser()
    ap.add_argument("--small", type=int, default=100000)
    ap.add_argument("--mid", type=int, default=2000)
    ap.add_argument("--big", type=int, default=5000)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ksw_ll_bench.json"))
    a = ap.parse_args(argv)
    rng = np.random.default_rng(7)
    L = mm.lib()
    sc = X.SCORINGS[0]
    mat = X.mat_of(sc)
    res = {"backend": L.mm2amd_backend_name().decode(), "scoring": list(sc), "limits": mm.ksw_ll_limits(), "repeat": a.repeat}
    try:
        res["commit"] = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], stderr=subprocess.DEVNULL).decode().strip()
    except Exception:  # noqa: BLE001
        res["commit"] = None

    def device(jobs, no_wg=False):
        n = len(jobs)
        arr = (mm.LlJob * n)()
        for i, (q, t) in enumerate(jobs):
            arr[i].query, arr[i].target = C.cast(C.c_char_p(q), C.c_void_p), C.cast(C.c_char_p(t), C.c_void_p)
            arr[i].qlen, arr[i].tlen, arr[i].flag = len(q), len(t), 0
        out = (mm.LlRes * n)()
        cells = float(sum(len(q) * len(t) for q, t in jobs))
        wall, kern, paths = [], [], {}
        with X.env(MM2AMD_LL_NO_WG=1 if no_wg else None, MM2AMD_LL_WG_MIN_CELLS=None):
            for it in range(a.repeat + 1):
                mm.profile_enable(True)
                t0 = time.perf_counter()
                mm._check(L.mm2amd_ksw_ll_batch(n, arr, 5, mat, sc[2], sc[3], out))
                dt = (time.perf_counter() - t0) * 1e3
                prof = mm.profile_get()
                mm.profile_enable(False)
                if it:
                    wall.append(dt)
                    kern.append(sum(v["ms"] for k, v in prof.items() if k.startswith("ksw_ll_kernel")))
        for r in out:
            paths[r.path] = paths.get(r.path, 0) + 1
        got = [(r.score, r.qe, r.te) for r in out]
        return got, {"jobs": n, "cells": cells, "paths": {"wave": paths.get(0, 0), "wg": paths.get(1, 0), "host": paths.get(2, 0)}, "call_ms": wall, "kernel_ms": kern,
                     "kernel_gcells_per_s": [cells / max(k, 1e-9) / 1e6 for k in kern], "call_gcells_per_s": [cells / w / 1e6 for w in wall]}

    def reference(jobs, got):
        if not X.HAVE_REF:
            return None
        t0 = time.perf_counter()
        want = [X.ref_ll(q, t, mat, sc[2], sc[3]) for q, t in jobs]
        ms = (time.perf_counter() - t0) * 1e3
        assert want == got, "the device's results and the reference's differ"
        cells = float(sum(len(q) * len(t) for q, t in jobs))
        return {"ms": ms, "gcells_per_s": cells / ms / 1e6, "threads": 1, "note": "ksw_ll_qinit + ksw_ll_i16 per job through ctypes"}

    small = [X.related(rng, int(rng.integers(50, 61)), int(rng.integers(50, 61)), 0.10) for _ in range(a.small)]
    got, res["a_small"] = device(small)
    res["a_small"]["reference"] = reference(small, got)
    mid = [X.related(rng, int(rng.integers(1400, 1601)), int(rng.integers(1400, 1601)), 0.10) for _ in range(a.mid)]
    got, res["b_mid"] = device(mid)
    res["b_mid"]["reference"] = reference(mid, got)
    big = [X.related(rng, a.big, a.big, 0.15)]
    got, wg = device(big)
    got2, wave = device(big, no_wg=True)
    assert got == got2
    res["c_big_wg"], res["c_big_wave"] = wg, wave
    res["c_big_wg"]["reference"] = reference(big, got)
    res["c_wg_faster_in_every_repeat"] = max(wg["kernel_ms"]) < min(wave["kernel_ms"]) and max(wg["call_ms"]) < min(wave["call_ms"])
    line = json.dumps(res, sort_keys=True)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(res, sort_keys=True, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
