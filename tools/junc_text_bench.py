#!/usr/bin/env python3
"""What --write-junc costs the HOST with the junction lines written by the host pool and by the device, on the same spliced hits.

    python tools/junc_text_bench.py [--reads 4000] [--ref-mb 5] [--out profiles/junc_text_bench.json]

Maps synthetic cDNA reads (tests/synth.py: gen_transcripts, 2-8 exons each) once with -x splice, then formats the same hits with MM_F_OUT_JUNC by
  * mm_gpu_format_batch_view -- the host writer (format.cpp: put_junc) -- on 2, 4 and 16 pool threads (both entry points format on half the
    context's threads, beside mapping: the contexts are opened with twice as many), and
  * mm_gpu_format_batch_dev -- junc_text_kernel -- in the same contexts,
taking of every call the wall time and the PROCESS's CPU seconds (resource.getrusage: user + system, all threads), and of the device path the
two kernel times (mm2amd_profile_get).  The texts must be equal.  No threshold: the tool reports.  One JSON object, printed and written to --out."""
import argparse
import ctypes as C
import json
import os
import resource
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

KERNELS = ("junc_text_kernel[size]", "junc_text_kernel[write]")


def cpu_seconds():
    r = resource.getrusage(resource.RUSAGE_SELF)
    return r.ru_utime + r.ru_stime


def main(argv=None):
    import numpy as np
    import minimap2_amd as mm
    import synth
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=4000)
    ap.add_argument("--ref-mb", type=float, default=5.0)
    ap.add_argument("--err", type=float, default=0.04)
    ap.add_argument("--threads", type=int, nargs="*", default=[2, 4, 16], help="formatting pool threads")
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "junc_text_bench.json"))
    a = ap.parse_args(argv)
    rng = np.random.default_rng(7)
    contigs = synth.gen_reference(rng, int(a.ref_mb * 1e6), 2)
    reads = synth.gen_transcripts(rng, contigs, a.reads, a.err)
    refs = [synth.ACGT[c].tobytes() for c in contigs]
    rds = [("read%d" % i, synth.ACGT[r].tobytes()) for i, r in enumerate(reads)]
    L = mm.lib()
    al = mm.Aligner(refs, preset="splice", names=["chr1", "chr2"], n_threads=16, write_junc=True)
    bases = sum(len(s) for _, s in rds)
    res = {"reads": a.reads, "read_bases": bases, "backend": L.mm2amd_backend_name().decode(), "cpus": len(os.sched_getaffinity(0)), "threads": {}}
    try:
        res["commit"] = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], stderr=subprocess.DEVNULL).decode().strip()
    except Exception:  # noqa: BLE001
        res["commit"] = None
    try:
        al.stage(rds)
        n_reg, reg, rep_len = al.run(raw=True)
        n, arr, items, seg_off, n_seg = al._staged
        res["hits"] = sum(n_reg[k] for k in range(n))

        def timed(call):
            """best of --repeat after one warm-up: (wall ms, CPU seconds, text, last call's extras)"""
            best = None
            for it in range(a.repeat + 1):
                out, out_len = C.c_void_p(), C.c_size_t()
                c0, t0 = cpu_seconds(), time.perf_counter()
                extra = call(out, out_len)
                t1, c1 = time.perf_counter(), cpu_seconds()
                cur = ((t1 - t0) * 1e3, c1 - c0, C.string_at(out, out_len.value), extra)
                if it > 0 and (best is None or cur[1] < best[1]):
                    best = cur
            return best

        for nt in a.threads:
            mm._check(L.mm_gpu_init_index_multi(al._idx, C.byref(al.map_opt), 2 * nt, 0, None))  # (the entry points format on half the context's threads: beside mapping)

            def host(out, out_len):
                mm._check(L.mm_gpu_format_batch_view(n, seg_off, n_seg, arr, n_reg, reg, rep_len, C.byref(out), C.byref(out_len)))

            def dev(out, out_len):
                path = C.c_int(-1)
                mm.profile_enable(True)
                mm._check(L.mm_gpu_format_batch_dev(n, seg_off, n_seg, arr, n_reg, reg, rep_len, C.byref(out), C.byref(out_len), C.byref(path)))
                prof = mm.profile_get()
                mm.profile_enable(False)
                assert path.value == mm.FMT_PATH_DEVICE, "the batch fell back to the host writer"
                return {k: prof[k]["ms"] for k in KERNELS if k in prof}

            h_ms, h_cpu, h_text, _ = timed(host)
            d_ms, d_cpu, d_text, kern = timed(dev)
            assert h_text == d_text, "the device's text differs from the host writer's"
            res["junction_lines"], res["text_bytes"] = h_text.count(b"\n"), len(h_text)
            res["threads"]["threads_%d" % nt] = {
                "pool_threads": nt, "context_threads": 2 * nt,
                "host": {"wall_ms": h_ms, "cpu_s": h_cpu, "core_s_per_gbase": h_cpu / bases * 1e9},
                "device": {"wall_ms": d_ms, "cpu_s": d_cpu, "core_s_per_gbase": d_cpu / bases * 1e9, "kernel_size_ms": kern.get(KERNELS[0]), "kernel_write_ms": kern.get(KERNELS[1])}}
        al.free_raw(n_reg, reg)
    finally:
        L.mm_gpu_destroy()
        al.close()
    line = json.dumps(res, sort_keys=True)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(res, sort_keys=True, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
