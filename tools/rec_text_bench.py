#!/usr/bin/env python3
"""What the output stage costs the HOST with the records written by the host pool and by the device, on the same hits.

    python tools/rec_text_bench.py [--reads 3000] [--ref-mb 5] [--out profiles/rec_text_bench.json]

Maps tools/aln_text_bench.py's synthetic ONT reads (tests/synth.py) once, then for SAM, PAF -c and PAF -c --cs formats the same records with
  * mm_gpu_format_batch_view -- the host writer -- on 2, 4 and 16 pool threads (both entry points format on half the context's threads,
    beside mapping: the contexts are opened with twice as many), and
  * mm_gpu_format_batch_dev -- rec_text_kernel -- in the same contexts,
taking of every call the wall time and the PROCESS's CPU seconds (resource.getrusage: user + system, all threads), and of the device path the
kernels' own milliseconds (mm2amd_profile_get).  The texts must be equal.  The figure that matters is host core-seconds per Gbase of reads.
One JSON object, printed and written to --out."""
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

F_CIGAR, F_OUT_SAM, F_OUT_CG, F_OUT_CS = 0x004, 0x008, 0x020, 0x040  # MM_F_* (minimap.h:12-16)
FORMATS = (("sam", F_OUT_SAM | F_CIGAR), ("paf_c", F_OUT_CG | F_CIGAR), ("paf_c_cs", F_OUT_CG | F_OUT_CS | F_CIGAR))


def cpu_seconds():
    r = resource.getrusage(resource.RUSAGE_SELF)
    return r.ru_utime + r.ru_stime


def main(argv=None):
    import numpy as np
    import minimap2_amd as mm
    import synth
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=3000)
    ap.add_argument("--ref-mb", type=float, default=5.0)
    ap.add_argument("--mean-len", type=int, default=6000)
    ap.add_argument("--err", type=float, default=0.1)
    ap.add_argument("--threads", type=int, nargs="*", default=[2, 4, 16], help="formatting pool threads")
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rec_text_bench.json"))
    a = ap.parse_args(argv)
    rng = np.random.default_rng(7)
    contigs = synth.gen_reference(rng, int(a.ref_mb * 1e6), 2)
    reads = synth.gen_reads(rng, contigs, a.reads, a.mean_len, a.mean_len // 4, a.err)
    refs = [synth.ACGT[c].tobytes() for c in contigs]
    rds = [("read%d" % i, synth.ACGT[r].tobytes()) for i, r in enumerate(reads)]
    L = mm.lib()
    al = mm.Aligner(refs, preset="map-ont", names=["chr1", "chr2"], n_threads=16)
    bases = sum(len(s) for _, s in rds)
    res = {"reads": a.reads, "read_bases": bases, "backend": L.mm2amd_backend_name().decode(), "cpus": len(os.sched_getaffinity(0)), "formats": {}}
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

        for name, flag in FORMATS:
            per = {}
            for nt in a.threads:
                mo = mm.MapOpt.from_buffer_copy(al.map_opt)
                mo.flag = (mo.flag & ~(F_OUT_SAM | F_OUT_CG | F_OUT_CS)) | flag
                mm._check(L.mm_gpu_init_index_multi(al._idx, C.byref(mo), 2 * nt, 0, None))  # (the entry points format on half the context's threads: beside mapping)

                def host(out, out_len):
                    mm._check(L.mm_gpu_format_batch_view(n, seg_off, n_seg, arr, n_reg, reg, rep_len, C.byref(out), C.byref(out_len)))

                def dev(out, out_len):
                    path = C.c_int(-1)
                    mm.profile_enable(True)
                    mm._check(L.mm_gpu_format_batch_dev(n, seg_off, n_seg, arr, n_reg, reg, rep_len, C.byref(out), C.byref(out_len), C.byref(path)))
                    prof = mm.profile_get()
                    mm.profile_enable(False)
                    assert path.value == mm.FMT_PATH_DEVICE, "the batch fell back to the host writer"
                    return {k: prof[k]["ms"] for k in ("rec_text_kernel[size]", "rec_text_kernel[write]") if k in prof}

                h_ms, h_cpu, h_text, _ = timed(host)
                d_ms, d_cpu, d_text, kern = timed(dev)
                assert h_text == d_text, "%s: the device's text differs from the host writer's" % name
                per["threads_%d" % nt] = {
                    "pool_threads": nt, "context_threads": 2 * nt, "text_bytes": len(h_text),
                    "host": {"wall_ms": h_ms, "cpu_s": h_cpu, "core_s_per_gbase": h_cpu / bases * 1e9},
                    "device": {"wall_ms": d_ms, "cpu_s": d_cpu, "core_s_per_gbase": d_cpu / bases * 1e9, "kernel_size_ms": kern.get("rec_text_kernel[size]"),
                               "kernel_write_ms": kern.get("rec_text_kernel[write]")}}
            res["formats"][name] = per
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
