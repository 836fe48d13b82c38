#!/usr/bin/env python3
"""What the alignment text costs on the device and on the host, on the same hits.

    python tools/aln_text_bench.py [--reads 3000] [--ref-mb 5] [--threads 8] [--out profiles/aln_text_bench.json]

Maps synthetic ONT reads (tests/synth.py), then
  * times mm2amd_hits_text_batch for cs, MD and ds over all hits of the batch: wall time of the sizing call and of the writing call (uploads,
    both passes of aln_text_kernel, the copy back), and the kernel's own milliseconds from mm2amd_profile_get; the ds row also as a ratio
    to the cs row of the same run (ds is cs plus the shift scans of every indel);
  * times the host writers on the same records: mm_gpu_format_batch (PAF) with and without MM_F_OUT_CS / MM_F_OUT_MD / MM_F_OUT_DS -- the
    difference is what put_cs (with is_ds for ds) / put_md cost on the host pool -- and, where the compiled reference is present
    (oracle/_ref), its mm_gen_cs / mm_gen_MD / mm_gen_ds called hit by hit on one thread.
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

F_OUT_CS, F_OUT_MD, F_OUT_DS = 0x040, 0x1000000, 0x2000000000  # MM_F_OUT_CS, MM_F_OUT_MD, MM_F_OUT_DS (minimap.h:16, :34, :47)


def main(argv=None):
    import numpy as np
    import minimap2_amd as mm
    import reflib
    import synth
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=3000)
    ap.add_argument("--ref-mb", type=float, default=5.0)
    ap.add_argument("--mean-len", type=int, default=6000)
    ap.add_argument("--err", type=float, default=0.1)
    ap.add_argument("--threads", type=int, default=8)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "aln_text_bench.json"))
    a = ap.parse_args(argv)
    rng = np.random.default_rng(7)
    contigs = synth.gen_reference(rng, int(a.ref_mb * 1e6), 2)
    reads = synth.gen_reads(rng, contigs, a.reads, a.mean_len, a.mean_len // 4, a.err)
    refs = [synth.ACGT[c].tobytes() for c in contigs]
    names = ["chr1", "chr2"]
    rds = [("read%d" % i, synth.ACGT[r].tobytes()) for i, r in enumerate(reads)]
    L = mm.lib()
    al = mm.Aligner(refs, preset="map-ont", names=names, n_threads=a.threads)
    res = {"reads": a.reads, "read_bases": sum(len(s) for _, s in rds), "threads": a.threads, "backend": L.mm2amd_backend_name().decode()}
    try:
        res["commit"] = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], stderr=subprocess.DEVNULL).decode().strip()
    except Exception:  # noqa: BLE001
        res["commit"] = None
    try:
        al.stage(rds)
        n_reg, reg, rep_len = al.run(raw=True)
        n, arr, items, seg_off, n_seg = al._staged
        ptrs = [reg[k] + j * C.sizeof(mm.Reg1) for k in range(n) for j in range(n_reg[k])]
        hit_reads = [items[k][1] for k in range(n) for j in range(n_reg[k])]
        nh = len(ptrs)
        res["hits"] = nh
        res["aligned_query_bases"] = sum(mm.Reg1.from_address(p).qe - mm.Reg1.from_address(p).qs for p in ptrs)
        harr, qarr, qlen = (C.c_void_p * nh)(*ptrs), (C.c_char_p * nh)(*hit_reads), (C.c_int32 * nh)(*[len(r) for r in hit_reads])
        out = (mm.TxtRes * nh)()
        # ---- the device ----
        for tag, what in (("cs", mm.TXT_CS), ("MD", mm.TXT_MD), ("ds", mm.TXT_DS)):
            best = None
            for _ in range(a.repeat + 1):  # (the first pass allocates)
                mm.profile_enable(True)
                t0 = time.perf_counter()
                mm._check(L.mm2amd_hits_text_batch(al._idx, nh, harr, qarr, qlen, what, 0, out, None, 0))
                t1 = time.perf_counter()
                total = sum(r.len for r in out)
                pool = C.create_string_buffer(max(total, 1))
                t2 = time.perf_counter()
                mm._check(L.mm2amd_hits_text_batch(al._idx, nh, harr, qarr, qlen, what, 0, out, pool, total))
                t3 = time.perf_counter()
                prof = mm.profile_get()
                mm.profile_enable(False)
                # (the writing call runs the sizing pass again: its launches are counted in the size kernel's total)
                cur = {"text_bytes": total, "sizing_call_ms": (t1 - t0) * 1e3, "writing_call_ms": (t3 - t2) * 1e3,
                       "kernel_size_ms_per_launch": prof["aln_text_kernel[size]"]["ms"] / max(1, prof["aln_text_kernel[size]"]["launches"]),
                       "kernel_write_ms": prof["aln_text_kernel[write]"]["ms"], "columns": prof["aln_text_kernel[write]"]["units"]}
                if best is None or cur["writing_call_ms"] < best["writing_call_ms"]:
                    best = cur
            best["kernel_write_gb_per_s"] = best["text_bytes"] / max(best["kernel_write_ms"], 1e-9) / 1e6
            res["device_" + tag] = best
        res["device_ds"]["over_cs"] = {k: res["device_ds"][k] / max(res["device_cs"][k], 1e-9)
                                       for k in ("sizing_call_ms", "writing_call_ms", "kernel_size_ms_per_launch", "kernel_write_ms", "text_bytes")}

        # ---- the host writers on the same records ----
        def format_ms(extra):
            mo = mm.MapOpt.from_buffer_copy(al.map_opt)
            mo.flag |= extra
            mm._check(L.mm_gpu_init_index_multi(al._idx, C.byref(mo), a.threads, 0, None))
            best, size = None, 0
            for _ in range(a.repeat):
                o, ol = C.c_void_p(), C.c_size_t()
                t0 = time.perf_counter()
                mm._check(L.mm_gpu_format_batch(n, seg_off, n_seg, arr, n_reg, reg, rep_len, C.byref(o), C.byref(ol)))
                dt = (time.perf_counter() - t0) * 1e3
                mm._libc_free(o)
                best, size = (dt if best is None else min(best, dt)), ol.value
            return best, size
        base, base_bytes = format_ms(0)
        cs_ms, cs_bytes = format_ms(F_OUT_CS)
        md_ms, md_bytes = format_ms(F_OUT_MD)
        ds_ms, ds_bytes = format_ms(F_OUT_DS)
        res["host_format_batch"] = {"paf_ms": base, "paf_cs_ms": cs_ms, "paf_md_ms": md_ms, "paf_ds_ms": ds_ms, "cs_ms": cs_ms - base, "md_ms": md_ms - base,
                                    "ds_ms": ds_ms - base, "cs_bytes": cs_bytes - base_bytes, "md_bytes": md_bytes - base_bytes, "ds_bytes": ds_bytes - base_bytes,
                                    "threads": a.threads}
        res["reference_loop"] = None
        if os.path.exists(reflib.REF_SO):  # the compiled reference's writers, hit by hit on one thread (ctypes call overhead included)
            R = C.CDLL(reflib.REF_SO)
            R.mm_idx_str.restype = C.c_void_p
            R.mm_idx_str.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_char_p)]
            R.mm_gen_cs.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.c_void_p, C.c_void_p, C.c_char_p, C.c_int]
            R.mm_gen_MD.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.c_void_p, C.c_void_p, C.c_char_p]
            R.mm_gen_ds.argtypes = R.mm_gen_cs.argtypes
            R.mm_idx_destroy.argtypes = [C.c_void_p]
            mi = R.mm_idx_str(al.idx_opt.w, al.idx_opt.k, 0, 14, 2, (C.c_char_p * 2)(*refs), (C.c_char_p * 2)(*[x.encode() for x in names]))
            buf, cap = C.c_void_p(), C.c_int(0)
            t0 = time.perf_counter()
            nb_cs = sum(R.mm_gen_cs(None, C.byref(buf), C.byref(cap), mi, p, r, 1) for p, r in zip(ptrs, hit_reads))
            t1 = time.perf_counter()
            nb_md = sum(R.mm_gen_MD(None, C.byref(buf), C.byref(cap), mi, p, r) for p, r in zip(ptrs, hit_reads))
            t2 = time.perf_counter()
            nb_ds = sum(R.mm_gen_ds(None, C.byref(buf), C.byref(cap), mi, p, r, 1) for p, r in zip(ptrs, hit_reads))
            t3 = time.perf_counter()
            mm._libc_free(buf)
            R.mm_idx_destroy(mi)
            res["reference_loop"] = {"cs_ms": (t1 - t0) * 1e3, "md_ms": (t2 - t1) * 1e3, "ds_ms": (t3 - t2) * 1e3, "cs_bytes": nb_cs, "md_bytes": nb_md,
                                     "ds_bytes": nb_ds, "threads": 1}
            assert nb_cs == res["device_cs"]["text_bytes"] and nb_md == res["device_MD"]["text_bytes"] and nb_ds == res["device_ds"]["text_bytes"], \
                "the device's text and the reference's differ in length"
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
