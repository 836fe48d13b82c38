#!/usr/bin/env python3
"""The counterpart of `minimap2 -d`: build the index of a FASTA / FASTQ file (plain or gzip) on the device and write it as a .mmi
(mm2amd_idx_str + mm2amd_idx_dump; the file loads with the unmodified minimap2).

    tools/mm2amd_index.py [-x preset] [-k K] [-w W] [-H] [--no-seq] [-b bucket_bits] [--json] [--device-reader] -d out.mmi ref.fa

--device-reader reads the reference through minimap2_amd.FastxReader on the device (fastx_lines_kernel / fastx_classify_kernel / fastx_copy_kernel;
comments dropped, qualities not kept) instead of the Python loop of read_fastx; the index is the same.

--json prints one line with the phase times (seconds): read and parse, device build, regroup and serialise (HIP events), device-to-host
copies (HIP events; they run beside the file write), file write, total, and the bytes written.  --load-back loads the written file again
(mm2amd_idx_load) and adds that call's phases."""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import minimap2_amd as mm  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("-x", dest="preset", default=None, help="preset (its k, w and -H; as minimap2 -x)")
    ap.add_argument("-k", type=int, default=None)
    ap.add_argument("-w", type=int, default=None)
    ap.add_argument("-H", dest="hpc", action="store_true", help="homopolymer-compressed minimizers")
    ap.add_argument("-b", dest="bucket_bits", type=int, default=None, help="bucket bits of the file (default: the preset's, 14)")
    ap.add_argument("--no-seq", action="store_true", help="write an index without the sequence (minimap2 --idx-no-seq)")
    ap.add_argument("-d", dest="out", required=True, help="the .mmi to write")
    ap.add_argument("--json", action="store_true", help="print the phase times as one JSON line")
    ap.add_argument("--load-back", action="store_true", help="load the file again and time that")
    ap.add_argument("--device-reader", action="store_true", help="read the reference with FastxReader(device=True) instead of read_fastx")
    ap.add_argument("ref", help="FASTA / FASTQ, plain or gzip")
    a = ap.parse_args(argv)
    L = mm.lib()
    io, mo = mm.IdxOpt(), mm.MapOpt()
    L.mm2amd_set_opt(None, C.byref(io), C.byref(mo))
    if a.preset is not None and L.mm2amd_set_opt(a.preset.encode(), C.byref(io), C.byref(mo)) != 0:
        sys.exit("unknown preset %r" % a.preset)
    k, w = a.k or io.k, a.w or io.w
    hpc = 1 if (a.hpc or io.flag & mm.I_HPC) else 0
    b = a.bucket_bits or io.bucket_bits
    t_start = time.time()
    if a.device_reader:  # the records stay where the reader left them: the index is built from their addresses
        import numpy as np
        batches = list(mm.FastxReader(a.ref, with_qual=False, device=True))
        if not batches:
            sys.exit("%s: no sequence" % a.ref)
        recs = np.concatenate([bt.records for bt in batches])
        n, bases = len(recs), int(recs["l_seq"].sum())
        seq_arr = (C.c_char_p * n).from_buffer(np.ascontiguousarray(recs["seq"]))
        name_arr = (C.c_char_p * n).from_buffer(np.ascontiguousarray(recs["name"]))
    else:
        names, seqs = mm.read_fastx(a.ref)
        n, bases = len(seqs), sum(len(s) for s in seqs)
        seq_arr, name_arr = (C.c_char_p * n)(*seqs), (C.c_char_p * n)(*names)
    t_read = time.time() - t_start
    t0 = time.time()
    h = L.mm2amd_idx_str(w, k, hpc, b, n, seq_arr, name_arr)
    if not h:
        sys.exit("index construction failed: " + L.mm2amd_last_error().decode())
    t_build = time.time() - t0
    try:
        t0 = time.time()
        mm.idx_dump(h, a.out, b, mm.DUMP_NO_SEQ if a.no_seq else 0)
        t_dump = time.time() - t0
        st = mm.idx_io_stats()
    finally:
        mm.idx_destroy(h)
    res = {"tool": "mm2amd_index", "ref": os.path.basename(a.ref), "k": k, "w": w, "hpc": hpc, "bucket_bits": b, "n_seq": n, "bases": bases, "reader": "FastxReader" if a.device_reader else "read_fastx",
           "read_parse_s": round(t_read, 4), "device_build_s": round(t_build, 4), "dump_s": round(t_dump, 4),
           "regroup_s": round(st["regroup_ms"] / 1e3, 5), "serialise_s": round(st["kernel_ms"] / 1e3, 5), "d2h_s": round(st["copy_ms"] / 1e3, 5),
           "file_write_s": round(st["file_ms"] / 1e3, 4), "image_bytes": int(st["image_bytes"]), "file_bytes": int(st["file_bytes"]),
           "n_chunks": int(st["n_chunks"]), "chunk_bytes": int(st["chunk_bytes"])}
    if st["kernel_ms"] > 0:
        res["serialise_GBps"] = round(st["image_bytes"] / st["kernel_ms"] / 1e6, 1)  # bytes of image written per second of kernel time
    if a.load_back:
        t0 = time.time()
        g, _ = mm.idx_load(a.out)
        t_load = time.time() - t0
        mm.idx_destroy(g)
        ls = mm.idx_io_stats()
        res.update({"load_s": round(t_load, 4), "load_file_read_s": round(ls["file_ms"] / 1e3, 4), "load_h2d_s": round(ls["copy_ms"] / 1e3, 5), "load_unpack_s": round(ls["kernel_ms"] / 1e3, 5),
                    "load_sort_s": round(ls["sort_ms"] / 1e3, 5), "load_tables_s": round(ls["tables_ms"] / 1e3, 5)})
        if ls["kernel_ms"] > 0:
            res["unpack_GBps"] = round(ls["image_bytes"] / ls["kernel_ms"] / 1e6, 1)
    res["total_s"] = round(time.time() - t_start, 4)
    if a.json:
        print(json.dumps(res))
    else:
        sys.stderr.write("[mm2amd_index] %d sequences, %d bases -> %s (%d bytes): read %.2f s, build %.2f s, dump %.2f s\n" % (n, res["bases"], a.out, res["file_bytes"], t_read, t_build, t_dump))
    return 0


if __name__ == "__main__":
    sys.exit(main())
