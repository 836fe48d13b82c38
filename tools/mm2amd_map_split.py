#!/usr/bin/env python3
"""Map reads against a multi-part index, as `minimap2 --split-prefix PREFIX` does: every part in turn, the parts' hits in temp files, then one merge
pass that ranks each read's hits across the parts and writes SAM (with the @SQ lines of all parts) or PAF.

    python tools/mm2amd_map_split.py --split-prefix PREFIX [-x map-ont] [-a] [-c] [-N n] [-p ratio] [--paf-no-hit] [-I bases] [-t threads] [-o out] index.mmi reads.fq [mates.fq]

index.mmi: a multi-part index (minimap2 -I ... -d), or a FASTA / FASTQ, which is cut into parts of -I bases as minimap2 cuts it.  MM2AMD_DEVICE_MERGE=1 runs the merge's
hit-list rules on the device."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(argv=None):
    import minimap2_amd as mm
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--split-prefix", required=True)
    ap.add_argument("-x", dest="preset", default=None)
    ap.add_argument("-a", dest="sam", action="store_true", help="SAM (default: PAF)")
    ap.add_argument("-c", dest="cg", action="store_true", help="PAF with the cg tag")
    ap.add_argument("-N", dest="best_n", type=int, default=None)
    ap.add_argument("-p", dest="pri_ratio", type=float, default=None)
    ap.add_argument("--paf-no-hit", action="store_true")
    ap.add_argument("-I", dest="idx_batch", default="8G", help="bases per index part when the reference is a sequence file (k / m / g suffix)")
    ap.add_argument("-t", dest="threads", type=int, default=0)
    ap.add_argument("-o", dest="out", default=None)
    ap.add_argument("index")
    ap.add_argument("reads", nargs="+")
    a = ap.parse_args(argv)
    over = {}
    if a.best_n is not None:
        over["best_n"] = a.best_n
    if a.pri_ratio is not None:
        over["pri_ratio"] = a.pri_ratio
    flags = (0x020 if a.cg else 0) | (0x8000000 if a.paf_no_hit else 0)  # MM_F_OUT_CG, MM_F_PAF_NO_HIT
    mult = {"k": 1000, "m": 1000000, "g": 1000000000}.get(a.idx_batch[-1].lower())
    idx_batch = int(float(a.idx_batch[:-1]) * mult) if mult else int(a.idx_batch)
    out = a.out if a.out else sys.stdout.buffer
    n = mm.map_split(a.index, a.reads if len(a.reads) > 1 else a.reads[0], a.split_prefix, out, preset=a.preset, sam=a.sam, n_threads=a.threads, extra_flags=flags,
                     cigar=a.sam or a.cg, opt_overrides=over, idx_batch_size=idx_batch)
    print("[mm2amd_map_split] %d index part%s" % (n, "" if n == 1 else "s"), file=sys.stderr)
    return 0


if __name__ == "__main__":
    sys.exit(main())
