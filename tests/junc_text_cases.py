"""Shared by tests/test_gpu_junc_text.py and tests/test_junc_text_emu.py (not a test): hits for junc_text_kernel (--write-junc behind
mm_gpu_format_batch_dev, and mm2amd_hits_junc_batch) and their judges -- never the code under test.  Hand-built hits: the UNMODIFIED compiled
reference's mm_write_junc (format.c:263-300) through ctypes on oracle/_ref/libminimap2_ref.so, driven by the rule of map.c:601-607.  Mapped
reads: the reference binary oracle/_ref/minimap2_ref with --write-junc on the same files.  Every device case asserts path == FMT_PATH_DEVICE,
and the host writer's text (mm_gpu_format_batch) is compared wherever both exist."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import aln_text_cases as A  # noqa: E402
import rec_text_cases as X  # noqa: E402
import reflib  # noqa: E402

HAVE_REF, HAVE_BIN = X.HAVE_REF, X.HAVE_BIN
F_CIGAR, F_OUT_SAM, F_PAF_NO_HIT = X.F_CIGAR, X.F_OUT_SAM, X.F_PAF_NO_HIT
F_OUT_JUNC = 0x10000000000  # MM_F_OUT_JUNC (minimap.h:50)
JUNC = F_OUT_JUNC | F_CIGAR  # what --write-junc sets (main.c)
IS_SPLICED = 1 << 27         # mm_reg1_t::is_spliced (minimap.h:112-127)
M, I, D, N, S, H, P, EQ, XM = 0, 1, 2, 3, 4, 5, 6, 7, 8


def cig(ops):
    return [n << 4 | op for op, n in ops]


def tlen(ops):
    return sum(n for op, n in ops if op in (M, D, N, EQ, XM))


def jhit(mm, rid, rs, ops, rev=0, ts=1, spliced=True, re=None, **kw):
    """a hit at rs of contig rid with the operations ops ((op, len) list; None: no base-level alignment); re: the hit's end when it is NOT where the operations end"""
    end = rs + (tlen(ops) if ops is not None else 50) if re is None else re
    r, keep = X.hit(mm, rid, rs, end, 0, 10, rev, cig(ops) if ops is not None else None, trans_strand=ts, **kw)
    if spliced:
        r.bits |= IS_SPLICED
    return r, keep


# ---------------------------------------------------------------------------------------------------------
# the judge: the compiled reference's mm_write_junc
# ---------------------------------------------------------------------------------------------------------
class RefJunc(object):
    def __init__(self, contigs, names):
        R = self.R = C.CDLL(reflib.REF_SO)
        R.mm_idx_str.restype = C.c_void_p
        R.mm_idx_str.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_char_p)]
        R.mm_idx_destroy.argtypes = [C.c_void_p]
        R.mm_write_junc.restype = None
        R.mm_write_junc.argtypes = [C.POINTER(X.KString), C.c_void_p, C.c_void_p, C.c_void_p]
        n = len(contigs)
        self._keep = (list(contigs), [x.encode() for x in names])
        self.mi = R.mm_idx_str(10, 15, 0, 14, n, (C.c_char_p * n)(*contigs), (C.c_char_p * n)(*self._keep[1]))
        assert self.mi
        self.ks = X.KString()

    def one(self, t, r):
        """mm_write_junc's kstring for hit r of read t"""
        self.R.mm_write_junc(C.byref(self.ks), self.mi, t, C.byref(r))
        return C.string_at(self.ks.s, self.ks.l) if self.ks.l else b""

    def text(self, mm, rec):
        """map.c:601-607 over every segment of every fragment"""
        out = []
        sz = C.sizeof(mm.Bseq1)
        for i in range(rec.n_reads):
            for j in range(rec.n_reg[i]):
                r = rec.regs[i][j]
                if r.id != r.parent or r.mapq < 10:
                    continue
                s = self.one(C.byref(rec.arr, i * sz), r)
                if s:
                    out.append(s + b"\n")
        return b"".join(out)

    def per_hit(self, mm, rec):
        sz = C.sizeof(mm.Bseq1)
        return [self.one(C.byref(rec.arr, i * sz), rec.regs[i][j]) for i in range(rec.n_reads) for j in range(rec.n_reg[i])]

    def close(self):
        if self.mi:
            self.R.mm_idx_destroy(self.mi)
            self.mi = None
            if self.ks.s:
                reflib._libc.free(self.ks.s)


def check_device(mm, ctx, ref, rec):
    """the device's text == the reference's == the host writer's, written by the device; returns the text"""
    want = ref.text(mm, rec)
    got, path = ctx.dev(rec)
    assert path == mm.FMT_PATH_DEVICE
    assert got == want, X.first_difference(got, want)
    assert ctx.host(rec) == want
    return want


def read(name, hits):
    return (name, b"ACGTACGTAC", None, None, hits, -1)


# ---------------------------------------------------------------------------------------------------------
# the contigs: 0 holds every donor / acceptor pair over codes 0-4 around an intron of 4 bases, with one base between two introns; 1-5 are
# random letters with a few N.  Lengths chosen so that sequences 1.. start at nibble offsets that are no multiple of 8.
# ---------------------------------------------------------------------------------------------------------
NAME_LENS = (1, 15, 16, 17, 64, 255)
TABLE_OPS = [(M, 1)] + [(N, 4), (M, 1)] * 625


def contigs_and_names():
    rng = np.random.default_rng(23)
    t = [0]
    for d in range(25):
        for a in range(25):
            t += [d // 5, d % 5, a // 5, a % 5, int(rng.integers(0, 4))]
    out = [np.array(t + [1, 2, 3, 3, 3], dtype=np.uint8)]  # 3131 bases
    for n in (910, 301, 423, 98, 77):
        c = rng.integers(0, 4, n, dtype=np.uint8)
        c[rng.integers(0, n, 6)] = 4
        out.append(c)
    off = np.cumsum([0] + [len(c) for c in out])
    assert all(o % 8 for o in off[1:6])
    return [A.LETTERS[c].tobytes() for c in out], ["t" * n if n < 3 else "c%d_" % n + "x" * (n - len("c%d_" % n)) for n in NAME_LENS]


def table_reads(mm):
    """the score table in the four orientations, and the hits mm_write_junc writes nothing for"""
    reads = [read(b"r%d_%d" % (rev, ts), [jhit(mm, 0, 0, TABLE_OPS, rev=rev, ts=ts)]) for rev in (0, 1) for ts in (1, 2)]
    reads.append(read(b"ts0", [jhit(mm, 0, 0, TABLE_OPS, ts=0)]))
    reads.append(read(b"ts3", [jhit(mm, 0, 0, TABLE_OPS, ts=3)]))
    reads.append(read(b"unspliced", [jhit(mm, 0, 0, TABLE_OPS, spliced=False)]))
    reads.append(read(b"no_p", [jhit(mm, 0, 0, None)]))
    reads.append(read(b"spliced_without_N", [jhit(mm, 1, 7, [(M, 30), (D, 2), (M, 9)])]))
    return reads


def filter_reads(mm):
    ops = [(M, 5), (N, 20), (M, 5)]
    return [read(b"mapq9", [jhit(mm, 1, 10, ops, mapq=9)]), read(b"mapq10", [jhit(mm, 1, 50, ops, mapq=10)]),
            read(b"secondary", [jhit(mm, 1, 90, ops, id=0), jhit(mm, 1, 130, ops, id=1, parent=0), jhit(mm, 2, 30, ops, id=2, rev=1)]),
            read(b"no_hits", []), read(b"mapq255", [jhit(mm, 3, 12, ops, mapq=255, ts=2)])]


def walk_reads(mm):
    """the carry across a 64-operation step, more than one ballot's worth of introns, operations that stand still, overlapping donor and acceptor"""
    at = [(N, 3) if k in (62, 63, 64, 65) else (M, 1) for k in range(70)]
    many = [(M, 1)] + [x for k in range(130) for x in ((N, 2 + k % 2), (M, 1))]
    mixed = [(S, 5), (M, 3), (I, 2), (N, 4), (EQ, 2), (XM, 1), (D, 3), (N, 3), (H, 2), (P, 1), (N, 2), (I, 7), (M, 2), (S, 1)]
    return [read(b"carry", [jhit(mm, 1, 3, at), jhit(mm, 1, 100, at, rev=1, ts=1, id=1)]), read(b"many", [jhit(mm, 1, 11, many, ts=2)]),
            read(b"mixed", [jhit(mm, 2, 9, mixed), jhit(mm, 3, 21, mixed, rev=1, id=1)])]


def packed_reads(mm, lens):
    """intron starts at every offset modulo 8 on three contigs (their sequences start at different nibbles), and an intron that ends on a contig's last base"""
    reads = []
    for rid in (1, 2, 3):
        hits = [jhit(mm, rid, rs, [(M, 1), (N, 5 + rs % 3), (M, 2)], rev=rs & 1, ts=1 + (rs >> 1 & 1), id=rs) for rs in range(16)]
        reads.append(read(b"mod8_c%d" % rid, hits))
    for rid in (1, 4, 5):
        n = lens[rid]
        reads.append(read(b"last_base_c%d" % rid, [jhit(mm, rid, n - 12, [(M, 3), (N, 9)], rev=rid & 1)]))
    return reads


def name_reads(mm):
    """read and target names of 1, 15, 16, 17, 64 and 255 bytes (contig k's name has NAME_LENS[k] bytes)"""
    return [(b"q" * n, b"ACGTACGTAC", None, None, [jhit(mm, k, 20 + k, [(M, 4), (N, 10 + k), (M, 4)], ts=1 + k % 2)], -1) for k, n in enumerate(NAME_LENS)] + \
           [(b"Q" * NAME_LENS[5 - k], b"ACGTACGTAC", None, None, [jhit(mm, k, 40, [(M, 2), (N, 6), (M, 2)], rev=1)], -1) for k in range(6)]


def check_formats(mm):
    """score table, filter, walk, packed reference, names, fragments and the bookkeeping behind the three format calls"""
    contigs, names = contigs_and_names()
    lens = [len(c) for c in contigs]
    ref = RefJunc(contigs, names)
    try:
        ctx = X.Ctx(mm, contigs, names, JUNC, preset="splice")
        try:
            rec = X.Records(mm, table_reads(mm))
            want = check_device(mm, ctx, ref, rec)
            lines = want.split(b"\n")[:-1]
            assert len(lines) == 4 * 625 and {ln.split(b"\t")[4] for ln in lines} == {b"%d" % s for s in range(7)}  # (the reference's text: every score, both signs)
            assert sum(ln.endswith(b"-") for ln in lines) == 2 * 625
            big = want
            # buffer reuse: a smaller batch after a larger one
            small = check_device(mm, ctx, ref, X.Records(mm, filter_reads(mm)))
            assert 0 < len(small) < len(big) and small.count(b"\n") == 4 and b"mapq9\t" not in small and b"mapq10\t" in small
            check_device(mm, ctx, ref, X.Records(mm, walk_reads(mm)))
            assert check_device(mm, ctx, ref, X.Records(mm, packed_reads(mm, lens))).count(b"\n") == 3 * 16 + 3
            assert check_device(mm, ctx, ref, X.Records(mm, name_reads(mm))).count(b"\n") == 12
            # fragments of two segments and of one, junctions in either mate
            fr = walk_reads(mm)[:1] + filter_reads(mm)[3:4] + name_reads(mm)[:1] + filter_reads(mm)[3:4] + walk_reads(mm)[1:2]
            assert check_device(mm, ctx, ref, X.Records(mm, fr, n_seg=[2, 1, 2])).count(b"\n") == 8 + 1 + 130
            # an empty batch, and batches that print nothing
            assert ctx.dev(X.Records(mm, [])) == (b"", mm.FMT_PATH_DEVICE)
            quiet = X.Records(mm, table_reads(mm)[4:] + filter_reads(mm)[:1] + filter_reads(mm)[3:4])
            assert ctx.dev(quiet) == (b"", mm.FMT_PATH_DEVICE) and ctx.host(quiet) == b"" and ref.text(mm, quiet) == b""
            # CIGARs the reference asserts on: MM2AMD_EINVAL from all three calls, and the context works afterwards
            for bad in (jhit(mm, 1, 10, [(M, 5), (N, 1), (M, 5)]), jhit(mm, 1, 10, [(M, 5), (N, 7), (M, 5)], re=10 + 18), jhit(mm, 1, 10, [(M, 5), (N, 7), (M, 5)], re=10 + 16)):
                rec = X.Records(mm, walk_reads(mm)[:1] + [read(b"bad", [bad])] + walk_reads(mm)[1:2])
                for rc in format_calls(ctx, rec):
                    assert rc == mm.EINVAL and b"write-junc" in ctx.L.mm2amd_last_error()
                check_device(mm, ctx, ref, X.Records(mm, walk_reads(mm)))
            # ... but not when the filter drops the hit
            ok = X.Records(mm, [read(b"bad_mapq0", [jhit(mm, 1, 10, [(M, 5), (N, 1), (M, 5)], mapq=3)])])
            assert ctx.dev(ok) == (b"", mm.FMT_PATH_DEVICE) and ctx.host(ok) == b""
        finally:
            ctx.close()
        # MM_F_OUT_SAM and MM_F_PAF_NO_HIT on top change nothing
        ctx = X.Ctx(mm, contigs, names, JUNC | F_OUT_SAM | F_PAF_NO_HIT, preset="splice")
        try:
            rec = X.Records(mm, filter_reads(mm) + walk_reads(mm))
            assert check_device(mm, ctx, ref, rec) == small + ref.text(mm, X.Records(mm, walk_reads(mm)))
        finally:
            ctx.close()
    finally:
        ref.close()
    # an index built without names
    ctx = X.Ctx(mm, contigs, None, JUNC, preset="splice")
    try:
        rec = X.Records(mm, filter_reads(mm))
        for rc in format_calls(ctx, rec):
            assert rc == mm.EINVAL and b"names" in ctx.L.mm2amd_last_error()
    finally:
        ctx.close()


def format_calls(ctx, rec):
    """the return codes of mm_gpu_format_batch, _view and _dev"""
    L = ctx.L
    out, n, path = C.c_void_p(), C.c_size_t(), C.c_int(-1)
    args = (rec.n_frag, rec.seg_off, rec.n_seg, rec.arr, rec.n_reg, rec.reg, rec.rep_len, C.byref(out), C.byref(n))
    rcs = [L.mm_gpu_format_batch(*args)]
    if rcs[0] == 0:
        reflib._libc.free(out)
    rcs.append(L.mm_gpu_format_batch_view(*args))
    rcs.append(L.mm_gpu_format_batch_dev(*(args + (C.byref(path),))))
    return rcs


# ---------------------------------------------------------------------------------------------------------
# mm2amd_hits_junc_batch
# ---------------------------------------------------------------------------------------------------------
def check_hits_junc(mm):
    contigs, names = contigs_and_names()
    lens = [len(c) for c in contigs]
    ref = RefJunc(contigs, names)
    ctx = X.Ctx(mm, contigs, names, JUNC, preset="splice")
    L = ctx.L
    try:
        reads = table_reads(mm) + filter_reads(mm) + walk_reads(mm) + packed_reads(mm, lens) + name_reads(mm)
        rec = X.Records(mm, reads)
        want = ref.per_hit(mm, rec)  # no mapq / parent filter: mapq9 and the secondary write their lines
        ptrs = [rec.reg[i] + j * C.sizeof(mm.Reg1) for i in range(rec.n_reads) for j in range(rec.n_reg[i])]
        qn = [reads[i][0] for i in range(rec.n_reads) for j in range(rec.n_reg[i])]
        got = mm.hits_junc(ctx.idx, ptrs, qn)
        assert [g.encode() for g in got] == want
        assert sum(1 for w in want if not w) == 5 and all(not w.endswith(b"\n") for w in want) and want[0].count(b"\n") == 624
        assert mm.hits_junc(ctx.idx, [], []) == []
        # the sizing call, and a pool that is too small: the lengths, nothing written
        n = len(ptrs)
        harr, narr = (C.c_void_p * n)(*ptrs), (C.c_char_p * n)(*qn)
        res = (mm.TxtRes * n)()
        assert L.mm2amd_hits_junc_batch(ctx.idx, n, harr, narr, res, None, 0) == 0
        assert [r.len for r in res] == [len(w) for w in want] and all(r.status == 0 for r in res)
        total = sum(len(w) for w in want)
        guard = 64
        pool = C.create_string_buffer(b"\xa5" * (total + guard), total + guard)
        res2 = (mm.TxtRes * n)()
        assert L.mm2amd_hits_junc_batch(ctx.idx, n, harr, narr, res2, pool, total - 1) == mm.ENOMEM
        assert [r.len for r in res2] == [len(w) for w in want] and pool.raw == b"\xa5" * (total + guard)
        assert L.mm2amd_hits_junc_batch(ctx.idx, n, harr, narr, res2, pool, total) == 0
        assert pool.raw[total:] == b"\xa5" * guard and pool.raw[:total] == b"".join(want)
        assert [r.off for r in res2] == [sum(len(w) for w in want[:k]) for k in range(n)]
        # CIGARs that break the reference's asserts: status -1 and no text for them, the others get theirs
        good = walk_reads(mm)
        bad1, bad2 = jhit(mm, 1, 10, [(M, 5), (N, 1), (M, 5)]), jhit(mm, 1, 10, [(M, 5), (N, 7), (M, 5)], re=10 + 16)
        rec = X.Records(mm, [good[0], read(b"bad1", [bad1]), good[1], read(b"bad2", [bad2]), good[2]])
        ptrs = [rec.reg[i] + j * C.sizeof(mm.Reg1) for i in range(rec.n_reads) for j in range(rec.n_reg[i])]
        qn = [rec.reads[i][0] for i in range(rec.n_reads) for j in range(rec.n_reg[i])]
        got = mm.hits_junc(ctx.idx, ptrs, qn)
        okrec = X.Records(mm, good)
        assert [g for g in got if g is not None] == [w.decode() for w in ref.per_hit(mm, okrec)] and [k for k, g in enumerate(got) if g is None] == [2, 4]
        # a hit outside its sequence
        out = jhit(mm, 4, 90, [(M, 5), (N, 7), (M, 5)])
        p = (C.c_void_p * 1)(C.addressof(out[0]))
        assert L.mm2amd_hits_junc_batch(ctx.idx, 1, p, (C.c_char_p * 1)(b"x"), res, None, 0) == mm.EINVAL
        out[0].rid = 6
        assert L.mm2amd_hits_junc_batch(ctx.idx, 1, p, (C.c_char_p * 1)(b"x"), res, None, 0) == mm.EINVAL
    finally:
        ctx.close()
        ref.close()
    ctx = X.Ctx(mm, contigs, None, JUNC, preset="splice")
    try:
        h = jhit(mm, 1, 10, [(M, 5), (N, 7), (M, 5)])
        res = (mm.TxtRes * 1)()
        assert ctx.L.mm2amd_hits_junc_batch(ctx.idx, 1, (C.c_void_p * 1)(C.addressof(h[0])), (C.c_char_p * 1)(b"x"), res, None, 0) == mm.EINVAL
    finally:
        ctx.close()


# ---------------------------------------------------------------------------------------------------------
# mapped reads against the reference binary
# ---------------------------------------------------------------------------------------------------------
def binary_junc(ref_fa, read_files, preset):
    return subprocess.run([reflib.REF_BIN, "-x", preset, "-t", "2", "--write-junc", ref_fa] + list(read_files), stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, check=True).stdout


def assert_reference_shapes(want):
    """the shapes the read sets are for, asserted on the REFERENCE's text: a junction on the minus strand and one with a score below 6"""
    lines = [ln.split(b"\t") for ln in want.split(b"\n") if ln]
    assert lines and any(f[5] == b"-" for f in lines) and any(f[5] == b"+" for f in lines) and any(int(f[4]) < 6 for f in lines)
