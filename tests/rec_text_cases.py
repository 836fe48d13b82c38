"""Shared by tests/test_gpu_rec_text.py and tests/test_rec_text_emu.py (not a test): records for rec_text_kernel (mm_gpu_format_batch_dev) and
their judges -- never the code under test.  Hand-built records: the UNMODIFIED compiled reference's mm_write_paf4 / mm_write_sam3 through
ctypes on oracle/_ref/libminimap2_ref.so, driven by the record rules of map.c:585-623.  Mapped reads: the reference binary
oracle/_ref/minimap2_ref on the same files.  Every case meant for the device asserts path == FMT_PATH_DEVICE, so that a fallback to the host
writer cannot stand in for the kernel; wherever both exist the text is compared with mm_gpu_format_batch's as well."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import aln_text_cases as A  # noqa: E402
import reflib  # noqa: E402
import synth  # noqa: E402

HAVE_REF = os.path.exists(reflib.REF_SO)
HAVE_BIN = os.path.exists(reflib.REF_BIN)

# MM_F_* (minimap.h:10-50)
F_CIGAR, F_OUT_SAM, F_OUT_CG, F_OUT_CS, F_OUT_CS_LONG, F_NO_PRINT_2ND, F_LONG_CIGAR, F_SOFTCLIP = 0x4, 0x8, 0x20, 0x40, 0x800, 0x4000, 0x10000, 0x80000
F_OUT_MD, F_COPY_COMMENT, F_PAF_NO_HIT, F_SAM_HIT_ONLY, F_QSTRAND, F_NO_INV = 0x1000000, 0x2000000, 0x8000000, 0x40000000, 0x100000000, 0x200000000
F_SECONDARY_SEQ, F_OUT_DS = 0x1000000000, 0x2000000000
PAF, PAF_C, SAM = 0, F_CIGAR | F_OUT_CG, F_CIGAR | F_OUT_SAM


class KString(C.Structure):  # kstring_t
    _fields_ = [("l", C.c_size_t), ("m", C.c_size_t), ("s", C.c_void_p)]


# ---------------------------------------------------------------------------------------------------------
# a batch of hand-built records: reads (mm_bseq1_t) and their hits (mm_reg1_t + mm_extra_t)
# ---------------------------------------------------------------------------------------------------------
def hit(mm, rid, rs, re, qs, qe, rev, cig, id=0, parent=None, mlen=0, blen=0, mapq=60, cnt=10, score=100, subsc=0, inv=0, sam_pri=None, split=0, div=0.0,
        dp_max0=90, dp_score=80, n_ambi=0, trans_strand=0):
    """(mm_reg1_t, keep-alive): cig None = a hit without base-level alignment"""
    r, keep = A.make_reg(mm, rid, rs, re, qs, qe, rev, cig)
    parent = id if parent is None else parent
    sam_pri = (1 if id == 0 else 0) if sam_pri is None else sam_pri
    r.id, r.parent, r.mlen, r.blen, r.cnt, r.score, r.subsc, r.div = id, parent, mlen, blen, cnt, score, subsc, div
    r.bits = mapq | split << 8 | (1 << 10 if rev else 0) | inv << 11 | sam_pri << 12
    if keep is not None:
        ex = mm.Extra.from_buffer(keep)
        ex.dp_max0, ex.dp_score, ex.n_ambi_strand = dp_max0, dp_score, n_ambi | trans_strand << 30
    return r, keep


class Records(object):
    """reads: list of (name, seq, qual or None, comment or None, [hit, ...], rep_len); n_seg: None, or the fragments' segment counts"""

    def __init__(self, mm, reads, n_seg=None):
        self.n_reads = n = len(reads)
        self.reads = reads
        self.arr = (mm.Bseq1 * max(1, n))()
        self.n_reg, self.reg, self.rep_len = (C.c_int * max(1, n))(), (C.c_void_p * max(1, n))(), (C.c_int * max(1, n))()
        self.keep = []
        for i, (name, seq, qual, comment, hits, rl) in enumerate(reads):
            b = self.arr[i]
            b.l_seq, b.rid, b.name, b.seq, b.qual, b.comment = len(seq), i, name, seq, qual, comment
            regs = (mm.Reg1 * max(1, len(hits)))()
            for j, (r, k) in enumerate(hits):
                C.memmove(C.byref(regs[j]), C.byref(r), C.sizeof(mm.Reg1))
                self.keep.append(k)
            self.keep.append(regs)
            self.n_reg[i], self.reg[i], self.rep_len[i] = len(hits), C.cast(regs, C.c_void_p), rl
        self.regs = [C.cast(self.reg[i], C.POINTER(mm.Reg1)) for i in range(n)]
        if n_seg is None:
            self.n_frag, self.seg_off, self.n_seg = n, None, None
        else:
            self.n_frag = len(n_seg)
            self.n_seg = (C.c_int * len(n_seg))(*n_seg)
            self.seg_off = (C.c_int * len(n_seg))(*[sum(n_seg[:k]) for k in range(len(n_seg))])


# ---------------------------------------------------------------------------------------------------------
# the judge for hand-built records: the compiled reference's writers under the rules of map.c:585-623
# ---------------------------------------------------------------------------------------------------------
class RefWriter(object):
    def __init__(self, contigs, names):
        R = self.R = C.CDLL(reflib.REF_SO)
        R.mm_idx_str.restype = C.c_void_p
        R.mm_idx_str.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_char_p)]
        R.mm_idx_destroy.argtypes = [C.c_void_p]
        R.mm_write_paf4.restype = None
        R.mm_write_paf4.argtypes = [C.POINTER(KString), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int]
        R.mm_write_sam3.restype = None
        R.mm_write_sam3.argtypes = [C.POINTER(KString), C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int]
        n = len(contigs)
        self._keep = (list(contigs), [x.encode() for x in names] if names else None)
        narr = (C.c_char_p * n)(*self._keep[1]) if names else None
        self.mi = R.mm_idx_str(10, 15, 0, 14, n, (C.c_char_p * n)(*contigs), narr)
        assert self.mi
        self.ks = KString()

    def text(self, mm, rec, flag):
        """single-segment reads only"""
        out = []
        sz = C.sizeof(mm.Bseq1)
        for i in range(rec.n_reads):
            t = C.byref(rec.arr, i * sz)
            if rec.n_reg[i] > 0:
                for j in range(rec.n_reg[i]):
                    r = rec.regs[i][j]
                    if (flag & F_NO_PRINT_2ND) and r.id != r.parent:
                        continue
                    if flag & F_OUT_SAM:
                        self.R.mm_write_sam3(C.byref(self.ks), self.mi, t, 0, j, 1, C.addressof(rec.n_reg) + 4 * i, C.addressof(rec.reg) + 8 * i, None, flag, rec.rep_len[i])
                    else:
                        self.R.mm_write_paf4(C.byref(self.ks), self.mi, t, C.byref(r), None, flag, rec.rep_len[i], 1, 0)
                    out.append(C.string_at(self.ks.s, self.ks.l))
            elif (flag & F_PAF_NO_HIT) or ((flag & F_OUT_SAM) and not (flag & F_SAM_HIT_ONLY)):
                if flag & F_OUT_SAM:
                    self.R.mm_write_sam3(C.byref(self.ks), self.mi, t, 0, -1, 1, C.addressof(rec.n_reg) + 4 * i, C.addressof(rec.reg) + 8 * i, None, flag, rec.rep_len[i])
                else:
                    self.R.mm_write_paf4(C.byref(self.ks), self.mi, t, None, None, flag, rec.rep_len[i], 1, 0)
                out.append(C.string_at(self.ks.s, self.ks.l))
        return b"".join(x + b"\n" for x in out)

    def close(self):
        if self.mi:
            self.R.mm_idx_destroy(self.mi)
            self.mi = None
            if self.ks.s:
                reflib._libc.free(self.ks.s)


# ---------------------------------------------------------------------------------------------------------
# the library under test: an index of the same contigs and a context with the given flags
# ---------------------------------------------------------------------------------------------------------
class Ctx(object):
    def __init__(self, mm, contigs, names, flag, preset="map-ont"):
        self.mm, L = mm, mm.lib()
        self.L = L
        io, self.mo = mm.IdxOpt(), mm.MapOpt()
        L.mm2amd_set_opt(None, C.byref(io), C.byref(self.mo))
        assert L.mm2amd_set_opt(preset.encode(), C.byref(io), C.byref(self.mo)) == 0
        self.mo.flag |= flag
        n = len(contigs)
        narr = (C.c_char_p * n)(*[x.encode() for x in names]) if names else None
        self.idx = L.mm2amd_idx_str(10, 15, 0, 14, n, (C.c_char_p * n)(*contigs), narr)
        assert self.idx, L.mm2amd_last_error()
        assert L.mm2amd_mapopt_update(C.byref(self.mo), self.idx) == 0
        assert L.mm_gpu_init_index(self.idx, C.byref(self.mo), 4) == 0, L.mm2amd_last_error()

    def dev(self, rec):
        """(text, path) of mm_gpu_format_batch_dev"""
        out, n, path = C.c_void_p(), C.c_size_t(), C.c_int(-1)
        rc = self.L.mm_gpu_format_batch_dev(rec.n_frag, rec.seg_off, rec.n_seg, rec.arr, rec.n_reg, rec.reg, rec.rep_len, C.byref(out), C.byref(n), C.byref(path))
        assert rc == 0, self.L.mm2amd_last_error()
        raw = C.string_at(out, n.value + 1)
        assert raw[-1:] == b"\0"  # NUL after the last byte, as mm_gpu_format_batch_view
        return raw[:-1], path.value

    def host(self, rec):
        out, n = C.c_void_p(), C.c_size_t()
        assert self.L.mm_gpu_format_batch(rec.n_frag, rec.seg_off, rec.n_seg, rec.arr, rec.n_reg, rec.reg, rec.rep_len, C.byref(out), C.byref(n)) == 0, self.L.mm2amd_last_error()
        try:
            return C.string_at(out, n.value)
        finally:
            reflib._libc.free(out)

    def close(self):
        self.L.mm_gpu_destroy()
        self.L.mm2amd_idx_destroy(self.idx)


def first_difference(got, want):
    if got == want:
        return ""
    g, w = got.split(b"\n"), want.split(b"\n")
    for k, (a, b) in enumerate(zip(g, w)):
        if a != b:
            p = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
            return "record %d, byte %d: got %r, want %r" % (k, p, a[max(0, p - 60):p + 60], b[max(0, p - 60):p + 60])
    return "%d records, want %d" % (len(g), len(w))


def check_device(mm, ctx, ref, rec, flag):
    """the device's text == the reference's == mm_gpu_format_batch's, written by the device; returns the text"""
    want = ref.text(mm, rec, flag)
    got, path = ctx.dev(rec)
    assert path == mm.FMT_PATH_DEVICE
    assert got == want, first_difference(got, want)
    assert ctx.host(rec) == want
    return want


# ---------------------------------------------------------------------------------------------------------
# 1. fractions
# ---------------------------------------------------------------------------------------------------------
GAP_CIGARS = ("4M", "2M1I1M2D1M", "1M3I1M1D2M2I1M")  # xM gI yD: n_gap - n_gapo = 0, 1, 4


def fraction_records(mm, max_den, contig_len):
    """PAF -c records whose mlen and denominator blen + n_ambi - n_gap + n_gapo sweep all pairs 0 <= mlen <= den, 1 <= den <= max_den (den == 0 is 0 / 0: a
    value outside [0, 1], check_fallbacks); every third pair has n_ambi > 0.  Returns (Records, [(mlen, den)])."""
    hits, pairs = [], []
    for den in range(1, max_den + 1):
        for m in range(den + 1):
            cig = A.parse_cigar(GAP_CIGARS[(m + den) % 3])
            n_gap = sum(w >> 4 for w in cig if w & 15 in (1, 2))
            n_gapo = sum(1 for w in cig if w & 15 in (1, 2))
            n_ambi = 2 if (m + 2 * den) % 3 == 0 else 0
            blen = den - n_ambi + n_gap - n_gapo
            if blen < 0:
                n_ambi, blen = 0, den + n_gap - n_gapo
            ql = sum(w >> 4 for w in cig if w & 15 in (0, 1))
            tl = sum(w >> 4 for w in cig if w & 15 in (0, 2))
            hits.append(hit(mm, 0, 5, 5 + tl, 0, ql, 0, cig, mlen=m, blen=blen, n_ambi=n_ambi))
            pairs.append((m, den))
    reads = [(b"f%d" % k, b"ACGTACGTACGT", None, None, [h], -1) for k, h in enumerate(hits)]  # one read, one record each
    return Records(mm, reads), pairs


def check_fractions(mm, max_den):
    rng = np.random.default_rng(7)
    contig = A.LETTERS[rng.integers(0, 4, 200, dtype=np.uint8)].tobytes()
    ref, ctx = RefWriter([contig], ["c0"]), Ctx(mm, [contig], ["c0"], PAF_C)
    try:
        rec, pairs = fraction_records(mm, max_den, len(contig))
        want = check_device(mm, ctx, ref, rec, PAF_C)
        lines = want.split(b"\n")
        de = {p: [f for f in ln.split(b"\t") if f.startswith(b"de:f:")][0][5:] for p, ln in zip(pairs, lines)}
        assert de[(31, 32)] == b"0.0312" and de[(29, 32)] == b"0.0938" and de[(63, 64)] == b"0.0156"  # the exact ties of %.4f: to even
        assert de[(5, 5)] == b"0" and de[(0, 7)] == b"1.0000"
    finally:
        ctx.close()
    ctx = Ctx(mm, [contig], ["c0"], PAF)
    try:  # hits without base-level alignment: dv:f from the hit's float
        divs = [0.0, 0.03125, 1.0, -1.0, 0.09375, 0.015625] + [float(np.float32(x)) for x in rng.random(40)] + [float(np.float32(x)) for x in rng.random(10) * 1e-4]
        reads = [(b"d%d" % k, b"ACGTACGTACGT", None, None, [hit(mm, 0, 3, 90, 1, 11, k & 1, None, div=d, mlen=8, blen=10)], -1) for k, d in enumerate(divs)]
        want = check_device(mm, ctx, ref, Records(mm, reads), PAF)
        lines = want.split(b"\n")
        assert b"dv:f:0\t" in lines[0] + b"\t" and b"dv:f:0.0312" in lines[1] and b"dv:f:1.0000" in lines[2] and b"dv:f" not in lines[3] and b"dv:f:0.0938" in lines[4]
    finally:
        ctx.close()
        ref.close()


# ---------------------------------------------------------------------------------------------------------
# 2. directed record shapes
# ---------------------------------------------------------------------------------------------------------
class Planter(object):
    """contigs (codes) into which alignments are planted, so that the CIGARs the records carry fit the sequences (cs / MD read them)"""

    def __init__(self, rng, lens):
        self.rng = rng
        self.contigs = [rng.integers(0, 4, n, dtype=np.uint8) for n in lens]
        self.next = [16] * len(lens)

    def plant(self, mm, rid, ops, rev, head, tail, qstrand, mis=0.1, **kw):
        """a hit of `ops` ((op, len) list) on contig rid with `head` / `tail` unaligned read bases in front / behind: (read letters, hit)"""
        rng = self.rng
        q, t, cig = A.build_job(rng, ops, mis)
        q, t = np.frombuffer(q, dtype=np.uint8), np.frombuffer(t, dtype=np.uint8)
        rs = self.next[rid]
        re = rs + len(t)
        self.next[rid] = re + 11
        n = len(self.contigs[rid])
        assert re + 16 <= n
        if qstrand and rev:
            self.contigs[rid][n - re:n - rs] = A.revcomp_codes(t)
        else:
            self.contigs[rid][rs:re] = t
        mid = A.revcomp_codes(q) if (rev and not qstrand) else q
        read = A.LETTERS[np.concatenate([rng.integers(0, 4, head, dtype=np.uint8), mid, rng.integers(0, 4, tail, dtype=np.uint8)])].tobytes()
        n_m = sum(l for o, l in ops if o in (0, 7, 8))
        blen = sum(l for o, l in ops if o in (0, 1, 2, 7, 8))
        h = hit(mm, rid, rs, re, head, head + len(q), rev, cig, mlen=int(n_m * 0.9), blen=blen, **kw)
        return read, h

    def letters(self):
        return [A.LETTERS[c].tobytes() for c in self.contigs]


def ops_of(rng, n_ops, intron=None):
    """n_ops operations: M / I / D in turn (every gap between two matches), lengths 1..20"""
    ops = []
    for k in range(n_ops):
        ops.append((0, int(rng.integers(1, 21))) if k % 2 == 0 else (int(rng.choice([1, 2])), int(rng.integers(1, 6))))
    if n_ops % 2 == 0:
        ops.append((0, 3))
    if intron:
        ops.insert(1, (3, intron)), ops.insert(2, (0, 9))
    return ops


def directed_reads(mm, rng, qstrand=False, named=True):
    """the record shapes of the issue, as reads with hand-built hits; returns (contig letters, reads)"""
    P = Planter(rng, [300000, 40000, 9000])
    qual = lambda s: bytes(33 + (i * 7) % 40 for i in range(len(s)))
    reads = []

    def one(name, ops, rev, head, tail, with_qual=False, rl=-1, rid=0, **kw):
        read, h = P.plant(mm, rid, ops, rev, head, tail, qstrand, **kw)
        reads.append((name, read, qual(read) if with_qual else None, None, [h], rl))

    one(b"fwd_clips", ops_of(rng, 9), 0, 7, 5, with_qual=True, rl=12)          # both clips, quality, rl:i
    one(b"rev_clips", ops_of(rng, 9), 1, 7, 5, with_qual=True)
    one(b"fwd_noclip", ops_of(rng, 5), 0, 0, 0)                                # qs = 0 and qe = qlen
    one(b"rev_noclip", ops_of(rng, 5), 1, 0, 0, rid=1)
    one(b"inv_P", ops_of(rng, 3), 0, 2, 2, inv=1)                              # tp:A:I
    one(b"split", ops_of(rng, 3), 1, 2, 2, split=2, rid=2)                     # zd:i
    one(b"ts1", ops_of(rng, 4, intron=200), 0, 1, 1, trans_strand=1)           # ts:A:+
    one(b"ts2", ops_of(rng, 4, intron=77), 1, 1, 1, trans_strand=2, n_ambi=1)  # ts:A:-
    for n in (1, 255, 256, 257, 700):                                          # around the 256-operation staging tile
        one(b"ops%d" % n, ops_of(rng, n), n & 1, 3, 4, rid=1 if n < 700 else 0)
    one(b"short_walk", [(0, 20)], 0, 1, 1)                                     # shorter than one 64-column step
    one(b"long_walk", [(0, 150), (2, 3), (0, 70)], 1, 1, 1)                    # longer
    one(b"big_intron", [(0, 40), (3, 200000), (0, 40)], 0, 2, 2, trans_strand=1)
    # a parent with a secondary (the secondary: tp:A:S, and an inverted one: tp:A:i)
    read, h0 = P.plant(mm, 0, ops_of(rng, 7), 0, 4, 6, qstrand, id=0, subsc=55)
    h1 = hit(mm, 1, 100, 100 + (h0[0].re - h0[0].rs), h0[0].qs, h0[0].qe, 1, None, id=1, parent=0, mapq=0, div=0.0625, mlen=30, blen=40)
    _, h2 = P.plant(mm, 1, ops_of(rng, 5), 1, 0, 0, qstrand, id=2, parent=0, mapq=0, inv=1, sam_pri=0)
    h2[0].qs, h2[0].qe = 4, 4 + (h2[0].qe - h2[0].qs)
    if h2[0].qe <= len(read):
        reads.append((b"parent_2nd", read, qual(read), None, [h0, h1, h2], 3))
    else:
        reads.append((b"parent_2nd", read, qual(read), None, [h0, h1], 3))
    # a supplementary pair: two parents with base-level alignment on one read, different strands; and a third hit without p that SA:Z: skips
    ra, ha = P.plant(mm, 0, ops_of(rng, 5), 0, 3, 0, qstrand, id=0, sam_pri=1)
    rb, hb = P.plant(mm, 1, ops_of(rng, 6), 1, 0, 2, qstrand, id=1, sam_pri=0, mapq=17, n_ambi=2)
    read = ra + rb  # (the second piece keeps its letters: only its coordinates move)
    hb[0].qs, hb[0].qe = hb[0].qs + len(ra), hb[0].qe + len(ra)
    hc = hit(mm, 2, 50, 90, 1, 40, 0, None, id=2, sam_pri=0, div=0.5)
    reads.append((b"suppl", read, qual(read), None, [ha, hb, hc], -1))
    reads.append((b"unmapped", b"ACGTTGCANNACGT", None, None, [], -1))
    reads.append((b"unmapped_q", b"ACGTTGCANNACGT", qual(b"ACGTTGCANNACGT"), None, [], 5))
    return P.letters(), reads


DIRECTED_FLAGS = [PAF_C, PAF_C | F_OUT_CS, PAF_C | F_OUT_CS | F_OUT_CS_LONG, PAF_C | F_PAF_NO_HIT | F_OUT_MD, PAF | F_NO_PRINT_2ND, SAM, SAM | F_SOFTCLIP, SAM | F_SECONDARY_SEQ,
                  SAM | F_SECONDARY_SEQ | F_SOFTCLIP | F_OUT_CS, SAM | F_OUT_MD | F_SAM_HIT_ONLY, SAM | F_NO_PRINT_2ND, SAM | F_LONG_CIGAR]


def check_directed(mm, flags=DIRECTED_FLAGS):
    for qstrand in (False, True):
        contigs, reads = directed_reads(mm, np.random.default_rng(11), qstrand)
        names = ["chrA", "b", "a_longer_contig_name_of_more_than_sixteen_bytes"]
        ref = RefWriter(contigs, names)
        try:
            for flag in flags if not qstrand else [PAF_C | F_OUT_CS, PAF_C | F_OUT_MD]:
                if qstrand:
                    flag |= F_QSTRAND | F_NO_INV
                ctx = Ctx(mm, contigs, names, flag)
                try:
                    want = check_device(mm, ctx, ref, Records(mm, reads), flag)
                    if flag == SAM:
                        assert want.count(b"SA:Z:") == 2 and b"tp:A:I" in want and b"tp:A:i" in want and b"zd:i:2" in want and b"ts:A:+" in want and b"ts:A:-" in want
                        assert b"200000N" in want and b"\trl:i:12" in want
                        fl = {int(ln.split(b"\t")[1]) for ln in want.split(b"\n") if ln}
                        assert {0, 4, 16, 256, 2048} <= fl | {f & ~16 for f in fl}
                        sup = [ln for ln in want.split(b"\n") if ln.startswith(b"suppl\t")]
                        assert b"H" in sup[1].split(b"\t")[5] and b"H" not in sup[0].split(b"\t")[5]  # hard clips on the supplementary record by default
                    if flag == SAM | F_SOFTCLIP:
                        assert all(b"H" not in ln.split(b"\t")[5] for ln in want.split(b"\n") if ln)
                finally:
                    ctx.close()
        finally:
            ref.close()
    # an index without names: the target's number in PAF
    contigs, reads = directed_reads(mm, np.random.default_rng(12))
    ref, ctx = RefWriter(contigs, None), Ctx(mm, contigs, None, PAF_C)
    try:
        want = check_device(mm, ctx, ref, Records(mm, reads[:8]), PAF_C)
        assert want.split(b"\n")[3].split(b"\t")[5] == b"1"
    finally:
        ctx.close()
        ref.close()


# ---------------------------------------------------------------------------------------------------------
# 4. fallbacks and bookkeeping (hand-built records)
# ---------------------------------------------------------------------------------------------------------
def check_fallbacks(mm):
    contigs, reads = directed_reads(mm, np.random.default_rng(13))
    names = ["chrA", "b", "c"]
    ref = RefWriter(contigs, names)
    try:
        # a pair batch: the first two reads as one two-segment fragment
        ctx = Ctx(mm, contigs, names, SAM)
        try:
            rec = Records(mm, reads[:6], n_seg=[2, 1, 1, 1, 1])
            got, path = ctx.dev(rec)
            assert path == mm.FMT_PATH_HOST and got == ctx.host(rec) and got.count(b"\n") >= 6
            # the same context: single-segment batches are the device's, also with the n_seg array given; the buffer is reused by a smaller batch
            rec = Records(mm, reads[:6], n_seg=[1] * 6)
            big, path = ctx.dev(rec)
            assert path == mm.FMT_PATH_DEVICE and big == ref.text(mm, rec, SAM)
            rec = Records(mm, reads[2:4])
            small, path = ctx.dev(rec)
            assert path == mm.FMT_PATH_DEVICE and small == ref.text(mm, rec, SAM) and len(small) < len(big)
            # an empty batch, and one where no read has a hit
            got, path = ctx.dev(Records(mm, []))
            assert (got, path) == (b"", mm.FMT_PATH_DEVICE)
            rec = Records(mm, [r for r in reads if not r[4]])
            got, path = ctx.dev(rec)
            assert path == mm.FMT_PATH_DEVICE and got == ref.text(mm, rec, SAM) and got.count(b"\n") == 2
            # bad arguments as the neighbours
            out, n, p = C.c_void_p(), C.c_size_t(), C.c_int()
            assert ctx.L.mm_gpu_format_batch_dev(-1, None, None, None, None, None, None, C.byref(out), C.byref(n), C.byref(p)) == mm.EINVAL
            assert ctx.L.mm_gpu_format_batch_dev(1, None, None, None, None, None, None, C.byref(out), C.byref(n), C.byref(p)) == mm.EINVAL
            assert ctx.L.mm_gpu_format_batch_dev(0, None, None, None, None, None, None, C.byref(out), C.byref(n), None) == mm.EINVAL
        finally:
            ctx.close()
        ctx = Ctx(mm, contigs, names, SAM | F_SAM_HIT_ONLY)
        try:
            got, path = ctx.dev(Records(mm, [r for r in reads if not r[4]]))
            assert (got, path) == (b"", mm.FMT_PATH_DEVICE)
        finally:
            ctx.close()
        # --ds
        ctx = Ctx(mm, contigs, names, PAF_C | F_OUT_CS | F_OUT_DS)
        try:
            rec = Records(mm, reads[:5])
            got, path = ctx.dev(rec)
            assert path == mm.FMT_PATH_HOST and got == ctx.host(rec) and b"ds:Z:" in got
        finally:
            ctx.close()
        # -y with a comment present; without one the batch is the device's
        ctx = Ctx(mm, contigs, names, SAM | F_COPY_COMMENT)
        try:
            with_c = [reads[0], reads[1][:3] + (b"BC:Z:ACGT",) + reads[1][4:], reads[2]]
            rec = Records(mm, with_c)
            got, path = ctx.dev(rec)
            assert path == mm.FMT_PATH_HOST and got == ctx.host(rec) == ref.text(mm, rec, SAM | F_COPY_COMMENT) and b"\tBC:Z:ACGT\n" in got
            rec = Records(mm, reads[:3])
            got, path = ctx.dev(rec)
            assert path == mm.FMT_PATH_DEVICE and got == ref.text(mm, rec, SAM | F_COPY_COMMENT)
        finally:
            ctx.close()
        # a fraction outside [0, 1]: 0 / 0 (a denominator of 0) and mlen > denominator
        ctx = Ctx(mm, contigs, names, PAF_C)
        try:
            bad = [(b"nan", b"ACGTACGT", None, None, [hit(mm, 0, 5, 9, 0, 4, 0, [4 << 4], mlen=0, blen=0)], -1),
                   (b"neg", b"ACGTACGT", None, None, [hit(mm, 0, 5, 9, 0, 4, 0, [4 << 4], mlen=9, blen=4)], -1)]
            for b in bad:
                rec = Records(mm, [reads[0], b, reads[1]])
                got, path = ctx.dev(rec)
                assert path == mm.FMT_PATH_HOST and got == ctx.host(rec) == ref.text(mm, rec, PAF_C)
        finally:
            ctx.close()
    finally:
        ref.close()


# ---------------------------------------------------------------------------------------------------------
# 3. mapped reads against the reference binary
# ---------------------------------------------------------------------------------------------------------
MAPPED_SEED = 5  # chosen on the CPU with the reference binary: its -a output has FLAG 4, 16, 256, 2048 and an SA:Z: (asserted in the test)
MAPPED_CASES = [  # (name, the binary's options, Aligner arguments)
    ("a", ["-a"], dict(sam=True)),
    ("a_Y", ["-a", "-Y"], dict(sam=True, extra_flags=F_SOFTCLIP)),
    ("a_secseq", ["-a", "--secondary-seq"], dict(sam=True, extra_flags=F_SECONDARY_SEQ)),
    ("a_hitonly", ["-a", "--sam-hit-only"], dict(sam=True, extra_flags=F_SAM_HIT_ONLY)),
    ("a_MD", ["-a", "--MD"], dict(sam=True, extra_flags=F_OUT_MD)),
    ("c", ["-c"], dict(extra_flags=F_OUT_CG)),
    ("c_cs", ["-c", "--cs"], dict(extra_flags=F_OUT_CG | F_OUT_CS)),
    ("c_cslong", ["-c", "--cs=long"], dict(extra_flags=F_OUT_CG | F_OUT_CS | F_OUT_CS_LONG)),
    ("c_nohit", ["-c", "--paf-no-hit"], dict(extra_flags=F_OUT_CG | F_PAF_NO_HIT)),
    ("dv", [], dict(cigar=False)),
    ("no2nd", ["--secondary=no"], dict(cigar=False, extra_flags=F_NO_PRINT_2ND)),
    ("qstrand_c_cs", ["--qstrand", "-c", "--cs"], dict(extra_flags=F_QSTRAND | F_NO_INV | F_OUT_CG | F_OUT_CS)),
]


def mapped_inputs(outdir, seed=MAPPED_SEED):
    """a 1 Mb two-contig reference with one segment planted twice; 16 reads of ~6 kb: one reverse-complemented on purpose, one of random bases, one
    chimeric across the contigs, one from the planted segment; every second read with quality.  Returns (ref.fa, reads.fq, refs, names, reads)."""
    rng = np.random.default_rng(seed)
    contigs = synth.gen_reference(rng, 1000000, 2)
    contigs[1][300000:307000] = contigs[0][100000:107000]  # the segment planted twice
    base = synth.gen_reads(rng, contigs, 12, 6000, 800, 0.08)
    rc = lambda a: (3 - a)[::-1]
    reads = [r for r in base]
    reads[1] = rc(synth.mutate_read(rng, contigs[0][400000:406000], 0.08))
    reads.append(rng.integers(0, 4, 5000, dtype=np.uint8))                                                           # random bases
    reads.append(np.concatenate([synth.mutate_read(rng, contigs[0][200000:203500], 0.05), rc(synth.mutate_read(rng, contigs[1][50000:53000], 0.05))]))  # chimeric
    reads.append(synth.mutate_read(rng, contigs[0][100500:106500], 0.05))                                            # from the planted segment
    reads.append(synth.mutate_read(rng, contigs[1][299000:305000], 0.05))
    refs = [synth.ACGT[c].tobytes() for c in contigs]
    names = ["chr1", "chr2"]
    rds = []
    for i, r in enumerate(reads):
        s = synth.ACGT[r].tobytes()
        rds.append((b"read%d" % i, s, bytes(35 + (k * 11 + i) % 38 for k in range(len(s))) if i % 2 == 0 else None))
    ref_fa, reads_fq = os.path.join(outdir, "ref.fa"), os.path.join(outdir, "reads.fq")
    synth.write_fasta(ref_fa, names, contigs)
    with open(reads_fq, "wb") as f:  # (quality for all in the file: a FASTQ record needs it; reads without one get '*' through their own file)
        for nm, s, q in rds:
            if q is not None:
                f.write(b"@" + nm + b"\n" + s + b"\n+\n" + q + b"\n")
            else:
                f.write(b">" + nm + b"\n" + s + b"\n")
    return ref_fa, reads_fq, refs, names, rds


def binary_text(ref_fa, reads_fq, opts, preset="map-ont"):
    out = subprocess.run([reflib.REF_BIN, "-x", preset, "-t", "2"] + opts + [ref_fa, reads_fq], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, check=True).stdout
    return b"".join(ln + b"\n" for ln in out.split(b"\n") if ln and not ln.startswith(b"@"))


def batch_with_quality(mm, rds):
    b = mm.Batch([(nm, s) for nm, s, _ in rds])
    b._qual = [q for _, _, q in rds]  # (kept alive with the batch)
    for k, q in enumerate(b._qual):
        b.arr[k].qual = q
    return b


def device_text(mm, al, batch):
    """(text, path, the host writer's text) of one mapped batch"""
    al.stage(batch)
    n_reg, reg, rep_len = al.run(raw=True)
    try:
        dev = al.format_raw(n_reg, reg, rep_len, device=True)
        return dev, al.last_format_path, al.format_raw(n_reg, reg, rep_len)
    finally:
        al.free_raw(n_reg, reg)
