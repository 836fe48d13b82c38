"""Shared by tests/test_gpu_aln_text.py and tests/test_aln_text_emu.py (not a test): jobs for aln_text_kernel and the oracle they are judged
by -- the UNMODIFIED compiled reference (oracle/_ref/libminimap2_ref.so) through ctypes: mm_idx_str with one contig per job, a hand-built
mm_reg1_t + mm_extra_t, mm_gen_cs_ds_or_MD (format.c:364-375).  The reference has no exported function for the CIGAR string; that text is
"<len><op>" per operation (write_sam_cigar)."""
import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import reflib  # noqa: E402

HAVE_REF = os.path.exists(reflib.REF_SO)
LETTERS = np.frombuffer(b"ACGTN", dtype=np.uint8)
COMP5 = np.array([3, 2, 1, 0, 4], dtype=np.uint8)
OPS = "MIDNSHP=XB"
CS, CS_LONG, MD = 1, 2, 3  # minimap2_amd.TXT_*
MODES = (CS, CS_LONG, MD)
STEP, TILE = 64, 256       # columns a wave walks per step; operations staged in LDS at a time (aln_text.hpp)
OP_COUNTS = (1, 2, 3, 8, 40, 63, 64, 65, 150, 255, 256, 257, 1500)


def cigar_text(cig):
    return "".join("%d%s" % (w >> 4, OPS[w & 15]) for w in cig)


def parse_cigar(s):
    out, n = [], 0
    for ch in s:
        if ch.isdigit():
            n = n * 10 + int(ch)
        else:
            out.append(n << 4 | OPS.index(ch))
            n = 0
    return out


def codes(s):
    return bytes(b"ACGTN".index(c) for c in s.upper().encode())


def job(q, t, cigar):
    """a job from letters and a CIGAR string"""
    return (codes(q), codes(t), parse_cigar(cigar))


# ---------------------------------------------------------------------------------------------------------
# the oracle
# ---------------------------------------------------------------------------------------------------------
def make_reg(mm, rid, rs, re, qs, qe, rev, cig):
    """(mm_reg1_t, the buffer that holds its mm_extra_t) -- keep both alive; cig None: a hit without base-level alignment"""
    r = mm.Reg1()
    r.rid, r.rs, r.re, r.qs, r.qe, r.bits = rid, rs, re, qs, qe, (1 << 10) if rev else 0
    if cig is None:
        return r, None
    n = len(cig)
    buf = C.create_string_buffer(C.sizeof(mm.Extra) + 4 * max(n, 1))
    ex = mm.Extra.from_buffer(buf)
    ex.capacity, ex.n_cigar = (C.sizeof(mm.Extra) + 4 * n + 15) // 16 * 4, n
    if n:
        (C.c_uint32 * n).from_buffer(buf, C.sizeof(mm.Extra))[:] = cig
    r.p = C.cast(buf, C.POINTER(mm.Extra))
    return r, buf


class RefText(object):
    """mm_gen_cs_ds_or_MD of the compiled reference over an index of the given contigs (letters)"""

    def __init__(self, contigs, names=None, lib=None):
        import minimap2_amd as mm
        self.mm = mm
        R = self.R = lib or C.CDLL(reflib.REF_SO)
        R.mm_idx_str.restype = C.c_void_p
        R.mm_idx_str.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_char_p)]
        R.mm_idx_destroy.argtypes = [C.c_void_p]
        R.mm_gen_cs_ds_or_MD.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.c_void_p, C.c_void_p, C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int]
        n = len(contigs)
        nm = [(x.encode() if isinstance(x, str) else x) for x in (names or ["c%d" % i for i in range(n)])]
        self._keep = (list(contigs), nm)
        self.mi = R.mm_idx_str(10, 15, 0, 14, n, (C.c_char_p * n)(*contigs), (C.c_char_p * n)(*nm))
        assert self.mi
        self.buf, self.cap = C.c_void_p(), C.c_int(0)

    def text(self, reg, read, mode, is_qstrand=0):
        is_md, no_iden = (1, 0) if mode == MD else (0, 1 if mode == CS else 0)
        n = self.R.mm_gen_cs_ds_or_MD(None, C.byref(self.buf), C.byref(self.cap), self.mi, C.byref(reg), read, is_md, 0, no_iden, is_qstrand)
        return C.string_at(self.buf, n).decode("ascii") if n else ""

    def close(self):
        if self.mi:
            self.R.mm_idx_destroy(self.mi)
            self.mi = None
            if self.buf:
                reflib._libc.free(self.buf)


def ref_texts(jobs):
    """{mode: [text per job]} -- every job as a hit that covers its own contig and its own read"""
    import minimap2_amd as mm
    R = RefText([LETTERS[np.frombuffer(t, dtype=np.uint8)].tobytes() for _, t, _ in jobs])
    out = {m: [] for m in MODES}
    for i, (q, t, cig) in enumerate(jobs):
        read = LETTERS[np.frombuffer(q, dtype=np.uint8)].tobytes()
        r, keep = make_reg(mm, i, 0, len(t), 0, len(q), 0, cig)
        for m in MODES:
            out[m].append(R.text(r, read, m))
    R.close()
    return out


# ---------------------------------------------------------------------------------------------------------
# jobs
# ---------------------------------------------------------------------------------------------------------
def build_job(rng, ops, mis=0.1, p_n=0.0):
    """sequences for a list of (op, len): the target random, the query a copy with `mis` of the aligned bases changed; N codes at p_n in both"""
    tlen = sum(l for o, l in ops if o in (0, 2, 3, 7, 8))
    t = rng.integers(0, 4, tlen, dtype=np.uint8)
    if p_n > 0 and tlen:
        t[rng.random(tlen) < p_n] = 4
    q, tp = [], 0
    for o, l in ops:
        if o in (0, 7, 8):
            seg = t[tp:tp + l].copy()
            if mis > 0:
                mut = rng.random(l) < mis
                seg[mut] = rng.integers(0, 5 if p_n > 0 else 4, int(mut.sum()), dtype=np.uint8)
            q.append(seg)
            tp += l
        elif o == 1:
            q.append(rng.integers(0, 5 if p_n > 0 else 4, l, dtype=np.uint8))
        else:
            tp += l
    q = np.concatenate(q) if q else np.zeros(0, dtype=np.uint8)
    return (q.tobytes(), t.tobytes(), [l << 4 | o for o, l in ops])


def random_job(rng, n_ops, mis, p_n, intron=None):
    ops = []
    for k in range(n_ops):
        u = rng.random()
        if k == 0 or u < 0.5:
            ops.append((int(rng.choice([0, 0, 0, 7, 8])), int(rng.integers(1, 40)) if rng.random() < 0.9 else int(rng.integers(60, 400))))
        elif u < 0.7:
            ops.append((1, int(rng.integers(1, 9))))
        elif u < 0.9:
            ops.append((2, int(rng.integers(1, 9))))
        else:
            ops.append((3, int(rng.integers(2, 301))))
    if intron:
        ops.insert(len(ops) // 2 + 1, (3, intron))
        ops.append((0, 5))
    return build_job(rng, ops, mis, p_n)


def random_jobs(rng, n):
    jobs = []
    for i in range(n):
        jobs.append(random_job(rng, int(OP_COUNTS[i % len(OP_COUNTS)]) if i < 2 * len(OP_COUNTS) else int(rng.choice(OP_COUNTS[:-1])),
                               float(rng.choice([0.0, 0.1, 0.5])), float(rng.choice([0.0, 0.0, 0.05])), 200000 if i == 5 else None))
    return jobs


def with_mismatches(n, at, rng):
    """nM over random bases, mismatches exactly at the columns `at`"""
    t = rng.integers(0, 4, n, dtype=np.uint8)
    q = t.copy()
    for c in at:
        q[c] = (q[c] + 1) % 4
    return (q.tobytes(), t.tobytes(), [n << 4])


FIXED = [  # (q, t, CIGAR, cs, cs-long, MD)
    ("NNA", "NNC", "3M", ":2*ca", "=NN*ca", "2C"),
    ("A", "CGA", "2D1M", "-cg:1", "-cg=A", "0^CG1"),
    ("CA", "A", "1I1M", "+c:1", "+c=A", "1"),
    ("AA", "AGTA", "1M2N1M", ":1~gt2gt:1", "=A~gt2gt=A", "2"),
]


def directed_jobs(rng):
    J = [job(q, t, c) for q, t, c, _, _, _ in FIXED]
    for n in (63, 64, 65, 127, 128, 129):  # total columns around the step size
        J.append(with_mismatches(n, [], rng))
        J.append(with_mismatches(n, [n // 2], rng))
    J.append(with_mismatches(230, [10, 211], rng))  # an identity run of 200 over three steps
    for r in (9, 10, 99, 100, 999, 1000, 9999, 10000):  # digit counts: a run of r, a mismatch, a trailing run of r
        J.append(with_mismatches(2 * r + 1, [r], rng))
    J.append(with_mismatches(130, [0, 63, 64, 129], rng))  # first column, lane 63, lane 0 of the next step, last column
    J.append(with_mismatches(64, [63], rng))
    J.append(with_mismatches(65, [64], rng))
    same = lambda ops: build_job(rng, ops, 0.0)
    J.append(same([(0, 64), (0, 64)]))                       # operation boundaries on step boundaries
    J.append(same([(0, 32), (1, 32), (0, 64), (2, 64), (0, 1)]))
    J.append(same([(7, 64), (8, 64), (7, 128)]))
    J.append(same([(0, 1000), (7, 234)]))                    # cs flushes per operation (":1000:234"), MD does not ("1234")
    J.append(build_job(rng, [(7, 5), (8, 1), (7, 7), (8, 2), (7, 64), (8, 1), (7, 3)], 0.3))  # = / X alternation
    J.append(same([(0, 10), (1, 3), (0, 10)]))               # MD across I, across N, across M|M
    J.append(same([(0, 10), (3, 50), (0, 10)]))
    J.append(same([(0, 10), (0, 10), (7, 10)]))
    t = rng.integers(0, 4, 12, dtype=np.uint8)               # a mismatch right after a deletion: MD counts 0
    q = np.concatenate([t[:5], [(t[7] + 1) % 4], t[8:]]).astype(np.uint8)
    J.append((q.tobytes(), t.tobytes(), parse_cigar("5M2D5M")))
    J.append(same([(2, 2), (0, 5)]))                         # a leading deletion, a leading insertion, gaps only
    J.append(same([(1, 3), (0, 5)]))
    J.append(same([(2, 3), (2, 2), (1, 2), (1, 1), (0, 1)])) # neighbours of one kind: every operation opens its own "-" / "+"
    J.append(same([(3, 2), (0, 1)]))                         # an intron of 2: the two base pairs overlap
    J.append(same([(0, 3), (3, 3), (0, 3)]))
    J.append(build_job(rng, [(0, 40), (3, 200000), (0, 40)], 0.1))
    J.append(build_job(rng, [(0, 300)], 0.2, 0.3))           # N against N
    return J


def profile(jobs, texts):
    """how many jobs reach the paths the tests are for"""
    n_cross = n_tiles = n_nn = 0
    for (q, t, cig), md in zip(jobs, texts[MD]):
        qa, ta = np.frombuffer(q, dtype=np.uint8), np.frombuffer(t, dtype=np.uint8)
        n_tiles += len(cig) > TILE
        qp = tp = col = 0
        cross = nn = False
        for w in cig:
            o, l = w & 15, w >> 4
            if o in (0, 7, 8):
                eq = qa[qp:qp + l] == ta[tp:tp + l]
                nn |= bool(np.any(eq & (qa[qp:qp + l] == 4)))
                if len(cig) <= TILE:  # (the steps of the first tile start at column 0)
                    for b in range((col // STEP + 1) * STEP, col + l, STEP):
                        cross |= bool(eq[b - 1 - col] and eq[b - col])
                qp, tp, col = qp + l, tp + l, col + l
            elif o == 1:
                qp, col = qp + l, col + l
            elif o == 2:
                tp, col = tp + l, col + l
            else:
                tp, col = tp + l, col + 1
        n_cross += cross
        n_nn += nn
    return n_cross, n_tiles, n_nn


# ---------------------------------------------------------------------------------------------------------
# the cases both suites run (mm: the package bound to the library under test)
# ---------------------------------------------------------------------------------------------------------
def check_jobs(mm, jobs, want):
    for m in MODES:
        got = mm.aln_text_batch(jobs, m)
        for i, (g, w) in enumerate(zip(got, want[m])):
            assert g == w, "mode %d, job %d (%d operations): %r != %r" % (m, i, len(jobs[i][2]), g and g[:200], w[:200])


def check_directed(mm):
    jobs = directed_jobs(np.random.default_rng(5))
    want = ref_texts(jobs)
    for i, (_, _, _, cs, csl, md) in enumerate(FIXED):
        assert (want[CS][i], want[CS_LONG][i], want[MD][i]) == (cs, csl, md)
    k = [cigar_text(c) for _, _, c in jobs].index("1000M234=")
    assert (want[CS][k], want[MD][k]) == (":1000:234", "1234")
    check_jobs(mm, jobs, want)
    n_cross, _, n_nn = profile(jobs, want)
    assert n_cross >= 10 and n_nn >= 2


def check_cigar_mode(mm, rng, n_jobs):
    lens = [1, 9, 10, 999, 1000, 65535, (1 << 28) - 1]
    jobs = []
    for i in range(n_jobs):
        n = int(OP_COUNTS[i % len(OP_COUNTS)])
        cig = [(int(rng.choice(lens)) if rng.random() < 0.5 else int(rng.integers(1, 1 << 28))) << 4 | int(rng.integers(0, 10)) for _ in range(n)]
        jobs.append((None, None, cig))
    jobs.append((None, None, [l << 4 | o for o in range(10) for l in lens]))
    got = mm.aln_text_batch(jobs, mm.TXT_CIGAR)
    for (_, _, cig), g in zip(jobs, got):
        assert g == cigar_text(cig)


def check_bookkeeping(mm):
    """valid jobs, an empty job and invalid jobs in one batch: status -1 and no text for the invalid ones, the neighbours' text exact, offsets contiguous"""
    rng = np.random.default_rng(9)
    good = [random_job(rng, n, 0.1, 0.0) for n in (3, 70, 300, 8)]
    want = ref_texts(good)
    a = rng.integers(0, 4, 10, dtype=np.uint8).tobytes()
    empty = (b"", b"", [])
    bad = [(a, a, parse_cigar("5M5S")),            # an operation cs / MD do not know
           (a, a, parse_cigar("5M0I5M")),          # an empty operation
           (a, a + b"\0", parse_cigar("5M1N5M")),  # an intron shorter than 2
           (a, a[:9], parse_cigar("9M")),          # the query is covered one base short ...
           (a[:9], a, parse_cigar("9M")),          # ... the target ...
           (a, a, parse_cigar("9M")),              # ... both
           (a, a, parse_cigar("11M"))]             # one base too many (nothing beyond the sequences may be read)
    jobs = [good[0], bad[0], good[1], empty, bad[1], bad[2], good[2], bad[3], bad[4], bad[5], bad[6], good[3]]
    is_good = [0, None, 1, "empty", None, None, 2, None, None, None, None, 3]
    for m in MODES:
        n = len(jobs)
        arr, keep = _job_array(mm, jobs)
        res = (mm.TxtRes * n)()
        assert mm.lib().mm2amd_aln_text_batch(n, arr, m, res, None, 0) == 0
        total = sum(r.len for r in res)
        pool = C.create_string_buffer(total + 64)
        pool.raw = b"\xa5" * (total + 64)
        res2 = (mm.TxtRes * n)()
        assert mm.lib().mm2amd_aln_text_batch(n, arr, m, res2, pool, total) == 0, mm.lib().mm2amd_last_error()
        assert [(r.off, r.len, r.status) for r in res] == [(r.off, r.len, r.status) for r in res2]  # the sizing call equals the real one
        raw, off = pool.raw, 0
        assert raw[total:] == b"\xa5" * 64  # nothing beyond the pool's capacity
        for r, g in zip(res2, is_good):
            assert r.off == off
            if g is None:
                assert (r.len, r.status) == (0, -1)
            elif g == "empty":
                assert (r.len, r.status) == (0, 0)
            else:
                assert r.status == 0 and raw[off:off + r.len].decode() == want[m][g]
            off += r.len
        assert off == total
        # one byte short: MM2AMD_ENOMEM, the lengths are there, the pool is untouched
        pool.raw = b"\xa5" * (total + 64)
        res3 = (mm.TxtRes * n)()
        assert mm.lib().mm2amd_aln_text_batch(n, arr, m, res3, pool, total - 1) == mm.ENOMEM
        assert [(r.len, r.status) for r in res3] == [(r.len, r.status) for r in res2] and pool.raw == b"\xa5" * (total + 64)
    # CIGAR mode refuses only an operation above 9
    got = mm.aln_text_batch([(None, None, parse_cigar("3M2S")), (None, None, [5 << 4 | 10]), (None, None, []), (None, None, [7 << 4 | 9, 0 << 4 | 1])], mm.TXT_CIGAR)
    assert got == ["3M2S", None, "", "7B0I"]


def _job_array(mm, jobs):
    arr, keep = (mm.TxtJob * len(jobs))(), []
    for i, (q, t, cig) in enumerate(jobs):
        ca = (C.c_uint32 * max(len(cig), 1))(*cig)
        keep.append((q, t, ca))
        arr[i].query, arr[i].target = C.cast(C.c_char_p(q), C.c_void_p), C.cast(C.c_char_p(t), C.c_void_p)
        arr[i].qlen, arr[i].tlen, arr[i].cigar, arr[i].n_cigar = len(q), len(t), ca, len(cig)
    return arr, keep


def revcomp_codes(a):
    return COMP5[a[::-1]]


def check_hits(mm):
    """hand-built hits on an index of contigs of odd lengths with N in them: every rs % 8, rid > 0, both strands x is_qstrand, qs > 0 and
    qe < qlen, reads with lower-case letters and N; the library and the reference get the same record, read and flags"""
    rng = np.random.default_rng(21)
    lens = [1001, 777, 1503, 2049, 333, 905]
    contigs = [rng.integers(0, 4, n, dtype=np.uint8) for n in lens]
    for c in contigs:
        c[rng.random(len(c)) < 0.02] = 4
    cases = []  # (rid, rs, re, qs, qe, rev, is_qstrand, cig, read)
    k = 0
    for rev in (0, 1):
        for qst in (0, 1):
            for r8 in range(8):
                rid = 1 + k % 5
                jb = random_job(rng, int(rng.choice([1, 5, 30, 70])), 0.1, 0.05)
                while len(jb[1]) + 16 > lens[rid]:
                    jb = random_job(rng, 5, 0.1, 0.05)
                q, t = np.frombuffer(jb[0], dtype=np.uint8), np.frombuffer(jb[1], dtype=np.uint8)
                rs = int(rng.integers(0, (lens[rid] - len(t) - 8) // 8 + 1)) * 8 + r8
                re = rs + len(t)
                if qst and rev:  # mm_idx_getseq2's window [rs, re) of the reverse strand
                    contigs[rid][lens[rid] - re:lens[rid] - rs] = revcomp_codes(t)
                else:
                    contigs[rid][rs:re] = t
                qs, tail = int(rng.integers(1, 20)), int(rng.integers(1, 20))
                mid = revcomp_codes(q) if (rev and not qst) else q
                read = bytearray(LETTERS[np.concatenate([rng.integers(0, 4, qs, dtype=np.uint8), mid, rng.integers(0, 4, tail, dtype=np.uint8)])].tobytes())
                for p in np.flatnonzero(rng.random(len(read)) < 0.3):
                    read[p] = ord(chr(read[p]).lower())
                cases.append((rid, rs, re, qs, qs + len(q), rev, qst, jb[2], bytes(read)))
                k += 1
    # (later cases may have overwritten the stretch of an earlier one on the same contig: the text only needs consistent lengths)
    ctg = [LETTERS[c].tobytes() for c in contigs]
    names = ["c%d" % i for i in range(len(ctg))]
    R = RefText(ctg, names)
    L = mm.lib()
    h = L.mm2amd_idx_str(10, 15, 0, 14, len(ctg), (C.c_char_p * len(ctg))(*ctg), (C.c_char_p * len(ctg))(*[n.encode() for n in names]))
    assert h, L.mm2amd_last_error()
    try:
        n_ident = 0
        for qst in (0, 1):
            sel = [c for c in cases if c[6] == qst]
            regs = [make_reg(mm, c[0], c[1], c[2], c[3], c[4], c[5], c[7]) for c in sel]
            regs.append(make_reg(mm, 2, 10, 50, 3, 40, 0, None))  # no base-level alignment
            reads = [c[8] for c in sel] + [b"ACGT" * 20]
            for m in MODES:
                got = mm.hits_text(h, [C.addressof(r) for r, _ in regs], reads, m, is_qstrand=bool(qst))
                want = [R.text(r, rd, m, qst) for (r, _), rd in zip(regs, reads)]
                assert got == want
                assert got[-1] == ""
                n_ident += sum(":" in g for g in got) if m == CS else 0
        assert n_ident >= 24  # the stretches were planted where the records point: identity runs, not noise
        got = mm.hits_text(h, [C.addressof(regs[0][0])], [reads[0]], mm.TXT_CIGAR)
        assert got == [cigar_text(sel[0][7])]
        # MM2AMD_EINVAL: rid / rs / re outside the sequence, qs / qe outside the read, an index without sequence
        c = sel[0]
        for bad in (dict(rid=len(ctg)), dict(rid=-1), dict(re=lens[c[0]] + 1), dict(rs=-1), dict(rs=c[2] + 1), dict(qe=len(c[8]) + 1), dict(qs=-1), dict(qs=c[4] + 1)):
            r, keep = make_reg(mm, c[0], c[1], c[2], c[3], c[4], c[5], c[7])
            for f, v in bad.items():
                setattr(r, f, v)
            res = (mm.TxtRes * 1)()
            rc = L.mm2amd_hits_text_batch(h, 1, (C.c_void_p * 1)(C.addressof(r)), (C.c_char_p * 1)(c[8]), (C.c_int32 * 1)(len(c[8])), MD, 0, res, None, 0)
            assert rc == mm.EINVAL, bad
        # mm2amd_idx_getseq (mm_idx_getseq, index.c:164-174)
        buf = C.create_string_buffer(3000)
        for rid, st, en in ((0, 0, lens[0]), (1, 5, 13), (3, 2040, 2049), (4, 333, 333), (5, 7, 8)):
            assert L.mm2amd_idx_getseq(h, rid, st, en, buf) == en - st
            assert buf.raw[:en - st] == contigs[rid][st:en].tobytes()
        for rid, st, en in ((6, 0, 1), (0, 5, 4), (0, 0, lens[0] + 1)):
            assert L.mm2amd_idx_getseq(h, rid, st, en, buf) == mm.EINVAL
    finally:
        L.mm2amd_idx_destroy(h)
        R.close()
    return ctg, names
