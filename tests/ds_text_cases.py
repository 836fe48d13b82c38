"""Shared by tests/test_gpu_ds_text.py and tests/test_ds_text_emu.py (not a test): jobs for the ds modes of aln_text_kernel and the oracle they
are judged by -- the UNMODIFIED compiled reference's mm_gen_cs_ds_or_MD with is_ds = 1 (format.c:364-375; write_cs_ds_core and write_indel_ds,
format.c:142-254), reached through the binding of tests/aln_text_cases.py.  The comparison is string equality everywhere."""
import ctypes as C
import os
import re
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import aln_text_cases as X  # noqa: E402
from aln_text_cases import RefText, build_job, job, make_reg, random_jobs  # noqa: E402,F401

HAVE_REF = X.HAVE_REF
DS, DS_LONG = 4, 5  # minimap2_amd.TXT_DS, TXT_DS_LONG
FORMS = (DS, DS_LONG)
LANE_SCAN = 6       # kTxtDsLaneScan (aln_text.hpp): an indel up to this long is scanned by one lane, a longer one by the wave

PINNED = [  # (q, t, CIGAR, ds in the short form): checked against the reference, so that the oracle itself is pinned
    ("ACAAAAGT", "ACAAAGT", "2M1I5M", ":2+[a]:5"),
    ("ACAAAGT", "ACAAAAGT", "2M1D5M", ":2-[a]:5"),
    ("GGCACACATT", "GGCACATT", "4M2I4M", ":4+[ca]:4"),
    ("GGCATCATT", "GGCATT", "3M3I3M", ":3+[atc]:3"),
    ("TTACGTT", "TTTT", "2M3I2M", ":2+acg:2"),
    ("ACGTTTGA", "ACGTGA", "4M2I2M", ":4+t[t]:2"),
    ("GATTACAGATTTT", "GATTTT", "3M7I3M", ":3+[t]aca[gat]:3"),
    ("AAAAAA", "AAA", "1M3I2M", ":1+[aaa]:2"),
    ("AANNAA", "AANAA", "2M1I3M", ":2+[n]:3"),
    ("CA", "A", "1I1M", "+c:1"),
    ("AC", "A", "1M1I", ":1+c"),
    ("A", "CGA", "2D1M", "-cg:1"),
    ("AA", "AGTA", "1M2N1M", ":1~gt2gt:1"),
]
PINNED_LONG = (6, "=GAT+[t]aca[gat]=TTT")  # the 3M7I3M row in the long form


# ---------------------------------------------------------------------------------------------------------
# the oracle
# ---------------------------------------------------------------------------------------------------------
def ds_text(R, reg, read, long, is_qstrand=0):
    """mm_gen_cs_ds_or_MD(is_MD = 0, is_ds = 1, no_iden = !long) of the RefText R for one record"""
    n = R.R.mm_gen_cs_ds_or_MD(None, C.byref(R.buf), C.byref(R.cap), R.mi, C.byref(reg), read, 0, 1, 0 if long else 1, is_qstrand)
    return C.string_at(R.buf, n).decode("ascii") if n else ""


def ref_ds(jobs, long):
    """[text per job] -- every job as a hit that covers its own contig and its own read"""
    import minimap2_amd as mm
    R = RefText([X.LETTERS[np.frombuffer(t, dtype=np.uint8)].tobytes() for _, t, _ in jobs])
    out = []
    for i, (q, t, cig) in enumerate(jobs):
        read = X.LETTERS[np.frombuffer(q, dtype=np.uint8)].tobytes()
        r, keep = make_reg(mm, i, 0, len(t), 0, len(q), 0, cig)
        out.append(ds_text(R, r, read, long))
    R.close()
    return out


def ref_both(jobs):
    return {DS: ref_ds(jobs, False), DS_LONG: ref_ds(jobs, True)}


_TWO = re.compile(r"[+-]\[[a-z]+\][a-z]+\[[a-z]+\]")


def profile(texts):
    """(indels, brackets, indels with two brackets and a plain middle, jobs with a bracket) of a list of ds texts"""
    return (sum(s.count("+") + s.count("-") for s in texts), sum(s.count("[") for s in texts),
            sum(len(_TWO.findall(s)) for s in texts), sum("[" in s for s in texts))


# ---------------------------------------------------------------------------------------------------------
# jobs
# ---------------------------------------------------------------------------------------------------------
def _arr(x):
    return np.asarray(x, dtype=np.uint8)


def spliced(flank_l, gap, flank_r, ins):
    """a job whose only gap is `gap` between the two flanks: an insertion (the query holds it) or a deletion (the target does)"""
    a, b = np.concatenate([flank_l, gap, flank_r]).astype(np.uint8), np.concatenate([flank_l, flank_r]).astype(np.uint8)
    cig = [len(flank_l) << 4, len(gap) << 4 | (1 if ins else 2), len(flank_r) << 4]
    cig = [w for w in cig if w >> 4]
    return (a.tobytes(), b.tobytes(), cig) if ins else (b.tobytes(), a.tobytes(), cig)


def low_job(rng, ops, n_letters=2):
    """build_job over an alphabet of n_letters: shifts and brackets everywhere"""
    tlen = sum(l for o, l in ops if o in (0, 2, 3, 7, 8))
    t = rng.integers(0, n_letters, tlen, dtype=np.uint8)
    q, tp = [], 0
    for o, l in ops:
        if o in (0, 7, 8):
            seg = t[tp:tp + l].copy()
            mut = rng.random(l) < 0.05
            seg[mut] = rng.integers(0, n_letters, int(mut.sum()), dtype=np.uint8)
            q.append(seg)
            tp += l
        elif o == 1:
            q.append(rng.integers(0, n_letters, l, dtype=np.uint8))
        else:
            tp += l
    q = np.concatenate(q) if q else np.zeros(0, dtype=np.uint8)
    return (q.tobytes(), t.tobytes(), [l << 4 | o for o, l in ops])


def directed_jobs(rng):
    J = [job(q, t, c) for q, t, c, _ in PINNED]
    hp = lambda n: np.zeros(n, dtype=np.uint8)
    for ins in (True, False):
        # a homopolymer: every comparison succeeds, the scans end at the operation's length or at the alignment's two ends
        J.append(spliced(hp(100), hp(1), hp(199), ins))
        J.append(spliced(hp(100), hp(50), hp(150), ins))
        J.append(spliced(hp(0), hp(200), hp(100), ins))   # leading: nothing to the left, the right scan stops at the alignment's end
        J.append(spliced(hp(100), hp(200), hp(0), ins))   # trailing: the left scan stops at the alignment's start
        J.append(spliced(hp(3), hp(LANE_SCAN), hp(2), ins))  # one lane, stopped by both ends
        # a period-3 tandem repeat of 600 with an in-phase copy in the middle: ll + lr >= len for len below, at, just above and far above
        # the per-lane threshold, and above 64
        unit = _arr([0, 1, 2] * 200)
        for n in (3, LANE_SCAN, LANE_SCAN + 3, 63, 64, 66, 200, 201):
            J.append(spliced(unit[:300], _arr(([0, 1, 2] * 67)[:n]), unit[300:], ins))
        # 200 bases into random sequence; the first 70 copy the right flank and the last 5 the left: ll = 70, lr = 5, the middle plain
        for n_l, n_r, n in ((70, 5, 200), (5, 70, 200), (64, 64, 129), (63, 1, 65), (2, 3, LANE_SCAN + 1), (2, 3, LANE_SCAN)):
            left, right, gap = rng.integers(0, 4, 150, dtype=np.uint8), rng.integers(0, 4, 150, dtype=np.uint8), rng.integers(0, 4, n, dtype=np.uint8)
            gap[:n_l], gap[n_l] = right[:n_l], (right[n_l] + 1) % 4
            gap[n - n_r:], gap[n - n_r - 1] = left[150 - n_r:], (left[150 - n_r - 1] + 1) % 4
            J.append(spliced(left, gap, right, ins))
    for g in (1, 2):  # the indel's first column on lane 63 and on lane 0 of a step
        for m in (63, 64):
            for n in (2, 10, 70):
                J.append(low_job(rng, [(0, m), (g, n), (0, 64)]))
    for first in (1, 2):  # the last operation of a 256-operation tile and the first of the next, short and long
        for n in (3, 40):
            ops = [(0, 3) if k % 2 == 0 else (1 + (k // 2) % 2, 1 + k % 3) for k in range(255)] + [(first, n), (3 - first, n), (0, 4)]
            J.append(low_job(rng, ops))
    for n_letters in (1, 2, 4):
        lo = lambda ops: low_job(rng, ops, n_letters)
        J.append(lo([(0, 5), (1, 2), (1, 3), (2, 2), (2, 1), (0, 5)]))       # neighbours: each operation scans the sequence, not the operation
        J.append(lo([(0, 5), (1, 9), (1, 70), (2, 80), (2, 7), (0, 5)]))
        J.append(lo([(1, 3), (0, 5)]))                                       # leading and trailing, short and long
        J.append(lo([(2, 3), (0, 5)]))
        J.append(lo([(0, 5), (1, 3)]))
        J.append(lo([(0, 5), (2, 3)]))
        J.append(lo([(1, 30), (0, 5), (2, 30)]))
        J.append(lo([(2, 100), (0, 5), (1, 100)]))
        J.append(lo([(1, 3), (2, 4)]))                                       # gaps only
        J.append(lo([(2, 9), (1, 7)]))
        J.append(lo([(1, 2), (2, 70), (1, 80), (2, 1)]))
        J.append(lo([(0, 5), (1, 2), (3, 20), (2, 2), (0, 5)]))              # an indel next to an intron
        J.append(lo([(0, 5), (2, 8), (3, 2), (1, 8), (0, 5)]))
        J.append(lo([(7, 5), (1, 2), (8, 1), (2, 3), (7, 6), (8, 2), (1, 9), (7, 3)]))  # = / X around indels
    J.append(build_job(rng, [(0, 20), (1, 3), (0, 20), (2, 3), (0, 20), (1, 10), (0, 20)], 0.2, 0.6))  # N against N in the scans
    return J


def check_jobs(mm, jobs, want):
    for m in FORMS:
        got = mm.aln_text_batch(jobs, m)
        for i, (g, w) in enumerate(zip(got, want[m])):
            assert g == w, "mode %d, job %d (%s): %r != %r" % (m, i, X.cigar_text(jobs[i][2])[:60], g and g[:200], w[:200])


def check_directed(mm):
    jobs = directed_jobs(np.random.default_rng(5))
    want = ref_both(jobs)
    for i, (_, _, _, ds) in enumerate(PINNED):
        assert want[DS][i] == ds, (i, want[DS][i], ds)
    assert want[DS_LONG][PINNED_LONG[0]] == PINNED_LONG[1]
    # the built cases are what they are meant to be, on the reference's text alone
    cig = [X.cigar_text(c) for _, _, c in jobs]
    assert want[DS][cig.index("100M1I199M")] == ":100+[a]:199" and want[DS][cig.index("100M1D199M")] == ":100-[a]:199"
    assert want[DS][cig.index("200I100M")] == "+[" + "a" * 100 + "]" + "a" * 100 + ":100"
    assert want[DS][cig.index("100M200I")] == ":100+" + "a" * 100 + "[" + "a" * 100 + "]"
    for n in (3, LANE_SCAN, 200):
        assert want[DS][cig.index("300M%dI300M" % n)] == ":300+[" + ("acg" * 67)[:n] + "]:300"
    k = cig.index("150M200I150M")
    assert re.fullmatch(r":150\+\[[acgt]{70}\][acgt]{125}\[[acgt]{5}\]:150", want[DS][k]), want[DS][k]
    check_jobs(mm, jobs, want)


def check_bookkeeping(mm):
    """valid jobs, an empty job and invalid jobs in one batch, in the two ds modes: status -1 and no text for the invalid ones, the neighbours'
    text exact, the sizing call equal to the real one, offsets contiguous, the bytes behind the pool untouched, one byte short MM2AMD_ENOMEM"""
    rng = np.random.default_rng(9)
    good = [X.random_job(rng, n, 0.1, 0.0) for n in (3, 70, 300, 8)] + [low_job(rng, [(0, 9), (1, 2), (0, 9), (2, 90), (0, 9)])]
    want = ref_both(good)
    a = rng.integers(0, 4, 10, dtype=np.uint8).tobytes()
    empty = (b"", b"", [])
    P = X.parse_cigar
    bad = [(a, a, P("5M5S")),            # an operation ds does not know
           (a, a, P("5M0I5M")),          # an empty operation
           (a, a + b"\0", P("5M1N5M")),  # an intron shorter than 2
           (a, a[:8], P("3M1I5M")),      # the query is covered one base short ... (an indel whose scans would leave the sequences)
           (a[:8], a, P("3M1D5M")),      # ... the target ...
           (a, a, P("9M")),              # ... both
           (a, a, P("5M1I5M"))]          # one base too many
    jobs = [good[0], bad[0], good[1], empty, bad[1], bad[2], good[2], bad[3], bad[4], bad[5], bad[6], good[3], good[4]]
    is_good = [0, None, 1, "empty", None, None, 2, None, None, None, None, 3, 4]
    L = mm.lib()
    for m in FORMS:
        n = len(jobs)
        arr, keep = X._job_array(mm, jobs)
        res = (mm.TxtRes * n)()
        assert L.mm2amd_aln_text_batch(n, arr, m, res, None, 0) == 0, L.mm2amd_last_error()
        total = sum(r.len for r in res)
        pool = C.create_string_buffer(total + 64)
        pool.raw = b"\xa5" * (total + 64)
        res2 = (mm.TxtRes * n)()
        assert L.mm2amd_aln_text_batch(n, arr, m, res2, pool, total) == 0, L.mm2amd_last_error()
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
        pool.raw = b"\xa5" * (total + 64)
        res3 = (mm.TxtRes * n)()
        assert L.mm2amd_aln_text_batch(n, arr, m, res3, pool, total - 1) == mm.ENOMEM
        assert [(r.len, r.status) for r in res3] == [(r.len, r.status) for r in res2] and pool.raw == b"\xa5" * (total + 64)
    arr, keep = X._job_array(mm, good[:1])
    for what in (6, -1):
        assert L.mm2amd_aln_text_batch(1, arr, what, (mm.TxtRes * 1)(), None, 0) == mm.EINVAL


def check_hits(mm):
    """hand-built hits with TXT_DS on an index of contigs of odd lengths with N in them: every rs % 8, rid > 0, both strands x is_qstrand,
    qs > 0 and qe < qlen, reads with lower-case letters and N; and, per strand x is_qstrand, a hit that starts and ends with an insertion
    and one that starts and ends with a deletion, with the gap's bases repeated just outside [qs, qe) / [rs, re): a scan that left the hit
    would shift into them.  The library and the reference get the same record, read and flags."""
    rng = np.random.default_rng(23)
    lens = [1001, 777, 1503, 2049, 333, 905]
    contigs = [rng.integers(0, 4, n, dtype=np.uint8) for n in lens]
    for c in contigs:
        c[rng.random(len(c)) < 0.02] = 4
    cases = []  # (rid, rs, re, qs, qe, rev, is_qstrand, cig, read, planted)
    k = 0
    for rev in (0, 1):
        for qst in (0, 1):
            for r8 in range(8):
                rid = 1 + k % 5
                mk = (lambda n: low_job(rng, [(0, 9) if i % 2 == 0 else (1 + (i // 2) % 2, int(rng.choice([1, 2, 5, 9, 70]))) for i in range(n)] + [(0, 3)], 3)) \
                    if r8 % 2 else (lambda n: X.random_job(rng, n, 0.1, 0.05))
                jb = mk(int(rng.choice([1, 5, 30, 70])))
                while len(jb[1]) + 16 > lens[rid]:
                    jb = mk(5)
                q, t = np.frombuffer(jb[0], dtype=np.uint8), np.frombuffer(jb[1], dtype=np.uint8)
                rs = int(rng.integers(0, (lens[rid] - len(t) - 8) // 8 + 1)) * 8 + r8
                re_ = rs + len(t)
                if qst and rev:  # mm_idx_getseq2's window [rs, re) of the reverse strand
                    contigs[rid][lens[rid] - re_:lens[rid] - rs] = X.revcomp_codes(t)
                else:
                    contigs[rid][rs:re_] = t
                qs, tail = int(rng.integers(1, 20)), int(rng.integers(1, 20))
                mid = X.revcomp_codes(q) if (rev and not qst) else q
                read = bytearray(X.LETTERS[np.concatenate([rng.integers(0, 4, qs, dtype=np.uint8), mid, rng.integers(0, 4, tail, dtype=np.uint8)])].tobytes())
                for p in np.flatnonzero(rng.random(len(read)) < 0.3):
                    read[p] = ord(chr(read[p]).lower())
                cases.append((rid, rs, re_, qs, qs + len(q), rev, qst, jb[2], bytes(read), None))
                k += 1
    # (later cases may have overwritten the stretch of an earlier one on the same contig: the text only needs consistent lengths)
    G, PAD = 4, 11
    for rev in (0, 1):
        for qst in (0, 1):
            for op in (1, 2):  # the gapped sequence: the query for insertions, the target for deletions
                core = rng.integers(0, 4, 30, dtype=np.uint8)
                g0, g1 = rng.integers(0, 4, G, dtype=np.uint8), rng.integers(0, 4, G, dtype=np.uint8)
                core[0], core[-1] = (g0[0] + 1) % 4, (g1[-1] + 1) % 4      # inside the hit nothing shifts: the text has no bracket at either end
                gapped = np.concatenate([g0, core, g1]).astype(np.uint8)
                ext = np.concatenate([rng.integers(0, 4, PAD - G, dtype=np.uint8), g0, gapped, g1, rng.integers(0, 4, PAD - G, dtype=np.uint8)]).astype(np.uint8)
                cig = [G << 4 | op, 30 << 4, G << 4 | op]
                rid = len(contigs)
                if op == 1:
                    q_ext, t_ext = ext, np.concatenate([rng.integers(0, 4, PAD, dtype=np.uint8), core, rng.integers(0, 4, PAD, dtype=np.uint8)]).astype(np.uint8)
                else:
                    t_ext, q_ext = ext, np.concatenate([rng.integers(0, 4, PAD, dtype=np.uint8), core, rng.integers(0, 4, PAD, dtype=np.uint8)]).astype(np.uint8)
                # both extended sequences hold the hit at [PAD, len - PAD) in the walk's orientation
                contigs.append(X.revcomp_codes(t_ext) if (qst and rev) else t_ext)
                lens.append(len(t_ext))
                read = X.LETTERS[X.revcomp_codes(q_ext) if (rev and not qst) else q_ext].tobytes()
                cases.append((rid, PAD, len(t_ext) - PAD, PAD, len(q_ext) - PAD, rev, qst, cig, read, "+-"[op - 1]))
    ctg = [X.LETTERS[c].tobytes() for c in contigs]
    names = ["c%d" % i for i in range(len(ctg))]
    R = RefText(ctg, names)
    L = mm.lib()
    h = L.mm2amd_idx_str(10, 15, 0, 14, len(ctg), (C.c_char_p * len(ctg))(*ctg), (C.c_char_p * len(ctg))(*[n.encode() for n in names]))
    assert h, L.mm2amd_last_error()
    try:
        n_planted, n_br = 0, {}
        for qst in (0, 1):
            sel = [c for c in cases if c[6] == qst]
            regs = [make_reg(mm, c[0], c[1], c[2], c[3], c[4], c[5], c[7]) for c in sel]
            regs.append(make_reg(mm, 2, 10, 50, 3, 40, 0, None))  # no base-level alignment
            reads = [c[8] for c in sel] + [b"ACGT" * 20]
            for m in FORMS:
                got = mm.hits_text(h, [C.addressof(r) for r, _ in regs], reads, m, is_qstrand=bool(qst))
                want = [ds_text(R, r, rd, m == DS_LONG, qst) for (r, _), rd in zip(regs, reads)]
                for c, w in zip(sel, want):
                    if c[9] and m == DS:  # the reference itself stops at the hit: no bracket, although the bases outside would match
                        assert re.fullmatch(r"\%s[acgt]{%d}:30\%s[acgt]{%d}" % (c[9], G, c[9], G), w), w
                        n_planted += 1
                assert got == want
                assert got[-1] == ""
                for c, w in zip(sel, want):
                    n_br[(c[5], qst)] = n_br.get((c[5], qst), 0) + ("[" in w and m == DS)
        # the planted hits were all seen, and every strand x is_qstrand has hits whose text (the reference's) holds a bracket
        assert n_planted == 8 and len(n_br) == 4 and min(n_br.values()) >= 2, n_br
        c = cases[0]
        r, keep = make_reg(mm, c[0], c[1], c[2], c[3], c[4], c[5], c[7])
        for what in (6, -1):
            rc = L.mm2amd_hits_text_batch(h, 1, (C.c_void_p * 1)(C.addressof(r)), (C.c_char_p * 1)(c[8]), (C.c_int32 * 1)(len(c[8])), what, 0, (mm.TxtRes * 1)(), None, 0)
            assert rc == mm.EINVAL
    finally:
        L.mm2amd_idx_destroy(h)
        R.close()
