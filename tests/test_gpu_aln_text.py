"""aln_text_kernel on the device -- the CIGAR string, cs (short and long) and MD of a batch of alignments -- through its three boundaries:
mm2amd_aln_text_batch (jobs of codes), mm2amd_hits_text_batch (mm_reg1_t records against the index's packed sequence) and the Aligner's
cs= / MD= / seq().  The judge is the UNMODIFIED compiled reference's mm_gen_cs_ds_or_MD / mm_gen_cs / mm_gen_MD (format.c:364-395) and
mm_idx_getseq; tests/aln_text_cases.py holds the jobs and the oracle."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import aln_text_cases as X  # noqa: E402
import reflib  # noqa: E402
import synth  # noqa: E402

pytestmark = pytest.mark.gpu
EMU = os.environ.get("MM2AMD_EMU") == "1"
needs_ref = pytest.mark.skipif(not X.HAVE_REF, reason="oracle/_ref absent")


@pytest.fixture(scope="module")
def random_cases():
    """(jobs, the reference's texts): computed once for the three modes"""
    jobs = X.random_jobs(np.random.default_rng(31), 60 if EMU else 600)
    return jobs, X.ref_texts(jobs)


@needs_ref
@pytest.mark.parametrize("mode", X.MODES)
def test_random_jobs_equal_the_reference(random_cases, mode):
    import minimap2_amd as mm
    jobs, want = random_cases
    got = mm.aln_text_batch(jobs, mode)
    for i, (g, w) in enumerate(zip(got, want[mode])):
        assert g == w, "job %d (%d operations): %r != %r" % (i, len(jobs[i][2]), g and g[:200], w[:200])
    n_cross, n_tiles, n_nn = X.profile(jobs, want)
    assert n_cross >= len(jobs) // 10 and n_tiles >= 3 and n_nn >= len(jobs) // 10  # the paths this test is for were taken
    assert any(200000 << 4 | 3 in c for _, _, c in jobs)


@needs_ref
def test_directed_jobs_equal_the_reference():
    import minimap2_amd as mm
    X.check_directed(mm)


def test_cigar_strings():
    import minimap2_amd as mm
    X.check_cigar_mode(mm, np.random.default_rng(33), 26 if EMU else 200)


@needs_ref
def test_invalid_jobs_sizing_call_and_pool_bounds():
    import minimap2_amd as mm
    X.check_bookkeeping(mm)


@needs_ref
def test_hits_equal_the_reference():
    import minimap2_amd as mm
    X.check_hits(mm)


def _gen(R, mi, regs, j, seq, md):
    buf, cap = C.c_void_p(), C.c_int(0)
    n = R.mm_gen_MD(None, C.byref(buf), C.byref(cap), mi, C.byref(regs[j]), seq) if md else R.mm_gen_cs(None, C.byref(buf), C.byref(cap), mi, C.byref(regs[j]), seq, 1)
    s = C.string_at(buf, n).decode() if n else ""
    reflib._libc.free(buf)
    return s


def _bind_gen(R):
    R.mm_gen_cs.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.c_void_p, C.c_void_p, C.c_char_p, C.c_int]
    R.mm_gen_MD.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.c_void_p, C.c_void_p, C.c_char_p]


@needs_ref
def test_aligner_cs_and_md_equal_the_reference():
    """the reads of smoke(): hits are the reference's (existing parity); here their cs and MD"""
    import minimap2_amd as mm
    rng = np.random.default_rng(3)
    contigs = synth.gen_reference(rng, 1000000, 2)
    reads = synth.gen_reads(rng, contigs, 12, 6000, 1500, 0.12)
    refs = [synth.ACGT[c].tobytes() for c in contigs]
    rds = [("read%d" % i, synth.ACGT[r].tobytes()) for i, r in enumerate(reads)]
    al = mm.Aligner(refs, preset="map-ont", names=["chr1", "chr2"], n_threads=4)
    try:
        hits = al.map_batch(rds, cs=True, MD=True)
        plain = al.map_batch(rds[:2])
    finally:
        al.close()
    assert all(a.cs == "" and a.MD == "" for h in plain for a in h)
    m = reflib.RefMapper(refs, "map-ont", ["chr1", "chr2"])
    _bind_gen(m.R)
    strands = set()
    try:
        for (nm, seq), h in zip(rds, hits):
            n = C.c_int(0)
            regs = m.R.mm_map(m.mi, len(seq), seq, C.byref(n), m.tbuf, C.byref(m.mo), nm.encode())
            assert [a.key() for a in h] == [a.key() for a in mm._regs_to_alignments(n.value, regs, None, None)]
            for j, a in enumerate(h):
                assert a.cs == _gen(m.R, m.mi, regs, j, seq, False) and a.MD == _gen(m.R, m.mi, regs, j, seq, True)
                assert a.cs and a.MD
                strands.add(a.strand)
            for j in range(n.value):
                if regs[j].p:
                    reflib._libc.free(C.cast(regs[j].p, C.c_void_p))
            if regs:
                reflib._libc.free(C.cast(regs, C.c_void_p))
    finally:
        m.close()
    assert strands == {1, -1}


@needs_ref
def test_aligner_pairs_cs_and_md_equal_the_reference(tmp_path):
    import minimap2_amd as mm
    ref, f1, f2, _ = synth.make_pairs(str(tmp_path), n_pairs=8)
    rn, rs = mm.read_fastx(ref)
    n1, s1 = mm.read_fastx(f1)
    _, s2 = mm.read_fastx(f2)
    pairs = [(nm[:-2], a, b) for nm, a, b in zip(n1, s1, s2)][:8]
    al = mm.Aligner(rs, preset="sr", names=[x.decode() for x in rn], n_threads=4)
    try:
        got = al.map_pairs(pairs, cs=True, MD=True)
        one = al.map(pairs[0][1], pairs[0][2], cs=True)
    finally:
        al.close()
    assert [[a.cs for a in seg] for seg in one] == [[a.cs for a in seg] for seg in got[0]] and all(a.MD == "" for seg in one for a in seg)
    D = C.CDLL(reflib.REFDRV_SO)
    _bind_gen(D)
    io, mo = mm.IdxOpt(), mm.MapOpt()
    D.mm_set_opt(None, C.byref(io), C.byref(mo))
    assert D.mm_set_opt(b"sr", C.byref(io), C.byref(mo)) == 0
    mo.flag |= mm.F_CIGAR
    D.mm_idx_str.restype = C.c_void_p
    D.mm_idx_str.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_char_p)]
    mi = D.mm_idx_str(io.w, io.k, 0, 14, len(rs), (C.c_char_p * len(rs))(*rs), (C.c_char_p * len(rs))(*rn))
    D.mm_mapopt_update.argtypes = [C.c_void_p, C.c_void_p]
    D.mm_mapopt_update(C.byref(mo), mi)
    n = len(pairs)
    D.refdrv_map_pairs.restype = C.c_double
    D.refdrv_map_pairs.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_int), C.POINTER(C.c_char_p), C.c_int,
                                   C.POINTER(C.c_int), C.POINTER(C.c_void_p)]
    flat = [s for p in pairs for s in p[1:]]
    nr, rg = (C.c_int * (2 * n))(), (C.c_void_p * (2 * n))()
    D.refdrv_map_pairs(mi, C.byref(mo), n, (C.c_char_p * (2 * n))(*flat), (C.c_int * (2 * n))(*[len(s) for s in flat]), (C.c_char_p * n)(*[p[0] for p in pairs]), 2, nr, rg)
    n_hits, strands = 0, set()
    for k in range(2 * n):
        regs = C.cast(rg[k], C.POINTER(mm.Reg1))
        ours = got[k // 2][k % 2]
        assert [a.key() for a in ours] == [a.key() for a in mm._regs_to_alignments(nr[k], regs, None, None)]
        for j, a in enumerate(ours):
            assert a.cs == _gen(D, mi, regs, j, flat[k], False) and a.MD == _gen(D, mi, regs, j, flat[k], True)
            n_hits += 1
            strands.add(a.strand)
    assert n_hits >= n and strands == {1, -1}
    mm.lib().mm2amd_free_regs(2 * n, nr, rg)
    D.mm_idx_destroy.argtypes = [C.c_void_p]
    D.mm_idx_destroy(mi)


def test_aligner_seq(tmp_path):
    """Aligner.seq (mappy's contract) from seq= and from a .mmi, against the input sequences"""
    import minimap2_amd as mm
    rng = np.random.default_rng(41)
    lens = [5001, 1234, 777]
    contigs = [rng.integers(0, 4, n, dtype=np.uint8) for n in lens]
    contigs[1][100:130] = 4
    refs = [X.LETTERS[c].tobytes() for c in contigs]
    names = ["a", "b", "c"]
    fn, fn_noseq = str(tmp_path / "x.mmi"), str(tmp_path / "noseq.mmi")

    def check(al):
        for _ in range(40):
            i = int(rng.integers(0, 3))
            st = int(rng.integers(0, lens[i]))
            en = int(rng.integers(st + 1, lens[i] + 1))
            assert al.seq(names[i], st, en) == refs[i][st:en].decode()
        assert al.seq("b") == refs[1].decode() and al.seq("c", 700) == refs[2][700:].decode()
        assert al.seq("b", 1200, 5000) == refs[1][1200:].decode()  # end beyond the contig: clipped, as mappy does
        assert al.seq("nope") is None and al.seq("a", 10, 10) is None and al.seq("a", 11, 10) is None and al.seq("a", 5001, 6000) is None

    al = mm.Aligner(refs, preset="map-ont", names=names, n_threads=2, fn_idx_out=fn)
    try:
        check(al)
        mm.idx_dump(al._idx, fn_noseq, 0, mm.DUMP_NO_SEQ)
    finally:
        al.close()
    al = mm.Aligner(fn_idx_in=fn, preset="map-ont", n_threads=2)
    try:
        check(al)
    finally:
        al.close()
    al = mm.Aligner(fn_idx_in=fn_noseq, preset="map-ont", n_threads=2, cigar=False)
    try:
        assert al.seq("a", 0, 10) is None
        res = (mm.TxtRes * 1)()
        r, keep = X.make_reg(mm, 0, 0, 4, 0, 4, 0, [4 << 4])
        rc = mm.lib().mm2amd_hits_text_batch(al._idx, 1, (C.c_void_p * 1)(C.addressof(r)), (C.c_char_p * 1)(b"ACGT"), (C.c_int32 * 1)(4), mm.TXT_CS, 0, res, None, 0)
        assert rc == mm.EINVAL  # an index without sequence
        assert mm.lib().mm2amd_idx_getseq(al._idx, 0, 0, 4, C.create_string_buffer(8)) == mm.EINVAL
    finally:
        al.close()
