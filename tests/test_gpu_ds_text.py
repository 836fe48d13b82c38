"""The ds modes of aln_text_kernel on the device -- TXT_DS / TXT_DS_LONG -- through the kernel's three boundaries: mm2amd_aln_text_batch (jobs
of codes), mm2amd_hits_text_batch (mm_reg1_t records against the index's packed sequence) and the Aligner's ds=.  The judge is the UNMODIFIED
compiled reference's mm_gen_cs_ds_or_MD with is_ds = 1 (format.c:364-375); tests/ds_text_cases.py holds the jobs and the oracle."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ds_text_cases as D  # noqa: E402
import reflib  # noqa: E402
import synth  # noqa: E402

pytestmark = pytest.mark.gpu
EMU = os.environ.get("MM2AMD_EMU") == "1"
needs_ref = pytest.mark.skipif(not D.HAVE_REF, reason="oracle/_ref absent")
# what the reference's own text holds for random_jobs(default_rng(31), n): indels, brackets, indels with two brackets and a plain middle,
# jobs with a bracket
REF_PROFILE = {600: (25798, 11804, 1003, 451), 60: (3800, 1777, 142, 45)}


@pytest.fixture(scope="module")
def random_cases():
    """(jobs, the reference's texts): computed once for the two forms"""
    jobs = D.random_jobs(np.random.default_rng(31), 60 if EMU else 600)
    return jobs, D.ref_both(jobs)


@needs_ref
def test_directed_jobs_equal_the_reference():
    import minimap2_amd as mm
    D.check_directed(mm)


@needs_ref
@pytest.mark.parametrize("form", D.FORMS)
def test_random_jobs_equal_the_reference(random_cases, form):
    import minimap2_amd as mm
    jobs, want = random_cases
    got = mm.aln_text_batch(jobs, form)
    for i, (g, w) in enumerate(zip(got, want[form])):
        assert g == w, "job %d (%d operations): %r != %r" % (i, len(jobs[i][2]), g and g[:200], w[:200])
    prof = D.profile(want[D.DS])
    print("profile of the reference's text:", prof)
    assert all(2 * p >= r for p, r in zip(prof, REF_PROFILE[len(jobs)]))  # the inputs reach the paths: at least half of what was recorded


@needs_ref
def test_invalid_jobs_sizing_call_and_pool_bounds():
    import minimap2_amd as mm
    D.check_bookkeeping(mm)


@needs_ref
def test_hits_equal_the_reference():
    import minimap2_amd as mm
    D.check_hits(mm)


def _gen_ds(R, mi, reg, seq):
    buf, cap = C.c_void_p(), C.c_int(0)
    n = R.mm_gen_cs_ds_or_MD(None, C.byref(buf), C.byref(cap), mi, C.byref(reg), seq, 0, 1, 1, 0)
    s = C.string_at(buf, n).decode() if n else ""
    reflib._libc.free(buf)
    return s


@needs_ref
def test_aligner_ds_equals_the_reference():
    """the reads of smoke(): hits are the reference's (existing parity); here their ds, and cs / MD beside it"""
    import minimap2_amd as mm
    rng = np.random.default_rng(3)
    contigs = synth.gen_reference(rng, 1000000, 2)
    reads = synth.gen_reads(rng, contigs, 12, 6000, 1500, 0.12)
    refs = [synth.ACGT[c].tobytes() for c in contigs]
    rds = [("read%d" % i, synth.ACGT[r].tobytes()) for i, r in enumerate(reads)]
    al = mm.Aligner(refs, preset="map-ont", names=["chr1", "chr2"], n_threads=4)
    try:
        hits = al.map_batch(rds, cs=True, MD=True, ds=True)
        tags = al.map_batch(rds, cs=True, MD=True)
    finally:
        al.close()
    assert all(a.ds == "" for h in tags for a in h)  # "" unless asked for
    # cs and MD are what they are without ds
    assert [[(a.key(), a.cs, a.MD) for a in h] for h in hits] == [[(a.key(), a.cs, a.MD) for a in h] for h in tags]
    assert all(a.cs and a.MD for h in hits for a in h)
    m = reflib.RefMapper(refs, "map-ont", ["chr1", "chr2"])
    m.R.mm_gen_cs_ds_or_MD.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.c_void_p, C.c_void_p, C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int]
    strands, n_br = set(), 0
    try:
        for (nm, seq), h in zip(rds, hits):
            n = C.c_int(0)
            regs = m.R.mm_map(m.mi, len(seq), seq, C.byref(n), m.tbuf, C.byref(m.mo), nm.encode())
            assert [a.key() for a in h] == [a.key() for a in mm._regs_to_alignments(n.value, regs, None, None)]
            for j, a in enumerate(h):
                assert a.ds == _gen_ds(m.R, m.mi, regs[j], seq)
                assert a.ds
                n_br += a.ds.count("[")
                strands.add(a.strand)
            for j in range(n.value):
                if regs[j].p:
                    reflib._libc.free(C.cast(regs[j].p, C.c_void_p))
            if regs:
                reflib._libc.free(C.cast(regs, C.c_void_p))
    finally:
        m.close()
    assert strands == {1, -1} and n_br >= 100


def test_aligner_pairs_ds(tmp_path):
    """map(seq, seq2, ds=True) is a batch of one pair: it equals map_pairs, pair by pair"""
    import minimap2_amd as mm
    ref, f1, f2, _ = synth.make_pairs(str(tmp_path), n_pairs=8)
    rn, rs = mm.read_fastx(ref)
    n1, s1 = mm.read_fastx(f1)
    _, s2 = mm.read_fastx(f2)
    pairs = [(nm[:-2], a, b) for nm, a, b in zip(n1, s1, s2)][:8]
    al = mm.Aligner(rs, preset="sr", names=[x.decode() for x in rn], n_threads=4)
    try:
        got = al.map_pairs(pairs, ds=True)
        ones = [al.map(p[1], p[2], name=p[0], ds=True) for p in pairs]  # (the name too: ties between equal hits are broken by its hash)
    finally:
        al.close()
    n_hits = 0
    for one, per in zip(ones, got):
        assert [[(a.key(), a.ds) for a in seg] for seg in one] == [[(a.key(), a.ds) for a in seg] for seg in per]
        assert all(a.ds and a.cs == "" and a.MD == "" for seg in per for a in seg)
        n_hits += sum(len(seg) for seg in per)
    assert n_hits >= len(pairs)
