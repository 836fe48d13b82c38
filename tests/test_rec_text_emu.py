"""rec_text_kernel in the CPU suite: the kernel's OWN source under the wave emulator (tests/_build/libmm2amd_emu.so) behind
mm_gpu_format_batch_dev, against the compiled reference's mm_write_paf4 / mm_write_sam3 -- the fraction sweep up to a denominator of 64, the
directed record shapes, the fallbacks and the buffer bookkeeping -- and Aligner(extra_flags=).  tests/test_gpu_rec_text.py runs the full set,
mapped reads against the reference binary included, on the hardware; tests/rec_text_cases.py holds the cases and the judges."""
import ctypes as C
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import rec_text_cases as X  # noqa: E402

EMU_SO = os.path.join(HERE, "_build", "libmm2amd_emu.so")
needs_ref = pytest.mark.skipif(not X.HAVE_REF, reason="oracle/_ref absent")


@pytest.fixture(scope="module")
def emu():
    if os.path.exists("/root/reference/minimap.h") or not os.path.exists(EMU_SO):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "oracle")], stdout=subprocess.DEVNULL)
        subprocess.check_call(["make", "-s", "-C", os.path.join(HERE, "cpucheck")], stdout=subprocess.DEVNULL)
    import minimap2_amd as mm
    saved = mm._lib
    mm._lib = mm._bind(C.CDLL(EMU_SO))
    yield mm
    mm._lib = saved


@needs_ref
def test_fractions_equal_the_reference(emu):
    X.check_fractions(emu, 64)


@needs_ref
def test_directed_records_equal_the_reference(emu):
    X.check_directed(emu)


@needs_ref
def test_fallbacks_and_bookkeeping(emu):
    X.check_fallbacks(emu)


def test_aligner_extra_flags(emu):
    """extra_flags is ORed into map_opt.flag (mappy's parameter); without it the flag is the preset's"""
    ref = b"ACGTTGCATGCCGATAGCTAGCTAGGATCGATCGATTTAGCGCGATATCGCGGCTA" * 40
    want = X.F_SOFTCLIP | X.F_SECONDARY_SEQ | X.F_OUT_MD
    al = emu.Aligner([ref], preset="map-ont", n_threads=2, sam=True, extra_flags=want)
    try:
        assert al.map_opt.flag & want == want and al.map_opt.flag & emu.F_OUT_SAM and al.last_format_path is None
    finally:
        al.close()
    al = emu.Aligner([ref], preset="map-ont", n_threads=2)
    try:
        assert al.map_opt.flag & (want | emu.F_OUT_SAM) == 0
    finally:
        al.close()
