"""junc_text_kernel in the CPU suite: the kernel's OWN source under the wave emulator (tests/_build/libmm2amd_emu.so) behind the three format
calls with MM_F_OUT_JUNC and behind mm2amd_hits_junc_batch, against the compiled reference's mm_write_junc -- the score table in the four
orientations, map.c's filter, the walk across 64-operation steps, the packed reference at every nibble offset, the names, two-segment
fragments and the bookkeeping.  tests/test_gpu_junc_text.py runs the same on the hardware, with mapped reads against the reference binary;
tests/junc_text_cases.py holds the cases and the judges."""
import ctypes as C
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import junc_text_cases as J  # noqa: E402

EMU_SO = os.path.join(HERE, "_build", "libmm2amd_emu.so")
needs_ref = pytest.mark.skipif(not J.HAVE_REF, reason="oracle/_ref absent")


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
def test_junction_text_equals_the_reference(emu):
    J.check_formats(emu)


@needs_ref
def test_hits_junc_batch_equals_the_reference(emu):
    J.check_hits_junc(emu)


def test_aligner_write_junc_sets_the_flags(emu):
    """write_junc=True is minimap2's --write-junc: MM_F_OUT_JUNC | MM_F_CIGAR; without it the flag is the preset's"""
    ref = b"ACGTTGCATGCCGATAGCTAGCTAGGATCGATCGATTTAGCGCGATATCGCGGCTA" * 40
    al = emu.Aligner([ref], preset="splice", n_threads=2, cigar=False, write_junc=True)
    try:
        assert al.map_opt.flag & emu.F_OUT_JUNC and al.map_opt.flag & emu.F_CIGAR and emu.F_OUT_JUNC == J.F_OUT_JUNC
    finally:
        al.close()
    al = emu.Aligner([ref], preset="splice", n_threads=2)
    try:
        assert al.map_opt.flag & emu.F_OUT_JUNC == 0
    finally:
        al.close()
