"""cigar_eqx_kernel in the CPU suite: the kernel's OWN source under the wave emulator (tests/_build/libmm2amd_emu.so) behind
mm2amd_update_extra_eqx_batch, against the UNMODIFIED reference's mm_update_extra with is_eqx = 1 -- the random regions, the directed ones, the
sizing call and the short pool -- and the reference's own output checked for the shapes the cases are for.  tests/test_gpu_eqx.py runs the same
cases, and mapped reads against the reference binary, on the hardware; tests/eqx_cases.py holds the cases and the judges."""
import ctypes as C
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import eqx_cases as X  # noqa: E402

EMU_SO = os.path.join(HERE, "_build", "libmm2amd_emu.so")
needs_refalign = pytest.mark.skipif(not X.HAVE_REFALIGN, reason="oracle/_ref/librefalign.so absent")


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


@needs_refalign
@pytest.mark.parametrize("log_gap", [1, 0])
def test_the_reference_alone_clears_the_thresholds(log_gap):
    X.check_reference_shapes(log_gap)


@needs_refalign
@pytest.mark.parametrize("log_gap", [1, 0])
def test_update_extra_eqx_batch_equals_the_reference(emu, log_gap):
    X.check_kernel(emu, log_gap)


@needs_refalign
def test_sizing_call_and_a_pool_one_word_short(emu):
    X.check_sizing(emu)


def test_aligner_eqx_sets_the_flag(emu):
    ref = b"ACGTTGCATGCCGATAGCTAGCTAGGATCGATCGATTTAGCGCGATATCGCGGCTA" * 40
    for kw, on in ((dict(eqx=True), True), (dict(extra_flags=emu.F_EQX), True), (dict(), False)):
        al = emu.Aligner([ref], preset="map-ont", n_threads=2, **kw)
        try:
            assert bool(al.map_opt.flag & emu.F_EQX) == on and emu.F_EQX == 0x4000000
        finally:
            al.close()


def test_fails_without_a_gpu():
    """the product library: no device, no answer"""
    import minimap2_amd as mm
    if not os.path.exists(mm.LIB_PATH):
        pytest.skip("libmm2amd.so is not built")
    L = mm.lib(mm.LIB_PATH)
    if L.mm2amd_device_count() > 0:
        pytest.skip("a GPU is visible")
    saved = mm._lib
    mm._lib = L
    try:
        with pytest.raises(mm.Mm2AmdError) as e:
            mm.update_extra_batch([(b"\0\1\2", b"\0\1\1", [[3 << 4]])], X.MAT, 4, 2, 1, eqx=True)
        assert e.value.code == mm.ENODEV
    finally:
        mm._lib = saved
