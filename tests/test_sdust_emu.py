"""sdust_kernel in the CPU suite: the kernel's OWN source under the wave emulator (tests/_build/libmm2amd_emu.so) against the compiled reference's
sdust() -- directed shapes at seven thresholds, generated sequences and the class each takes, small narrow lists and the wide class alone, a mixed
batch with reuse and the profile, the bookkeeping, and the `-T` mapping path with MM2AMD_DEVICE_SDUST=1.  tests/test_gpu_sdust.py runs the same cases
on the hardware; tests/sdust_cases.py holds them."""
import ctypes as C
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import sdust_cases as X  # noqa: E402

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
def test_directed_shapes_equal_the_reference(emu):
    X.check_directed(emu)


@needs_ref
@pytest.mark.parametrize("T", X.THRESHOLDS)
def test_generated_sequences_equal_the_reference(emu, T):
    X.check_generated(emu, T)


@needs_ref
def test_small_narrow_lists_and_the_wide_class_alone(emu):
    X.check_classes(emu)


@needs_ref
def test_mixed_batch_reuse_and_profile(emu):
    X.check_mixed(emu)


@needs_ref
def test_bookkeeping(emu):
    X.check_bookkeeping(emu)


@needs_ref
@pytest.mark.parametrize("T", [20, 5])
def test_mapping_single_reads_with_the_device_scan(emu, T):
    X.check_mapping_singles(emu, T)


@needs_ref
def test_mapping_pairs_with_the_device_scan(emu):
    X.check_mapping_pairs(emu)


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
            mm.sdust_batch([b"A" * 80], 20)
        assert e.value.code == mm.ENODEV
    finally:
        mm._lib = saved
