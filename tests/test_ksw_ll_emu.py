"""ksw_ll_kernel in the CPU suite: the kernel's OWN source under the wave emulator (tests/_build/libmm2amd_emu.so) against the compiled reference's
ksw_ll_qinit + ksw_ll_i16 -- directed shapes, generated jobs, the orientation flags, the workgroup class at its smallest shapes, limits and routing,
a mixed batch with reuse, and the bookkeeping.  tests/test_gpu_ksw_ll.py runs the same cases, and the large jobs, on the hardware."""
import ctypes as C
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import ksw_ll_cases as X  # noqa: E402

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
def test_generated_jobs_equal_the_reference_and_bite(emu):
    X.check_generated(emu)


@needs_ref
def test_orientation_flags(emu):
    X.check_flags(emu)


@needs_ref
def test_workgroup_class_at_its_smallest_shapes(emu):
    X.check_workgroup(emu)


@needs_ref
def test_limits_and_routing(emu):
    X.check_limits(emu)


@needs_ref
def test_mixed_batch_and_reuse(emu):
    X.check_mixed(emu)


@needs_ref
def test_bookkeeping(emu):
    X.check_bookkeeping(emu)


def test_fails_without_a_gpu():
    """the product library: no device, no answer -- also for a job the host routine would compute"""
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
            mm.ksw_ll_batch([(b"\0\1\2", b"\0\1\2")], X.mat_of((2, 4, 0, 2, 1, 0)), 0, 2)  # a free gap opening: HOST-routed
        assert e.value.code == mm.ENODEV
    finally:
        mm._lib = saved
