"""hits_merge_kernel in the CPU suite: the kernel's OWN source under the wave emulator (tests/_build/libmm2amd_emu.so) against the compiled reference's
mm_hit_sort, mm_set_parent, mm_select_sub and mm_set_sam_pri -- the directed lists and the class each takes, random lists with equal keys and overlaps on
the mask_level boundary, the bookkeeping.  tests/test_gpu_split.py runs the same cases on the hardware; tests/split_cases.py holds them."""
import ctypes as C
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import split_cases as X  # noqa: E402

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


def test_limits(emu):
    X.check_limits(emu)


@needs_ref
def test_directed_lists_equal_the_reference(emu):
    X.check_directed(emu)


@needs_ref
def test_random_lists_equal_the_reference(emu):
    X.check_random(emu, 2000)


@needs_ref
def test_bookkeeping(emu):
    X.check_bookkeeping(emu)


@needs_ref
def test_map_split_two_parts_long_reads(emu, tmp_path):
    """the whole route on the emulator: first pass per part, temp files, merge, SAM -- against the reference binary's --split-prefix run"""
    X.check_e2e(emu, tmp_path, "ont2")


@needs_ref
def test_map_split_with_the_kernel_in_the_merge(emu, tmp_path):
    X.check_switch(emu, tmp_path)


def test_fails_without_a_gpu():
    """the product library: no device, no answer -- but the host twin needs none"""
    import minimap2_amd as mm
    if not os.path.exists(mm.LIB_PATH):
        pytest.skip("libmm2amd.so is not built")
    L = mm.lib(mm.LIB_PATH)
    if L.mm2amd_device_count() > 0:
        pytest.skip("a GPU is visible")
    saved = mm._lib
    mm._lib = L
    try:
        seg = X.arr(mm, [X.hit(mm, 0, 100, 50, hash=1), X.hit(mm, 10, 90, 40, hash=2)])
        with pytest.raises(mm.Mm2AmdError) as e:
            mm.hits_merge_batch([seg])
        assert e.value.code == mm.ENODEV
        out, kept, path, _ = mm.hits_merge_host_batch([seg])
        assert kept == [2] and path == [X.HOST] and list(out[0]["parent"]) == [0, 0]
    finally:
        mm._lib = saved
