"""pair_kernel in the CPU suite: the kernel's OWN source under the wave emulator (tests/_build/libmm2amd_emu.so) against the compiled reference's
mm_pair -- the directed fragments and the class each takes, random fragments with equal keys and reach boundaries, the bookkeeping.
tests/test_gpu_pair.py runs the same cases on the hardware; tests/pair_cases.py holds them."""
import ctypes as C
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import pair_cases as X  # noqa: E402

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
def test_directed_fragments_equal_the_reference(emu):
    X.check_directed(emu)


@needs_ref
def test_random_fragments_equal_the_reference(emu):
    X.check_random(emu, 2000)


@needs_ref
def test_bookkeeping(emu):
    X.check_bookkeeping(emu)


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
        fr = X.frag(mm, [X.hit(mm, 1000, 1100)], [X.hit(mm, 1300, 1400)])
        with pytest.raises(mm.Mm2AmdError) as e:
            mm.pair_batch([fr])
        assert e.value.code == mm.ENODEV
        out, res, _ = mm.pair_host_batch([fr])
        assert list(res[0]["best"]) == [0, 0] and res[0]["path"] == X.HOST and list(out[0][0]["mapq"]) == [2]
    finally:
        mm._lib = saved
