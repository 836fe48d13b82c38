"""The ds modes of aln_text_kernel in the CPU suite: the kernel's OWN source under the wave emulator (tests/_build/libmm2amd_emu.so) against
the compiled reference's mm_gen_cs_ds_or_MD with is_ds = 1 -- the directed list, 60 random jobs in both forms, invalid jobs / sizing / pool
bounds, and hand-built hits against an index's packed sequence.  tests/test_gpu_ds_text.py runs the full set on the hardware."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import ds_text_cases as D  # noqa: E402

EMU_SO = os.path.join(HERE, "_build", "libmm2amd_emu.so")
needs_ref = pytest.mark.skipif(not D.HAVE_REF, reason="oracle/_ref absent")
# what the reference's own text holds for random_jobs(default_rng(31), 60): indels, brackets, indels with two brackets and a plain middle,
# jobs with a bracket
REF_PROFILE_60 = (3800, 1777, 142, 45)


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
def test_directed_jobs_equal_the_reference(emu):
    D.check_directed(emu)


@needs_ref
def test_random_jobs_equal_the_reference(emu):
    jobs = D.random_jobs(np.random.default_rng(31), 60)
    want = D.ref_both(jobs)
    D.check_jobs(emu, jobs, want)
    prof = D.profile(want[D.DS])
    print("profile of the reference's text:", prof)
    assert all(2 * p >= r for p, r in zip(prof, REF_PROFILE_60))  # the inputs reach the paths: at least half of what was recorded


@needs_ref
def test_invalid_jobs_sizing_call_and_pool_bounds(emu):
    D.check_bookkeeping(emu)


@needs_ref
def test_hits_equal_the_reference(emu):
    D.check_hits(emu)
