"""aln_text_kernel in the CPU suite: the kernel's OWN source under the wave emulator (tests/_build/libmm2amd_emu.so) against the compiled
reference's mm_gen_cs_ds_or_MD -- the directed list, 60 random jobs per mode, invalid jobs / sizing / pool bounds, and hand-built hits
against an index's packed sequence.  tests/test_gpu_aln_text.py runs the full set on the hardware."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import aln_text_cases as X  # noqa: E402

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
def test_directed_jobs_equal_the_reference(emu):
    X.check_directed(emu)


@needs_ref
def test_random_jobs_equal_the_reference(emu):
    jobs = X.random_jobs(np.random.default_rng(31), 60)
    want = X.ref_texts(jobs)
    X.check_jobs(emu, jobs, want)
    n_cross, n_tiles, n_nn = X.profile(jobs, want)
    assert n_cross >= 6 and n_tiles >= 3 and n_nn >= 6


def test_cigar_strings(emu):
    X.check_cigar_mode(emu, np.random.default_rng(33), 26)


@needs_ref
def test_invalid_jobs_sizing_call_and_pool_bounds(emu):
    X.check_bookkeeping(emu)


@needs_ref
def test_hits_equal_the_reference(emu):
    X.check_hits(emu)
