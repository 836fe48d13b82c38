"""ksw_ll_kernel on the device behind mm2amd_ksw_ll_batch -- the local score with end coordinates of ksw_ll_qinit + ksw_ll_i16 -- in its two launch
classes (a wavefront per job, a workgroup per job).  The judge is the UNMODIFIED compiled reference (ksw2_ll_sse.c:37-152) on the explicitly
transformed sequences; tests/ksw_ll_cases.py holds the jobs and the oracle, tests/test_ksw_ll_emu.py runs the same cases under the wave emulator."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ksw_ll_cases as X  # noqa: E402

pytestmark = pytest.mark.gpu
needs_ref = pytest.mark.skipif(not X.HAVE_REF, reason="oracle/_ref absent")


@needs_ref
def test_directed_shapes_equal_the_reference():
    import minimap2_amd as mm
    X.check_directed(mm)


@needs_ref
def test_generated_jobs_equal_the_reference_and_bite():
    import minimap2_amd as mm
    X.check_generated(mm)


@needs_ref
def test_orientation_flags():
    import minimap2_amd as mm
    X.check_flags(mm)


@needs_ref
def test_workgroup_class_at_its_smallest_shapes():
    import minimap2_amd as mm
    X.check_workgroup(mm)


@needs_ref
def test_limits_and_routing():
    import minimap2_amd as mm
    X.check_limits(mm)


@needs_ref
def test_mixed_batch_and_reuse():
    import minimap2_amd as mm
    X.check_mixed(mm)


@needs_ref
def test_bookkeeping():
    import minimap2_amd as mm
    X.check_bookkeeping(mm)


@pytest.fixture(scope="module")
def large_jobs():
    """(jobs, the reference's answers): 5 000 x 5 000 and 10 000 x 3 000, related at 15 % divergence"""
    rng = np.random.default_rng(29)
    jobs = [X.related(rng, 5000, 5000, 0.15), X.related(rng, 10000, 3000, 0.15)]
    return jobs, X.want_of(jobs, X.SCORINGS[0])


@needs_ref
def test_large_jobs_in_both_classes(large_jobs):
    import minimap2_amd as mm
    jobs, want = large_jobs
    assert want[0][0] > 3000 and want[1][0] > 2000
    mm.profile_enable(True)
    try:
        with X.env(MM2AMD_LL_NO_WG=None, MM2AMD_LL_WG_MIN_CELLS=None):
            X.check(mm, jobs, X.SCORINGS[0], path=X.WG, want=want)
            with X.env(MM2AMD_LL_NO_WG=1):
                X.check(mm, jobs, X.SCORINGS[0], path=X.WAVE, want=want)
        prof = mm.profile_get()
    finally:
        mm.profile_enable(False)
    cells = float(sum(len(q) * len(t) for q, t in jobs))
    for name in ("ksw_ll_kernel[wave]", "ksw_ll_kernel[wg]"):
        assert name in prof and prof[name]["units"] == cells and prof[name]["launches"] == 1, prof.get(name)
