"""sdust_kernel on the device behind mm2amd_sdust_batch -- the masked regions of sdust() (sdust.c:134-175, W = 64), one wavefront per sequence, in its
two launch classes (a short list of perfect intervals in LDS, the full one) -- and behind the `-T` mapping path with MM2AMD_DEVICE_SDUST=1.  The judge
is the UNMODIFIED compiled reference; tests/sdust_cases.py holds the sequences and the checks, tests/test_sdust_emu.py runs them under the wave emulator."""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import sdust_cases as X  # noqa: E402

pytestmark = pytest.mark.gpu
needs_ref = pytest.mark.skipif(not X.HAVE_REF, reason="oracle/_ref absent")


@needs_ref
def test_directed_shapes_equal_the_reference():
    import minimap2_amd as mm
    X.check_directed(mm)


@needs_ref
@pytest.mark.parametrize("T", X.THRESHOLDS)
def test_generated_sequences_equal_the_reference(T):
    import minimap2_amd as mm
    X.check_generated(mm, T)


@needs_ref
def test_small_narrow_lists_and_the_wide_class_alone():
    import minimap2_amd as mm
    X.check_classes(mm)


@needs_ref
def test_mixed_batch_reuse_and_profile():
    import minimap2_amd as mm
    X.check_mixed(mm)


@needs_ref
def test_bookkeeping():
    import minimap2_amd as mm
    X.check_bookkeeping(mm)


@needs_ref
@pytest.mark.parametrize("T", [20, 5])
def test_mapping_single_reads_with_the_device_scan(T):
    import minimap2_amd as mm
    X.check_mapping_singles(mm, T)


@needs_ref
def test_mapping_pairs_with_the_device_scan():
    import minimap2_amd as mm
    X.check_mapping_pairs(mm)
