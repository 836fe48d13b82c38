"""=/X CIGARs on the device (cigar_eqx_kernel behind mm2amd_update_extra_eqx_batch, Backend::finish_regions and Backend::align_regions): regions
against the UNMODIFIED reference's mm_update_extra with is_eqx = 1, mapped reads against the reference binary's --eqx -- long reads in PAF and SAM
with cs and MD, reads that are handed back to the host's rounds, short-read pairs -- with the routing asserted: --eqx reads stay where they are
without it, and MM2AMD_DEVICE_EQX=0 gives the same records from the host's route.  tests/eqx_cases.py holds the cases and the judges."""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import eqx_cases as X  # noqa: E402

pytestmark = pytest.mark.gpu
needs_refalign = pytest.mark.skipif(not X.HAVE_REFALIGN, reason="oracle/_ref/librefalign.so absent")
needs_bin = pytest.mark.skipif(not X.HAVE_BIN, reason="oracle/_ref/minimap2_ref absent")


@needs_refalign
@pytest.mark.parametrize("log_gap", [1, 0])
def test_update_extra_eqx_batch_equals_the_reference(log_gap):
    import minimap2_amd as mm
    X.check_kernel(mm, log_gap)


@needs_refalign
def test_sizing_call_and_a_pool_one_word_short():
    import minimap2_amd as mm
    X.check_sizing(mm)


@pytest.fixture(scope="module")
def mapped(tmp_path_factory):
    return X.R.mapped_inputs(str(tmp_path_factory.mktemp("eqx")))


@needs_bin
@pytest.mark.parametrize("case", X.MAPPED_CASES, ids=[c[0] for c in X.MAPPED_CASES])
def test_mapped_reads_equal_the_reference_binary(mapped, case, monkeypatch):
    import minimap2_amd as mm
    X.check_mapped(mm, monkeypatch, mapped, case)


@needs_bin
def test_handed_back_reads_equal_the_reference_binary(tmp_path, monkeypatch):
    import minimap2_amd as mm
    X.check_handbacks(mm, monkeypatch, str(tmp_path))


@needs_bin
def test_short_read_pairs_equal_the_reference_binary(tmp_path, monkeypatch):
    import minimap2_amd as mm
    X.check_short(mm, monkeypatch, str(tmp_path))
