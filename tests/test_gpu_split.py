"""hits_merge_kernel on the device behind mm2amd_hits_merge_batch -- the hit-list rules of a split-index merge (merge_hits, map.c:520-531), one
wavefront per read segment, in its narrow and wide launch classes and the host class.  The judge is the UNMODIFIED compiled reference;
tests/split_cases.py holds the lists and the checks, tests/test_split_emu.py runs them under the wave emulator."""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import split_cases as X  # noqa: E402

pytestmark = pytest.mark.gpu
needs_ref = pytest.mark.skipif(not X.HAVE_REF, reason="oracle/_ref absent")


def test_limits():
    import minimap2_amd as mm
    X.check_limits(mm)


@needs_ref
def test_directed_lists_equal_the_reference():
    import minimap2_amd as mm
    X.check_directed(mm)


@needs_ref
@pytest.mark.parametrize("seed", [7, 8, 9])
def test_random_lists_equal_the_reference(seed):
    import minimap2_amd as mm
    X.check_random(mm, 1000, seed)


@needs_ref
def test_bookkeeping():
    import minimap2_amd as mm
    X.check_bookkeeping(mm)


# ---- the whole feature: map_split (SplitWriter, SplitMerger) against the reference binary's --split-prefix run, byte for byte
needs_bin = pytest.mark.skipif(not os.path.exists(X.reflib.REF_BIN), reason="oracle/_ref absent")


@needs_bin
@pytest.mark.parametrize("which", ["ont2", "ont4", "paf4", "sr2", "paf_no_hit", "one_part"])
def test_map_split_equals_the_reference_binary(which, tmp_path):
    import minimap2_amd as mm
    X.check_e2e(mm, tmp_path, which)


@needs_bin
def test_map_split_cuts_a_fasta_into_parts(tmp_path):
    import minimap2_amd as mm
    X.check_fasta_parts(mm, tmp_path)


@needs_bin
def test_the_same_contig_in_two_parts(tmp_path):
    import minimap2_amd as mm
    X.check_equal_keys_e2e(mm, tmp_path)


@needs_bin
def test_temp_files_read_by_the_reference_and_the_reference_s_read_by_us(tmp_path):
    import minimap2_amd as mm
    X.check_temp_files_both_ways(mm, tmp_path)


@needs_bin
def test_cs_md_ds_and_junctions_are_refused(tmp_path):
    import minimap2_amd as mm
    X.check_refusals(mm, tmp_path)


@needs_bin
def test_device_merge_switch(tmp_path):
    import minimap2_amd as mm
    X.check_switch(mm, tmp_path)
