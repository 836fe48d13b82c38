"""fastx_lines_kernel, fastx_classify_kernel and fastx_copy_kernel on the device behind mm2amd_fastx_parse, and minimap2_amd.FastxReader over them: FASTA
and FASTQ text into the records and batches of the reference's reader.  The judge is the UNMODIFIED compiled reference (mm_bseq_read3 /
mm_bseq_read_frag2, and `minimap2 -a` for the mapping case); tests/fastx_cases.py holds the cases, tests/test_fastx_emu.py runs them under the wave emulator."""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import fastx_cases as X  # noqa: E402

pytestmark = pytest.mark.gpu
needs_ref = pytest.mark.skipif(not X.HAVE_REF, reason="oracle/_ref absent")
needs_bin = pytest.mark.skipif(not (X.HAVE_REF and X.HAVE_BIN), reason="oracle/_ref absent")


@needs_ref
def test_directed_texts_equal_the_reference():
    import minimap2_amd as mm
    X.check_directed(mm)


@needs_ref
def test_line_shapes_alignments_and_line_ends():
    import minimap2_amd as mm
    X.check_line_shapes(mm)


@needs_ref
def test_long_class():
    import minimap2_amd as mm
    X.check_long_class(mm)


@needs_ref
def test_fasta_multiline():
    import minimap2_amd as mm
    X.check_fasta_multiline(mm)


@needs_ref
def test_incremental_blocks():
    import minimap2_amd as mm
    X.check_incremental(mm)


@needs_ref
def test_reader_batches(tmp_path):
    import minimap2_amd as mm
    X.check_reader_batches(mm, str(tmp_path))


@needs_ref
def test_host_class():
    import minimap2_amd as mm
    X.check_host_class(mm)


@needs_ref
def test_bookkeeping():
    import minimap2_amd as mm
    X.check_bookkeeping(mm)


@needs_bin
def test_mapping_from_file(tmp_path):
    import minimap2_amd as mm
    X.check_mapping_from_file(mm, str(tmp_path))
