"""The readers' kernels in the CPU suite: fastx_lines_kernel, fastx_classify_kernel and fastx_copy_kernel -- their OWN source under the wave emulator
(tests/_build/libmm2amd_emu.so) -- the host's parser and minimap2_amd.FastxReader against the compiled reference's mm_bseq_read3 / mm_bseq_read_frag2.
tests/test_gpu_fastx.py runs the same cases on the hardware; tests/fastx_cases.py holds them."""
import ctypes as C
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import fastx_cases as X  # noqa: E402

EMU_SO = os.path.join(HERE, "_build", "libmm2amd_emu.so")
needs_ref = pytest.mark.skipif(not X.HAVE_REF, reason="oracle/_ref absent")
needs_bin = pytest.mark.skipif(not (X.HAVE_REF and X.HAVE_BIN), reason="oracle/_ref absent")


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
def test_directed_texts_equal_the_reference(emu):
    X.check_directed(emu)


@needs_ref
def test_line_shapes_alignments_and_line_ends(emu):
    X.check_line_shapes(emu)


@needs_ref
def test_long_class(emu):
    X.check_long_class(emu)


@needs_ref
def test_fasta_multiline(emu):
    X.check_fasta_multiline(emu)


@needs_ref
def test_incremental_blocks(emu):
    X.check_incremental(emu)


@needs_ref
def test_reader_batches(emu, tmp_path):
    X.check_reader_batches(emu, str(tmp_path))


@needs_ref
def test_host_class(emu):
    X.check_host_class(emu)


@needs_ref
def test_bookkeeping(emu):
    X.check_bookkeeping(emu)


@needs_bin
def test_mapping_from_file(emu, tmp_path):
    X.check_mapping_from_file(emu, str(tmp_path))


def test_fails_without_a_gpu():
    """the product library: no device, no answer from the device entry point; the host's parser needs none"""
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
            mm.parse_fastx(b"@a\nAC\n+\nII\n", device=True)
        assert e.value.code == mm.ENODEV
        assert mm.parse_fastx(b"@a\nAC\n+\nII\n", device=False) == ([(b"a", None, b"AC", b"II")], 11, mm.FASTX_PATH_HOST)
    finally:
        mm._lib = saved
