"""rec_text_kernel on the device, behind mm_gpu_format_batch_dev and Aligner.format_raw(device=True): whole PAF and SAM records.  Judges
(tests/rec_text_cases.py): the UNMODIFIED compiled reference's mm_write_paf4 / mm_write_sam3 for hand-built records, the reference binary for
mapped reads, and mm_gpu_format_batch wherever both exist.  Every case meant for the device asserts that the device wrote the text."""
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import rec_text_cases as X  # noqa: E402

pytestmark = pytest.mark.gpu
EMU = os.environ.get("MM2AMD_EMU") == "1"
needs_ref = pytest.mark.skipif(not X.HAVE_REF, reason="oracle/_ref absent")
needs_bin = pytest.mark.skipif(not X.HAVE_BIN, reason="oracle/_ref/minimap2_ref absent")


@needs_ref
def test_fractions_equal_the_reference():
    """de:f over all pairs 0 <= mlen <= den, 1 <= den <= 400 (the exact ties of %.4f among them), dv:f from the hits' floats"""
    import minimap2_amd as mm
    X.check_fractions(mm, 64 if EMU else 400)


@needs_ref
def test_directed_records_equal_the_reference():
    import minimap2_amd as mm
    X.check_directed(mm)


@needs_ref
def test_fallbacks_and_bookkeeping():
    import minimap2_amd as mm
    X.check_fallbacks(mm)


@pytest.fixture(scope="module")
def mapped(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("rec_text"))
    return X.mapped_inputs(d)


@needs_bin
@pytest.mark.parametrize("case", X.MAPPED_CASES, ids=[c[0] for c in X.MAPPED_CASES])
def test_mapped_reads_equal_the_reference_binary(mapped, case):
    import minimap2_amd as mm
    ref_fa, reads_fq, refs, names, rds = mapped
    _, opts, kw = case
    want = X.binary_text(ref_fa, reads_fq, opts)
    if opts == ["-a"]:  # the shapes this read set is for are in the REFERENCE's text
        fl = [int(ln.split(b"\t")[1]) for ln in want.split(b"\n") if ln]
        assert all(any(f & bit for f in fl) for bit in (4, 16, 256, 2048)) and b"SA:Z:" in want
    al = mm.Aligner(refs, preset="map-ont", names=names, n_threads=4, **kw)
    try:
        got, path, host = X.device_text(mm, al, X.batch_with_quality(mm, rds))
    finally:
        al.close()
    assert path == mm.FMT_PATH_DEVICE
    assert got == want, X.first_difference(got, want)
    assert host == want


@needs_bin
def test_spliced_reads_equal_the_reference_binary(tmp_path):
    import minimap2_amd as mm
    import synth
    ref_fa, reads_fa, _ = synth.make_junctions(str(tmp_path), n_reads=8)
    rn, rs = mm.read_fastx(ref_fa)
    qn, qs = mm.read_fastx(reads_fa)
    want = X.binary_text(ref_fa, reads_fa, ["-a"], preset="splice")
    assert b"ts:A:" in want
    al = mm.Aligner(rs, preset="splice", names=[x.decode() for x in rn], n_threads=4, sam=True)
    try:
        got, path, host = X.device_text(mm, al, mm.Batch(list(zip(qn, qs))))
    finally:
        al.close()
    assert path == mm.FMT_PATH_DEVICE
    assert got == want, X.first_difference(got, want)
    assert host == want


CHILD = """
import sys
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import os
if os.environ.get("MM2AMD_EMU") == "1":
    import conftest  # (binds the emulator build, as the parent's suite does)
import minimap2_amd as mm
import rec_text_cases as X
ref_fa, reads_fq, refs, names, rds = X.mapped_inputs(sys.argv[1])
al = mm.Aligner(refs, preset="map-ont", names=names, n_threads=4, sam=True)
mm.profile_enable(True)
al.stage(X.batch_with_quality(mm, rds))
n_reg, reg, rep_len = al.run(raw=True)
text = al.format_raw(n_reg, reg, rep_len)
launches = mm.profile_get().get("rec_text_kernel[write]", {}).get("launches", 0)
al.free_raw(n_reg, reg)
al.close()
open(sys.argv[2], "wb").write(text)
print("launches", launches)
"""


@needs_bin
def test_device_text_switch_gives_format_raw_the_same_bytes(mapped, tmp_path):
    """MM2AMD_DEVICE_TEXT=1 routes mm_gpu_format_batch through the record kernel (a child process: the switch is read from the environment); unset, the
    kernel is not launched"""
    ref_fa, reads_fq, refs, names, rds = mapped
    want = X.binary_text(ref_fa, reads_fq, ["-a"])
    for value, launched in (("1", True), (None, False)):
        env = {k: v for k, v in os.environ.items() if k != "MM2AMD_DEVICE_TEXT"}
        if value is not None:
            env["MM2AMD_DEVICE_TEXT"] = value
        out = str(tmp_path / ("text_%s" % value))
        r = subprocess.run([sys.executable, "-c", CHILD % (ROOT, HERE), str(tmp_path), out], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=170)
        assert r.returncode == 0, r.stdout.decode()
        assert open(out, "rb").read() == want
        n = int(r.stdout.decode().split("launches")[-1].split()[0])
        assert (n > 0) == launched
