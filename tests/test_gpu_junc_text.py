"""junc_text_kernel on the device: --write-junc behind mm_gpu_format_batch_dev / Aligner(write_junc=True), and mm2amd_hits_junc_batch.  Judges
(tests/junc_text_cases.py): the UNMODIFIED compiled reference's mm_write_junc for hand-built hits, the reference binary with --write-junc for
mapped reads, and the host writer wherever both exist.  Every device case asserts that the device wrote the text."""
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import junc_text_cases as J  # noqa: E402
import rec_text_cases as X  # noqa: E402

pytestmark = pytest.mark.gpu
needs_ref = pytest.mark.skipif(not J.HAVE_REF, reason="oracle/_ref absent")
needs_bin = pytest.mark.skipif(not J.HAVE_BIN, reason="oracle/_ref/minimap2_ref absent")


@needs_ref
def test_junction_text_equals_the_reference():
    import minimap2_amd as mm
    J.check_formats(mm)


@needs_ref
def test_hits_junc_batch_equals_the_reference():
    import minimap2_amd as mm
    J.check_hits_junc(mm)


@pytest.fixture(scope="module")
def spliced(tmp_path_factory):
    import synth
    d = str(tmp_path_factory.mktemp("junc_text"))
    ref_fa, reads_fa, _ = synth.make_junctions(d, n_reads=8)
    return ref_fa, reads_fa, J.binary_junc(ref_fa, [reads_fa], "splice")


@needs_bin
def test_spliced_reads_equal_the_reference_binary(spliced):
    import minimap2_amd as mm
    ref_fa, reads_fa, want = spliced
    J.assert_reference_shapes(want)
    rn, rs = mm.read_fastx(ref_fa)
    qn, qs = mm.read_fastx(reads_fa)
    al = mm.Aligner(rs, preset="splice", names=[x.decode() for x in rn], n_threads=4, write_junc=True)
    try:
        got, path, host = X.device_text(mm, al, mm.Batch(list(zip(qn, qs))))
    finally:
        al.close()
    assert path == mm.FMT_PATH_DEVICE
    assert got == want, X.first_difference(got, want)
    assert host == want


@needs_bin
def test_rna_pairs_equal_the_reference_binary(tmp_path):
    """splice:sr read pairs through map_pairs(text=True): junctions of either mate.  Both mates carry the first mate's name (map_pairs names a
    pair once), so the reference binary reads a second file whose records are named as the first's."""
    import minimap2_amd as mm
    import synth
    ref_fa, f1, f2, _ = synth.make_rna_pairs(str(tmp_path))
    rn, rs = mm.read_fastx(ref_fa)
    n1, s1 = mm.read_fastx(f1)
    _, s2 = mm.read_fastx(f2)
    f2n = str(tmp_path / "r2_named_as_r1.fa")
    with open(f2n, "wb") as f:
        for nm, s in zip(n1, s2):
            f.write(b">" + nm + b"\n" + s + b"\n")
    want = J.binary_junc(ref_fa, [f1, f2n], "splice:sr")
    J.assert_reference_shapes(want)
    mates = {ln.split(b"\t")[3] for ln in want.split(b"\n") if ln}
    assert len(mates) > 4
    al = mm.Aligner(rs, preset="splice:sr", names=[x.decode() for x in rn], n_threads=4, write_junc=True)
    try:
        pairs = [(nm, a, b) for nm, a, b in zip(n1, s1, s2)]
        host = al.map_pairs(pairs, text=True)
        al.stage(pairs)
        n_reg, reg, rep_len = al.run(raw=True)
        try:
            got, path = al.format_raw(n_reg, reg, rep_len, device=True), al.last_format_path
        finally:
            al.free_raw(n_reg, reg)
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
rn, rs = mm.read_fastx(sys.argv[1])
qn, qs = mm.read_fastx(sys.argv[2])
al = mm.Aligner(rs, preset="splice", names=[x.decode() for x in rn], n_threads=4, write_junc=True)
mm.profile_enable(True)
al.stage(mm.Batch(list(zip(qn, qs))))
n_reg, reg, rep_len = al.run(raw=True)
text = al.format_raw(n_reg, reg, rep_len)
launches = mm.profile_get().get("junc_text_kernel[write]", {}).get("launches", 0)
al.free_raw(n_reg, reg)
al.close()
open(sys.argv[3], "wb").write(text)
print("launches", launches)
"""


@needs_bin
def test_device_text_switch_gives_format_raw_the_same_junctions(spliced, tmp_path):
    """MM2AMD_DEVICE_TEXT=1 routes mm_gpu_format_batch through junc_text_kernel (a child process: the switch is read from the environment); unset,
    the kernel is not launched"""
    ref_fa, reads_fa, want = spliced
    for value, launched in (("1", True), (None, False)):
        env = {k: v for k, v in os.environ.items() if k != "MM2AMD_DEVICE_TEXT"}
        if value is not None:
            env["MM2AMD_DEVICE_TEXT"] = value
        out = str(tmp_path / ("text_%s" % value))
        r = subprocess.run([sys.executable, "-c", CHILD % (ROOT, HERE), ref_fa, reads_fa, out], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=170)
        assert r.returncode == 0, r.stdout.decode()
        assert open(out, "rb").read() == want
        n = int(r.stdout.decode().split("launches")[-1].split()[0])
        assert (n > 0) == launched
