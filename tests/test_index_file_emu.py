"""The index-file path (mm2amd_idx_dump / mm2amd_idx_load, index_build.hip) in the CPU suite: the regroup, serialise and unpack kernels' OWN
source under the wave emulator (tests/_build/libmm2amd_emu.so), on the MT fixture and on a 300 kb reference with a 120-copy repeat, with a
chunk size small enough that the section crosses many chunks.  tests/test_gpu_index_file.py runs the full set on the hardware."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import index_file_cases as X  # noqa: E402
import mmi_file  # noqa: E402

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


def _input(emu, which, tmp):
    """(names, seqs, fasta path)"""
    if which == "mt":
        fa = os.path.join(X.FIX, "MT-human.fa")
        names, seqs = emu.read_fastx(fa)
        return names, seqs, fa
    names, seqs = X.repeat_reference(np.random.default_rng(5))
    fa = os.path.join(str(tmp), "rep.fa")
    X.write_fasta(fa, names, seqs)
    return names, seqs, fa


def test_round_trip_without_the_reference(emu, tmp_path):
    """dump, then load: the loaded handle equals the built one, chunk by chunk; the file's content (whatever its order) is the tables'"""
    names, seqs, _ = _input(emu, "rep", tmp_path)
    h = X.build(emu, seqs, names, 15, 10, 0)
    try:
        fn = str(tmp_path / "rt.mmi")
        with X.chunk_env(4096):
            assert emu.lib().mm2amd_idx_dump(h, os.fsencode(fn), 10, 0) == 0, emu.lib().mm2amd_last_error()
            assert emu.idx_io_stats()["n_chunks"] > 10
        P = mmi_file.parse_file(fn)[0]
        assert P.header == (10, 15, 10, 2, 0) and P.names == names and P.lens == [len(s) for s in seqs]
        assert X.has_heavy_key(P)
        st, _, _, keys, val_off, pos, S = X.export(emu, h)
        fh, fp = P.flat()
        assert np.array_equal(fh, np.repeat(keys, np.diff(val_off).astype(np.int64))) and np.array_equal(fp, pos) and np.array_equal(P.S, S)
    finally:
        emu.lib().mm2amd_idx_destroy(h)
    X.load_and_compare(emu, fn, seqs, names, "map-ont")


@needs_ref
@pytest.mark.parametrize("which", ["mt", "rep"])
def test_dump_equals_the_reference_file(emu, tmp_path, which):
    names, seqs, fa = _input(emu, which, tmp_path)
    theirs = str(tmp_path / "ref.mmi")
    X.ref_dash_d(fa, theirs, X.PRESET_ARGS["map-ont"])
    if which == "rep":
        assert X.has_heavy_key(mmi_file.parse_file(theirs)[0]), "the input must have a key of 100 occurrences in the reference's own file"
    ours, _ = X.dump_and_compare(emu, tmp_path, seqs, names, "map-ont", theirs)
    assert X.ref_digests(emu, ours) == X.ref_digests(emu, theirs)


@needs_ref
@pytest.mark.parametrize("which", ["mt", "rep"])
def test_load_of_the_reference_file_equals_the_built_index(emu, tmp_path, which):
    names, seqs, fa = _input(emu, which, tmp_path)
    theirs, noseq = str(tmp_path / "ref.mmi"), str(tmp_path / "noseq.mmi")
    X.ref_dash_d(fa, theirs, X.PRESET_ARGS["map-ont"])
    X.load_and_compare(emu, theirs, seqs, names, "map-ont")
    X.ref_dash_d(fa, noseq, X.PRESET_ARGS["map-ont"] + ["--idx-no-seq"])
    X.load_and_compare(emu, noseq, seqs, names, "map-ont", with_S=False)


@needs_ref
def test_bad_files_are_refused(emu, tmp_path):
    names, seqs, fa = _input(emu, "rep", tmp_path)
    theirs = str(tmp_path / "ref.mmi")
    X.ref_dash_d(fa, theirs, X.PRESET_ARGS["map-ont"])
    with X.chunk_env(4096):
        X.check_errors(emu, tmp_path, theirs, seqs, names, "map-ont")


def test_index_tool(emu, tmp_path, capsys):
    """tools/mm2amd_index.py, the counterpart of `minimap2 -d`: FASTA (gzip) in, .mmi out, one JSON line of phase times"""
    import gzip
    import importlib.util
    import json
    spec = importlib.util.spec_from_file_location("mm2amd_index_tool", os.path.join(ROOT, "tools", "mm2amd_index.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    names, seqs, fa = _input(emu, "rep", tmp_path)
    gz, out = str(tmp_path / "rep.fa.gz"), str(tmp_path / "tool.mmi")
    with open(fa, "rb") as f, gzip.open(gz, "wb") as g:
        g.write(f.read())
    assert tool.main(["-x", "map-hifi", "-H", "--json", "--load-back", "-d", out, gz]) == 0
    res = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert (res["k"], res["w"], res["hpc"], res["n_seq"]) == (19, 19, 1, 2) and res["file_bytes"] == os.path.getsize(out)
    for key in ("read_parse_s", "device_build_s", "regroup_s", "serialise_s", "d2h_s", "file_write_s", "total_s", "load_s"):
        assert res[key] >= 0
    P = mmi_file.parse_file(out)[0]
    assert P.header == (19, 19, 14, 2, 1) and P.names == names
    assert tool.main(["-x", "map-ont", "--no-seq", "-d", out, fa]) == 0
    assert mmi_file.parse_file(out)[0].S is None
    if X.HAVE_REF:
        theirs = str(tmp_path / "theirs.mmi")
        X.ref_dash_d(fa, theirs, ["-x", "map-ont", "--idx-no-seq"])
        X.assert_files_match(out, theirs)
