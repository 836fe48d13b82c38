"""Index files from and into the device-built index: mm2amd_idx_dump / mm2amd_idx_load / mm2amd_idx_is_idx / mm2amd_idx_seq, the Aligner's
fn_idx_in / fn_idx_out, against the UNMODIFIED reference (oracle/_ref: `minimap2_ref -d`, mm_idx_str + mm_idx_dump, mm_idx_reader_read).

  1. our file equals the reference's section by section (pairs: ours ascending by key, the reference's in khash slot order -- compared sorted)
  2. the reference binary maps from our file exactly as from its own; its reader's digest of our file equals that of its own
  3. the reference's file, our own, and an --idx-no-seq file load into tables equal to the device-built ones
  4. multi-part files   5. the Aligner's arguments   6. files that must be refused   7. a 100 Mb reference at the default chunk size

The cases run on the emulator as well (MM2AMD_EMU=1), except 7."""
import ctypes as C
import gzip
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
import index_file_cases as X  # noqa: E402
import make_golden as G  # noqa: E402
import mmi_file  # noqa: E402
import reflib  # noqa: E402
import synth  # noqa: E402
import minimap2_amd as mm  # noqa: E402

pytestmark = pytest.mark.gpu
EMU = os.environ.get("MM2AMD_EMU") == "1"
needs_ref = pytest.mark.skipif(not X.HAVE_REF, reason="oracle/_ref absent")


def _fixture(name):
    fa = os.path.join(X.FIX, name)
    names, seqs = mm.read_fastx(fa)
    return names, seqs, fa


def _repeats(tmp):
    """synth.make_repeats's contig (12 copies of a unit) with a 120-copy repeat planted as well, and synth.gen_duplicated_reference's contig"""
    ref, reads = synth.make_repeats(os.path.join(str(tmp), "rep"))
    _, (c1,) = mm.read_fastx(ref)
    rng = np.random.default_rng(17)
    names, seqs = X.repeat_reference(rng)
    names, seqs = [b"c1"] + names + [b"dup"], [c1] + seqs + [synth.ACGT[synth.gen_duplicated_reference(rng, 10, 3000)].tobytes()]
    fa = os.path.join(str(tmp), "repeats.fa")
    X.write_fasta(fa, names, seqs)
    return names, seqs, fa, reads


INPUTS = ["MT-human.fa", "x3s-ref.fa", "repeats"]


def _input(which, tmp):
    if which == "repeats":
        return _repeats(tmp)[:3]
    return _fixture(which)


# ---- 1 ----
@needs_ref
@pytest.mark.parametrize("preset", ["map-ont", "map-hifi", "sr", "hpc"])
@pytest.mark.parametrize("which", INPUTS)
def test_dump_equals_the_reference_file(tmp_path, which, preset):
    names, seqs, fa = _input(which, tmp_path)
    theirs = str(tmp_path / "ref.mmi")
    X.ref_dash_d(fa, theirs, X.PRESET_ARGS[preset])
    if which == "repeats":
        assert X.has_heavy_key(mmi_file.parse_file(theirs)[0]), "the reference's own file must hold a bucket with n > 0 and a key of >= 100 occurrences"
    _, ours = X.dump_and_compare(mm, tmp_path, seqs, names, preset, theirs)
    if which == "repeats":
        assert X.has_heavy_key(ours)


@needs_ref
@pytest.mark.parametrize("b", [14, 10])
def test_dump_without_names_and_with_other_bucket_bits(tmp_path, b):
    """against mm_idx_str + mm_idx_dump called through libminimap2_ref.so with a libc FILE*: no names (MM_I_NO_NAME), and b = 10"""
    names, seqs, _ = _repeats(tmp_path)[:3]
    for nm in (None, names):
        theirs = str(tmp_path / ("str_%d_%s.mmi" % (b, "named" if nm else "anon")))
        X.ref_str_dump(seqs, nm, 15, 10, 0, b, theirs)
        _, ours = X.dump_and_compare(mm, tmp_path, seqs, nm, "map-ont", theirs, b=b, tag="b%d%s" % (b, "n" if nm else "a"))
        assert ours.b == b and bool(ours.flag & 4) == (nm is None)


# ---- 2 ----
@needs_ref
@pytest.mark.parametrize("which", ["mt", "repeats"])
def test_the_reference_maps_from_our_file(tmp_path, which):
    if which == "mt":
        names, seqs, fa = _fixture("MT-human.fa")
        reads = os.path.join(X.FIX, "MT-orang.fa")
    else:
        names, seqs, fa, reads = _repeats(tmp_path)
    theirs = str(tmp_path / "ref.mmi")
    X.ref_dash_d(fa, theirs, X.PRESET_ARGS["map-ont"])
    ours, _ = X.dump_and_compare(mm, tmp_path, seqs, names, "map-ont", theirs, chunks=(None,))
    sam = [subprocess.run([reflib.REF_BIN, "-a", "-x", "map-ont", "-t", "2", idx, reads], check=True, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL).stdout for idx in (ours, theirs)]
    assert sam[0].count(b"\n") > 3 and G.strip_pg(sam[0]) == G.strip_pg(sam[1])
    assert X.ref_digests(mm, ours) == X.ref_digests(mm, theirs)


# ---- 3 ----
@needs_ref
@pytest.mark.parametrize("preset", ["map-ont", "hpc"])
@pytest.mark.parametrize("which", INPUTS)
def test_load_equals_the_built_index(tmp_path, which, preset):
    names, seqs, fa = _input(which, tmp_path)
    theirs, noseq = str(tmp_path / "ref.mmi"), str(tmp_path / "noseq.mmi")
    X.ref_dash_d(fa, theirs, X.PRESET_ARGS[preset])
    X.load_and_compare(mm, theirs, seqs, names, preset)                       # the reference's file
    ours, _ = X.dump_and_compare(mm, tmp_path, seqs, names, preset, theirs, chunks=(4096,))
    X.load_and_compare(mm, ours, seqs, names, preset)                         # round trip
    X.ref_dash_d(fa, noseq, X.PRESET_ARGS[preset] + ["--idx-no-seq"])
    X.load_and_compare(mm, noseq, seqs, names, preset, with_S=False)          # no S section


@needs_ref
def test_index_without_sequence_maps_at_chain_level(tmp_path):
    names, seqs, fa, reads_fa = _repeats(tmp_path)
    noseq, ours = str(tmp_path / "noseq.mmi"), str(tmp_path / "ours_noseq.mmi")
    X.ref_dash_d(fa, noseq, X.PRESET_ARGS["map-ont"] + ["--idx-no-seq"])
    rn, rs = mm.read_fastx(reads_fa)
    reads = list(zip(rn, rs))
    al = mm.Aligner(seq=seqs, names=names, preset="map-ont", cigar=False, n_threads=4)
    try:
        want = [[a.key() for a in h] for h in al.map_batch(reads)]
    finally:
        al.close()
    assert sum(1 for h in want if h) > len(reads) // 2
    al = mm.Aligner(fn_idx_in=noseq, preset="map-ont", cigar=False, n_threads=4, fn_idx_out=ours)
    try:
        assert al.index_stat()["flag"] & mm.I_NO_SEQ
        assert [[a.key() for a in h] for h in al.map_batch(reads)] == want
    finally:
        al.close()
    assert open(ours, "rb").read() != b"" and mmi_file.parse_file(ours)[0].S is None
    X.assert_files_match(ours, noseq)
    with pytest.raises(mm.Mm2AmdError, match="MM_I_NO_SEQ"):
        mm.Aligner(fn_idx_in=noseq, preset="map-ont", cigar=True, n_threads=4).close()
    # without MM2AMD_DUMP_NO_SEQ such an index cannot be written
    h, _ = mm.idx_load(noseq)
    try:
        p = str(tmp_path / "refused.mmi")
        assert mm.lib().mm2amd_idx_dump(h, os.fsencode(p), 0, 0) == mm.EINVAL and not os.path.exists(p)
    finally:
        mm.idx_destroy(h)


# ---- 4 ----
@needs_ref
def test_multi_part_file(tmp_path):
    rng = np.random.default_rng(23)
    contigs = synth.gen_reference(rng, 700000, 7)
    names, seqs = [b"ctg%d" % i for i in range(7)], [synth.ACGT[c].tobytes() for c in contigs]
    fa, multi = str(tmp_path / "multi.fa"), str(tmp_path / "multi.mmi")
    X.write_fasta(fa, names, seqs)
    X.ref_dash_d(fa, multi, ["-x", "map-ont", "-I", "100k"])
    parts = mmi_file.parse_file(multi)
    want = X.ref_digests(mm, multi)
    assert len(parts) >= 3 and len(want) == len(parts)
    seen = []
    for p in range(len(parts)):
        for ch in (None, 4096):
            with X.chunk_env(ch):
                h, more = mm.idx_load(multi, p)
            try:
                assert more == (p < len(parts) - 1)
                st, _, _, keys, val_off, pos, S = X.export(mm, h)
                assert X.flat_digest(keys, val_off, pos) == want[p]
                assert np.array_equal(S, parts[p].S)
                tab = X.seq_table(mm, h)
                assert [t[0] for t in tab] == parts[p].names and [t[1] for t in tab] == parts[p].lens
            finally:
                mm.idx_destroy(h)
        seen += parts[p].names
    assert seen == names
    code, msg = X.load_fails(mm, multi, part=len(parts))
    assert code == mm.EINVAL and "no such part" in msg
    with pytest.raises(mm.Mm2AmdError, match="more than one index part"):
        mm.Aligner(fn_idx_in=multi, preset="map-ont", n_threads=4)
    al = mm.Aligner(fn_idx_in=multi, preset="map-ont", n_threads=4, part=1)
    try:
        assert al.seq_names == [x.decode() for x in parts[1].names]
    finally:
        al.close()


# ---- 5 ----
@needs_ref
def test_aligner_from_files(tmp_path):
    names, seqs, fa, reads_fa = _repeats(tmp_path)
    gz, theirs, out = str(tmp_path / "ref.fa.gz"), str(tmp_path / "ref.mmi"), str(tmp_path / "out.mmi")
    with open(fa, "rb") as f, gzip.open(gz, "wb") as g:
        g.write(f.read())
    X.ref_dash_d(fa, theirs, X.PRESET_ARGS["map-hifi"])
    rn, rs = mm.read_fastx(reads_fa)
    reads = list(zip(rn, rs))[:24]
    results = []
    # the index file was built with map-hifi's k and w: it wins over the preset's, as with the reference's reader -- so every way of giving the reference says k 19, w 19
    for kw in (dict(seq=seqs, names=names, k=19, w=19, fn_idx_out=out), dict(fn_idx_in=fa, k=19, w=19), dict(fn_idx_in=gz, k=19, w=19), dict(fn_idx_in=theirs), dict(fn_idx_in=out)):
        al = mm.Aligner(preset="map-ont", n_threads=4, **kw)
        try:
            assert al.seq_names == [x.decode() for x in names] and al.lens == [len(s) for s in seqs]
            assert (al.idx_opt.k, al.idx_opt.w) == (19, 19)
            results.append([[a.key() for a in h] + [a.ctg for a in h] for h in al.map_batch(reads)])
        finally:
            al.close()
    assert sum(1 for h in results[0] if h) > len(reads) // 2
    assert all(r == results[0] for r in results[1:])
    X.assert_files_match(out, theirs)
    with pytest.raises(mm.Mm2AmdError, match="exactly one"):
        mm.Aligner(seq=seqs, fn_idx_in=fa)
    with pytest.raises(mm.Mm2AmdError, match="exactly one"):
        mm.Aligner(preset="map-ont")


# ---- 6 ----
@needs_ref
def test_bad_files_are_refused(tmp_path):
    names, seqs, fa = _repeats(tmp_path)[:3]
    theirs = str(tmp_path / "ref.mmi")
    X.ref_dash_d(fa, theirs, X.PRESET_ARGS["map-ont"])
    X.check_errors(mm, tmp_path, theirs, seqs, names, "map-ont")
    ours, _ = X.dump_and_compare(mm, tmp_path, seqs, names, "map-ont", theirs, chunks=(None,))
    X.check_errors(mm, tmp_path, ours, seqs, names, "map-ont")


# ---- 7 ----
def scale_reference(rng, total=100 * 1000 * 1000, n_contigs=4):
    """random contigs with planted repeats: a 300-base unit 20 000 times, a 2 kb unit 500 times, a 50 kb segment duplicated"""
    out = []
    per = total // n_contigs
    small, big = rng.integers(0, 4, 300, dtype=np.uint8), rng.integers(0, 4, 2000, dtype=np.uint8)
    for c in range(n_contigs):
        s = rng.integers(0, 4, per, dtype=np.uint8)
        for st in rng.integers(0, per - 300, 5000):
            s[st:st + 300] = small
        for st in rng.integers(0, per - 2000, 125):
            s[st:st + 2000] = big
        s[per // 2:per // 2 + 50000] = s[1000:51000]
        out.append(synth.ACGT[s].tobytes())
    return [b"chr%d" % (i + 1) for i in range(n_contigs)], out


@needs_ref
@pytest.mark.timeout(900)
@pytest.mark.skipif(EMU, reason="hardware only: a 100 Mb reference")
def test_scale_100mb(tmp_path):
    """dump, the reference reader's digest of our file, and load-back, at the default chunk size (several real chunks); prints the figures README / DESIGN.md quote"""
    assert "MM2AMD_IDX_IO_CHUNK" not in os.environ
    names, seqs = scale_reference(np.random.default_rng(41))
    ours = str(tmp_path / "scale.mmi")
    try:
        t0 = time.time()
        h = X.build(mm, seqs, names, 15, 10, 0)
        t_build = time.time() - t0
        try:
            t0 = time.time()
            assert mm.lib().mm2amd_idx_dump(h, os.fsencode(ours), 0, 0) == 0, mm.lib().mm2amd_last_error()
            t_dump, dump_stats = time.time() - t0, mm.idx_io_stats()
            assert dump_stats["n_chunks"] >= 3 and os.path.getsize(ours) > 300 * 1000 * 1000
            st, _, _, keys, val_off, pos, S = X.export(mm, h)
            ncpu = max(2, min(mm.host_cpus(), 16))
            dg = X.ref_digests(mm, ours, ncpu)
            assert dg == [X.flat_digest(keys, val_off, pos, ncpu)]
            assert int(np.diff(val_off).max()) >= 10000  # (the 300-base unit is planted 20 000 times; plants that overlap cost some copies)
            t0 = time.time()
            got, more = mm.idx_load(ours)
            t_load, load_stats = time.time() - t0, mm.idx_io_stats()
            try:
                assert not more
                X.assert_same_index(mm, h, got)
            finally:
                mm.idx_destroy(got)
        finally:
            mm.idx_destroy(h)
        print("IDXFILE " + json.dumps({"case": "scale_100mb", "build_s": round(t_build, 3), "dump_s": round(t_dump, 3), "load_s": round(t_load, 3), "file_bytes": os.path.getsize(ours),
                                       "n_keys": st["n_distinct"], "n_pos": st["n_minimizers"], "dump": dump_stats, "load": load_stats}))
    finally:
        if os.path.exists(ours):
            os.remove(ours)
