"""Checks of the index-file entry points (mm2amd_idx_dump / _load / _is_idx / _seq) shared by tests/test_gpu_index_file.py (the hardware, or
the emulator with MM2AMD_EMU=1) and tests/test_index_file_emu.py (the CPU suite's share): every function takes the minimap2_amd module whose
library is under test.  The reference side is the UNMODIFIED reference: oracle/_ref/minimap2_ref -d, and mm_idx_str + mm_idx_dump /
mm_idx_reader_read through oracle/_ref/libminimap2_ref.so."""
import ctypes as C
import os
import subprocess

import numpy as np

import mmi_file
import reflib

HERE = os.path.dirname(os.path.abspath(__file__))
FIX = os.path.join(HERE, "golden", "ref_fixtures")
HAVE_REF = os.path.exists(reflib.REF_BIN) and os.path.exists(reflib.REF_SO) and os.path.exists(reflib.REFDRV_SO)
PRESETS = {"map-ont": (15, 10, 0), "map-hifi": (19, 19, 0), "sr": (21, 11, 0), "hpc": (15, 10, 1)}  # k, w, is_hpc ("hpc": map-ont with -H)
PRESET_ARGS = {"map-ont": ["-x", "map-ont"], "map-hifi": ["-x", "map-hifi"], "sr": ["-x", "sr"], "hpc": ["-x", "map-ont", "-H"]}


class chunk_env(object):
    """MM2AMD_IDX_IO_CHUNK for the duration of a with block (None: the default chunk size)"""

    def __init__(self, chunk):
        self.chunk = chunk

    def __enter__(self):
        self.saved = os.environ.pop("MM2AMD_IDX_IO_CHUNK", None)
        if self.chunk is not None:
            os.environ["MM2AMD_IDX_IO_CHUNK"] = str(self.chunk)

    def __exit__(self, *a):
        os.environ.pop("MM2AMD_IDX_IO_CHUNK", None)
        if self.saved is not None:
            os.environ["MM2AMD_IDX_IO_CHUNK"] = self.saved


# ---- our side ----
def build(mm, seqs, names, k, w, hpc):
    """mm2amd_idx_str; names None: an index without names"""
    n = len(seqs)
    sarr = (C.c_char_p * n)(*seqs)
    narr = (C.c_char_p * n)(*names) if names is not None else None
    h = mm.lib().mm2amd_idx_str(w, k, hpc, 14, n, sarr, narr)
    assert h, mm.lib().mm2amd_last_error()
    return h


def stat(mm, h):
    k, w, flag, n_seq = C.c_int(), C.c_int(), C.c_int(), C.c_uint32()
    sl, nd, nm = C.c_uint64(), C.c_uint64(), C.c_uint64()
    assert mm.lib().mm2amd_idx_stat(h, k, w, flag, n_seq, sl, nd, nm) == 0
    return {"k": k.value, "w": w.value, "flag": flag.value, "n_seq": n_seq.value, "sum_len": sl.value, "n_distinct": nd.value, "n_minimizers": nm.value}


def export(mm, h, with_S=True):
    """(stat, shape, bucket_start, keys, val_off, pos, S) of a handle"""
    st = stat(mm, h)
    bb, ks = C.c_int(), C.c_int()
    assert mm.lib().mm2amd_idx_table_shape(h, bb, ks) == 0
    bucket_start = np.zeros((1 << bb.value) + 1, np.uint32)
    keys = np.zeros(st["n_distinct"], np.uint64)
    val_off = np.zeros(st["n_distinct"] + 1, np.uint32)
    pos = np.zeros(st["n_minimizers"], np.uint64)
    S = np.zeros((st["sum_len"] + 7) // 8, np.uint32) if with_S else None
    rc = mm.lib().mm2amd_idx_export(h, bucket_start.ctypes.data, keys.ctypes.data, val_off.ctypes.data, pos.ctypes.data, S.ctypes.data if with_S else None)
    assert rc == 0, mm.lib().mm2amd_last_error()
    return st, (bb.value, ks.value), bucket_start, keys, val_off, pos, S


def assert_same_index(mm, h1, h2, with_S=True, ignore_flag=0):
    a, b = export(mm, h1, with_S), export(mm, h2, with_S)
    sa, sb = dict(a[0]), dict(b[0])
    sa["flag"] &= ~ignore_flag
    sb["flag"] &= ~ignore_flag
    assert sa == sb
    assert a[1] == b[1]
    for x, y, what in zip(a[2:], b[2:], ("bucket_start", "keys", "val_off", "pos", "S")):
        if x is not None:
            assert np.array_equal(x, y), what
    return a


def seq_table(mm, h):
    st = stat(mm, h)
    nm, ln = C.c_char_p(), C.c_uint32()
    out = []
    for i in range(st["n_seq"]):
        assert mm.lib().mm2amd_idx_seq(h, i, C.byref(nm), C.byref(ln)) == 0
        out.append((nm.value, ln.value))
    return out


def load_fails(mm, fn, part=0):
    """mm2amd_idx_load must refuse the file; returns (code, message)"""
    more = C.c_int(0)
    h = mm.lib().mm2amd_idx_load(os.fsencode(fn), part, C.byref(more))
    if h:
        mm.lib().mm2amd_idx_destroy(h)
    assert not h, "a bad file was loaded"
    return mm.lib().mm2amd_last_error_code(), mm.lib().mm2amd_last_error().decode()


# ---- the reference's side ----
def ref_dash_d(fa, mmi, args):
    subprocess.run([reflib.REF_BIN] + list(args) + ["-t", "2", "-d", mmi, fa], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)


_R = None


def _ref():
    global _R
    if _R is None:
        R = C.CDLL(reflib.REF_SO)
        R.mm_idx_str.restype = C.c_void_p
        R.mm_idx_str.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_char_p)]
        R.mm_idx_dump.argtypes = [C.c_void_p, C.c_void_p]
        R.mm_idx_dump.restype = None
        R.mm_idx_destroy.argtypes = [C.c_void_p]
        R.mm_idx_destroy.restype = None
        R.mm_idx_reader_open.restype = C.c_void_p
        R.mm_idx_reader_open.argtypes = [C.c_char_p, C.c_void_p, C.c_char_p]
        R.mm_idx_reader_read.restype = C.c_void_p
        R.mm_idx_reader_read.argtypes = [C.c_void_p, C.c_int]
        R.mm_idx_reader_close.argtypes = [C.c_void_p]
        R.mm_idx_reader_close.restype = None
        _R = R
    return _R


def ref_str_dump(seqs, names, k, w, hpc, b, out):
    """mm_idx_str + mm_idx_dump of the reference, through a libc FILE*"""
    R, libc = _ref(), C.CDLL(None)
    libc.fopen.restype = C.c_void_p
    libc.fopen.argtypes = [C.c_char_p, C.c_char_p]
    libc.fclose.argtypes = [C.c_void_p]
    n = len(seqs)
    sarr = (C.c_char_p * n)(*seqs)
    narr = (C.c_char_p * n)(*names) if names is not None else None
    mi = R.mm_idx_str(w, k, hpc, b, n, sarr, narr)
    assert mi
    fp = libc.fopen(os.fsencode(out), b"wb")
    assert fp
    R.mm_idx_dump(fp, mi)
    libc.fclose(fp)
    R.mm_idx_destroy(mi)


def ref_digests(mm, fn, n_threads=2):
    """refdrv_idx_digest of every part mm_idx_reader_read returns for the file: [[sum, n_keys, n_pos], ...]"""
    R, D = _ref(), C.CDLL(reflib.REFDRV_SO)
    D.refdrv_idx_digest.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    io, mo = mm.IdxOpt(), mm.MapOpt()
    R.mm_set_opt(None, C.byref(io), C.byref(mo))
    rd = R.mm_idx_reader_open(os.fsencode(fn), C.byref(io), None)
    assert rd
    out = []
    while True:
        mi = R.mm_idx_reader_read(rd, n_threads)
        if not mi:
            break
        dg = (C.c_uint64 * 3)()
        D.refdrv_idx_digest(mi, n_threads, dg)
        out.append(list(dg))
        R.mm_idx_destroy(mi)
    R.mm_idx_reader_close(rd)
    return out


def flat_digest(keys, val_off, pos, n_threads=2):
    D = C.CDLL(reflib.REFDRV_SO)
    D.refdrv_flat_digest.argtypes = [C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    dg = (C.c_uint64 * 3)()
    D.refdrv_flat_digest(len(keys), keys.ctypes.data, val_off.ctypes.data, pos.ctypes.data, n_threads, dg)
    return list(dg)


# ---- check 1: our file against the reference's, section by section ----
def assert_files_match(ours, theirs):
    """magic + header, names, per bucket n / p / size, S: byte-identical; pairs: ours ascending by key, equal to the reference's once those are sorted.
    Returns (our parts, the reference's parts)."""
    A, B = mmi_file.parse_file(ours), mmi_file.parse_file(theirs)
    assert len(A) == len(B) == 1
    a, b = A[0], B[0]
    assert a.header == b.header
    assert a.names == b.names and a.lens == b.lens
    assert a.n == b.n, "per-bucket n"
    assert a.size == b.size, "per-bucket size"
    for bk in range(1 << a.b):
        assert np.array_equal(a.p[bk], b.p[bk]), "p of bucket %d" % bk
        if a.size[bk]:
            assert np.all(a.keys[bk][1:] > a.keys[bk][:-1]), "our keys of bucket %d are not ascending" % bk
            k, v = b.sorted_pairs(bk)
            assert np.array_equal(a.keys[bk], k) and np.array_equal(a.vals[bk], v), "pairs of bucket %d" % bk
    assert (a.S is None) == (b.S is None)
    if a.S is not None:
        assert np.array_equal(a.S, b.S)
    assert os.path.getsize(ours) == os.path.getsize(theirs)
    return a, b


def dump_and_compare(mm, tmp, seqs, names, preset, theirs, chunks=(None, 4096), b=0, tag="x"):
    """our dump of (seqs, names) under `preset`, with each chunk size, against the reference's file `theirs`; returns our last file"""
    k, w, hpc = PRESETS[preset]
    h = build(mm, seqs, names, k, w, hpc)
    try:
        for ch in chunks:
            ours = os.path.join(str(tmp), "ours_%s_%s_%s.mmi" % (tag, preset, ch))
            with chunk_env(ch):
                rc = mm.lib().mm2amd_idx_dump(h, os.fsencode(ours), b, 0)
            assert rc == 0, mm.lib().mm2amd_last_error()
            assert mm.lib().mm2amd_idx_is_idx(os.fsencode(ours)) == 1
            if ch is not None:
                assert mm.idx_io_stats()["n_chunks"] > 1, "the small chunk size must give several chunks"
            a, _ = assert_files_match(ours, theirs)
    finally:
        mm.lib().mm2amd_idx_destroy(h)
    return ours, a


def has_heavy_key(part, min_occ=100):
    """a bucket with n > 0, and some key with at least min_occ occurrences"""
    if not any(n > 0 for n in part.n):
        return False
    for bk in range(1 << part.b):
        k, v = part.keys[bk], part.vals[bk]
        multi = (k & np.uint64(1)) == 0
        if multi.any() and int((v[multi] & np.uint64(0xffffffff)).max()) >= min_occ:
            return True
    return False


def repeat_reference(rng, total=300000, unit_len=1500, copies=120):
    """a random contig with `copies` identical copies of one unit (every minimizer of the unit occurs that often) and a second, plain contig"""
    c = rng.integers(0, 4, total, dtype=np.uint8)
    unit = rng.integers(0, 4, unit_len, dtype=np.uint8)
    step = (total - unit_len) // copies
    for i in range(copies):
        c[i * step:i * step + unit_len] = unit
    d = rng.integers(0, 4, total // 6, dtype=np.uint8)
    A = np.frombuffer(b"ACGT", np.uint8)
    return [b"rep1", b"plain2"], [A[c].tobytes(), A[d].tobytes()]


def write_fasta(fn, names, seqs, width=70):
    with open(fn, "wb") as f:
        for nm, s in zip(names, seqs):
            f.write(b">" + nm + b" some comment\n")
            for i in range(0, len(s), width):
                f.write(s[i:i + width] + b"\n")


# ---- check 3: load ----
def load_and_compare(mm, fn, seqs, names, preset, chunks=(None, 4096), with_S=True):
    """mm2amd_idx_load(fn) against mm2amd_idx_str on the same sequences: stat and every exported array equal"""
    k, w, hpc = PRESETS[preset]
    want = build(mm, seqs, names, k, w, hpc)
    try:
        for ch in chunks:
            with chunk_env(ch):
                got, more = mm.idx_load(fn)
            try:
                assert not more
                assert_same_index(mm, want, got, with_S=with_S, ignore_flag=0 if with_S else mmi_file.NO_SEQ)
                assert seq_table(mm, got) == [(nm if names is not None else None, len(s)) for nm, s in zip(names or [None] * len(seqs), seqs)]
            finally:
                mm.lib().mm2amd_idx_destroy(got)
    finally:
        mm.lib().mm2amd_idx_destroy(want)


# ---- check 6: files that must be refused ----
def truncation_offsets(part, n=20):
    """n deterministic cut points spread over every section of a one-part file: header, name table, bucket headers, p arrays, pairs, S"""
    cuts = [2, 4, 13, 23, 24 + 1, part.sec_start - 2, part.sec_start, part.sec_start + 3]
    full = [bk for bk in range(1 << part.b) if part.n[bk] > 0] or [bk for bk in range(1 << part.b) if part.size[bk] > 0]
    for bk in (full[0], full[len(full) // 2], full[-1]):
        o = part.bucket_off[bk]
        cuts += [o + 2, o + 4 + 8 * part.n[bk] - 3, o + 4 + 8 * part.n[bk] + 2, o + 8 + 8 * part.n[bk] + 16 * part.size[bk] - 5]
    cuts += [part.sec_end - 1, part.sec_end, part.sec_end + (part.end - part.sec_end) // 2, part.end - 1]
    cuts = sorted(set(c for c in cuts if 0 <= c < part.end))
    assert len(cuts) >= n, cuts
    step = len(cuts) / float(n)
    return [cuts[int(i * step)] for i in range(n)]


def corrupt_copies(fn, tmp):
    """{what: path}: copies of a good one-part file (which must hold a bucket with two multi-occurrence keys), each with one defect"""
    buf = bytearray(open(fn, "rb").read())
    P = mmi_file.parse_part(bytes(buf))
    out = {}

    def save(what, b):
        p = os.path.join(str(tmp), "bad_%s.mmi" % what)
        open(p, "wb").write(bytes(b))
        out[what] = p

    b = bytearray(buf)
    b[0:4] = b"MMI\1"
    save("magic", b)
    # a bucket with at least two keys, one of them with several positions
    bk = next(i for i in range(1 << P.b) if P.size[i] >= 2 and P.n[i] >= 2)
    pairs = P.bucket_off[bk] + 8 + 8 * P.n[bk]
    multi = next(j for j in range(P.size[bk]) if not int(P.keys[bk][j]) & 1)
    b = bytearray(buf)  # two equal keys: the second pair's key becomes the first's
    b[pairs + 16:pairs + 24] = b[pairs:pairs + 8]
    save("duplicate_key", b)
    b = bytearray(buf)  # a swapped position pair inside a key's run
    st = int(P.vals[bk][multi]) >> 32
    o = P.bucket_off[bk] + 4 + 8 * st
    b[o:o + 8], b[o + 8:o + 16] = b[o + 8:o + 16], b[o:o + 8]
    save("swapped_positions", b)
    b = bytearray(buf)  # start_p beyond the bucket's n
    v = (P.n[bk] << 32) | (int(P.vals[bk][multi]) & 0xffffffff)
    b[pairs + 16 * multi + 8:pairs + 16 * multi + 16] = int(v).to_bytes(8, "little")
    save("start_p_beyond_n", b)
    b = bytearray(buf)  # a count of zero
    v = (int(P.vals[bk][multi]) >> 32) << 32
    b[pairs + 16 * multi + 8:pairs + 16 * multi + 16] = int(v).to_bytes(8, "little")
    save("zero_count", b)
    b = bytearray(buf)  # a bucket count larger than the file
    b[P.bucket_off[bk]:P.bucket_off[bk] + 4] = (0x7fffffff).to_bytes(4, "little")
    save("huge_n", b)
    b = bytearray(buf)  # a sequence count larger than the file
    b[16:20] = (0xfffffff0).to_bytes(4, "little")
    save("huge_n_seq", b)
    return out


def check_errors(mm, tmp, good, seqs, names, preset):
    """check 6 on the good one-part file `good` (ours or the reference's)"""
    L = mm.lib()
    k, w, hpc = PRESETS[preset]
    h = build(mm, seqs, names, k, w, hpc)
    try:
        # an unwritable path
        nowhere = os.path.join(str(tmp), "no_such_dir", "x.mmi")
        assert L.mm2amd_idx_dump(h, os.fsencode(nowhere), 0, 0) == mm.EIO
        assert "No such file" in L.mm2amd_last_error().decode()
        assert not os.path.exists(nowhere)
        # bucket bits the format or the index cannot hold
        for bad_b in (29, 2 * k + 1):
            p = os.path.join(str(tmp), "bad_b.mmi")
            assert L.mm2amd_idx_dump(h, os.fsencode(p), bad_b, 0) == mm.EINVAL
            assert not os.path.exists(p)
    finally:
        L.mm2amd_idx_destroy(h)
    # a name of 300 bytes
    h = build(mm, seqs[:1], [b"n" * 300], k, w, hpc)
    try:
        p = os.path.join(str(tmp), "long_name.mmi")
        assert L.mm2amd_idx_dump(h, os.fsencode(p), 0, 0) == mm.EINVAL
        assert "255" in L.mm2amd_last_error().decode()
        assert not os.path.exists(p)
    finally:
        L.mm2amd_idx_destroy(h)
    # not an index / no such file
    fa = os.path.join(str(tmp), "plain.fa")
    write_fasta(fa, [b"a"], [b"ACGT" * 10])
    assert L.mm2amd_idx_is_idx(os.fsencode(fa)) == 0
    assert L.mm2amd_idx_is_idx(os.fsencode(os.path.join(str(tmp), "missing.mmi"))) < 0
    code, msg = load_fails(mm, os.path.join(str(tmp), "missing.mmi"))
    assert code == mm.EIO, msg
    # defects
    for what, p in sorted(corrupt_copies(good, tmp).items()):
        for ch in (None, 4096):
            with chunk_env(ch):
                code, msg = load_fails(mm, p)
            assert code == mm.EINVAL and msg, (what, code, msg)
    # a file cut at 20 offsets spread over every section
    data = open(good, "rb").read()
    P = mmi_file.parse_part(data)
    cut = os.path.join(str(tmp), "cut.mmi")
    for off in truncation_offsets(P):
        open(cut, "wb").write(data[:off])
        code, msg = load_fails(mm, cut)
        assert code == mm.EINVAL and msg, (off, code, msg)
    # a part beyond the last
    code, msg = load_fails(mm, good, part=1)
    assert code == mm.EINVAL and "no such part" in msg, msg
    # the library is still usable
    load_and_compare(mm, good, seqs, names, preset, chunks=(None,))
