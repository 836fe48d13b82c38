"""The readers' cases: FASTA / FASTQ text into sequence records (mm2amd_fastx_parse: fastx_lines_kernel, fastx_classify_kernel, fastx_copy_kernel;
mm2amd_fastx_parse_host: the host's parser) and the batches of minimap2_amd.FastxReader.  The judge is the UNMODIFIED compiled reference --
mm_bseq_open / mm_bseq_read3 / mm_bseq_read_frag2 / mm_bseq_close of oracle/_ref/libminimap2_ref.so on a temporary file.  tests/test_fastx_emu.py
runs the checks on the kernels' own source under the wave emulator, tests/test_gpu_fastx.py on the hardware.

FALLBACK RULE: every case meant for the device asserts that `path` is FASTQ4 or FASTA; a fall-back to the host never makes a device case pass."""
import ctypes as C
import gzip
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import reflib  # noqa: E402
import synth  # noqa: E402

HAVE_REF = os.path.exists(reflib.REF_SO)
HAVE_BIN = os.path.exists(reflib.REF_BIN)
FIXTURES = os.path.join(HERE, "golden", "ref_fixtures")
TILE = 4096  # kFastxTile: the lines kernel's tile
LENGTHS = [1, 2, 15, 16, 17, 63, 64, 65, 255, 256, 257, TILE - 1, TILE, TILE + 1]
HOST, FASTQ4, FASTA = 0, 1, 2

_R = None


def _ref():
    global _R
    if _R is None:
        import minimap2_amd as mm
        R = C.CDLL(reflib.REF_SO)
        R.mm_bseq_open.restype = C.c_void_p
        R.mm_bseq_open.argtypes = [C.c_char_p]
        R.mm_bseq_close.argtypes = [C.c_void_p]
        R.mm_bseq_read3.restype = C.POINTER(mm.Bseq1)
        R.mm_bseq_read3.argtypes = [C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)]
        R.mm_bseq_read_frag2.restype = C.POINTER(mm.Bseq1)
        R.mm_bseq_read_frag2.argtypes = [C.c_int, C.POINTER(C.c_void_p), C.c_int64, C.c_int, C.c_int, C.POINTER(C.c_int)]
        _R = R
    return _R


def _take(arr, n):
    """the records of a reference batch as (name, comment | None, seq, qual | None), freed afterwards"""
    libc = C.CDLL(None)
    libc.free.argtypes = [C.c_void_p]
    out = []
    for k in range(n):
        r = arr[k]
        assert r.l_seq == len(r.seq)
        out.append((r.name, r.comment, r.seq, r.qual))
    raw = C.cast(arr, C.POINTER(C.c_void_p * 5))  # l_seq + rid, then the four strings
    for k in range(n):
        for j in range(1, 5):
            if raw[k][j]:
                libc.free(raw[k][j])
    if n:
        libc.free(C.cast(arr, C.c_void_p))
    return out


def ref_batches(files, chunk=500000000, with_qual=True, with_comment=False, frag_mode=False):
    """the batches of successive mm_bseq_read3 (one file) / mm_bseq_read_frag2 (several) calls, up to the first that returns nothing -- where
    the reference's pipeline stops reading (map.c:553,573)"""
    R = _ref()
    files = [files] if isinstance(files, str) else list(files)
    fps = [R.mm_bseq_open(os.fsencode(f)) for f in files]
    assert all(fps)
    out, n = [], C.c_int(0)
    try:
        while True:
            if len(fps) == 1:
                arr = R.mm_bseq_read3(fps[0], chunk, int(with_qual), int(with_comment), int(frag_mode), C.byref(n))
            else:
                arr = R.mm_bseq_read_frag2(len(fps), (C.c_void_p * len(fps))(*fps), chunk, int(with_qual), int(with_comment), C.byref(n))
            if n.value == 0:
                return out
            out.append(_take(arr, n.value))
    finally:
        for fp in fps:
            R.mm_bseq_close(fp)


def ref_records(data, with_qual=True, with_comment=False, tmp=None):
    """every record the reference reads from a file holding `data`, batches joined: a malformed record ends a batch and the next call reads on, so the
    calls go on until one returns nothing at the end of the file"""
    R = _ref()
    with tempfile.NamedTemporaryFile(dir=tmp, suffix=".fx", delete=False) as f:
        f.write(data)
    try:
        fp = R.mm_bseq_open(os.fsencode(f.name))
        out, n = [], C.c_int(0)
        R.mm_bseq_eof.argtypes = [C.c_void_p]
        while True:  # (an empty batch before the end: a malformed record with nothing in front of it)
            arr = R.mm_bseq_read3(fp, 500000000, int(with_qual), int(with_comment), 0, C.byref(n))
            out += _take(arr, n.value)
            if n.value == 0 and R.mm_bseq_eof(fp):
                break
        R.mm_bseq_close(fp)
        return out
    finally:
        os.unlink(f.name)


def device_records(mm, data, with_qual=True, with_comment=False, want=None, is_final=True):
    recs, used, path = mm.parse_fastx(data, is_final, with_qual, with_comment, device=True)
    if want is not None:
        assert path == want, "class %d, expected %d for %r" % (path, want, bytes(data[:60]))
    return recs, used


def host_records(mm, data, with_qual=True, with_comment=False, is_final=True):
    recs, used, path = mm.parse_fastx(data, is_final, with_qual, with_comment, device=False)
    assert path == HOST
    return recs, used


def both_equal_reference(mm, data, want, flags=((True, False), (False, True), (True, True), (False, False))):
    for wq, wc in flags:
        ref = ref_records(data, wq, wc)
        dev, used = device_records(mm, data, wq, wc, want)
        assert dev == ref, (data[:80], wq, wc, dev[:3], ref[:3])
        assert used == len(data)
        host, used = host_records(mm, data, wq, wc)
        assert host == ref, (data[:80], wq, wc, host[:3], ref[:3])
        assert used == len(data)


# ---------------------------------------------------------------------------------------------------------------------------------------------
DIRECTED = [
    # (text, class, the records the issue's author saw the compiled reference return -- or None: the reference alone decides)
    (b"@r1 c x\r\nACGU\r\n+\r\nIIII\r\n@r2\tz\nA\n+r2\n@\n", FASTQ4, [(b"r1", b"c x", b"ACGT", b"IIII"), (b"r2", b"z", b"A", b"@")]),
    (b">a\nAC\n\nGT\r\nuu\n>b desc  \n>c\nN", FASTA, [(b"a", None, b"ACGTtt", None), (b"b", b"desc  ", b"", None), (b"c", None, b"N", None)]),
    (b"@e\n\n+\n\n@f\nAC\n+\nII", HOST, [(b"e", None, b"", None), (b"f", None, b"AC", b"II")]),
    (b"@e\r\n\r\n+\r\n\r\n@f\r\nAC\r\n+\r\nII\r\n", HOST, None),
    (b"@e\r\n\r\n+\r\n\r\n", HOST, [(b"e", None, b"\r", b"\r")]),
    (b"junk\n>a\nAC\n@b\nGG\n+\n@@\n", HOST, [(b"a", None, b"AC", None), (b"b", None, b"GG", b"@@")]),
    (b"ju>nk\n>a\nAC\n", HOST, None),
    (b"@q\nAC\nGT\n+\nII\nII\n>z\nA\n", HOST, [(b"q", None, b"ACGT", b"IIII"), (b"z", None, b"A", None)]),
    (b"@t\nACGT\n+\nII\n@u\nAC\n+\nII\n", HOST, [(b"t", None, b"ACGT", b"II@u")]),
    # the two rules read from the code
    (b"@r1\r\nAC\r\n+\r\nII\r\n", FASTQ4, None),
    (b"@r1 \r\nAC\r\n+\r\nII\r\n", FASTQ4, None),
    (b">r1\r\nAC\r\n", FASTA, None),
    (b">r1 \r\nAC\r\n", FASTA, None),
    # an empty name; a header alone; a file that ends inside a record
    (b">\nAC\n> c\nGG\n", FASTA, None),
    (b"@\nAC\n+\nII\n", FASTQ4, None),
    (b">a", FASTA, None),
    (b">a\n>", HOST, None),
    (b">", HOST, None),
    (b">a\nAC\n\r\nGT\n", HOST, None),
    (b">a\n\r\nGT\n", HOST, None),
    (b">a\nAC\n\r", HOST, None),
    (b"@a\nAC\n+\n", HOST, None),
    (b"@a\nAC\n+", HOST, None),
    (b"@a\nAC\n", HOST, None),
    (b"@a\nAC\n+\nII\n@b\nAC\n+\nIII\n@c\nA\n+\nI\n", HOST, None),
    (b"@a\nAC\n+\nI\n", HOST, None),
    (b"@a\nA\r\r\n+\nI\r\r\n", FASTQ4, None),
    (b"@a\nA\r\r\n+\nI\r\n", HOST, None),
    (b"@a\nA\n+\n\r\n", FASTQ4, None),
    (b">a\nAC\n+\nGG\n", HOST, None),
    (b">a\nAC\n@b\nGG\n", HOST, None),
    (b"\n>a\nAC\n", HOST, None),
    (b"no record at all\n", HOST, None),
] + [(b">n" + sp + b"rest x\nACGT\n", FASTA, None) for sp in (b" ", b"\t", b"\v", b"\f", b"\r")] + [(b"@n" + sp + b"rest x\nACGT\n+\nIIII\n", FASTQ4, None) for sp in (b" ", b"\t", b"\v", b"\f", b"\r")] \
  + [(b">n\nACGT\n", FASTA, None), (b"@n\nACGT\n+\nIIII", FASTQ4, None)]


def check_directed(mm):
    for data, want, seen in DIRECTED:
        if seen is not None:
            assert ref_records(data, True, True) == seen, (data, ref_records(data, True, True))
        both_equal_reference(mm, data, want)
    # the batches of the issue: chunk_size 5 gives [a, b] and [c]; chunk_size 1 with frag_mode keeps the pairs together
    with tempfile.TemporaryDirectory() as d:
        fa, fq = os.path.join(d, "a.fa"), os.path.join(d, "p.fq")
        open(fa, "wb").write(b">a\nACGT\n>b\nAC\n>c\nA\n")
        open(fq, "wb").write(b"".join(b"@%s\nACGT\n+\nIIII\n" % nm for nm in (b"a/1", b"a/2", b"b/1", b"b/2")))
        assert [[r[0] for r in b] for b in ref_batches(fa, 5)] == [[b"a", b"b"], [b"c"]]
        assert [[r[0] for r in b] for b in ref_batches(fq, 1, frag_mode=True)] == [[b"a/1", b"a/2"], [b"b/1", b"b/2"]]
        for dev in (True, False):
            assert [[r[0] for r in b] for b in reader_batches(mm, fa, chunk_bases=5, device=dev)[0]] == [[b"a", b"b"], [b"c"]]
            assert [[r[0] for r in b] for b in reader_batches(mm, fq, chunk_bases=1, frag_mode=True, device=dev)[0]] == [[b"a/1", b"a/2"], [b"b/1", b"b/2"]]


# ---------------------------------------------------------------------------------------------------------------------------------------------
def _seq(rng, n, alphabet=b"ACGTNacgtnUu"):
    return bytes(np.frombuffer(alphabet, dtype=np.uint8)[rng.integers(0, len(alphabet), n)])


def _qual(rng, n):
    return bytes(rng.integers(33, 127, n, dtype=np.uint8))  # ('@', '+' and '>' included: a quality line may begin with any of them)


def fastq4(rng, lens, eol=b"\n", last_eol=True, comments=True):
    out = []
    for i, n in enumerate(lens):
        head = b"@r%d" % i + (b" c%d x" % i if comments and i % 3 == 0 else b"\tt" if comments and i % 3 == 1 else b"")
        out.append(head + eol + _seq(rng, n) + eol + (b"+" if i % 2 else b"+r%d" % i) + eol + _qual(rng, n) + eol)
    data = b"".join(out)
    return data if last_eol else data[:len(data) - len(eol)]


def fasta(rng, lens, width, eol=b"\n", last_eol=True, empty_lines=False):
    """width: the line width, or a callable giving each line's"""
    out = []
    for i, n in enumerate(lens):
        out.append(b">s%d" % i + (b" d%d  " % i if i % 2 == 0 else b"") + eol)
        s, p = _seq(rng, n), 0
        while p < n:
            w = width(rng) if callable(width) else width
            out.append(s[p:p + w] + eol)
            p += w
            if empty_lines and eol == b"\n" and rng.integers(0, 4) == 0:
                out.append(eol)
    data = b"".join(out)
    return data if last_eol else data[:len(data) - len(eol)]


def _at_alignment(data, a):
    """the same bytes in a buffer whose address is `a` modulo 16"""
    raw = np.empty(len(data) + 32, dtype=np.uint8)
    off = (a - raw.ctypes.data) % 16
    view = raw[off:off + len(data)]
    view[:] = np.frombuffer(data, dtype=np.uint8)
    assert view.ctypes.data % 16 == a
    return view


def check_line_shapes(mm):
    """line payloads of every length around the vector, the wavefront, the short-class loop and the lines kernel's tile; the text at each of the 16
    alignments; LF and CRLF; the last newline present and missing; a single record; records across every tile boundary"""
    rng = np.random.default_rng(11)
    a = 0
    for eol in (b"\n", b"\r\n"):
        for last_eol in (True, False):
            fq, fa = fastq4(rng, LENGTHS, eol, last_eol), _fasta_of_widths(rng, LENGTHS, eol, last_eol)
            ref_q, ref_a = ref_records(fq), ref_records(fa)
            assert [len(r[2]) for r in ref_q] == LENGTHS
            for _ in range(8):  # (the 16 alignments, over the four line-end combinations and the two classes)
                got, used = device_records(mm, _at_alignment(fq, a % 16), want=FASTQ4)
                assert got == ref_q and used == len(fq), (a % 16, eol, last_eol)
                got, used = device_records(mm, _at_alignment(fa, (a + 8) % 16), want=FASTA)
                assert got == ref_a and used == len(fa), (a % 16, eol, last_eol)
                a += 1
    for a in range(16):  # every alignment once more on one shape, both classes
        fq, fa = fastq4(rng, [17, 1, 300]), fasta(rng, [100, 0, 17], 60)
        assert device_records(mm, _at_alignment(fq, a), want=FASTQ4)[0] == ref_records(fq)
        assert device_records(mm, _at_alignment(fa, a), want=FASTA)[0] == ref_records(fa)
    for data, want in ((b"@one\nACGTU\n+\nIIIII\n", FASTQ4), (b">one\nACGTU\n", FASTA), (b">one", FASTA)):
        both_equal_reference(mm, data, want, flags=((True, True),))
    # records across every tile boundary: 150-byte reads and 70-column lines over ten tiles
    fq, fa = fastq4(rng, [150] * 140), fasta(rng, [1000] * 45, 70)
    for data, want in ((fq, FASTQ4), (fa, FASTA)):
        assert len(data) > 10 * TILE
        starts = set(_record_starts(data))
        assert not any(t in starts for t in range(TILE, len(data), TILE)), "a record starts on a tile boundary: nothing straddles it"
        both_equal_reference(mm, data, want, flags=((True, True),))


def _fasta_of_widths(rng, widths, eol=b"\n", last_eol=True):
    """a record of three lines for every width"""
    data = b"".join(fasta(rng, [3 * w], w, eol) for w in widths)
    return data if last_eol else data[:len(data) - len(eol)]


def _record_starts(data):
    """offsets of the records of a well-formed FASTQ4 / FASTA text (what `consumed` may be)"""
    if data[:1] == b"@":
        nl = [-1] + [i for i, c in enumerate(data) if c == 10]
        return [nl[k] + 1 for k in range(0, len(nl), 4) if nl[k] + 1 < len(data)]
    return [0] + [i + 1 for i in range(len(data) - 1) if data[i] == 10 and data[i + 1] == 62]


def check_long_class(mm):
    """the same records with MM2AMD_FASTX_LONG_LINE=100: every path of the long class on lines of 100-300 bytes; then one line beyond the
    default threshold without the variable"""
    rng = np.random.default_rng(12)
    lens = [99, 100, 101, 150, 255, 256, 257, 300, 1, 17]
    fq, fa = fastq4(rng, lens, b"\r\n"), _fasta_of_widths(rng, lens)
    ref_q, ref_a = ref_records(fq, True, True), ref_records(fa, True, True)
    saved = os.environ.get("MM2AMD_FASTX_LONG_LINE")
    os.environ["MM2AMD_FASTX_LONG_LINE"] = "100"
    try:
        assert mm.fastx_limits()["long_line"] == 100
        mm.profile_enable(True)
        assert device_records(mm, fq, True, True, FASTQ4)[0] == ref_q
        assert device_records(mm, fa, True, True, FASTA)[0] == ref_a
        assert device_records(mm, fq, False, True, FASTQ4)[0] == [(a, b, c, None) for a, b, c, _ in ref_q]  # (no quality: its long lines are not listed)
        prof = mm.profile_get()
        mm.profile_enable(False)
        # lines of at least 100 payload bytes: 7 sequence and 7 quality lines, the quality once more skipped; the FASTA's lines of 100 and more
        n_fa = sum(1 for ln in fa.split(b"\n") if not ln.startswith(b">") and len(ln) >= 100)
        assert prof["fastx_copy_kernel[long]"]["launches"] == 3 and prof["fastx_copy_kernel[long]"]["units"] == 14 + n_fa + 7, prof
    finally:
        mm.profile_enable(False)
        if saved is None:
            del os.environ["MM2AMD_FASTX_LONG_LINE"]
        else:
            os.environ["MM2AMD_FASTX_LONG_LINE"] = saved
    assert mm.fastx_limits()["long_line"] == 4096
    # a read and a contig line of 40 000 bytes: three chunks of the long class each
    fq, fa = fastq4(rng, [40000, 120, 4096]), fasta(rng, [40000, 100], lambda r: 40000)
    mm.profile_enable(True)
    try:
        assert device_records(mm, fq, want=FASTQ4)[0] == ref_records(fq)
        assert device_records(mm, fa, want=FASTA)[0] == ref_records(fa)
        assert mm.profile_get()["fastx_copy_kernel[long]"]["units"] == 2 * 3 + 2 * 1 + 3
    finally:
        mm.profile_enable(False)


def check_fasta_multiline(mm):
    rng = np.random.default_rng(13)
    lens = [0, 1, 59, 60, 61, 140, 0, 700, 5000, 0]
    for width in (1, 60, 70, lambda r: int(r.integers(1, 90))):
        for eol in (b"\n", b"\r\n"):
            for empty in (False, True):
                data = fasta(rng, lens if width != 1 else [0, 1, 61, 0], width, eol, bool(rng.integers(0, 2)), empty)
                both_equal_reference(mm, data, FASTA, flags=((True, True), (False, False)))
    for fn in sorted(os.listdir(FIXTURES)):
        if fn.endswith(".fa"):
            data = open(os.path.join(FIXTURES, fn), "rb").read()
            both_equal_reference(mm, data, FASTA, flags=((True, True),))


def _feed(mm, data, block, device, want):
    """the file in blocks of `block` bytes with the tail carried over; returns the records and checks what `consumed` may be"""
    starts = set(_record_starts(data)) | {len(data)}
    out, tail, pos, base = [], b"", 0, 0  # base: the file offset of tail[0]
    while True:
        chunk = data[pos:pos + block]
        pos += len(chunk)
        final = pos >= len(data)
        text = tail + chunk
        recs, used, path = mm.parse_fastx(text, final, True, True, device=device)
        assert path == (want if device else HOST)
        if not recs:
            assert used == (len(text) if final else 0), "no complete record: nothing is consumed"
        assert base + used in starts, "consumed %d is no record start" % (base + used)
        out += recs
        tail, base = text[used:], base + used
        if final:
            assert used == len(text)
            return out


def check_incremental(mm):
    rng = np.random.default_rng(14)
    fq = fastq4(rng, [int(x) for x in rng.integers(1, 200, 200)], last_eol=False)
    fa = fasta(rng, [int(x) for x in rng.integers(0, 400, 200)], 60, last_eol=False)
    for data, want in ((fq, FASTQ4), (fa, FASTA)):
        ref = ref_records(data, True, True)
        assert len(ref) == 200
        for block in (64, 257, 4096):
            assert _feed(mm, data, block, True, want) == ref, (want, block)
            assert _feed(mm, data, block, False, want) == ref, (want, block)


def batch_records(b):
    out = []
    for k in range(len(b.items)):
        r = b.arr[k]
        assert r.l_seq == len(r.seq)
        out.append((r.name, r.comment, r.seq, r.qual))
    return out


def reader_batches(mm, files, **kw):
    rd = mm.FastxReader(files, **kw)
    out, tables = [], []
    n_seen = 0
    for b in rd:
        out.append(batch_records(b))
        tables.append((list(b.seg_off[:b.n]), list(b.n_seg[:b.n])))
        assert [b.arr[k].rid for k in range(len(b.items))] == list(range(n_seen, n_seen + len(b.items)))  # (map.c:555-556)
        assert b.bases == sum(len(r[2]) for r in out[-1])
        n_seen += len(b.items)
    return out, tables, rd.paths


def _qname(s):
    return s[:-2] if len(s) >= 3 and s[-1:].isdigit() and s[-2:-1] == b"/" else s


def _frag_table(recs, frag_mode):
    """map.c:566-571"""
    seg_off, n_seg, j = [], [], 0
    for i in range(1, len(recs) + 1):
        if i == len(recs) or not frag_mode or _qname(recs[i - 1][0]) != _qname(recs[i][0]):
            n_seg.append(i - j), seg_off.append(j)
            j = i
    return seg_off, n_seg


def _same_batches(mm, files, want_paths, **kw):
    n_files = 1 if isinstance(files, str) else len(files)
    ref = ref_batches(files, kw.get("chunk_bases", 500000000), kw.get("with_qual", True), kw.get("with_comment", False), kw.get("frag_mode", False))
    frag = kw.get("frag_mode", False) or n_files > 1
    for dev in (True, False):
        got, tables, paths = reader_batches(mm, files, device=dev, **kw)
        assert got == ref, (files, kw, dev, [len(b) for b in got], [len(b) for b in ref])
        assert tables == [_frag_table(b, frag) for b in ref], (files, kw, dev)
        if dev:
            assert paths and all(p in want_paths for p in paths), paths
        else:
            assert all(p == HOST for p in paths)
    return ref


def check_reader_batches(mm, tmp):
    rng = np.random.default_rng(15)
    fq, fa = os.path.join(tmp, "r.fq"), os.path.join(tmp, "r.fa")
    open(fq, "wb").write(fastq4(rng, [int(x) for x in rng.integers(1, 400, 120)]))
    open(fa, "wb").write(fasta(rng, [int(x) for x in rng.integers(0, 900, 60)], 60))
    for chunk in (1, 5, 1000, None):
        kw = {} if chunk is None else {"chunk_bases": chunk}
        for block in (300, 64 << 20):
            ref = _same_batches(mm, fq, (FASTQ4,), block_bytes=block, with_comment=True, **kw)
            _same_batches(mm, fa, (FASTA,), block_bytes=block, with_qual=False, **kw)
        assert chunk not in (None, 1) or len(ref) == (1 if chunk is None else 120)
    # interleaved pairs; reads of 200 bases and chunks of 1000: pairs straddle chunk boundaries; blocks of 500 bytes: pairs straddle block boundaries
    pe = os.path.join(tmp, "pe.fq")
    with open(pe, "wb") as f:
        for i in range(60):
            n1, n2 = int(rng.integers(150, 250)), int(rng.integers(150, 250))
            f.write(b"@p%d/1\n%s\n+\n%s\n@p%d/2\n%s\n+\n%s\n" % (i, _seq(rng, n1), b"I" * n1, i, _seq(rng, n2), b"J" * n2))
        f.write(b"@single\nACGT\n+\nIIII\n@trio/1\nAC\n+\nII\n@trio/2\nAC\n+\nII\n@trio/3\nAC\n+\nII\n")
    for chunk in (1, 1000, 1100, None):
        kw = {} if chunk is None else {"chunk_bases": chunk}
        for block in (500, 64 << 20):
            ref = _same_batches(mm, pe, (FASTQ4,), block_bytes=block, frag_mode=True, **kw)
            assert all(_qname(b[-1][0]) != _qname(nb[0][0]) for b, nb in zip(ref, ref[1:])), "a pair was split"
    ref = ref_batches(pe, 1000, frag_mode=True)
    plain = ref_batches(pe, 1000, frag_mode=False)
    assert [len(b) for b in ref] != [len(b) for b in plain], "no pair straddles a chunk boundary: the case proves nothing"
    # two files against mm_bseq_read_frag2, with unequal record counts
    f1, f2 = os.path.join(tmp, "m1.fq"), os.path.join(tmp, "m2.fq")
    open(f1, "wb").write(fastq4(rng, [int(x) for x in rng.integers(50, 150, 50)]))
    open(f2, "wb").write(fastq4(rng, [int(x) for x in rng.integers(50, 150, 43)]))
    for chunk in (1, 1000, None):
        kw = {} if chunk is None else {"chunk_bases": chunk}
        for block in (700, 64 << 20):
            ref = _same_batches(mm, [f1, f2], (FASTQ4,), block_bytes=block, **kw)
            assert sum(len(b) for b in ref) == 86
    # a gzip file
    gz = os.path.join(tmp, "r.fq.gz")
    with gzip.open(gz, "wb") as f:
        f.write(open(fq, "rb").read())
    _same_batches(mm, gz, (FASTQ4,), chunk_bases=1000, block_bytes=1000)
    # a malformed record ends a batch; the reading stops at the first empty one
    bad = os.path.join(tmp, "bad.fq")
    open(bad, "wb").write(b"@a\nAC\n+\nII\n@b\nAC\n+\nIIII\n@c\nAC\n+\nII\n@d\nAC\n+\nII\n")
    for block in (16, 64 << 20):
        ref = _same_batches(mm, bad, (HOST, FASTQ4), block_bytes=block)
        assert [[r[0] for r in b] for b in ref] == [[b"a"], [b"c", b"d"]]
    open(bad, "wb").write(b"@b\nAC\n+\nIIII\n@c\nAC\n+\nII\n")
    assert _same_batches(mm, bad, (HOST,)) == []


HOST_CLASS = [
    b">a\nACGT\nAC\n@b\nGG\n+\nII\n>c\nA\n",                      # mixed FASTA and FASTQ
    b"@q\nAC\nGT\n+\nII\nII\n@r\nACGT\n+\nIIII\n",                 # multi-line FASTQ
    b"some junk\nmore\n@q\nAC\n+\nII\n",                            # leading junk
    b"@e\n\n+\n\n@f\nAC\n+\nII\n",                                  # an empty FASTQ sequence
    b"@t\nACGT\n+\nII\n@u\nAC\n+\nII\n@v\nAC\n+\nII\n",             # a short quality
]


def check_host_class(mm):
    rng = np.random.default_rng(16)
    big = fastq4(rng, [int(x) for x in rng.integers(1, 300, 100)])
    cases = HOST_CLASS + [big + b"@q\nAC\nGT\n+\nII\nII\n" + big, big.replace(b"\n+", b"\n\n+", 1)]  # (a violation deep inside an otherwise regular file)
    for data in cases:
        both_equal_reference(mm, data, HOST)


def _raw(mm, data, is_final, flags, recs_cap, pool_cap, device=True, sizing=False):
    """one call of the C entry point with canaries behind both capacities: (rc, n_recs, pool_len, consumed, path, table, pool)"""
    L = mm.lib()
    text = np.frombuffer(data, dtype=np.uint8) if data is not None else None
    recs = np.full((recs_cap + 2) * 48, 0xA5, dtype=np.uint8)
    pool = np.full(pool_cap + 64, 0xA5, dtype=np.uint8)
    n, pl, used, path = C.c_size_t(77), C.c_size_t(77), C.c_size_t(77), C.c_int(77)
    call = L.mm2amd_fastx_parse if device else L.mm2amd_fastx_parse_host
    rc = call(text.ctypes.data if text is not None and text.size else None, 0 if text is None else text.size, int(is_final), flags,
              None if sizing else recs.ctypes.data, recs_cap, None if sizing else pool.ctypes.data, pool_cap, C.byref(n), C.byref(pl), C.byref(used), C.byref(path))
    assert (recs[recs_cap * 48:] == 0xA5).all() and (pool[pool_cap:] == 0xA5).all(), "bytes at or beyond a capacity were written"
    return rc, n.value, pl.value, used.value, path.value, recs, pool


def check_bookkeeping(mm):
    rng = np.random.default_rng(17)
    L = mm.lib()
    fq, fa = fastq4(rng, [30, 1, 200, 77]), fasta(rng, [100, 0, 61], 60)
    for data, want, dev in ((fq, FASTQ4, True), (fa, FASTA, True), (fq, HOST, False), (HOST_CLASS[0], HOST, True)):
        n_ref = len(ref_records(data))
        rc, n, pl, used, path, _, _ = _raw(mm, data, True, 3, 0, 0, dev, sizing=True)  # the sizing call
        assert (rc, n, used, path) == (0, n_ref, len(data), want) and 0 < pl <= len(data) + 1
        rc, n2, pl2, used2, path2, recs, pool = _raw(mm, data, True, 3, n, pl, dev)  # exactly the sizes
        assert (rc, n2, pl2, used2, path2) == (0, n, pl, used, path)
        assert pool[pl - 1] == 0 and (pool[:pl] != 0xA5).any()
        for rcap, pcap in ((n - 1, pl), (n, pl - 1), (0, 0), (n, 1)):  # too small: the sizes, and nothing beyond the capacities
            rc, n3, pl3, _, path3, _, _ = _raw(mm, data, True, 3, rcap, pcap, dev)
            assert (rc, n3, pl3, path3) == (mm.ENOMEM, n, pl, want), (rc, n3, pl3, rcap, pcap)
    # EINVAL
    n, pl, used, path = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0), C.c_int(0)
    buf = np.frombuffer(fq, dtype=np.uint8)
    for call in (L.mm2amd_fastx_parse, L.mm2amd_fastx_parse_host):
        assert call(None, 5, 1, 0, None, 0, None, 0, C.byref(n), C.byref(pl), C.byref(used), C.byref(path)) == mm.EINVAL
        for k in range(4):
            args = [C.byref(n), C.byref(pl), C.byref(used), C.byref(path)]
            args[k] = None
            assert call(buf.ctypes.data, buf.size, 1, 0, None, 0, None, 0, *args) == mm.EINVAL
        assert call(None, 0, 1, 0, None, 0, None, 0, C.byref(n), C.byref(pl), C.byref(used), C.byref(path)) == 0 and n.value == 0 and used.value == 0  # len == 0
    lim = mm.fastx_limits()
    assert lim["max_text"] == 1 << 30 and lim["long_line"] == 4096
    assert L.mm2amd_fastx_parse(buf.ctypes.data, lim["max_text"] + 1, 1, 0, None, 0, None, 0, C.byref(n), C.byref(pl), C.byref(used), C.byref(path)) == mm.EINVAL
    assert mm.parse_fastx(b"", device=True) == ([], 0, HOST) and mm.parse_fastx(b"", device=False) == ([], 0, HOST)
    # a non-final buffer without a complete record
    for data, want in ((b"@a\nACGT\n+\nII", FASTQ4), (b">a\nACGT\nAC\n", FASTA), (b"junk\n@a\nAC\n", HOST)):
        assert mm.parse_fastx(data, False, device=True) == ([], 0, want)
        assert mm.parse_fastx(data, False, device=False) == ([], 0, HOST)
    # reuse of the buffers: a large call, a smaller one, the large one again -- with the profile: the slot names the three kernels
    big = fastq4(rng, [int(x) for x in rng.integers(1, 500, 300)])
    ref_big, ref_small = ref_records(big), ref_records(fq)
    mm.profile_enable(True)
    try:
        for data, ref in ((big, ref_big), (fq, ref_small), (fa, ref_records(fa)), (big, ref_big)):
            assert device_records(mm, data)[0] == ref
        prof = mm.profile_get()
    finally:
        mm.profile_enable(False)
    for name, launches in (("fastx_lines_kernel[count]", 4), ("fastx_lines_kernel[write]", 4), ("fastx_classify_kernel", 4), ("fastx_copy_kernel[short]", 4)):
        assert prof[name]["launches"] == launches, prof
    assert prof["fastx_classify_kernel"]["units"] == 2 * (4 * 300) + 16 + len(fa.split(b"\n")) - 1
    assert "fastx_copy_kernel[long]" not in prof


def mapping_case(tmp, seed=18):
    """a 300 kb reference and 50 reads of about 1 kb with qualities, every third with a comment"""
    rng = np.random.default_rng(seed)
    contigs = synth.gen_reference(rng, 300000, 2)
    reads = synth.gen_reads(rng, contigs, 50, 1000, 200, 0.06, min_len=300)
    ref_fa, fq = os.path.join(tmp, "ref.fa"), os.path.join(tmp, "reads.fq")
    synth.write_fasta(ref_fa, ["chr1", "chr2"], contigs)
    with open(fq, "wb") as f:
        for i, r in enumerate(reads):
            s = synth.ACGT[r].tobytes()
            f.write(b"@read%d%s\n%s\n+\n%s\n" % (i, b"\tBC:Z:tag%d  rest" % i if i % 3 == 0 else b"", s, bytes(35 + (k * 7 + i) % 40 for k in range(len(s)))))
    return ref_fa, fq


def check_mapping_from_file(mm, tmp):
    """a FASTQ from the file to SAM: Aligner.pipeline over FastxReader against `minimap2 -a` on the same files, QUAL column and -y comments included"""
    ref_fa, fq = mapping_case(tmp)
    for opts, kw, flags in ((["-a"], {}, 0), (["-a", "-y"], {"with_comment": True}, mm.F_COPY_COMMENT)):
        out = subprocess.run([reflib.REF_BIN, "-x", "map-ont", "-t", "2"] + opts + [ref_fa, fq], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, check=True).stdout
        want = b"".join(ln + b"\n" for ln in out.split(b"\n") if ln and not ln.startswith(b"@"))
        assert want.count(b"\n") >= 45
        al = mm.Aligner(fn_idx_in=ref_fa, preset="map-ont", n_threads=2, sam=True, extra_flags=flags)
        try:
            for dev in (True, False):
                text = []
                rd = mm.FastxReader(fq, chunk_bases=20000, block_bytes=30000, device=dev, **kw)
                al.pipeline(rd, text=True, on_text=lambda b, addr, n: text.append(C.string_at(addr, n)))
                assert len(text) >= 2 and all(p == (FASTQ4 if dev else HOST) for p in rd.paths)
                assert b"".join(text) == want, (opts, dev)
        finally:
            al.close()
        if flags:
            assert b"BC:Z:tag0  rest\n" in want
