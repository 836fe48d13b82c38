"""Shared by tests/test_gpu_sdust.py and tests/test_sdust_emu.py (not a test): sequences for sdust_kernel behind mm2amd_sdust_batch, the judge they are
measured by -- the UNMODIFIED compiled reference (oracle/_ref/libminimap2_ref.so) through ctypes: sdust(NULL, seq, len, T, 64, &n) (sdust.c:134-175),
freed with kfree(NULL, .) -- a plain Python restatement of the length of the list of perfect intervals (which launch class a sequence takes), and
the `-T` mapping cases (MM2AMD_DEVICE_SDUST=1 against the host scan and the reference)."""
import ctypes as C
import os
import random
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import reflib  # noqa: E402

HAVE_REF = os.path.exists(reflib.REF_SO)
NARROW, WIDE = 0, 1  # minimap2_amd.SDUST_PATH_*
THRESHOLDS = [1, 2, 4, 5, 20, 64, 100]  # 4 and 5 lie on either side of the `cv * 10 > 2T` step; 1 makes every step fire
NT4 = bytes(0 if c in b"Aa" else 1 if c in b"Cc" else 2 if c in b"Gg" else 3 if c in b"TtUu" else c if c < 4 else 4 for c in range(256))  # seq_nt4_table

_R = None


class env(object):
    """environment variables for the duration of a call (the entry points read them at every call); None removes one"""

    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        for k, v in self.kv.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, str(v))

    def __exit__(self, *a):
        for k, v in self.old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


def _ref():
    global _R
    if _R is None:
        _R = C.CDLL(reflib.REF_SO)
        _R.sdust.restype = C.POINTER(C.c_uint64)
        _R.sdust.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)]
        _R.kfree.restype = None
        _R.kfree.argtypes = [C.c_void_p, C.c_void_p]
    return _R


def ref_sdust(seq, T):
    """the reference's regions as a list of start << 32 | finish"""
    seq = bytes(seq)
    R, n = _ref(), C.c_int(0)
    p = R.sdust(None, seq, len(seq), T, 64, C.byref(n))
    out = [int(p[i]) for i in range(n.value)]
    R.kfree(None, C.cast(p, C.c_void_p))
    return out


def packed(a):
    return [int(s) << 32 | int(f) for s, f in a]


# ---------------------------------------------------------------------------------------------------------
# which class a sequence takes: the length of the list of perfect intervals, restated from sdust.c
# ---------------------------------------------------------------------------------------------------------
def list_growth(seq, T, cap):
    """(the largest length the list P of sdust_core reaches, the number of bases read when it first exceeds cap or None), restated step by step: the
    window is the FIFO w of 3-mer codes, e[k] the number of later words equal to w[k]; find_perfect's candidate i has r = sum(e[i:]) and l = n - i - 1
    and is inserted iff r / l is >= the ratios of the live entries with start >= its own and of the passing candidates above it.  Only the entries'
    starts and ratios matter to that, so P is kept as a list of [start, r, l]; it stops at the first excess (the maximum is then a lower bound)."""
    codes = bytes(seq).translate(NT4)
    w, e, P = [], [], []
    l = t = 0
    max_p = 0
    for i, b in enumerate(codes):
        if b >= 4:
            P, l, t = [], 0, 0
            continue
        l, t = l + 1, (t << 2 | b) & 63
        if l < 3:
            continue
        start = max(0, l - 64) + (i + 1 - l)
        if P and P[-1][0] < start:
            P = [p for p in P if p[0] >= start]
        if len(w) >= 62:
            w.pop(0), e.pop(0)
        e = [x + (c == t) for x, c in zip(e, w)]
        w.append(t), e.append(0)
        n, rw = len(w), sum(e)
        L = n
        if (max(e) + 1) * 10 > 2 * T:
            L = n - 1 - max(k for k in range(n) if (e[k] + 1) * 10 > 2 * T)
        if rw * 10 <= L * T:
            continue
        best = {}  # start -> the largest (r, l) among the live entries with that start
        for s, r, ll in P:
            if s not in best or r * best[s][1] > best[s][0] * ll:
                best[s] = (r, ll)
        new, r, mr, ml = [], sum(e[n - L:]), 0, 1
        for k in range(n - L - 1, -1, -1):
            r += e[k]
            ll = n - k - 1
            if k + start in best and best[k + start][0] * ml > mr * best[k + start][1]:
                mr, ml = best[k + start]
            if r * 10 > T * ll:
                if r * ml >= mr * ll:
                    new.append([k + start, r, ll])
                if r * ml > mr * ll:
                    mr, ml = r, ll
        if new:
            P = sorted(P + new, key=lambda p: -p[0])  # (stable: a new entry goes behind the old ones of its start)
            max_p = max(max_p, len(P))
            if len(P) > cap:
                return max_p, i + 1
    return max_p, None


def class_of(seq, T, cap):
    """(NARROW or WIDE, the bases the narrow class scans of it)"""
    _, stop = list_growth(seq, T, cap)
    return (NARROW, len(seq)) if stop is None else (WIDE, stop)


# ---------------------------------------------------------------------------------------------------------
# sequences
# ---------------------------------------------------------------------------------------------------------
def random_seq(rng, n):
    return bytes(rng.choice(b"ACGT") for _ in range(n))


def directed_shapes():
    """(name, sequence)"""
    rng = random.Random(11)
    out = [("len%d" % n, b"ACGTA"[:n]) for n in (0, 1, 2, 3)]
    out += [("A x %d" % n, b"A" * n) for n in (61, 62, 63, 64, 65, 66, 200)]
    out += [("(AC) x 100", b"AC" * 100), ("(ACG) x 70", b"ACG" * 70), ("random 300", random_seq(rng, 300))]
    out += [("N first", b"N" + b"T" * 80), ("N last", b"T" * 80 + b"N"), ("N alone", b"N"), ("NNN run", b"G" * 70 + b"NNN" + b"G" * 70),
            ("words of 1 and 2 between Ns", b"C" * 30 + b"NCNCCNCCCNCCCCN" + b"C" * 30),
            ("the window survives an N", b"A" * 70 + b"N" + b"A" * 10 + b"N" + b"C" * 40),
            ("lower case", b"a" * 40 + b"ACacACacgt" * 8 + b"t" * 40), ("IUPAC", b"A" * 50 + b"R" + b"A" * 50 + b"YKM" + b"AC" * 40 + b"n" + b"T" * 70),
            ("entries expire one start at a time", b"T" * 64 + random_seq(rng, 64))]
    return out


def generated(n=400, seed=7):
    """the piece generator of tests/cpucheck/sdust_test.cpp: random / homopolymer / mutated tandem repeat / N-run pieces, lengths <= 600 and every tenth
    <= 20 000, a third of every ninth in lower case; -> (sequence, T) with T cycling through THRESHOLDS"""
    rng = random.Random(seed)
    out = []
    for it in range(n):
        ln = rng.randrange(20000 if it % 10 == 0 else 600) + 1
        s = bytearray()
        while len(s) < ln:
            kind, piece = rng.randrange(5), 1 + rng.randrange(300)
            unit = bytes(rng.choice(b"ACGT") for _ in range(1 + rng.randrange(7)))
            k = min(piece, ln - len(s))
            if kind == 0:
                s += bytes(rng.choices(b"ACGT", k=k))
            elif kind == 1:
                s += unit[:1] * k
            elif kind in (2, 3):
                rep = bytearray((unit * (k // len(unit) + 1))[:k])
                for p in range(k):
                    if rng.randrange(40) == 0:
                        rep[p] = rng.choice(b"ACGT")
                s += rep
            else:
                run = bytearray(rng.choices(b"ACGT", k=k))
                if piece < 6:
                    run[:] = b"N" * k
                else:
                    run[:3] = b"N" * min(3, k)
                s += run
        if it % 9 == 0:
            s = bytearray(c + 32 if rng.randrange(3) == 0 else c for c in s)
        out.append((bytes(s), THRESHOLDS[it % len(THRESHOLDS)]))
    return out


# ---------------------------------------------------------------------------------------------------------
# checks
# ---------------------------------------------------------------------------------------------------------
def check(mm, seqs, T, want=None, path=None):
    """every sequence's regions equal the reference's: the same count, the same 64-bit values; path: the class every one must report; -> paths"""
    got, paths = mm.sdust_batch(seqs, T, paths=True)
    assert len(got) == len(seqs) == len(paths)
    for i, s in enumerate(seqs):
        w = want[i] if want is not None else ref_sdust(s, T)
        g = packed(got[i])
        assert g == w, "sequence %d (%d bases, T %d, path %d): got %d regions %r, the reference %d %r" % (i, len(s), T, paths[i], len(g), g[:4], len(w), w[:4])
        assert got[i].shape == (len(w), 2) and got[i].dtype == np.int32
        if path is not None:
            assert paths[i] == path, "sequence %d (%d bases, T %d): path %d, expected %d" % (i, len(s), T, paths[i], path)
    return paths


def check_directed(mm):
    shapes = directed_shapes()
    seqs = [s for _, s in shapes]
    n_masked = 0
    with env(MM2AMD_SDUST_NARROW_CAP=None, MM2AMD_SDUST_NO_NARROW=None):
        for T in THRESHOLDS:
            want = [ref_sdust(s, T) for s in seqs]
            n_masked += sum(1 for w in want if w)
            check(mm, seqs, T, want)
    assert n_masked > 5 * len(THRESHOLDS)
    w = ref_sdust(seqs[[n for n, _ in shapes].index("the window survives an N")], 20)
    assert len(w) >= 2 and w[0] >> 32 == 0  # (masked on both sides of the Ns: the case is no empty one)


_GEN = {}  # the generated set and the reference's answers, computed once a process: the reference takes seconds on the long repeats at T = 1 and 2


def _generated_want(idx):
    if "jobs" not in _GEN:
        _GEN["jobs"], _GEN["want"] = generated(400), {}
    for i in idx:
        if i not in _GEN["want"]:
            _GEN["want"][i] = ref_sdust(*_GEN["jobs"][i])
    return _GEN["jobs"], _GEN["want"]


def check_generated(mm, T):
    """the generated sequences that carry threshold T: the reference's regions, and the class the list's length says; the set as a whole bites"""
    jobs, want = _generated_want(range(400))
    assert sum(1 for i in range(400) if want[i]) * 2 >= len(jobs)
    assert max(len(w) for w in want.values()) >= 20
    assert all(len(want[i]) < len(jobs[i][0]) / 4.0 for i in range(400) if want[i])
    sel = [i for i, (_, t) in enumerate(jobs) if t == T]
    assert len(sel) >= 50 and max(len(jobs[i][0]) for i in sel) <= 20000
    with env(MM2AMD_SDUST_NARROW_CAP=None, MM2AMD_SDUST_NO_NARROW=None):
        cap = mm.sdust_limits()["narrow_cap"]
        paths = check(mm, [jobs[i][0] for i in sel], T, [want[i] for i in sel])
    for i, p in zip(sel, paths):  # a sequence is wide iff its list exceeded narrow_cap
        cls = NARROW if not want[i] else class_of(jobs[i][0], T, cap)[0]  # (no region: the list was never in use)
        assert p == cls, "sequence %d (%d bases, T %d): path %d, the list's length says %d" % (i, len(jobs[i][0]), T, p, cls)
    if T <= 20:
        assert NARROW in paths and WIDE in paths


def check_classes(mm):
    """the directed shapes through small narrow lists and through the wide class alone; which shapes stop where"""
    shapes = directed_shapes()
    names, seqs = [n for n, _ in shapes], [s for _, s in shapes]
    want = {T: [ref_sdust(s, T) for s in seqs] for T in THRESHOLDS}
    for cap in (8, 64, 65):
        with env(MM2AMD_SDUST_NARROW_CAP=cap, MM2AMD_SDUST_NO_NARROW=None):
            assert mm.sdust_limits()["narrow_cap"] == cap
            for T in THRESHOLDS:
                paths = check(mm, seqs, T, want[T])
                if T == 20:
                    for nm, s, p in zip(names, seqs, paths):
                        assert p == class_of(s, T, cap)[0], (nm, cap, p)
                        if nm in ("A x 66", "A x 200"):
                            assert p == WIDE, (nm, cap)
                        if nm == "random 300":
                            assert p == NARROW, (nm, cap)
    with env(MM2AMD_SDUST_NARROW_CAP=None, MM2AMD_SDUST_NO_NARROW=1):
        for T in THRESHOLDS:
            check(mm, seqs, T, want[T], path=WIDE)
    with env(MM2AMD_SDUST_NARROW_CAP=None, MM2AMD_SDUST_NO_NARROW=None):
        lim = mm.sdust_limits()
        assert lim["wide_cap"] == 4096 and 1 <= lim["narrow_cap"] < lim["wide_cap"] and lim["max_len"] >= 1 << 30


def check_mixed(mm):
    """one batch with both classes, empty jobs and a 20 000-base read, then a smaller one on the same buffers; the profile's launches and units"""
    rng = random.Random(23)
    T, cap = 20, 64
    first = [b"", random_seq(rng, 20000), b"A" * 100, b"AC" * 50, b"", random_seq(rng, 100), b"ACG" * 33 + b"N" + b"T" * 99, b"G" * 70 + random_seq(rng, 30), b""]
    first += [random_seq(rng, 40) + b"T" * rng.randrange(20, 90) + random_seq(rng, 40) for _ in range(60)]
    second = [b"C" * 100, random_seq(rng, 57), b"", b"AT" * 40]
    with env(MM2AMD_SDUST_NARROW_CAP=cap, MM2AMD_SDUST_NO_NARROW=None):
        mm.profile_enable(True)
        try:
            p1 = check(mm, first, T)
            prof = mm.profile_get()
        finally:
            mm.profile_enable(False)
        p2 = check(mm, second, T)
    cls = [class_of(s, T, cap) for s in first]
    assert p1 == [c for c, _ in cls] and NARROW in p1 and WIDE in p1 and p1[1] == NARROW and p1[2] == WIDE
    assert p2 == [class_of(s, T, cap)[0] for s in second] and p2[0] == WIDE and p2[2] == NARROW
    narrow, wide = prof.get("sdust_kernel[narrow]"), prof.get("sdust_kernel[wide]")
    assert narrow and wide and narrow["launches"] == 1 and wide["launches"] == 1, prof
    assert wide["units"] == sum(len(s) for s, (c, _) in zip(first, cls) if c == WIDE)
    assert narrow["units"] == sum(stop for _, stop in cls), (narrow["units"], sum(stop for _, stop in cls))  # (a read that stopped counts up to there)


def check_bookkeeping(mm):
    L = mm.lib()
    seqs = [b"A" * 80, b"", b"ACGT" * 10, b"AC" * 60 + b"N" + b"T" * 70]
    want = [ref_sdust(s, 20) for s in seqs]
    total = sum(len(w) for w in want)
    assert total >= 4 and not want[1]
    n = len(seqs)
    arr, keep = mm._sdust_jobs(seqs)
    res = (mm.SdustRes * n)()
    # sizing call, then the real one
    assert L.mm2amd_sdust_batch(n, arr, 20, res, None, 0) == 0
    assert [r.n for r in res] == [len(w) for w in want] and [r.off for r in res] == [sum(len(w) for w in want[:i]) for i in range(n)]
    pool = np.full(total + 2, 0xdeadbeefdeadbeef, dtype=np.uint64)
    assert L.mm2amd_sdust_batch(n, arr, 20, res, pool.ctypes.data, total) == 0
    assert pool[:total].tolist() == [v for w in want for v in w] and pool[total:].tolist() == [0xdeadbeefdeadbeef] * 2
    # a pool one short: the counts are filled, nothing lands behind it
    res = (mm.SdustRes * n)()
    pool[:] = 0xdeadbeefdeadbeef
    assert L.mm2amd_sdust_batch(n, arr, 20, res, pool.ctypes.data, total - 1) == mm.ENOMEM
    assert [r.n for r in res] == [len(w) for w in want] and pool[total - 1:].tolist() == [0xdeadbeefdeadbeef] * 3
    assert b"sdust_batch" in L.mm2amd_last_error()
    # arguments
    assert L.mm2amd_sdust_batch(n, arr, 0, res, None, 0) == mm.EINVAL
    assert L.mm2amd_sdust_batch(n, arr, -3, res, None, 0) == mm.EINVAL
    assert L.mm2amd_sdust_batch(n, None, 20, res, None, 0) == mm.EINVAL
    assert L.mm2amd_sdust_batch(n, arr, 20, None, None, 0) == mm.EINVAL
    assert L.mm2amd_sdust_batch(-1, arr, 20, res, None, 0) == mm.EINVAL
    bad, _ = mm._sdust_jobs([b"ACGT"])
    bad[0].len = -1
    assert L.mm2amd_sdust_batch(1, bad, 20, res, None, 0) == mm.EINVAL
    bad[0].len, bad[0].seq = 4, None
    assert L.mm2amd_sdust_batch(1, bad, 20, res, None, 0) == mm.EINVAL
    assert L.mm2amd_sdust_batch(0, None, 20, None, None, 0) == 0
    assert mm.sdust_batch([], 20) == []
    assert L.mm2amd_sdust_limits(None, None, None) == 0
    # a threshold beyond every score masks nothing, as in the reference
    assert packed(mm.sdust_batch([b"A" * 300], 1 << 24)[0]) == ref_sdust(b"A" * 300, 1 << 24) == []
    # the host routine behind the default -T path gives the same regions
    host, _ = mm.sdust_host_batch(seqs, 20, 2)
    assert [packed(h) for h in host] == want


# ---------------------------------------------------------------------------------------------------------
# the -T mapping path
# ---------------------------------------------------------------------------------------------------------
def mapping_case(seed=41):
    """a small reference with the same low-complexity stretches planted in several places -- (AC)n, poly-A, a 7-mer tandem, so that seeds inside them
    hit many positions -- and reads that start, end or lie in them; pairs over short stretches of their own (the pair preset aligns every copy of a
    repeat, which is the emulator's slowest work): (refs, names, single reads, pairs)"""
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    comp = np.array([3, 2, 1, 0], dtype=np.uint8)
    contigs = [rng.integers(0, 4, 40000, dtype=np.uint8) for _ in range(3)]
    islands = [np.tile(np.array([0, 1], dtype=np.uint8), 150), np.zeros(200, dtype=np.uint8), np.tile(np.array([2, 0, 3, 3, 0, 1, 0], dtype=np.uint8), 60)]
    spots = []
    for c in contigs:
        for k, p in enumerate(range(3000, 39000, 4000)):
            isl = islands[k % 3]
            c[p:p + len(isl)] = isl
            spots.append(p)

    def mutate(s, rate):
        s = s.copy()
        hit = rng.random(len(s)) < rate
        s[hit] = (s[hit] + rng.integers(1, 4, int(hit.sum()), dtype=np.uint8)) & 3
        return s

    singles, pairs = [], []
    for i in range(24):
        c = contigs[i % 3]
        p = spots[i % len(spots)] + int(rng.integers(-700, 300))
        s = mutate(c[p:p + 700], 0.04)
        if i % 2:
            s = comp[s[::-1]]
        singles.append(("r%d" % i, acgt[s].tobytes()))
    units = [b"GT", b"CTT", b"AGG", b"CCG", b"GAAG", b"TCTG", b"AAT", b"GGT", b"CT", b"ACCT", b"TTG", b"GCA"]  # one short stretch each, met nowhere else
    for i, u in enumerate(units):
        c = contigs[i % 3]
        p = 5000 + 4000 * (i // 3)
        c[p:p + 40] = np.frombuffer((u * 20)[:40].translate(NT4), dtype=np.uint8)
        p += int(rng.integers(-100, 0))
        a, b = mutate(c[p:p + 150], 0.01), comp[mutate(c[p + 200:p + 350], 0.01)[::-1]]
        pairs.append(("p%d" % i, acgt[a].tobytes(), acgt[b].tobytes()))
    return [acgt[c].tobytes() for c in contigs], ["c1", "c2", "c3"], singles, pairs


def _map(mm, refs, names, reads, preset, T, device):
    """(hit keys per read and segment, SAM text, profile) of one mapping pass over the reads, with the device scan or the host's"""
    with env(MM2AMD_DEVICE_SDUST=1 if device else None, MM2AMD_SDUST_NARROW_CAP=None, MM2AMD_SDUST_NO_NARROW=None):
        al = mm.Aligner(refs, preset=preset, names=names, n_threads=2, sam=True, sdust_thres=T)
        mm.profile_enable(True)
        try:
            al.stage(reads)
            b = al._staged
            n_reg, reg, rep_len = al.run(raw=True)
            try:
                sam = al.format_raw(n_reg, reg, rep_len)
                hits = [tuple(mm._regs_to_alignments(n_reg[k], C.cast(reg[k], C.POINTER(mm.Reg1)) if n_reg[k] else None, al.names, al.lens)
                              for k in range(b[3][i], b[3][i] + b[4][i])) for i in range(b[0])]
            finally:
                al.free_raw(n_reg, reg)
            prof = mm.profile_get()
        finally:
            mm.profile_enable(False)
            al.close()
    keys = [[[a.key() for a in seg] for seg in h] for h in hits]
    return keys, sam, prof


def _units(seqs, T, cap):
    """what the two classes scan of these units in one seeding pass: a unit that stops counts up to there for the narrow class"""
    cls = [class_of(s, T, cap) for s in seqs]
    return {"sdust_kernel[narrow]": sum(stop for _, stop in cls), "sdust_kernel[wide]": sum(len(s) for s, (c, _) in zip(seqs, cls) if c == WIDE)}


def check_mapping_singles(mm, T):
    """single reads with -T: hits and SAM text of the device scan equal the host scan's; the hit records (every field the SAM writer reads,
    Alignment.key()) equal the compiled reference's mm_map; the profile; and the masking changes the SAM"""
    refs, names, singles, _ = mapping_case()
    cap = mm.sdust_limits()["narrow_cap"]
    host = _map(mm, refs, names, singles, "map-ont", T, False)
    dev = _map(mm, refs, names, singles, "map-ont", T, True)
    assert dev[0] == host[0] and dev[1] == host[1], "-T %d: the device scan and the host scan give different hits" % T
    for name, u in _units([s for _, s in singles], T, cap).items():
        assert name in dev[2] and dev[2][name]["units"] == u, (name, dev[2].get(name), u)
    assert "sdust_kernel[narrow]" not in host[2] and "dust_filter_kernel" in host[2] and "dust_filter_kernel" in dev[2]
    assert sum(1 for k in dev[0] if k[0]) >= len(singles) // 2, "the reads must map"
    plain = _map(mm, refs, names, singles, "map-ont", 0, False)
    assert "sdust_kernel[narrow]" not in plain[2] and "dust_filter_kernel" not in plain[2]
    assert dev[1] != plain[1], "masking changed nothing on these reads: the case proves nothing"
    m = reflib.RefMapper(refs, "map-ont", names)
    m.mo.flag |= mm.F_OUT_SAM
    m.mo.sdust_thres = T
    want = [[m.map(nm, s)] for nm, s in singles]
    m.close()
    assert dev[0] == want, "-T %d: hits differ from the compiled reference" % T


def _ref_pairs(mm, refs, names, pairs, T):
    """the compiled reference's mm_map_frag over the pairs (oracle/_ref/librefdrv.so on the device-built tables): hit keys per pair and segment"""
    al = mm.Aligner(refs, preset="sr", names=names, n_threads=2, sam=True)
    try:
        st = al.index_stat()
        S, keys, val_off, pos = reflib.export_index(al)
        lens = list(al.lens)
    finally:
        al.close()
    drv = reflib.RefDriver(st["w"], st["k"], st["flag"], names, lens, S, keys, val_off, pos, 2)
    try:
        mo = drv.map_opt("sr", extra_flag=mm.F_OUT_SAM)
        mo.sdust_thres = T
        _, nr, rg = drv.map(mo, pairs, 2)
        out = [[[a.key() for a in mm._regs_to_alignments(nr[k], C.cast(rg[k], C.POINTER(mm.Reg1)) if nr[k] else None, None, None)] for k in (2 * i, 2 * i + 1)]
               for i in range(len(pairs))]
        mm.lib().mm2amd_free_regs(len(nr), nr, rg)
    finally:
        drv.close()
    return out


def check_mapping_pairs(mm):
    """one set of pairs with -T 20 -- the units of a pair are scanned one by one, each into its own slots: the same four checks as for single reads"""
    refs, names, _, pairs = mapping_case()
    cap = mm.sdust_limits()["narrow_cap"]
    host = _map(mm, refs, names, pairs, "sr", 20, False)
    dev = _map(mm, refs, names, pairs, "sr", 20, True)
    assert dev[0] == host[0] and dev[1] == host[1], "pairs: the device scan and the host scan give different hits"
    for name, u in _units([s for p in pairs for s in p[1:]], 20, cap).items():  # (no pair of this set is seeded a second time: none has repetitive minimizers)
        assert name in dev[2] and dev[2][name]["units"] == u, (name, dev[2].get(name), u)
    assert "sdust_kernel[narrow]" not in host[2] and "dust_filter_kernel" in host[2]
    assert sum(1 for k in dev[0] if k[0] and k[1]) >= len(pairs) // 2, "the pairs must map"
    plain = _map(mm, refs, names, pairs, "sr", 0, False)
    assert dev[1] != plain[1], "masking changed nothing on these pairs: the case proves nothing"
    assert dev[0] == _ref_pairs(mm, refs, names, pairs, 20), "pairs: hits differ from the compiled reference"
