"""Shared by tests/test_gpu_ksw_ll.py and tests/test_ksw_ll_emu.py (not a test): jobs for ksw_ll_kernel behind mm2amd_ksw_ll_batch and the oracle they
are judged by -- the UNMODIFIED compiled reference (oracle/_ref/libminimap2_ref.so) through ctypes: ksw_ll_qinit(km = NULL, size = 2, ...) +
ksw_ll_i16 (ksw2_ll_sse.c:37-152) on the explicitly transformed sequences.  Shapes come from ksw_ll_limits(), not from literals."""
import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import reflib  # noqa: E402

HAVE_REF = os.path.exists(reflib.REF_SO)
QREV, QCOMP, TREV = 1, 2, 4        # minimap2_amd.LL_*
WAVE, WG, HOST = 0, 1, 2           # minimap2_amd.LL_PATH_*
COMP5 = np.array([3, 2, 1, 0, 4], dtype=np.uint8)
# (a, b, q, e, sc_ambi, transition)
SCORINGS = [(2, 4, 4, 2, 1, 0), (1, 2, 2, 1, 1, 0), (1, 19, 39, 3, 1, 0), (2, 6, 4, 2, 1, 1), (2, 8, 12, 2, 1, 0), (1, 4, 6, 1, 1, 0), (4, 4, 1, 1, 1, 0),
            (2, 4, 0, 2, 1, 0), (2, 9, 1, 1, 1, 0)]
DIRECTED_SCORINGS = [(2, 4, 4, 2, 1, 0), (1, 2, 2, 1, 1, 0), (2, 6, 4, 2, 1, 1)]  # map-ont; splice; transitions, on sequences with about 3 % N

_R = None


def _ref():
    global _R
    if _R is None:
        _R = C.CDLL(reflib.REF_SO)
        _R.ksw_ll_qinit.restype = C.c_void_p
        _R.ksw_ll_qinit.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_char_p, C.c_int, C.c_char_p]
        _R.ksw_ll_i16.argtypes = [C.c_void_p, C.c_int, C.c_char_p, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        _R.kfree.restype = None
        _R.kfree.argtypes = [C.c_void_p, C.c_void_p]
    return _R


def mat_of(sc):
    return reflib.ts_mat(sc[0], sc[1], sc[4], sc[5])


def transform(q, t, flag):
    """the sequences the DP sees (align.c:91-96, :938-941)"""
    q, t = np.frombuffer(bytes(q), dtype=np.uint8), np.frombuffer(bytes(t), dtype=np.uint8)
    if flag & QREV:
        q = q[::-1]
    if flag & QCOMP:
        q = COMP5[q]
    if flag & TREV:
        t = t[::-1]
    return q.tobytes(), t.tobytes()


def ref_ll(q, t, mat, gapo, gape):
    """(score, qe, te) of the compiled reference; an empty job is the contract's (0, -1, -1): the reference reads outside its arrays there"""
    q, t = bytes(q), bytes(t)
    if not q or not t:
        return (0, -1, -1)
    R = _ref()
    p = R.ksw_ll_qinit(None, 2, len(q), q, 5, bytes(mat))
    qe, te = C.c_int(-1), C.c_int(-1)
    s = R.ksw_ll_i16(p, len(t), t, gapo, gape, C.byref(qe), C.byref(te))
    R.kfree(None, p)
    return (s, qe.value, te.value)


def plain_class(qlen, tlen, mat, gapo, gape):
    m = np.frombuffer(bytes(mat), dtype=np.int8).astype(int)
    return -min(0, m.min()) <= 2 * (gapo + gape) and gapo >= 1 and gape > 0 and max(0, m.max()) * min(qlen, tlen) < 32000 and 0 <= gapo + gape < 16000


def tied_columns(q, t, mat, gapo, gape):
    """(G, te, the columns with H(te, p) == G) from the plain affine local recurrence, a row at a time (plain class only: gapo + gape >= gape > 0, so a
    horizontal gap opened from a cell that itself ends a horizontal gap never beats extending that gap, and F is a running maximum over the row)"""
    m = np.frombuffer(bytes(mat), dtype=np.int8).astype(np.int64).reshape(5, 5)
    q, t = np.frombuffer(bytes(q), dtype=np.uint8), np.frombuffer(bytes(t), dtype=np.uint8)
    n, goe, ge = len(q), gapo + gape, gape
    H, E = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    ramp = np.arange(n, dtype=np.int64) * ge
    rows = []
    for i in range(len(t)):
        E = np.maximum(np.maximum(E - ge, H - goe), 0)
        diag = np.concatenate(([0], H[:-1]))
        h0 = np.maximum(diag + m[t[i]][q], E)
        best = np.maximum.accumulate(h0 + ramp)                           # max over k <= j of h0[k] + k * ge
        F = np.maximum(np.concatenate(([0], best[:-1] - goe - ramp[:-1])), 0)  # F[j] = max over k < j of h0[k] - goe - (j - 1 - k) * ge
        H = np.maximum(h0, F)
        rows.append(H)
    A = np.array(rows)
    G = int(A.max())
    te = max(i for i in range(len(t)) if A[i].max() == G)
    return G, te, [int(p) for p in np.nonzero(A[te] == G)[0]]


# ---------------------------------------------------------------------------------------------------------
# sequences
# ---------------------------------------------------------------------------------------------------------
def _mutate(rng, s, div, n_frac=0.0):
    """a copy with a share div of the bases deleted, preceded by an inserted base, or substituted (a third each)"""
    n = len(s)
    r = rng.random(n)
    sub = (r >= 2 * div / 3) & (r < div) & (s < 4)
    s2 = np.where(sub, (s + 1 + rng.integers(0, 3, n)) % 4, s).astype(np.uint8)
    cnt = np.where(r < div / 3, 0, np.where(r < 2 * div / 3, 2, 1))
    a = np.repeat(s2, cnt)
    ins = (np.cumsum(cnt) - cnt)[cnt == 2]
    a[ins] = rng.integers(0, 4, len(ins), dtype=np.uint8)
    if n_frac > 0 and len(a):
        a[rng.random(len(a)) < n_frac] = 4
    return a


def related(rng, qlen, tlen, div=0.10, n_frac=0.0):
    """two noisy copies of one sequence, cut or padded to the lengths asked for"""
    n = max(qlen, tlen)
    src = rng.integers(0, 4, n + n // 4 + 8, dtype=np.uint8)
    if n_frac > 0:
        src[rng.random(len(src)) < n_frac] = 4
    q, t = _mutate(rng, src, div / 2), _mutate(rng, src, div / 2)

    def fit(a, want):
        if len(a) < want:
            a = np.concatenate([a, rng.integers(0, 4, want - len(a), dtype=np.uint8)])
        return a[:want]
    return fit(q, qlen).tobytes(), fit(t, tlen).tobytes()


def gen_random(rng, qlen, tlen):
    return rng.integers(0, 4, qlen, dtype=np.uint8).tobytes(), rng.integers(0, 4, tlen, dtype=np.uint8).tobytes()


def gen_tandem(rng, qlen, tlen):
    """both sequences repeat one unit of 1-4 bases, out of phase, with an occasional substitution: many end cells share the best score"""
    unit = rng.integers(0, 4, int(rng.integers(1, 5)), dtype=np.uint8)

    def rep(n):
        ph = int(rng.integers(0, len(unit)))
        a = np.resize(np.roll(unit, -ph), n).copy()
        hit = rng.random(n) < 0.02
        a[hit] = rng.integers(0, 4, int(hit.sum()), dtype=np.uint8)
        return a.tobytes()
    return rep(qlen), rep(tlen)


def gen_homopolymer(rng, qlen, tlen):
    return bytes([int(rng.integers(0, 4))]) * qlen, bytes([int(rng.integers(0, 4))]) * tlen


GENERATORS = [("random", gen_random), ("related", lambda rng, a, b: related(rng, a, b, 0.10)), ("tandem", gen_tandem), ("homopolymer", gen_homopolymer)]


def generated_jobs(rng, n, max_len=149):
    """[(generator name, scoring, q, t)]"""
    out = []
    for i in range(n):
        name, g = GENERATORS[i % 4]
        sc = SCORINGS[int(rng.integers(0, len(SCORINGS)))]
        q, t = g(rng, int(rng.integers(1, max_len + 1)), int(rng.integers(1, max_len + 1)))
        out.append((name, sc, q, t))
    return out


# ---------------------------------------------------------------------------------------------------------
# checks
# ---------------------------------------------------------------------------------------------------------
class env(object):
    """environment variables for the duration of a call (the entry point reads them at every call)"""

    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        for k, v in self.kv.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = str(v)

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def run(mm, jobs, sc):
    return mm.ksw_ll_batch(jobs, mat_of(sc), sc[2], sc[3])


def want_of(jobs, sc):
    mat = mat_of(sc)
    return [ref_ll(*transform(j[0], j[1], j[2] if len(j) > 2 else 0), mat, sc[2], sc[3]) for j in jobs]


def check(mm, jobs, sc, path=None, want=None):
    """every job's (score, qe, te) equals the reference's; path: the class every job must report (None: any); returns the paths"""
    got = run(mm, jobs, sc)
    want = want or want_of(jobs, sc)
    assert len(got) == len(jobs)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g[:3] == w, "job %d (%d x %d, flag %d, scoring %r, path %d): got %r, the reference %r" % (
            i, len(jobs[i][0]), len(jobs[i][1]), jobs[i][2] if len(jobs[i]) > 2 else 0, sc, g[3], g[:3], w)
        if path is not None:
            assert g[3] == path, "job %d (%d x %d): path %d, expected %d" % (i, len(jobs[i][0]), len(jobs[i][1]), g[3], path)
    return [g[3] for g in got]


def check_directed(mm):
    """case 1: lengths around the lane, wave and strip widths, under three scorings"""
    W = mm.ksw_ll_limits()["strip_cols"]
    rng = np.random.default_rng(11)
    qlens = [1, 7, 8, 9, 63, 64, 65, W - 1, W, W + 1, 2 * W + 1]
    tlens = [1, 2, 63, 64, 65, 129, 300]
    for sc in DIRECTED_SCORINGS:
        jobs = [related(rng, ql, tl, 0.10, 0.03 if sc[5] else 0.0) for ql in qlens for tl in tlens]
        paths = check(mm, jobs, sc)
        assert HOST not in paths
        want = want_of(jobs, sc)
        assert sum(1 for w in want if w[0] > 20) > len(jobs) // 3  # where both sequences are long the maximum is not trivial


def check_generated(mm, n=300, seed=5):
    """case 2: four generators x nine scorings; and the inputs bite"""
    rng = np.random.default_rng(seed)
    jobs = generated_jobs(rng, n)
    n_host = 0
    tandem = [0, 0, 0]   # plain-class tandem jobs; qe not the largest tied column; not the smallest
    homo = [0, 0]        # homopolymer jobs; scoring 0
    for sc in SCORINGS:
        mine = [j for j in jobs if j[1] == sc]
        if not mine:
            continue
        pairs = [(j[2], j[3]) for j in mine]
        want = want_of(pairs, sc)
        paths = check(mm, pairs, sc, want=want)
        mat = mat_of(sc)
        for j, w, p in zip(mine, want, paths):
            plain = plain_class(len(j[2]), len(j[3]), mat, sc[2], sc[3])
            assert (p == HOST) == (not plain)
            n_host += p == HOST
            if j[0] == "homopolymer":
                homo[0] += 1
                homo[1] += w[0] == 0
            if j[0] == "tandem" and plain:
                G, te, cols = tied_columns(j[2], j[3], mat, sc[2], sc[3])
                assert (G, te) == (w[0], w[2])
                tandem[0] += 1
                if G > 0:
                    assert w[1] in cols
                    tandem[1] += w[1] != max(cols)
                    tandem[2] += w[1] != min(cols)
    print("generated jobs: %d, HOST %d; tandem (plain class) %d, qe not the largest tied column %d, not the smallest %d; homopolymer %d, scoring 0: %d" % (
        n, n_host, tandem[0], tandem[1], tandem[2], homo[0], homo[1]))
    assert tandem[0] >= n // 8 and tandem[1] >= 0.20 * tandem[0] and tandem[2] >= 0.20 * tandem[0]
    assert n_host >= 0.15 * n
    assert homo[1] >= 0.5 * homo[0]


def check_flags(mm):
    """case 3: every combination of the three flags on 20 related pairs"""
    rng = np.random.default_rng(13)
    W = mm.ksw_ll_limits()["strip_cols"]
    pairs = [related(rng, int(rng.integers(20, 200)), int(rng.integers(20, 200)), 0.10, 0.02) for _ in range(18)]
    pairs += [related(rng, W + 30, 90, 0.10), related(rng, 90, W + 30, 0.10)]
    # a reverse complement that aligns: the query is the target's other strand
    t0 = rng.integers(0, 4, 120, dtype=np.uint8)
    pairs[0] = (COMP5[t0[::-1]].tobytes(), t0.tobytes())
    jobs = [(q, t, f) for q, t in pairs for f in range(8)]
    check(mm, jobs, SCORINGS[0])
    want = want_of(jobs, SCORINGS[0])
    assert want[QREV | QCOMP][0] == 2 * len(pairs[0][1]) and want[0][0] < want[QREV | QCOMP][0]
    assert len(set(w for w in want[8:16])) > 2  # the flags change the answer


def check_workgroup(mm):
    """case 4: the workgroup class at its smallest shapes (MM2AMD_LL_WG_MIN_CELLS=0)"""
    lim = mm.ksw_ll_limits()
    W, n = lim["strip_cols"], lim["wg_waves"]
    rng = np.random.default_rng(17)
    qlens = [W + 1, 2 * W, n * W + 1, 2 * n * W + 1]
    tlens = [1, 2, 63, 64, 65, 127, 128, 129, 191, 193, 257]
    with env(MM2AMD_LL_WG_MIN_CELLS=0, MM2AMD_LL_NO_WG=None):
        assert mm.ksw_ll_limits()["wg_min_cells"] == 0
        for sc in (SCORINGS[0], SCORINGS[3]):
            jobs = [related(rng, ql, tl, 0.10, 0.03 if sc[5] else 0.0) for ql in qlens for tl in tlens]
            check(mm, jobs, sc, path=WG)
        # a job of one strip stays with the wave class whatever the threshold
        assert check(mm, [related(rng, W, 70, 0.1)], SCORINGS[0]) == [WAVE]


def check_limits(mm, wg_min_cells=None):
    """case 5: the length limit, the score limit, the workgroup threshold and MM2AMD_LL_NO_WG.  wg_min_cells: a threshold to run the third and fourth
    part at (the emulator's suite; None: the library's own)"""
    lim = mm.ksw_ll_limits()
    assert lim["max_len"] == 65535
    rng = np.random.default_rng(19)
    sc = SCORINGS[0]
    q8, t = related(rng, 8, lim["max_len"] + 1, 0.10)
    assert check(mm, [(q8, t[:-1]), (q8, t)], sc)[1] == HOST
    assert check(mm, [(q8, t[:-1])], sc)[0] != HOST
    a100 = (100, 4, 4, 2, 1, 0)
    s = rng.integers(0, 4, 320, dtype=np.uint8).tobytes()
    got = run(mm, [(s[:319], s[:319]), (s, s)], a100)
    assert got[0][0] == 31900 and got[0][3] != HOST and got[1][0] == 32000 and got[1][3] == HOST
    check(mm, [(s[:319], s[:319]), (s, s)], a100)
    with env(MM2AMD_LL_WG_MIN_CELLS=wg_min_cells, MM2AMD_LL_NO_WG=None):
        lim = mm.ksw_ll_limits()
        cells, W = lim["wg_min_cells"], lim["strip_cols"]
        ql = next(x for x in range(W + 1, lim["max_len"] + 1) if cells % x == 0 and cells // x <= lim["max_len"])
        tl = cells // ql
        q, t = related(rng, ql, tl, 0.10)
        want = want_of([(q, t), (q, t[:-1])], sc)
        assert check(mm, [(q, t), (q, t[:-1])], sc, want=want) == [WG, WAVE]
        with env(MM2AMD_LL_NO_WG=1):
            assert check(mm, [(q, t)], sc, want=want[:1]) == [WAVE]


def check_mixed(mm, n_small=2000, big=1500):
    """case 6: a mixed batch comes back in job order, and buffers kept between calls carry nothing over"""
    rng = np.random.default_rng(23)
    sc = SCORINGS[1]
    small = [related(rng, int(rng.integers(50, 61)), int(rng.integers(50, 61)), 0.10) for _ in range(n_small)]  # mm_seed_ext_score: span 15 + 2 * 20
    bigs = [related(rng, big, big, 0.10) for _ in range(3)]
    jobs = small[:n_small // 2] + [bigs[0], (b"", b"\1\2")] + small[n_small // 2:] + [bigs[1], (b"\0", b""), bigs[2]]
    want = want_of(jobs, sc)
    first = run(mm, jobs, sc)
    assert [g[:3] for g in first] == want
    assert first[n_small // 2 + 1] == (0, -1, -1, HOST) and first[-2] == (0, -1, -1, HOST)
    assert run(mm, jobs, sc) == first
    fewer = jobs[5:n_small // 3] + [bigs[2]]
    assert [g[:3] for g in run(mm, fewer, sc)] == want[5:n_small // 3] + [want[-1]]
    assert run(mm, jobs, sc) == first


def check_bookkeeping(mm):
    """case 7: the EINVAL cases and the empty batch"""
    L = mm.lib()
    mat = mat_of(SCORINGS[0])
    qb, tb = b"\0\1\2\3", b"\0\1\2\3"

    def one(qlen=4, tlen=4, q=qb, t=tb):
        a = (mm.LlJob * 1)()
        a[0].query, a[0].target = C.cast(C.c_char_p(q), C.c_void_p), C.cast(C.c_char_p(t), C.c_void_p)
        a[0].qlen, a[0].tlen, a[0].flag = qlen, tlen, 0
        return a
    res = (mm.LlRes * 1)()
    assert L.mm2amd_ksw_ll_batch(1, one(), 5, mat, 4, 2, res) == 0 and (res[0].score, res[0].qe, res[0].te) == (8, 3, 3)
    assert L.mm2amd_ksw_ll_batch(1, one(), 4, mat, 4, 2, res) == mm.EINVAL
    assert L.mm2amd_ksw_ll_batch(1, one(), 5, None, 4, 2, res) == mm.EINVAL
    assert L.mm2amd_ksw_ll_batch(1, None, 5, mat, 4, 2, res) == mm.EINVAL
    assert L.mm2amd_ksw_ll_batch(1, one(), 5, mat, 4, 2, None) == mm.EINVAL
    assert L.mm2amd_ksw_ll_batch(-1, one(), 5, mat, 4, 2, res) == mm.EINVAL
    assert L.mm2amd_ksw_ll_batch(1, one(qlen=-1), 5, mat, 4, 2, res) == mm.EINVAL
    assert L.mm2amd_ksw_ll_batch(1, one(tlen=-1), 5, mat, 4, 2, res) == mm.EINVAL
    assert L.mm2amd_ksw_ll_batch(1, one(q=b"\0\1\5\3"), 5, mat, 4, 2, res) == mm.EINVAL
    assert L.mm2amd_ksw_ll_batch(1, one(t=b"\0\1\2\7"), 5, mat, 4, 2, res) == mm.EINVAL
    j = one()
    j[0].query = None
    assert L.mm2amd_ksw_ll_batch(1, j, 5, mat, 4, 2, res) == mm.EINVAL
    assert b"ksw_ll_batch" in L.mm2amd_last_error()
    assert L.mm2amd_ksw_ll_batch(0, None, 5, mat, 4, 2, None) == 0
    assert mm.ksw_ll_batch([], mat, 4, 2) == []
    assert L.mm2amd_ksw_ll_limits(None, None, None, None) == 0
