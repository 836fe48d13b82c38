"""Shared by tests/test_gpu_split.py and tests/test_split_emu.py (not a test): hit lists for hits_merge_kernel behind mm2amd_hits_merge_batch -- the
rules merge_hits (map.c:520-531) applies to a read segment's hits once the records of all index parts are in one list -- and the judge they are
measured by: the UNMODIFIED compiled reference (oracle/_ref/libminimap2_ref.so) through ctypes, mm_hit_sort, mm_set_parent, mm_select_sub and
mm_set_sam_pri (hit.c:125-281) on mm_reg1_t records whose mm_extra_t blocks are libc allocations, as the reference frees the ones it drops.
Every list goes three more ways: the kernel, the host twin, and the host twin running the kernel's lane-wise mm_set_parent."""
import ctypes as C
import os
import random
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import reflib  # noqa: E402

HAVE_REF = os.path.exists(reflib.REF_SO)
NARROW, WIDE, HOST = 0, 1, 2  # minimap2_amd.HM_PATH_*
REV, INV, ALT, ALIGNED, SAM_PRI, STRAND_RETAINED = 1, 2, 4, 8, 16, 32  # minimap2_amd.HM_*
HARD_MLEVEL, ALL_CHAINS, CHECK_STRAND = 1, 2, 4
NARROW_CAP, WIDE_CAP, SORT_EXACT = 64, 448, 64  # what hits_merge_limits() must say; RS_MIN_SIZE
FIELDS = ("pos", "id", "parent", "subsc", "n_sub", "dp_max2", "flags")

_R = None
_libc = C.CDLL(None)
_libc.calloc.restype = C.c_void_p
_libc.calloc.argtypes = [C.c_size_t, C.c_size_t]
_libc.free.argtypes = [C.c_void_p]


def _ref(mm):
    global _R
    if _R is None:
        _R = C.CDLL(reflib.REF_SO)
        ip, rp = C.POINTER(C.c_int), C.POINTER(mm.Reg1)
        _R.mm_hit_sort.restype = None
        _R.mm_hit_sort.argtypes = [C.c_void_p, ip, rp, C.c_float]
        _R.mm_set_parent.restype = None
        _R.mm_set_parent.argtypes = [C.c_void_p, C.c_float, C.c_int, C.c_int, rp, C.c_int, C.c_int, C.c_float]
        _R.mm_select_sub.restype = None
        _R.mm_select_sub.argtypes = [C.c_void_p, C.c_float, C.c_int, C.c_int, C.c_int, C.c_int, ip, rp]
        _R.mm_set_sam_pri.argtypes = [C.c_int, rp]
    return _R


def ref_merge(mm, hits, opt):
    """the reference's steps on one list -> (an HM_OUT_DTYPE array answering the hits one by one, the length of the final list).  The input position
    travels in mm_reg1_t::blen, which none of the four routines reads."""
    R = _ref(mm)
    n0 = len(hits)
    out = np.zeros(n0, dtype=mm.HM_OUT_DTYPE)
    out["pos"] = -1
    if n0 == 0:
        return out, 0
    r = (mm.Reg1 * n0)()
    for i, h in enumerate(hits):
        x, f = r[i], int(h["flags"])
        x.cnt, x.rid, x.score, x.qs, x.qe, x.rs, x.re, x.hash = (int(h[k]) for k in ("cnt", "rid", "score", "qs", "qe", "rs", "re", "hash"))
        x.blen, x.parent = i, -1
        x.bits = (1 << 10 if f & REV else 0) | (1 << 11 if f & INV else 0) | (1 << 12 if f & SAM_PRI else 0) | (1 << 25 if f & ALT else 0) | (1 << 26 if f & STRAND_RETAINED else 0)
        if f & ALIGNED:
            x.p = C.cast(_libc.calloc(8, 4), C.POINTER(mm.Extra))
            x.p.contents.capacity, x.p.contents.dp_max = 8, int(h["dp_max"])
    n = C.c_int(n0)
    R.mm_hit_sort(None, C.byref(n), r, opt.alt_drop)
    R.mm_set_parent(None, opt.mask_level, opt.mask_len, n.value, r, opt.sub_diff, 1 if opt.flags & HARD_MLEVEL else 0, opt.alt_drop)
    if not opt.flags & ALL_CHAINS:
        R.mm_select_sub(None, opt.pri_ratio, opt.min_diff, opt.best_n, 1 if opt.flags & CHECK_STRAND else 0, opt.min_strand_sc, C.byref(n), r)
        R.mm_set_sam_pri(n.value, r)
    for k in range(n.value):
        x, o = r[k], out[r[k].blen]
        o["pos"], o["id"], o["parent"], o["subsc"], o["n_sub"] = k, x.id, x.parent, x.subsc, x.n_sub
        o["dp_max2"] = x.p.contents.dp_max2 if x.p else 0
        o["flags"] = (SAM_PRI if x.bits >> 12 & 1 else 0) | (STRAND_RETAINED if x.bits >> 26 & 1 else 0)
        if x.p:
            _libc.free(C.cast(x.p, C.c_void_p))
    return out, n.value


# ---------------------------------------------------------------------------------------------------------
# lists
# ---------------------------------------------------------------------------------------------------------
def hit(mm, qs, qe, score, rid=0, rs=None, re=None, cnt=10, hash=0, flags=0, dp_max=None):
    h = np.zeros(1, dtype=mm.HM_HIT_DTYPE)[0]
    h["qs"], h["qe"], h["score"], h["rid"], h["cnt"], h["hash"] = qs, qe, score, rid, cnt, hash
    h["rs"], h["re"] = (qs + 1000 if rs is None else rs), (qe + 1000 if re is None else re)
    if dp_max is not None:
        flags |= ALIGNED
        h["dp_max"] = dp_max
    h["flags"] = flags
    return h


def arr(mm, hs):
    return np.array(hs, dtype=mm.HM_HIT_DTYPE) if len(hs) else np.zeros(0, dtype=mm.HM_HIT_DTYPE)


def random_list(mm, rng, n, aligned, grid=100, span=4000, tie_every=0, n_parts=4, alt=0.0, dead=0.0):
    """n hits on a read of `span` bases with ends on a grid -- overlaps of exactly half of the shorter hit, the mask_level boundary, are common --
    and scores from a small range; distinct hashes unless tie_every, where every tie_every-th hit repeats its predecessor's score and hash (the same
    sequence at the same place of two parts)."""
    hs, hashes = [], rng.sample(range(1, 1 << 32), n)
    for i in range(n):
        a = rng.randrange(0, span // grid - 1)
        b = rng.randrange(a + 1, min(span // grid, a + 12) + 1)
        sc = rng.randrange(40, 120)
        hsh = hashes[i]
        if tie_every and i and i % tie_every == 0:
            sc, hsh = int(hs[-1]["dp_max"] if aligned else hs[-1]["score"]), int(hs[-1]["hash"])
        fl = (REV if rng.random() < 0.5 else 0) | (ALT if rng.random() < alt else 0)
        cnt = 0 if rng.random() < dead else rng.randrange(3, 30)
        rs = rng.randrange(0, 5) * 1000
        hs.append(hit(mm, a * grid, b * grid, sc if not aligned else rng.randrange(40, 120), rid=rng.randrange(n_parts), rs=rs, re=rs + (b - a) * grid,
                      cnt=cnt, hash=hsh, flags=fl, dp_max=sc if aligned else None))
    return arr(mm, hs)


def expected_class(hits, alt_drop):
    """which class a list takes: by its length, and -- above 64 live hits -- by whether two live hits have equal keys"""
    n = len(hits)
    if n > WIDE_CAP:
        return HOST
    live = [h for h in hits if (int(h["flags"]) & INV) or h["cnt"] > 0]
    if n > 1 and len(live) > SORT_EXACT:
        keys = [key_of(h, alt_drop) for h in live]
        if len(set(keys)) < len(keys):
            return HOST
    return NARROW if n <= NARROW_CAP else WIDE


def key_of(h, alt_drop):
    f = int(h["flags"])
    sc = int(h["dp_max"] if f & ALIGNED else h["score"])
    if f & ALT and sc >= 0:
        sc = max(int(sc * (1.0 - float(np.float32(alt_drop))) + .499), 1)  # mm_alt_score (hit.c:99-104), in double as there
    return sc << 32 | int(h["hash"])


def has_tie(hits, alt_drop):
    live = [key_of(h, alt_drop) for h in hits if (int(h["flags"]) & INV) or h["cnt"] > 0]
    return len(hits) > 1 and len(set(live)) < len(live)


def boundary_pairs(hits):
    """pairs of hits whose overlap is exactly half of the shorter one: (float)ol / min == mask_level for the default 0.5"""
    c = 0
    for i in range(len(hits)):
        for j in range(i):
            a, b = hits[i], hits[j]
            ol = min(int(a["qe"]), int(b["qe"])) - max(int(a["qs"]), int(b["qs"]))
            mn = min(int(a["qe"]) - int(a["qs"]), int(b["qe"]) - int(b["qs"]))
            c += ol > 0 and 2 * ol == mn
    return c


def directed(mm):
    """(name, list, options) -- see the issue's list of shapes; the classes follow from expected_class()"""
    rng = random.Random(20260101)
    D, cases = mm.hm_opt, []
    for n in (0, 1, 2, 63, 64, 65, WIDE_CAP, WIDE_CAP + 1):
        for aligned in (False, True):
            cases.append(("n%d_%s" % (n, "dp" if aligned else "chain"), random_list(mm, rng, n, aligned), D()))
    cases.append(("one_part", random_list(mm, rng, 30, True, n_parts=1), D()))
    cases.append(("one_dead_hit_alone", arr(mm, [hit(mm, 0, 100, 50, cnt=0, hash=7)]), D()))
    cases.append(("nested", arr(mm, [hit(mm, 0, 5000, 900, hash=1, dp_max=900)] + [hit(mm, 100 * i, 100 * i + 50 + 13 * i, 800 - i, rid=i % 3, hash=10 + i, dp_max=800 - 7 * i)
                                                                                   for i in range(1, 40)]), D()))
    cases.append(("disjoint", arr(mm, [hit(mm, 100 * i, 100 * i + 100, 50 + (i * 37) % 41, hash=100 + i) for i in range(70)]), D()))
    for where in ("front", "middle", "end"):
        hs = [hit(mm, 50 * i, 50 * i + 400, 300 - i, hash=1000 + i, dp_max=280 - 2 * i) for i in range(12)]
        for k in {"front": (0, 1), "middle": (5, 6), "end": (10, 11)}[where]:
            hs[k]["cnt"] = 0
        cases.append(("dead_" + where, arr(mm, hs), D()))
    hs = [hit(mm, 0, 1000, 500, hash=5, dp_max=500), hit(mm, 200, 260, 30, hash=6, cnt=0, flags=INV | REV, dp_max=30), hit(mm, 100, 900, 300, hash=7, dp_max=300),
          hit(mm, 150, 850, 90, hash=8, dp_max=90)]
    cases.append(("inversion", arr(mm, hs), D()))
    # equal keys: pairs and a run of five, among few hits (the insertion sort's fixed order) and among more than 64 live ones (the host's replay)
    for n, name in ((20, "ties_below"), (64, "ties_at_bound"), (65, "ties_above"), (200, "ties_wide")):
        for aligned in (False, True):
            l = random_list(mm, rng, n, aligned, tie_every=3)
            for k in range(5, 10):  # a run of five
                l[k]["hash"], l[k]["score"], l[k]["dp_max"] = l[5]["hash"], l[5]["score"], l[5]["dp_max"]
            cases.append(("%s_%s" % (name, "dp" if aligned else "chain"), l, D()))
    l = random_list(mm, rng, 70, True, tie_every=3, dead=0.0)
    for k in range(0, 70, 9):  # 70 hits, ties, but only 62 alive: the fixed order holds
        l[k]["cnt"] = 0
    cases.append(("ties_wide_list_few_alive", l, D()))
    for aligned in (False, True):
        l = random_list(mm, rng, 50, aligned)
        cases.append(("hard_mlevel_%d" % aligned, l, D(flags=HARD_MLEVEL)))
        cases.append(("all_chains_%d" % aligned, l, D(flags=ALL_CHAINS)))
        cases.append(("best_n_0_%d" % aligned, l, D(best_n=0)))
        cases.append(("best_n_1_%d" % aligned, l, D(best_n=1)))
        cases.append(("mask_len_%d" % aligned, l, D(mask_len=150)))
        cases.append(("pri_ratio_0_%d" % aligned, l, D(pri_ratio=0.0)))
        cases.append(("check_strand_%d" % aligned, l, D(flags=CHECK_STRAND, min_strand_sc=60, pri_ratio=0.95, min_diff=2)))
    # mask_len decides: the second hit overlaps the first by 0.8 of itself with 200 bases uncovered (0.8 - 200 / 1100 > 0.5), a secondary unless 200 > mask_len
    hs = [hit(mm, 0, 1100, 700, hash=21, dp_max=700), hit(mm, 300, 1300, 650, hash=22, dp_max=650), hit(mm, 350, 1250, 600, hash=23, dp_max=600),
          hit(mm, 0, 1000, 500, rid=1, hash=24, dp_max=500)]
    cases.append(("mask_len_binding", arr(mm, hs), D(mask_len=150)))
    l = random_list(mm, rng, 90, True)
    l["flags"] |= SAM_PRI
    cases.append(("all_chains_wide_keeps_sam_pri", l, D(flags=ALL_CHAINS)))
    # ALT: as owned (score marked down in the sort, in subsc and in dp_max2) and as owner (no handicap for an ALT hit under an ALT hit)
    hs = [hit(mm, 0, 1000, 400, hash=1, dp_max=400), hit(mm, 0, 990, 401, hash=2, flags=ALT, dp_max=403), hit(mm, 10, 1000, 333, hash=3, flags=ALT, dp_max=399),
          hit(mm, 2000, 3000, 377, hash=4, flags=ALT, dp_max=377), hit(mm, 2000, 2990, 300, hash=5, flags=ALT, dp_max=311), hit(mm, 2010, 3000, 310, hash=6, dp_max=318),
          hit(mm, 4000, 4500, 1, hash=7, flags=ALT, dp_max=1), hit(mm, 4000, 4400, -3, hash=8, flags=ALT, dp_max=-3)]
    cases.append(("alt_dp", arr(mm, hs), D(alt_drop=0.15)))
    hs2 = [hit(mm, int(h["qs"]), int(h["qe"]), int(h["dp_max"]), hash=int(h["hash"]), flags=int(h["flags"]) & ~ALIGNED, rid=i % 2) for i, h in enumerate(hs)]
    cases.append(("alt_chain", arr(mm, hs2), D(alt_drop=0.15)))
    for aligned in (False, True):
        cases.append(("alt_random_%d" % aligned, random_list(mm, rng, 120, aligned, alt=0.4), D(alt_drop=0.15)))
    # the same alignment found in two parts: mm_set_parent leaves dp_max2 alone, mm_select_sub drops the second
    hs = [hit(mm, 0, 800, 500, rid=2, rs=100, re=900, hash=11, dp_max=500), hit(mm, 0, 800, 500, rid=2, rs=100, re=900, hash=12, dp_max=500),
          hit(mm, 0, 800, 500, rid=3, rs=100, re=900, hash=13, dp_max=500), hit(mm, 0, 790, 480, rid=2, rs=100, re=890, hash=14, dp_max=480)]
    cases.append(("identical_pair", arr(mm, hs), D()))
    return cases


def compare(mm, cases, what=""):
    """every list through the kernel, the host twin in both forms and the reference; every field of every hit, the kept counts and the classes"""
    by_opt = {}
    for name, l, o in cases:
        by_opt.setdefault(bytes(o), (o, []))[1].append((name, l))
    classes = {NARROW: 0, WIDE: 0, HOST: 0}
    for o, group in by_opt.values():
        segs = [l for _, l in group]
        dev, dev_kept, dev_path = mm.hits_merge_batch(segs, o)
        host, host_kept, host_path, _ = mm.hits_merge_host_batch(segs, o, n_threads=2)
        lanes, lanes_kept, _, _ = mm.hits_merge_host_batch(segs, o, n_threads=2, wave_parents=True)
        for k, (name, l) in enumerate(group):
            want, want_kept = ref_merge(mm, l, o)
            for who, got, kept in (("kernel", dev[k], dev_kept[k]), ("host", host[k], host_kept[k]), ("host, lane-wise parents", lanes[k], lanes_kept[k])):
                assert kept == want_kept, "%s%s: %s keeps %d hits, the reference %d" % (what, name, who, kept, want_kept)
                for f in FIELDS:
                    bad = np.nonzero(got[f] != want[f])[0]
                    assert len(bad) == 0, "%s%s: %s, field %s of hit %d: %d, the reference has %d" % (what, name, who, f, bad[0], got[f][bad[0]], want[f][bad[0]])
                assert not got["reserved"].any()
            assert dev_path[k] == expected_class(l, o.alt_drop), "%s%s ran in class %d, not %d" % (what, name, dev_path[k], expected_class(l, o.alt_drop))
            assert host_path[k] == HOST
            classes[dev_path[k]] += 1
    return classes


# ---------------------------------------------------------------------------------------------------------
# the checks
# ---------------------------------------------------------------------------------------------------------
def check_limits(mm):
    assert mm.hits_merge_limits() == {"narrow_cap": NARROW_CAP, "wide_cap": WIDE_CAP, "max_hits": 1 << 20}


def check_directed(mm):
    cases = directed(mm)
    classes = compare(mm, cases)
    names = {n: l for n, l, _ in cases}
    want_host = {n for n, l, o in cases if expected_class(l, o.alt_drop) == HOST}
    # the host class holds the cases built for it and nothing else
    assert want_host == {"n449_chain", "n449_dp", "ties_above_chain", "ties_above_dp", "ties_wide_chain", "ties_wide_dp"}, sorted(want_host)
    assert classes[HOST] == len(want_host) and classes[NARROW] > 30 and classes[WIDE] >= 8, classes
    assert expected_class(names["ties_at_bound_dp"], 0.15) == NARROW and expected_class(names["ties_wide_list_few_alive"], 0.15) == WIDE
    # mask_len binds in its cases: with the bound lifted the reference gives some hit another parent, so at that hit the ratio test passed and only
    # `uncov <= mask_len` failed
    for n, l, o in cases:
        if n.startswith("mask_len_"):
            bound, _ = ref_merge(mm, l, o)
            free, _ = ref_merge(mm, l, mm.hm_opt(mask_len=0x7fffffff))
            both = (bound["pos"] >= 0) & (free["pos"] >= 0)
            assert o.mask_len == 150 and (((bound["pos"] >= 0) != (free["pos"] >= 0)).any() or (bound["parent"][both] != free["parent"][both]).any()), n
    b = ref_merge(mm, names["mask_len_binding"], mm.hm_opt(mask_len=150))[0]
    f = ref_merge(mm, names["mask_len_binding"], mm.hm_opt())[0]
    assert b["parent"][1] == b["id"][1] and f["parent"][1] == f["id"][0] and f["parent"][1] != f["id"][1]  # a primary under the bound, the first hit's secondary without it


def check_random(mm, n_lists, seed=7):
    """lists of 2 .. 130 hits: a third with equal keys, the ends on a grid that puts overlaps on the mask_level boundary; the counts of both are asserted"""
    rng = random.Random(seed)
    cases, n_tie, n_bound, n_host = [], 0, 0, 0
    opts = [mm.hm_opt(), mm.hm_opt(flags=HARD_MLEVEL, best_n=2), mm.hm_opt(mask_len=250, pri_ratio=0.5, best_n=20, alt_drop=0.15)]
    for k in range(n_lists):
        n = rng.randrange(2, 30) if k % 8 else rng.randrange(30, 131)
        l = random_list(mm, rng, n, aligned=k % 2 == 1, tie_every=(rng.randrange(2, 6) if k % 3 == 0 and n <= SORT_EXACT else 0), alt=0.2 if k % 5 == 0 else 0.0,
                        dead=0.1 if k % 7 == 0 else 0.0)
        if all(h["cnt"] == 0 for h in l):  # (the reference asserts that a list of two or more has a live hit)
            l[0]["cnt"] = 5
        o = opts[k % 3]
        n_tie += has_tie(l, o.alt_drop)
        n_bound += boundary_pairs(l)
        n_host += expected_class(l, o.alt_drop) == HOST
        cases.append(("random%d" % k, l, o))
    assert n_tie >= n_lists // 5 and n_bound >= n_lists and n_host == 0, (n_tie, n_bound, n_host)
    classes = compare(mm, cases, "seed %d, " % seed)
    assert classes[HOST] == 0 and classes[WIDE] >= n_lists // 20 and classes[NARROW] >= n_lists // 2, classes


def check_bookkeeping(mm):
    """an empty batch, empty segments between others, offsets that do not start at 0 (through the C entry), bad arguments, the profile's rows"""
    assert mm.hits_merge_batch([]) == ([], [], [])
    rng = random.Random(3)
    segs = [random_list(mm, rng, 0, False), random_list(mm, rng, 5, False), random_list(mm, rng, 0, False), random_list(mm, rng, 100, True), random_list(mm, rng, 0, True)]
    mm.profile_enable(True)
    out, kept, path = mm.hits_merge_batch(segs)
    prof = mm.profile_get()
    mm.profile_enable(False)
    assert path == [NARROW, NARROW, NARROW, WIDE, NARROW] and kept[0] == kept[2] == kept[4] == 0
    assert prof["hits_merge_kernel[narrow]"]["launches"] == 1 and prof["hits_merge_kernel[wide]"]["launches"] == 1
    assert prof["hits_merge_kernel[narrow]"]["units"] == 5 and prof["hits_merge_kernel[wide]"]["units"] == 100
    for k in (1, 3):
        want, want_kept = ref_merge(mm, segs[k], mm.hm_opt())
        assert kept[k] == want_kept and all((out[k][f] == want[f]).all() for f in FIELDS)
    # offsets counted from the middle of an array
    L, o = mm.lib(), mm.hm_opt()
    hits = np.concatenate([segs[1], segs[3]])
    off = np.array([5, 105], dtype=np.uint64)
    res = np.zeros(105, dtype=mm.HM_OUT_DTYPE)
    res["pos"] = -7
    seg = np.zeros((1, 2), dtype=np.int32)
    assert L.mm2amd_hits_merge_batch(1, off.ctypes.data, hits.ctypes.data, C.byref(o), res.ctypes.data, seg.ctypes.data) == 0
    assert (res["pos"][:5] == -7).all() and all((res[5:][f] == out[3][f]).all() for f in FIELDS) and list(seg[0]) == [kept[3], WIDE]
    bad = np.array([5, 3], dtype=np.uint64)
    assert L.mm2amd_hits_merge_batch(1, bad.ctypes.data, hits.ctypes.data, C.byref(o), res.ctypes.data, seg.ctypes.data) == mm.EINVAL
    assert L.mm2amd_hits_merge_batch(1, off.ctypes.data, hits.ctypes.data, None, res.ctypes.data, seg.ctypes.data) == mm.EINVAL


# ---------------------------------------------------------------------------------------------------------
# end to end: map_split against the reference binary's --split-prefix run
# ---------------------------------------------------------------------------------------------------------
import subprocess  # noqa: E402

FIX = os.path.join(HERE, "golden", "ref_fixtures")
_COMP = bytes.maketrans(b"ACGT", b"TGCA")


def _fasta(fn):
    with open(fn, "rb") as f:
        return b"".join(l.strip() for l in f if not l.startswith(b">")).upper()


def _mutate(rng, s, rate):
    out = bytearray()
    for c in s:
        x = rng.random()
        if x < rate / 3:
            continue  # deletion
        if x < 2 * rate / 3:
            out.append(rng.choice(b"ACGT"))  # substitution
            continue
        out.append(c)
        if x < rate:
            out.append(rng.choice(b"ACGT"))  # insertion
    return bytes(out)


def four_contigs(seed=5):
    """MT-human, MT-orang, a 3 %-diverged copy of MT-human and 9 kb of random sequence"""
    rng = random.Random(seed)
    human, orang = _fasta(os.path.join(FIX, "MT-human.fa")), _fasta(os.path.join(FIX, "MT-orang.fa"))
    human = bytes(c if c in b"ACGT" else 65 for c in human)
    orang = bytes(c if c in b"ACGT" else 65 for c in orang)
    return [(b"MT_human", human), (b"MT_orang", orang), (b"MT_human_div", _mutate(rng, human, 0.03)), (b"random9k", bytes(rng.choice(b"ACGT") for _ in range(9000)))]


def long_reads(contigs, n=60, seed=9, err=0.08):
    """n simulated 0.4-3 kb reads at 8 % error, half reverse-complemented, every tenth a chimera of two places"""
    rng = random.Random(seed)

    def piece():
        s = contigs[rng.randrange(len(contigs))][1]
        ln = rng.randrange(400, 3000)
        a = rng.randrange(0, len(s) - ln)
        return s[a:a + ln]
    reads = []
    for i in range(n):
        s = piece() if i % 10 else piece()[:1500] + piece()[:1500]
        s = _mutate(rng, s, err)
        if rng.random() < 0.5:
            s = s.translate(_COMP)[::-1]
        reads.append((b"read%d" % i, s))
    return reads


def short_pairs(contigs, n=80, seed=13):
    rng = random.Random(seed)
    r1, r2 = [], []
    for i in range(n):
        s = contigs[rng.randrange(3)][1]
        a = rng.randrange(0, len(s) - 400)
        ins = rng.randrange(250, 400)
        f = _mutate(rng, s[a:a + ins], 0.01)
        x, y = f[:100], f[-100:].translate(_COMP)[::-1]
        if rng.random() < 0.5:
            x, y = y, x
        r1.append((b"pair%d" % i, x)), r2.append((b"pair%d" % i, y))
    return r1, r2


def write_fasta(fn, recs):
    with open(fn, "wb") as f:
        for nm, s in recs:
            f.write(b">" + nm + b"\n" + s + b"\n")


def write_fastq(fn, recs):
    with open(fn, "wb") as f:
        for nm, s in recs:
            f.write(b"@" + nm + b"\n" + s + b"\n+\n" + b"I" * len(s) + b"\n")


def ref_index(tmp, contigs, preset, batch):
    """a .mmi built by the reference binary with -I batch; returns (file name, number of parts the binary reports)"""
    fa, mmi = os.path.join(tmp, "ref.fa"), os.path.join(tmp, "ref_%s.mmi" % batch)
    write_fasta(fa, contigs)
    subprocess.run([reflib.REF_BIN, "-x", preset, "-I", batch, "-d", mmi, fa], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    return mmi


def ref_run(args):
    """the reference binary's stdout without its @PG line"""
    out = subprocess.run([reflib.REF_BIN] + args, check=True, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL).stdout
    return b"".join(l for l in out.splitlines(True) if not l.startswith(b"@PG"))


def flags_of(sam):
    return [int(l.split(b"\t")[1]) for l in sam.splitlines() if not l.startswith(b"@")]


def check_map_split(mm, tmp, preset, batch, want_parts, sam=True, ref_args=(), pairs=False, contigs=None, min_parts=2, **kw):
    """map_split against `minimap2 --split-prefix`; returns (our text, the reference's text of the same run, the reference's without the prefix)"""
    tmp = str(tmp)
    contigs = contigs or four_contigs()
    mmi = ref_index(tmp, contigs, preset, batch)
    if pairs:
        r1, r2 = short_pairs(contigs)
        files = [os.path.join(tmp, "r1.fq"), os.path.join(tmp, "r2.fq")]
        write_fastq(files[0], r1), write_fastq(files[1], r2)
    else:
        files = [os.path.join(tmp, "reads.fq")]
        write_fastq(files[0], long_reads(contigs))
    base = (["-a"] if sam else []) + ["-x", preset] + list(ref_args)
    want = ref_run(base + ["--split-prefix", os.path.join(tmp, "refpre"), mmi] + files)
    apart = ref_run(base + [mmi] + files)
    out = os.path.join(tmp, "ours.txt")
    n = mm.map_split(mmi, files if pairs else files[0], os.path.join(tmp, "ourpre"), out, preset=preset, sam=sam, n_threads=2, **kw)
    with open(out, "rb") as f:
        got = f.read()
    assert n == want_parts and n >= min_parts, n
    assert not [x for x in os.listdir(tmp) if x.endswith(".tmp")], "temp files left behind"
    assert got == want, _first_difference(got, want)
    return got, want, apart


def _first_difference(got, want):
    g, w = got.splitlines(), want.splitlines()
    for i, (a, b) in enumerate(zip(g, w)):
        if a != b:
            return "line %d:\nours      %r\nreference %r" % (i, a[:300], b[:300])
    return "%d lines against %d" % (len(g), len(w))


def per_read(text):
    """records per read name (header lines left out)"""
    c = {}
    for l in text.splitlines():
        if not l.startswith(b"@"):
            c[l.split(b"\t")[0]] = c.get(l.split(b"\t")[0], 0) + 1
    return c


def check_preconditions(got, apart, contigs_per_part, sam=True):
    """what makes an end-to-end run a test of the merge: hits of one read from several parts, secondary and supplementary records, a result other than the
    parts' own, and no read with more hits than the kernel's exact sort takes (so none in the host class)"""
    assert got != apart
    col = 2 if sam else 5
    by_read = {}
    for l in apart.splitlines():
        if not l.startswith(b"@"):
            f = l.split(b"\t")
            by_read.setdefault(f[0], set()).add(contigs_per_part[f[col]] if f[col] in contigs_per_part else None)
    assert sum(1 for v in by_read.values() if len(v - {None}) > 1) >= 5, "few reads with hits in more than one part"
    assert max(per_read(apart).values()) <= SORT_EXACT
    if sam:
        fl = flags_of(got)
        assert any(f & 2048 for f in fl) and any(f & 256 for f in fl)


def part_of(contigs, n_parts):
    """contig name -> part, for the four contigs cut into 2 or 4 parts"""
    return {nm: (i * n_parts) // len(contigs) for i, (nm, _) in enumerate(contigs)}


def check_e2e(mm, tmp, which):
    c = four_contigs()
    if which == "ont2":
        got, want, apart = check_map_split(mm, tmp, "map-ont", "30k", 2)
        check_preconditions(got, apart, part_of(c, 2))
    elif which == "ont4":
        got, want, apart = check_map_split(mm, tmp, "map-ont", "10k", 4)
        check_preconditions(got, apart, part_of(c, 4))
        assert [l for l in got.splitlines() if l.startswith(b"@SQ")] == [b"@SQ\tSN:%s\tLN:%d" % (nm, len(s)) for nm, s in c]
    elif which == "paf4":
        got, want, apart = check_map_split(mm, tmp, "map-ont", "10k", 4, sam=False, ref_args=["-c", "-N", "20", "-p", "0.3"], extra_flags=0x020,
                                           opt_overrides={"best_n": 20, "pri_ratio": 0.3})
        check_preconditions(got, apart, part_of(c, 4), sam=False)
    elif which == "sr2":
        got, want, apart = check_map_split(mm, tmp, "sr", "30k", 2, pairs=True)
        assert got != apart and all(f & 1 for f in flags_of(got)) and sum(1 for f in flags_of(got) if f & 2) >= 100
    elif which == "paf_no_hit":
        got, want, apart = check_map_split(mm, tmp, "map-ont", "30k", 2, sam=False, ref_args=["--paf-no-hit"], extra_flags=0x8000000, cigar=False)
        assert got != apart
    elif which == "one_part":
        check_map_split(mm, tmp, "map-ont", "1G", 1, min_parts=1)
    else:
        raise ValueError(which)


def read_tmp(fn, cigar=True):
    """a temp file -> (header bytes, [per segment (n_reg, rep_len, frag_gap, [(the 72 bytes of mm_reg1_t before p, the alignment block)])])"""
    import struct
    with open(fn, "rb") as f:
        d = f.read()
    k, n_seq = struct.unpack_from("<II", d, 0)
    o = 8
    for _ in range(n_seq):
        l, = struct.unpack_from("<I", d, o)
        o += 4 + l + 4
    head, segs = d[:o], []
    while o < len(d):
        n_reg, rep_len, frag_gap = struct.unpack_from("<iii", d, o)
        o += 12
        hits = []
        for _ in range(n_reg):
            rec = d[o:o + 72]
            o += 80
            blk = b""
            if cigar:
                cap, = struct.unpack_from("<I", d, o)
                blk = d[o + 4:o + 4 + 4 * cap]
                o += 4 + 4 * cap
            hits.append((rec, blk))
        segs.append((n_reg, rep_len, frag_gap, hits))
    return head, segs


def check_equal_keys_e2e(mm, tmp):
    """two parts that both begin with a copy of one contig: the same hit with the same score and hash from either part"""
    tmp = str(tmp)
    c = four_contigs()
    contigs = [(b"dupA", c[0][1]), (b"x_orang", c[1][1]), (b"dupB", c[0][1]), (b"y_random", c[3][1])]
    mmi = ref_index(tmp, contigs, "map-ont", "30k")
    fq = os.path.join(tmp, "reads.fq")
    write_fastq(fq, long_reads(contigs))
    want = ref_run(["-a", "-x", "map-ont", "--split-prefix", os.path.join(tmp, "refpre"), mmi, fq])
    pre, out = os.path.join(tmp, "ourpre"), os.path.join(tmp, "ours.sam")
    assert mm.map_split(mmi, fq, pre, out, preset="map-ont", sam=True, n_threads=2, keep_tmp=True) == 2
    import struct
    s0, s1 = read_tmp(pre + ".0000.tmp")[1], read_tmp(pre + ".0001.tmp")[1]
    key = lambda rec: (struct.unpack_from("<i", rec, 12)[0], struct.unpack_from("<I", rec, 64)[0])  # noqa: E731  (score, hash)
    ties = sum(1 for a, b in zip(s0, s1) if {key(r) for r, _ in a[3]} & {key(r) for r, _ in b[3]})
    assert ties >= 10, ties
    os.remove(pre + ".0000.tmp"), os.remove(pre + ".0001.tmp")
    with open(out, "rb") as f:
        got = f.read()
    assert got == want, _first_difference(got, want)


def check_refusals(mm, tmp):
    tmp = str(tmp)
    mmi = ref_index(tmp, four_contigs(), "map-ont", "30k")
    fq = os.path.join(tmp, "reads.fq")
    write_fastq(fq, long_reads(four_contigs(), n=3))
    for kw in ({"cs": True}, {"MD": True}, {"ds": True}, {"write_junc": True}):
        try:
            mm.map_split(mmi, fq, os.path.join(tmp, "p"), os.path.join(tmp, "o"), preset="map-ont", **kw)
        except mm.Mm2AmdError as e:
            assert e.code == mm.EINVAL and "split-prefix" in str(e)
        else:
            raise AssertionError("map_split took %r" % kw)
    # the merge handle itself refuses the flags, as the reference's option check refuses cs and MD
    o = mm.MapOpt()
    mm.lib().mm2amd_mapopt_init(C.byref(o))
    o.flag |= 0x040
    assert not mm.lib().mm2amd_split_merge_open(os.path.join(tmp, "p").encode(), 1, C.byref(o)) and mm.lib().mm2amd_last_error_code() == mm.EINVAL


_MERGE_CHILD = r"""
import ctypes as C, sys
sys.path.insert(0, sys.argv[1])
import minimap2_amd as mm
R = C.CDLL(sys.argv[2])
io, mo = mm.IdxOpt(), mm.MapOpt()
R.mm_set_opt(None, C.byref(io), C.byref(mo))
assert R.mm_set_opt(sys.argv[3].encode(), C.byref(io), C.byref(mo)) == 0
mo.flag |= mm.F_CIGAR | mm.F_OUT_SAM
keep = sys.argv[4].encode()
mo.split_prefix = keep
files = [a.encode() for a in sys.argv[6:]]
arr = (C.c_char_p * len(files))(*files)
R.mm_split_merge.argtypes = [C.c_int, C.POINTER(C.c_char_p), C.c_void_p, C.c_int]
rc = R.mm_split_merge(len(files), arr, C.byref(mo), int(sys.argv[5]))
C.CDLL(None).fflush(None)
sys.exit(0 if rc == 0 else 3)
"""

_FIRST_PASS_CHILD = r"""
import ctypes as C, sys
sys.path.insert(0, sys.argv[1])
import minimap2_amd as mm
R = C.CDLL(sys.argv[2])
io, mo = mm.IdxOpt(), mm.MapOpt()
R.mm_set_opt(None, C.byref(io), C.byref(mo))
assert R.mm_set_opt(sys.argv[3].encode(), C.byref(io), C.byref(mo)) == 0
mo.flag |= mm.F_CIGAR | mm.F_OUT_SAM
keep = sys.argv[4].encode()
mo.split_prefix = keep
R.mm_idx_reader_open.restype = C.c_void_p
R.mm_idx_reader_open.argtypes = [C.c_char_p, C.c_void_p, C.c_char_p]
R.mm_idx_reader_read.restype = C.c_void_p
R.mm_idx_reader_read.argtypes = [C.c_void_p, C.c_int]
R.mm_mapopt_update.argtypes = [C.c_void_p, C.c_void_p]
R.mm_map_file_frag.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_char_p), C.c_void_p, C.c_int]
R.mm_idx_destroy.argtypes = [C.c_void_p]
files = [a.encode() for a in sys.argv[6:]]
arr = (C.c_char_p * len(files))(*files)
rd = R.mm_idx_reader_open(sys.argv[5].encode(), C.byref(io), None)
n = 0
while True:
    mi = R.mm_idx_reader_read(rd, 2)
    if not mi:
        break
    R.mm_mapopt_update(C.byref(mo), mi)
    assert R.mm_map_file_frag(mi, len(files), arr, C.byref(mo), 2) == 0
    R.mm_idx_destroy(mi)
    n += 1
C.CDLL(None).fflush(None)
sys.exit(0 if n else 3)
"""


def check_temp_files_both_ways(mm, tmp):
    """our temp files merged by the reference's mm_split_merge; the reference's own temp files against ours byte by byte outside the p field, and merged by us"""
    tmp = str(tmp)
    contigs = four_contigs()
    mmi = ref_index(tmp, contigs, "map-ont", "30k")
    fq = os.path.join(tmp, "reads.fq")
    write_fastq(fq, long_reads(contigs))
    want = ref_run(["-a", "-x", "map-ont", "--split-prefix", os.path.join(tmp, "refpre"), mmi, fq])
    body = b"".join(l for l in want.splitlines(True) if not l.startswith(b"@HD"))
    ours, theirs, out = os.path.join(tmp, "ours"), os.path.join(tmp, "theirs"), os.path.join(tmp, "ours.sam")
    assert mm.map_split(mmi, fq, ours, out, preset="map-ont", sam=True, n_threads=2, keep_tmp=True) == 2
    root = os.path.dirname(HERE)
    subprocess.run([sys.executable, "-c", _FIRST_PASS_CHILD, root, reflib.REF_SO, "map-ont", theirs, mmi, fq], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    for j in range(2):
        a, b = read_tmp("%s.%.4d.tmp" % (ours, j)), read_tmp("%s.%.4d.tmp" % (theirs, j))
        assert a[0] == b[0], "the header of part %d differs" % j
        assert len(a[1]) == len(b[1])
        for k, (x, y) in enumerate(zip(a[1], b[1])):
            assert x[:3] == y[:3], "part %d, segment %d: counts %r against %r" % (j, k, x[:3], y[:3])
            for (r1, b1), (r2, b2) in zip(x[3], y[3]):
                assert r1 == r2, "part %d, segment %d: a record differs outside p" % (j, k)
                n1 = int.from_bytes(b1[24:28], "little")
                assert b1[4:28 + 4 * n1] == b2[4:28 + 4 * n1], "part %d, segment %d: an alignment block differs" % (j, k)  # (beyond capacity itself, up to the CIGAR's end)
    # ours, merged by the reference (which removes the files)
    got = subprocess.run([sys.executable, "-c", _MERGE_CHILD, root, reflib.REF_SO, "map-ont", ours, "2", fq], check=True, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL).stdout
    assert got == body, _first_difference(got, body)
    # theirs, merged by us
    al_opt = mm.MapOpt()
    io = mm.IdxOpt()
    mm.lib().mm2amd_set_opt(None, C.byref(io), C.byref(al_opt))
    mm.lib().mm2amd_set_opt(b"map-ont", C.byref(io), C.byref(al_opt))
    al_opt.flag |= mm.F_CIGAR | mm.F_OUT_SAM
    mg = mm.SplitMerger(theirs, 2, al_opt)
    text = mg.sq_lines()
    for b in mm.FastxReader(fq):
        n_reg, reg, rep_len, _ = mg.merge(b)
        text += mg.format(b, n_reg, reg, rep_len)
        mm.lib().mm2amd_free_regs(len(n_reg), n_reg, reg)
    mg.close()
    assert text == body, _first_difference(text, body)
    assert not [x for x in os.listdir(tmp) if x.endswith(".tmp")]


def check_switch(mm, tmp):
    """MM2AMD_DEVICE_MERGE: 0 and unset take the host's routines (no launch of hits_merge_kernel), 1 the kernel; the bytes are the same"""
    from sdust_cases import env
    texts = []
    for v, launched in ((0, False), (None, False), (1, True)):
        d = os.path.join(str(tmp), "v%s" % v)
        os.makedirs(d)
        with env(MM2AMD_DEVICE_MERGE=v):
            mm.profile_enable(True)
            try:
                got, _, _ = check_map_split(mm, d, "map-ont", "30k", 2)
                prof = mm.profile_get()
            finally:
                mm.profile_enable(False)
        n = sum(r["launches"] for k, r in prof.items() if k.startswith("hits_merge_kernel"))
        assert (n > 0) == launched, (v, n)
        texts.append(got)
    assert texts[0] == texts[1] == texts[2]


def check_fasta_parts(mm, tmp):
    """the reference as a FASTA cut into -I-sized chunks by map_split itself, against the reference binary doing the same"""
    tmp = str(tmp)
    contigs = four_contigs()
    fa, fq = os.path.join(tmp, "ref.fa"), os.path.join(tmp, "reads.fq")
    write_fasta(fa, contigs), write_fastq(fq, long_reads(contigs))
    want = ref_run(["-a", "-x", "map-ont", "-I", "30k", "--split-prefix", os.path.join(tmp, "refpre"), fa, fq])
    out = os.path.join(tmp, "ours.sam")
    assert mm.map_split(fa, fq, os.path.join(tmp, "ourpre"), out, preset="map-ont", sam=True, n_threads=2, idx_batch_size=30000) == 2
    with open(out, "rb") as f:
        got = f.read()
    assert got == want, _first_difference(got, want)
