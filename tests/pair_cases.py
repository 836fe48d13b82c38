"""Shared by tests/test_gpu_pair.py and tests/test_pair_emu.py (not a test): fragments for pair_kernel behind mm2amd_pair_batch -- mm_pair and
mm_set_pe_thru (pe.c:50-68, :81-182) -- and the judge they are measured by: the UNMODIFIED compiled reference's mm_pair
(oracle/_ref/libminimap2_ref.so) through ctypes, on mm_reg1_t records whose mm_extra_t headers are ctypes objects.  Every fragment goes three ways:
the kernel, the host twin and the reference; parent, mapq, sam_pri, proper_frag and pe_thru are compared hit by hit.

A note on two shapes the rules cannot take.  The key's lowest bit is seg ^ rev, so an OPENING end has rev == seg and a closing one rev != seg: the
nearest earlier opening end of a closing end's strand (last[rev], pe.c:119) always belongs to the OTHER segment.  The "last[] trap" below is
therefore built from other-segment ends alone: the nearest one out of reach, one further back in reach, and no pair."""
import ctypes as C
import os
import random
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import reflib  # noqa: E402

HAVE_REF = os.path.exists(reflib.REF_SO)
HAVE_BIN = os.path.exists(reflib.REF_BIN)
NARROW, WIDE, HOST = 0, 1, 2  # minimap2_amd.PE_PATH_*
REV, SAM_PRI, PROPER_FRAG, THRU = 1, 2, 4, 8  # minimap2_amd.PE_*
NARROW_CAP, WIDE_CAP, SORT_EXACT = 64, 1024, 64  # what pair_limits() must say; RS_MIN_SIZE
OPT = dict(pe_bonus=33, sub_diff=8, match_sc=2)  # minimap2's defaults (a = 2, b = 4)
FIELDS = ("parent", "mapq", "flags")

_R = None


def _ref(mm):
    global _R
    if _R is None:
        _R = C.CDLL(reflib.REF_SO)
        _R.mm_pair.restype = None
        _R.mm_pair.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.POINTER(mm.Reg1))]
    return _R


def ref_pair(mm, frag, opt=OPT):
    """the reference's mm_pair on one fragment -> a pair of PE_OUT_DTYPE arrays answering the hits one by one"""
    R = _ref(mm)
    segs, keep = [], []
    for hs in frag[:2]:
        r = (mm.Reg1 * max(len(hs), 1))()
        for i, h in enumerate(hs):
            x, f = r[i], int(h["flags"])
            x.rid, x.rs, x.re, x.qs, x.qe, x.id, x.parent, x.hash = (int(h[k]) for k in ("rid", "rs", "re", "qs", "qe", "id", "parent", "hash"))
            x.bits = (int(h["mapq"]) & 0xff) | (1 << 10 if f & REV else 0) | (1 << 12 if f & SAM_PRI else 0)
            e = mm.Extra()
            e.capacity, e.dp_max = 8, int(h["dp_max"])
            keep.append(e)
            x.p = C.pointer(e)
        segs.append(r)
    n_regs = (C.c_int * 2)(len(frag[0]), len(frag[1]))
    qlens = (C.c_int * 2)(*frag[2])
    regs = (C.POINTER(mm.Reg1) * 2)(C.cast(segs[0], C.POINTER(mm.Reg1)), C.cast(segs[1], C.POINTER(mm.Reg1)))
    R.mm_pair(None, frag[3], opt["pe_bonus"], opt["sub_diff"], opt["match_sc"], qlens, n_regs, regs)
    outs = []
    for s in range(2):
        o = np.zeros(len(frag[s]), dtype=mm.PE_OUT_DTYPE)
        for i in range(len(frag[s])):
            x = segs[s][i]
            o[i]["parent"], o[i]["mapq"] = x.parent, x.bits & 0xff
            o[i]["flags"] = (SAM_PRI if x.bits >> 12 & 1 else 0) | (PROPER_FRAG if x.bits >> 13 & 1 else 0) | (THRU if x.bits >> 14 & 1 else 0)
        outs.append(o)
    return outs


# ---------------------------------------------------------------------------------------------------------
# fragments
# ---------------------------------------------------------------------------------------------------------
def hit(mm, rs, re, rev=0, dp=100, rid=0, hash=0, qs=0, qe=100, parent=None, mapq=0, sam_pri=None, id=None):
    """parent None: a primary; id None: the position in the segment (set by seg())"""
    h = np.zeros(1, dtype=mm.PE_HIT_DTYPE)[0]
    h["rid"], h["rs"], h["re"], h["qs"], h["qe"], h["dp_max"], h["hash"], h["mapq"] = rid, rs, re, qs, qe, dp, hash, mapq
    h["id"], h["parent"] = (-1 if id is None else id), (-1 if parent is None else parent)
    h["flags"] = (REV if rev else 0) | (0x80000000 if sam_pri is None else SAM_PRI if sam_pri else 0)
    return h


def seg(mm, hs):
    """ids are positions unless given, a hit without a parent is its own, sam_pri unless given goes to the first primary"""
    a = np.array(hs, dtype=mm.PE_HIT_DTYPE) if len(hs) else np.zeros(0, dtype=mm.PE_HIT_DTYPE)
    first = True
    for i in range(len(a)):
        if a[i]["id"] < 0:
            a[i]["id"] = i
        if a[i]["parent"] < 0:
            a[i]["parent"] = a[i]["id"]
        if a[i]["flags"] & 0x80000000:
            a[i]["flags"] = (a[i]["flags"] & 0x7fffffff) | (SAM_PRI if first and a[i]["parent"] == a[i]["id"] else 0)
            first = first and not a[i]["flags"] & SAM_PRI
    return a


def frag(mm, h0, h1, qlens=(100, 100), gap=500):
    return (seg(mm, h0), seg(mm, h1), qlens, gap)


def key_of(h, s):
    return int(h["rid"]) << 32 | (int(h["rs"]) << 1 | (s ^ (int(h["flags"]) & REV)))


def has_tie(fr):
    keys = [key_of(h, 0) for h in fr[0]] + [key_of(h, 1) for h in fr[1]]
    return len(set(keys)) < len(keys)


def expected_class(fr):
    """which class a fragment takes: by its ends, and -- above 64 -- by whether two of them have equal keys; an unmapped mate is the entry point's"""
    n0, n1 = len(fr[0]), len(fr[1])
    if n0 == 0 or n1 == 0:
        return NARROW
    if n0 + n1 > WIDE_CAP or (n0 + n1 > SORT_EXACT and has_tie(fr)):
        return HOST
    return NARROW if n0 + n1 <= NARROW_CAP else WIDE


def spread(mm, n0, n1, step=7, gap=100, rs0=1000, dp=100, tie=False):
    """n0 opening ends of segment 0 and n1 closing ends of segment 1, interleaved on one sequence `step` apart: every closing end reaches the opening
    ends of the last gap + 100 bases; dp and hash vary so that the best pair is unique"""
    h0 = [hit(mm, rs0 + step * i, rs0 + step * i + 100, dp=dp + (i * 37) % 23, hash=1000 + i) for i in range(n0)]
    h1 = [hit(mm, rs0 + step * i + 3, rs0 + step * i + 103, dp=dp + (i * 29) % 19, hash=5000 + i) for i in range(n1)]
    if tie:
        h0[1]["rs"] = h0[0]["rs"]
    return frag(mm, h0, h1, gap=gap)


def directed(mm):
    """(name, fragment, options, expected class or None for expected_class()) -- the issue's list of shapes"""
    H = lambda *a, **k: hit(mm, *a, **k)  # noqa: E731
    c = []

    def add(name, fr, opt=OPT):
        c.append((name, fr, opt))
    # one mate unmapped: nothing changes, pe_thru included (the two hits of (2, 0) are end-to-end copies of each other)
    add("unmapped_0_1", frag(mm, [], [H(1000, 1100, mapq=7)]))
    add("unmapped_2_0", frag(mm, [H(1000, 1100, mapq=3), H(1001, 1101, rid=1, mapq=4)], []))
    # (1, 1)
    add("one_pair", frag(mm, [H(1000, 1100, dp=90)], [H(1300, 1400, dp=95)]))
    add("one_pair_mapq_raised", frag(mm, [H(1000, 1100, mapq=40)], [H(1300, 1400, mapq=3)]))
    add("wrong_orientation", frag(mm, [H(1000, 1100, rev=1)], [H(1300, 1400, rev=0)]))
    add("wrong_order", frag(mm, [H(1300, 1400)], [H(1000, 1100)]))
    add("reach_at_gap", frag(mm, [H(1000, 1100)], [H(1600, 1700)]))          # rs - re == max_gap_ref
    add("reach_gap_plus_1", frag(mm, [H(1000, 1100)], [H(1601, 1701)]))      # one base too far
    add("other_rid", frag(mm, [H(1000, 1100)], [H(1300, 1400, rid=1)]))
    add("no_pair_but_thru", frag(mm, [H(1000, 1100, rev=1)], [H(1001, 1101, rev=1)]))  # the closing end sorts first: no pair; pe_thru holds
    # the last[] trap: the nearest opening end is short and out of reach, a long one further back is in reach -- no pair
    add("last_trap", frag(mm, [H(1000, 1900), H(1200, 1250)], [H(2000, 2100)]))
    # the break: nearest in reach, the next out of reach (short), the farthest in reach again -- one candidate
    add("walk_break", frag(mm, [H(1000, 1900, dp=120), H(1200, 1250, dp=110), H(1300, 1700, dp=90)], [H(2000, 2100)]))
    # dp_thres: the bar is 100 + 100 - 33 = 167
    add("bar_exact_and_below", frag(mm, [H(1000, 1100, dp=100, hash=1), H(1010, 1110, dp=67, hash=2), H(1020, 1120, dp=66, hash=3)], [H(1300, 1400, dp=100)]))
    add("bar_floored_at_0", frag(mm, [H(1000, 1100, dp=100, hash=1), H(1010, 1110, dp=67, hash=2), H(1020, 1120, dp=1, hash=3)], [H(1300, 1400, dp=100)]),
        dict(pe_bonus=1000, sub_diff=8, match_sc=2))
    # equal dp sums decided by the hash sum; fully equal scores decided by the order of the walk
    add("tie_by_hash", frag(mm, [H(1000, 1100, hash=5), H(1010, 1110, hash=9)], [H(1300, 1400, hash=1)]))
    add("tie_across_closing_ends", frag(mm, [H(1000, 1100, hash=5, mapq=5)], [H(1300, 1400, hash=1), H(1310, 1410, hash=1)]))
    add("tie_inside_a_walk", frag(mm, [H(1000, 1100, hash=5), H(1010, 1110, hash=5), H(1020, 1120, hash=5)], [H(1300, 1400, hash=1, mapq=9)]))
    # the runner-up: equal to the best (floor 0, logf(2) and logf(3)), below it (floor 1), close with company (a negative alternative)
    add("runner_up_equal", frag(mm, [H(1000, 1100, hash=5, mapq=5), H(1010, 1110, hash=5)], [H(1300, 1400, hash=1)]))
    add("runner_up_below", frag(mm, [H(1000, 1100, dp=100), H(1010, 1110, dp=90)], [H(1300, 1400)]))
    add("runner_up_below_raised", frag(mm, [H(1000, 1100, dp=100, mapq=40), H(1010, 1110, dp=90)], [H(1300, 1400, mapq=3)]))
    add("runner_up_within_sub_diff", frag(mm, [H(1000, 1100, dp=100, mapq=40), H(1010, 1110, dp=94)], [H(1300, 1400, mapq=3)]))
    add("negative_alternative", frag(mm, [H(1000, 1100, dp=100, mapq=20), H(1010, 1110, dp=99), H(1020, 1120, dp=99)], [H(1300, 1400, mapq=30)]))
    # a secondary and a primary: the lift
    add("lift", frag(mm, [H(50000, 50100, dp=120, mapq=30), H(1000, 1100, dp=110, parent=0), H(2000, 2100, rid=1, dp=100, parent=0), H(3000, 3100, rid=1, dp=90, mapq=11)],
                     [H(1300, 1400, dp=100, mapq=25)]))
    add("lift_both", frag(mm, [H(50000, 50100, dp=120, mapq=30), H(1000, 1100, dp=110, parent=0)],
                          [H(70000, 70100, dp=130, mapq=31), H(9000, 9100, rid=1, dp=60, parent=0), H(1300, 1400, dp=100, parent=0)]))
    add("lift_keeps_sam_pri", frag(mm, [H(50000, 50100, dp=120, mapq=30, sam_pri=0), H(1000, 1100, dp=110, parent=0, sam_pri=1)], [H(1300, 1400)]))
    # equal keys among up to 64 ends: the input's order -- inside a segment (openings, closings), and across the two (an opening of each)
    add("equal_keys_openings", frag(mm, [H(1000, 1100, hash=5), H(1000, 1150, hash=5), H(1000, 1120, hash=5)], [H(1300, 1400)]))
    add("equal_keys_closings", frag(mm, [H(1000, 1100)], [H(1300, 1400, hash=3), H(1300, 1450, hash=3), H(1300, 1350, hash=3)]))
    add("equal_keys_across", frag(mm, [H(1000, 1100, hash=5), H(1300, 1400, rev=1, hash=6)], [H(1000, 1100, rev=1, hash=7), H(1300, 1400, hash=8)]))
    add("equal_keys_rev_strand", frag(mm, [H(1300, 1400, rev=1, hash=2), H(1300, 1410, rev=1, hash=2)], [H(1000, 1100, rev=1, hash=7), H(1000, 1105, rev=1, hash=7)]))
    # pe_thru: the two positive shapes, each single condition broken
    T = lambda **k: frag(mm, [H(1000, 1080, qs=k.get("qs0", 0), qe=k.get("qe0", 80), rev=k.get("rev0", 0), rid=k.get("rid0", 0))] + k.get("more0", []),  # noqa: E731
                         [H(k.get("rs1", 1002), k.get("re1", 1078), qs=k.get("qs1", 10), qe=k.get("qe1", 90))], qlens=(100, 90))
    add("thru_p_starts", T())                                       # p.qs == 0 and qlens[1] - q.qe == 0
    add("thru_q_starts", T(qs0=20, qe0=100, qs1=0, qe1=70))         # q.qs == 0 and qlens[0] - p.qe == 0
    add("thru_not_rid", T(rid0=1))
    add("thru_not_rev", T(rev0=1))
    add("thru_rs_3_apart", T(rs1=1003))
    add("thru_re_3_apart", T(re1=1077))
    add("thru_p_not_at_0", T(qs0=1))
    add("thru_q_not_at_end", T(qe1=89))
    add("thru_two_primaries", T(more0=[H(9000, 9080, rid=1)]))
    # class boundaries
    add("n64_all_in_reach", frag(mm, [H(1000 + 3 * i, 1100 + 3 * i, hash=i, dp=100 + i % 3) for i in range(32)], [H(1200 + 3 * i, 1300 + 3 * i, hash=100 + i) for i in range(32)]))
    add("n64_equal_keys", spread(mm, 32, 32, tie=True))
    add("n65_wide", spread(mm, 33, 32))
    add("n65_equal_key_host", spread(mm, 33, 32, tie=True))
    add("n_wide_cap", spread(mm, WIDE_CAP // 2, WIDE_CAP // 2))
    add("n_wide_cap_plus_1_host", spread(mm, WIDE_CAP // 2 + 1, WIDE_CAP // 2))
    return c


WANT_CLASS = {"n64_all_in_reach": NARROW, "n64_equal_keys": NARROW, "n65_wide": WIDE, "n65_equal_key_host": HOST, "n_wide_cap": WIDE, "n_wide_cap_plus_1_host": HOST}


def compare(mm, cases, what=""):
    """every fragment through the kernel, the host twin and the reference; every field of every hit, the pair, the count and the classes"""
    by_opt = {}
    for name, fr, o in cases:
        by_opt.setdefault(tuple(sorted(o.items())), (o, []))[1].append((name, fr))
    classes, stats = {NARROW: 0, WIDE: 0, HOST: 0}, {"paired": 0, "lifted": 0, "several": 0}
    for o, group in by_opt.values():
        frs = [fr for _, fr in group]
        dev, dev_res = mm.pair_batch(frs, **o)
        host, host_res, _ = mm.pair_host_batch(frs, n_threads=2, **o)
        for k, (name, fr) in enumerate(group):
            want = ref_pair(mm, fr, o)
            for who, got in (("kernel", dev[k]), ("host", host[k])):
                for s in range(2):
                    for f in FIELDS:
                        bad = np.nonzero(got[s][f] != want[s][f])[0]
                        assert len(bad) == 0, "%s%s: %s, field %s of hit %d of segment %d: %d, the reference has %d" % (what, name, who, f, bad[0], s, got[s][f][bad[0]], want[s][f][bad[0]])
                    assert not got[s]["reserved"].any()
            for r in (dev_res[k], host_res[k]):
                assert r["status"] == 0 and r["reserved"] == 0
                for s in range(2):
                    pf = np.nonzero(want[s]["flags"] & PROPER_FRAG)[0]
                    assert ([int(r["best"][s])] if r["best"][s] >= 0 else []) == [int(x) for x in pf], "%s%s: the pair's hit of segment %d" % (what, name, s)
            assert dev_res[k]["n_pairs"] == host_res[k]["n_pairs"], "%s%s: %d candidates on the device, %d on the host" % (what, name, dev_res[k]["n_pairs"], host_res[k]["n_pairs"])
            assert dev_res[k]["path"] == expected_class(fr), "%s%s ran in class %d, not %d" % (what, name, dev_res[k]["path"], expected_class(fr))
            assert host_res[k]["path"] == HOST
            classes[int(dev_res[k]["path"])] += 1
            b = [int(x) for x in host_res[k]["best"]]
            stats["paired"] += b[0] >= 0
            stats["lifted"] += b[0] >= 0 and any(fr[s][b[s]]["id"] != fr[s][b[s]]["parent"] for s in range(2))
            stats["several"] += host_res[k]["n_pairs"] > 1
    return classes, stats


# ---------------------------------------------------------------------------------------------------------
# the checks
# ---------------------------------------------------------------------------------------------------------
def check_limits(mm):
    assert mm.pair_limits() == {"narrow_cap": NARROW_CAP, "wide_cap": WIDE_CAP, "max_hits": 1 << 20}


def check_directed(mm):
    cases = directed(mm)
    for name, fr, _ in cases:
        if name in WANT_CLASS:
            assert expected_class(fr) == WANT_CLASS[name], name
        for s in range(2):
            assert len(fr[s]) == 0 or max(int(fr[s]["rs"].max()), int(fr[s]["re"].max())) < 1 << 30
    classes, _ = compare(mm, cases)
    assert classes[HOST] == 2 and classes[WIDE] == 2, classes
    by = {n: (fr, o) for n, fr, o in cases}
    # what the shapes are for, in the reference's own answers and the twin's counts
    def ref_flags(n):
        return [o["flags"] for o in ref_pair(mm, *by[n])]

    def n_pairs(n):
        return int(mm.pair_host_batch([by[n][0]], **by[n][1])[1][0]["n_pairs"])

    def mapqs(n):
        return [[int(x) for x in o["mapq"]] for o in ref_pair(mm, *by[n])]
    for n in ("unmapped_0_1", "unmapped_2_0", "wrong_orientation", "wrong_order", "reach_gap_plus_1", "other_rid", "last_trap", "no_pair_but_thru"):
        assert not any((f & PROPER_FRAG).any() for f in ref_flags(n)) and n_pairs(n) == 0, n
    assert not any((f & THRU).any() for f in ref_flags("unmapped_2_0")) and all((f & THRU).all() for f in ref_flags("no_pair_but_thru"))
    assert n_pairs("one_pair") == 1 and mapqs("one_pair") == [[2], [2]] and n_pairs("reach_at_gap") == 1
    assert mapqs("one_pair_mapq_raised") == [[40], [int(np.float32(.2) * np.float32(3) + np.float32(.8) * np.float32(40) + np.float32(.499))]]
    assert n_pairs("walk_break") == 1 and n_pairs("bar_exact_and_below") == 2 and n_pairs("bar_floored_at_0") == 3
    assert list(ref_flags("tie_by_hash")[0] & PROPER_FRAG) == [0, PROPER_FRAG]
    assert list(ref_flags("tie_across_closing_ends")[1] & PROPER_FRAG) == [PROPER_FRAG, 0]
    assert list(ref_flags("tie_inside_a_walk")[0] & PROPER_FRAG) == [0, 0, PROPER_FRAG]
    assert mapqs("runner_up_equal") == [[5, 0], [0]] and mapqs("tie_inside_a_walk")[0] == [0, 0, 0]
    assert mapqs("runner_up_below") == [[1, 0], [1]]
    assert mapqs("runner_up_below_raised") == [[40, 0], [25]] and mapqs("negative_alternative") == [[20, 0, 0], [30]]
    lift = ref_pair(mm, *by["lift"])
    assert list(lift[0]["parent"]) == [1, 1, 1, 3] and list(lift[0]["mapq"])[0] == 0 and list(lift[0]["flags"]) == [0, SAM_PRI | PROPER_FRAG, 0, 0]
    assert list(ref_flags("equal_keys_openings")[0] & PROPER_FRAG) == [0, 0, PROPER_FRAG] and list(ref_flags("equal_keys_closings")[1] & PROPER_FRAG) == [PROPER_FRAG, 0, 0]
    for n, fr, o in cases:
        if n.startswith("thru_"):
            assert all((f & THRU).all() for f in ref_flags(n)) == (n in ("thru_p_starts", "thru_q_starts")), n
    assert n_pairs("n64_all_in_reach") == 1024


def random_fragment(mm, rng):
    def segment(s):
        n = rng.randrange(13) if rng.randrange(20) else rng.randrange(13, 41)
        hs, prim = [], []
        for i in range(n):
            rs = 1000 + 10 * rng.randrange(300)
            ln = rng.choice((40, 100, 100, 100, 150, 700))
            rev = rng.random() < 0.5
            par = None if not prim or rng.random() < 0.35 else rng.choice(prim)
            if par is None:
                prim.append(i)
            hs.append(hit(mm, rs, rs + ln, rev=rev, dp=rng.randrange(50, 150), rid=rng.randrange(3), hash=rng.randrange(1, 40), qs=rng.choice((0, 0, 5)), qe=rng.choice((100, 100, 90)),
                          parent=par, mapq=0 if par is not None else rng.randrange(0, 61)))
        return hs
    return frag(mm, segment(0), segment(1), gap=rng.choice((100, 300, 800, 2000)))


def check_random(mm, n_frags, seed=11):
    rng = random.Random(seed)
    cases = [("random%d" % k, random_fragment(mm, rng), OPT) for k in range(n_frags)]
    n_host = sum(expected_class(fr) == HOST for _, fr, _ in cases)
    n_tie = sum(has_tie(fr) for _, fr, _ in cases)
    classes, stats = compare(mm, cases, "seed %d, " % seed)
    assert classes[HOST] == n_host and n_tie >= n_frags // 20, (classes, n_host, n_tie)
    assert classes[NARROW] >= n_frags // 2, classes
    scale = n_frags / 2000.0
    assert stats["paired"] >= 100 * scale and stats["lifted"] >= 20 * scale and stats["several"] >= 20 * scale, stats
    return classes, stats


def check_bookkeeping(mm):
    """an empty batch, a batch of unmapped mates only, buffers reused by a smaller batch, bad arguments, a parent out of range, the profile's rows"""
    assert mm.pair_batch([])[0] == [] and len(mm.pair_batch([])[1]) == 0
    H = lambda *a, **k: hit(mm, *a, **k)  # noqa: E731
    lonely = [frag(mm, [H(1000, 1100, mapq=9)], []), frag(mm, [], [H(1000, 1100, mapq=8), H(2000, 2100, mapq=0, parent=0)]), frag(mm, [], [])]
    mm.profile_enable(True)
    out, res = mm.pair_batch(lonely)
    prof = mm.profile_get()
    mm.profile_enable(False)
    assert not any(k.startswith("pair_kernel") for k in prof), "a launch for unmapped mates"
    assert [int(x) for x in res["path"]] == [NARROW] * 3 and not res["n_pairs"].any() and (res["best"] == -1).all()
    assert list(out[0][0]["mapq"]) == [9] and list(out[1][1]["parent"]) == [0, 0] and list(out[1][1]["flags"]) == [SAM_PRI, 0]
    # a larger batch, then a smaller one through the same buffers
    rng = random.Random(5)
    big = [random_fragment(mm, rng) for _ in range(300)] + [spread(mm, 40, 40)]
    small = big[17:23]
    mm.profile_enable(True)
    b_out, b_res = mm.pair_batch(big)
    prof = mm.profile_get()
    mm.profile_enable(False)
    assert prof["pair_kernel[narrow]"]["launches"] == 1 and prof["pair_kernel[wide]"]["launches"] == 1 and prof["pair_kernel[wide]"]["units"] == 80
    s_out, s_res = mm.pair_batch(small)
    h_out, h_res, _ = mm.pair_host_batch(small)
    for k in range(len(small)):
        for s in range(2):
            assert all((s_out[k][s][f] == h_out[k][s][f]).all() and (s_out[k][s][f] == b_out[17 + k][s][f]).all() for f in FIELDS)
        assert list(s_res[k]["best"]) == list(h_res[k]["best"]) == list(b_res[17 + k]["best"])
    # a parent that does not index its segment: refused with its status by the kernel and by the twin, the fragment's hits as they came
    for par in (-1, 2, 1 << 20):
        bad = frag(mm, [H(1000, 1100, mapq=5), H(1010, 1110, parent=0)], [H(1300, 1400, mapq=6)])
        bad[0][1]["parent"] = par
        good = frag(mm, [H(1000, 1100)], [H(1300, 1400)])
        for call in (mm.pair_batch, mm.pair_host_batch):
            r = call([good, bad, good])
            o, rs = r[0], r[1]
            assert [int(x) for x in rs["status"]] == [mm.PE_OK, mm.PE_BAD_PARENT, mm.PE_OK] and rs[1]["n_pairs"] == 0 and list(rs[1]["best"]) == [-1, -1]
            assert list(o[1][0]["parent"]) == [0, par] and list(o[1][0]["mapq"]) == [5, 0] and list(o[1][1]["mapq"]) == [6] and list(o[1][0]["flags"]) == [SAM_PRI, 0]
            assert list(o[0][0]["mapq"]) == [2] and list(o[2][1]["flags"]) == [SAM_PRI | PROPER_FRAG]
    # bad arguments, through the C entries
    L = mm.lib()
    fr = np.zeros(2, dtype=mm.PE_FRAG_DTYPE)
    fr["n"], fr["qlen"], fr["max_gap_ref"] = (1, 1), (100, 100), 500
    fr["hit0"] = (0, 2)
    hits = np.concatenate([frag(mm, [H(1000, 1100)], [H(1300, 1400)])[s] for s in (0, 1)] * 2)
    outb, resb = np.zeros(4, dtype=mm.PE_OUT_DTYPE), np.zeros(2, dtype=mm.PE_RES_DTYPE)
    o = mm.PeOpt(33, 8, 2, 0)
    for entry in (lambda *a: L.mm2amd_pair_batch(*a), lambda n, f, h, op, ou, r: L.mm2amd_pair_host_batch(n, f, h, op, 1, ou, r, None)):
        assert entry(2, fr.ctypes.data, hits.ctypes.data, C.byref(o), outb.ctypes.data, resb.ctypes.data) == 0 and list(outb["mapq"]) == [2, 2, 2, 2]
        assert entry(-1, fr.ctypes.data, hits.ctypes.data, C.byref(o), outb.ctypes.data, resb.ctypes.data) == mm.EINVAL
        assert entry(2, None, hits.ctypes.data, C.byref(o), outb.ctypes.data, resb.ctypes.data) == mm.EINVAL
        assert entry(2, fr.ctypes.data, None, C.byref(o), outb.ctypes.data, resb.ctypes.data) == mm.EINVAL
        assert entry(2, fr.ctypes.data, hits.ctypes.data, None, outb.ctypes.data, resb.ctypes.data) == mm.EINVAL
        assert entry(2, fr.ctypes.data, hits.ctypes.data, C.byref(o), None, resb.ctypes.data) == mm.EINVAL
        assert entry(2, fr.ctypes.data, hits.ctypes.data, C.byref(o), outb.ctypes.data, None) == mm.EINVAL
        assert entry(2, fr.ctypes.data, hits.ctypes.data, C.byref(mm.PeOpt(33, 8, 0, 0)), outb.ctypes.data, resb.ctypes.data) == mm.EINVAL
        for hit0, n1 in (((0, 1), (1, 1)), ((1, 0), (1, 1)), ((0, 2), (-1, 1)), ((0, 2), (1, (1 << 20) + 1)), ((0, 1 << 40), (1, 1))):  # overlaps in either order, counts, span
            bad = fr.copy()
            bad["hit0"] = hit0
            bad["n"][1] = n1
            assert entry(2, bad.ctypes.data, hits.ctypes.data, C.byref(o), outb.ctypes.data, resb.ctypes.data) == mm.EINVAL, (hit0, n1)
        assert entry(0, None, None, None, None, None) == 0
    # fragments listed against the order of their hits are fine
    back = fr.copy()
    back["hit0"] = (2, 0)
    assert L.mm2amd_pair_batch(2, back.ctypes.data, hits.ctypes.data, C.byref(o), outb.ctypes.data, resb.ctypes.data) == 0


# ---------------------------------------------------------------------------------------------------------
# MM2AMD_DEVICE_PAIR end to end, in child processes (the switch is read where the context or the merger is created)
# ---------------------------------------------------------------------------------------------------------
MAPPER_CHILD = """
import sys
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import os
if os.environ.get("MM2AMD_EMU") == "1":
    import conftest  # (binds the emulator build, as the parent's suite does)
import minimap2_amd as mm


def fasta(path):
    names, seqs = [], []
    for line in open(path, "rb"):
        (names if line.startswith(b">") else seqs).append(line.strip().lstrip(b">"))
    return names, seqs


rn, rs = fasta(sys.argv[1])
n1, s1 = fasta(sys.argv[2])
_, s2 = fasta(sys.argv[3])
al = mm.Aligner(rs, preset="sr", names=[x.decode() for x in rn], sam=True, n_threads=4)
mm.profile_enable(True)
text = al.map_pairs([(nm, a, b) for nm, a, b in zip(n1, s1, s2)], text=True)
launches = sum(r["launches"] for k, r in mm.profile_get().items() if k.startswith("pair_kernel"))
al.close()
open(sys.argv[4], "wb").write(text)
print("launches", launches)
"""

MERGE_CHILD = """
import sys
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import os
if os.environ.get("MM2AMD_EMU") == "1":
    import conftest
import minimap2_amd as mm
mm.profile_enable(True)
n = mm.map_split(sys.argv[1], [sys.argv[2], sys.argv[3]], sys.argv[4], sys.argv[5], preset="sr", sam=True, n_threads=2)
launches = sum(r["launches"] for k, r in mm.profile_get().items() if k.startswith("pair_kernel"))
print("parts", n, "launches", launches)
"""


def _child(code, args, value):
    import subprocess
    env = {k: v for k, v in os.environ.items() if k != "MM2AMD_DEVICE_PAIR"}
    if value is not None:
        env["MM2AMD_DEVICE_PAIR"] = value
    r = subprocess.run([sys.executable, "-c", code % (ROOT, HERE)] + args, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=170)
    assert r.returncode == 0, r.stdout.decode()[-3000:]
    return int(r.stdout.decode().split("launches")[-1].split()[0]), r.stdout.decode()


def check_mapper_switch(tmp):
    """synth.make_pairs(n_pairs=300) mapped with -x sr -a, the switch set and unset: the reference binary's SAM both times, pair_kernel launched only when set"""
    import subprocess
    import synth
    tmp = str(tmp)
    ref, f1, f2, _ = synth.make_pairs(tmp, n_pairs=300)
    p = subprocess.run([reflib.REF_BIN, "-t", "4", "-x", "sr", "-a", ref, f1, f2], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, check=True)
    want = b"\n".join(l for l in p.stdout.split(b"\n") if not l.startswith(b"@"))
    assert sum(1 for l in want.split(b"\n") if l and int(l.split(b"\t")[1]) & 2) >= 400  # proper pairs: mm_pair has work
    for value, launched in (("1", True), (None, False)):
        out = os.path.join(tmp, "sam_%s" % value)
        n, _ = _child(MAPPER_CHILD, [ref, f1, f2, out], value)
        with open(out, "rb") as f:
            got = f.read()
        assert got.rstrip(b"\n") == want.rstrip(b"\n"), "MM2AMD_DEVICE_PAIR=%s: the SAM text differs from the reference's" % value
        assert (n > 0) == launched, (value, n)


def check_merge_switch(tmp):
    """two pair files through map_split() against a two-part index with the switch set: the text of `minimap2 --split-prefix`, pair_kernel launched"""
    import split_cases as S
    tmp = str(tmp)
    contigs = S.four_contigs()
    mmi = S.ref_index(tmp, contigs, "sr", "30k")
    r1, r2 = S.short_pairs(contigs)
    files = [os.path.join(tmp, "r1.fq"), os.path.join(tmp, "r2.fq")]
    S.write_fastq(files[0], r1), S.write_fastq(files[1], r2)
    want = S.ref_run(["-a", "-x", "sr", "--split-prefix", os.path.join(tmp, "refpre"), mmi] + files)
    assert sum(1 for f in S.flags_of(want) if f & 2) >= 100
    for value, launched in (("1", True), (None, False)):
        out = os.path.join(tmp, "ours_%s.sam" % value)
        n, text = _child(MERGE_CHILD, [mmi] + files + [os.path.join(tmp, "ourpre%s" % value), out], value)
        assert "parts 2 " in text
        with open(out, "rb") as f:
            got = f.read()
        assert got == want, S._first_difference(got, want)
        assert (n > 0) == launched, (value, n)
