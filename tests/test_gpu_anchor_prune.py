"""Anchor pruning before the per-read sort (seed_chain.hip: anchor_sort_prune_kernel): anchors with no other anchor of their strand and target inside
the chaining window are dropped before the sort, the fill and the backtrack.  That must be invisible.  For every read of every run here

  * the chain dump (MM2AMD_CHAIN_DUMP) is identical, block for block, between MM2AMD_ANCHOR_PRUNE=0 and 1;
  * its final chains are the reference binary's CN lines (as tests/test_gpu_chains.py compares them);
  * the SAM text is identical, byte for byte, between the two settings;
  * the number of anchors the chaining kernels were given (the dump's KP line, MM2AMD_CHAIN_DUMP_KEPT=1) is EXACTLY the number of anchors of the
    reference's seed list (SD lines) that have another anchor of their strand and target within max_dist -- computed here, on the CPU, from the
    reference's output alone -- unless the read was sorted unpruned after all (KP says so), in which case it is the whole list.

The input: 1.5 Mb in three contigs; thirty 2-4 kb reads with a true locus, 19-base snippets of each planted 5 200 bases apart all over the reference
(isolated single hits: the benchmark's random hits against 3 Gb, made at this size); and reads of random sequence that only have planted hits, for
the edge cases -- pairs exactly max_dist and max_dist + 1 apart, a pair across a bin boundary, the same position on two contigs and both strands,
reads that lose every anchor, reads with 0 / 1 / 2 anchors, a read with a duplicated key.  Every case asserts from the reference's seed list that
the input holds what it is about, and from the KP lines that the run took the path."""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import chainlib  # noqa: E402
import synth  # noqa: E402
import test_gpu_chains as tgc  # noqa: E402  (the reference side and the block bookkeeping of the chain tests)

pytestmark = pytest.mark.gpu
EMU = tgc.EMU
SLOT, SNIP, BIN = 5200, 24, 8192  # planting grid (> max_dist + SNIP), snippet length (k + w - 1: one whole minimizer window, so at least one hit), 2^s for max_dist = 5000
SNIP_LOC = 19  # the located reads' snippets: five 15-mers


# ---------------------------------------------------------------------------------------------------------
# input
# ---------------------------------------------------------------------------------------------------------
def _plant(contigs, c, pos, s, rev):
    contigs[c][pos:pos + len(s)] = synth.COMP[s[::-1]] if rev else s


def _make_input(d):
    os.makedirs(d, exist_ok=True)
    rng = np.random.default_rng(2026)
    contigs = synth.gen_reference(rng, 1500000, 3)
    n_slot = len(contigs[0]) // SLOT - 1
    names, reads = [], []
    # reads with a true locus, and 450 planted snippets each, sites of one read whole slots apart.  A snippet of 24 bases (a whole
    # minimizer window) usually brings TWO hits, which keep each other; one of 19 bases brings one hit or none -- measured with the reference alone
    src = synth.gen_reads(rng, contigs, 30, 3000, 500, 0.12, min_len=2000)
    for i, r in enumerate(src):
        r = r[:4000]
        sites = rng.permutation(3 * n_slot * 2)[:450]
        for j, site in enumerate(sites):
            c, slot, rev = int(site) // 2 // n_slot, int(site) // 2 % n_slot, int(site) & 1
            q = int(rng.integers(0, len(r) - SNIP_LOC))
            _plant(contigs, c, slot * SLOT + 200 + i * 40, r[q:q + SNIP_LOC], rev)
        names.append("loc%d" % i), reads.append(r)
    # reads of random sequence: every hit is planted.  Offsets 2000 + .. of a slot are theirs (the reads above stay below 200 + 30 * 40 + 25).
    def rnd(n=2500):
        return rng.integers(0, 4, n, dtype=np.uint8)

    for i in range(8):  # pairs exactly max_dist apart (kept) and max_dist + 1 apart (dropped, where the snippet gave one anchor)
        for tag, dist in (("at", 5000), ("past", 5001)):
            r = rnd()
            for c in range(3):
                s = r[300 * c + 100:300 * c + 100 + SNIP]
                base = (2 * i + 3 + 20 * c) * SLOT + 2000 + (600 if tag == "at" else 0)
                _plant(contigs, c, base, s, c == 1), _plant(contigs, c, base + dist, s, c == 1)
            names.append("%s%d" % (tag, i)), reads.append(r)
    for i in range(4):  # a pair in range of each other on the two sides of a multiple of 2^s
        r = rnd()
        edge = BIN * (7 + 5 * i)
        _plant(contigs, i % 3, edge - 60, r[500:500 + SNIP], False), _plant(contigs, i % 3, edge + 40, r[900:900 + SNIP], False)
        names.append("edge%d" % i), reads.append(r)
    for i in range(8):  # the same position on two contigs and on both strands: four anchors, none in range of another
        r = rnd()
        pos = (60 + i) * SLOT + 3000
        _plant(contigs, 0, pos, r[700:700 + SNIP], False), _plant(contigs, 1, pos, r[700:700 + SNIP], False)
        _plant(contigs, 2, pos, r[1200:1200 + SNIP], False), _plant(contigs, 2, pos + SLOT + 300, r[1200:1200 + SNIP], True)
        names.append("same%d" % i), reads.append(r)
    for i in range(6):  # one or two single hits, nothing else: reads with 1 / 2 anchors that lose all of them
        r = rnd(2000)
        for j in range(1 + i % 2):
            _plant(contigs, j, (70 + i) * SLOT + 3500, r[400 + 600 * j:400 + 600 * j + SNIP], i == 3)
        names.append("few%d" % i), reads.append(r)
    names.append("none"), reads.append(rnd(2000))  # no anchor at all
    for i in range(3):  # the same snippet twice in the read, once in the reference: two anchors with equal x
        r = rnd()
        r[1500:1500 + SNIP] = r[400:400 + SNIP]
        _plant(contigs, i, (80 + i) * SLOT + 4000, r[400:400 + SNIP], i == 1)
        for j in range(20):  # ... among isolated hits, which the unpruned sort then keeps
            _plant(contigs, (i + j) % 3, (5 + j * 4) * SLOT + 4500 + 30 * i, r[1700 + 30 * j:1700 + 30 * j + SNIP], j % 2 == 1)
        names.append("dup%d" % i), reads.append(r)
    ref, rd = os.path.join(d, "ref.fa"), os.path.join(d, "reads.fa")
    synth.write_fasta(ref, ["c1", "c2", "c3"], contigs)
    synth.write_fasta(rd, names, reads)
    return ref, [rd]


# ---------------------------------------------------------------------------------------------------------
# the reference's side: seed lists, CN lines, and from the seed lists alone what pruning must keep
# ---------------------------------------------------------------------------------------------------------
def _near_mask(sd, max_dist):
    """per anchor of a read's sorted seed list: is another anchor of the same target and strand at most max_dist away (either side)"""
    n = len(sd)
    near = np.zeros(n, dtype=bool)
    for i in range(n - 1):
        a, b = sd[i], sd[i + 1]
        if a[0] == b[0] and a[2] == b[2] and b[1] - a[1] <= max_dist:
            near[i] = near[i + 1] = True
    return near


class Truth(object):
    def __init__(self, files, args):
        self.ref, self.files = files
        self.args = list(args)
        self.want = {r.name: r for r in tgc._ref_run(self.args, self.ref, self.files)}
        recs = tgc._fasta(self.ref)
        self.tnames = [n for n, _ in recs]
        self.opts = tgc.Opts(recs, self.args)
        self.qlen = {n: len(s) for f in self.files for n, s in tgc._fasta(f)}

    def max_dist(self, name):
        return max(self.opts.gaps(self.qlen[name])[0], self.opts.bw)

    def near(self, name):
        return _near_mask(self.want[name].sd, self.max_dist(name))


class Run(object):
    """one run of the mapper: SAM text, chain-dump blocks per read, KP lines per read ((kept, redone) of the first pass; absent: the call did not prune)"""

    def __init__(self, truth, env, path):
        if os.path.exists(path):
            os.unlink(path)
        p = subprocess.run([tgc.DROPIN] + truth.args + ["-a", "-t", "4", "--stats", truth.ref] + truth.files, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                           env=dict(os.environ, MM2AMD_CHAIN_DUMP=path, MM2AMD_CHAIN_DUMP_KEPT="1", **env))
        if p.returncode < 0 or p.returncode in (124, 134, 137, 139):  # killed by a signal: after a fault nothing more is started on the device
            pytest.exit("the mapper died (status %d) with %r: %s" % (p.returncode, env, p.stderr.decode()[-1500:]), returncode=3)
        assert p.returncode == 0, (env, p.stderr.decode()[-2000:])
        assert "backend=hip:gfx950" in p.stderr.decode()
        self.sam = p.stdout
        self.kp, plain, cur = {}, [], None
        for l in open(path).read().split("\n"):
            if l.startswith("CH\t"):
                cur = l.split("\t")[1]
            if l.startswith("KP\t"):
                f = l.split("\t")
                assert cur not in self.kp
                self.kp[cur] = (int(f[1]), int(f[2]))
                continue
            plain.append(l)
        self.blocks = chainlib.chain_dump_blocks("\n".join(plain))

    def contents(self):
        return {n: sorted(b.key() for b in bl) for n, bl in self.blocks.items()}


def _check(truth, run, base, pruned=True, redone_all=False):
    """`run` against the reference and against `base` (MM2AMD_ANCHOR_PRUNE=0); returns (anchors, kept anchors, redone reads)"""
    assert run.sam == base.sam, "the SAM text differs from MM2AMD_ANCHOR_PRUNE=0"
    assert run.contents() == base.contents(), "the chain dump differs from MM2AMD_ANCHOR_PRUNE=0"
    assert set(run.blocks) == set(truth.want)
    if not pruned:
        assert not run.kp, "this configuration must not prune"
        return None
    n_in = n_kept = n_redo = 0
    for name, want in truth.want.items():
        rd = tgc.ReadDump(name, run.blocks[name], 1)
        assert tgc._sd_tuples(rd.inp, truth.tnames) == want.sd, name
        assert sorted(tgc._cn_tuples(rd.final, truth.tnames)) == sorted(want.cn), (name, "final chains differ from the reference's CN lines")
        if not want.sd:
            assert run.kp.get(name, (0, 0)) == (0, 0), name
            continue
        kept, redone = run.kp[name]
        keys = [(t, pos, strand) for t, pos, strand, _, _ in want.sd]
        if len(set(keys)) < len(keys):
            assert redone, (name, "a duplicated key: the read goes through the unpruned sort")
        if redone_all:
            assert redone, name
        assert kept == (len(want.sd) if redone else int(truth.near(name).sum())), (name, kept, redone, len(want.sd), int(truth.near(name).sum()))
        n_in, n_kept, n_redo = n_in + len(want.sd), n_kept + kept, n_redo + redone
    return n_in, n_kept, n_redo


@pytest.fixture(scope="module")
def planted(tmp_path_factory):
    return _make_input(str(tmp_path_factory.mktemp("planted")))


@pytest.fixture(scope="module")
def ont(planted, tmp_path_factory):
    d = str(tmp_path_factory.mktemp("prune"))
    t = Truth(planted, ["-x", "map-ont"])
    t.dir = d
    t.base = Run(t, {"MM2AMD_ANCHOR_PRUNE": "0"}, os.path.join(d, "base.txt"))
    assert not t.base.kp
    return t


# ---------------------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------------------
def test_input_holds_its_cases(ont):
    """from the reference's seed lists alone: most anchors are isolated, and every edge case is there"""
    t = ont
    near = {n: t.near(n) for n in t.want}
    loc = [n for n in t.want if n.startswith("loc")]
    assert len(loc) == 30 and all(t.max_dist(n) == 5000 for n in t.want)
    assert sum(int(near[n].sum()) for n in loc) * 2 <= sum(len(near[n]) for n in loc), "at least half of the located reads' anchors are isolated"
    assert all(len(t.want[n].cn) > 0 for n in loc)

    def pairs(n, dist):  # consecutive anchors of a read exactly `dist` apart, with nothing else in range of either
        sd, out = t.want[n].sd, []
        for i in range(len(sd) - 1):
            a, b = sd[i], sd[i + 1]
            if a[0] == b[0] and a[2] == b[2] and b[1] - a[1] == dist:
                alone_l = i == 0 or not (sd[i - 1][0] == a[0] and sd[i - 1][2] == a[2] and a[1] - sd[i - 1][1] <= 5000)
                alone_r = i + 2 >= len(sd) or not (sd[i + 2][0] == b[0] and sd[i + 2][2] == b[2] and sd[i + 2][1] - b[1] <= 5000)
                if alone_l and alone_r:
                    out.append(i)
        return out

    at = [(n, i) for n in t.want if n.startswith("at") for i in pairs(n, 5000)]
    past = [(n, i) for n in t.want if n.startswith("past") for i in pairs(n, 5001)]
    assert len(at) >= 3 and all(near[n][i] and near[n][i + 1] for n, i in at)
    assert len(past) >= 3 and all(not near[n][i] and not near[n][i + 1] for n, i in past)
    assert {t.want[n].sd[i][2] for n, i in at + past} == {"+", "-"}
    edge = 0
    for n in t.want:
        sd = t.want[n].sd
        edge += sum(1 for i in range(len(sd) - 1) if n.startswith("edge") and near[n][i] and near[n][i + 1] and sd[i][0] == sd[i + 1][0] and sd[i][2] == sd[i + 1][2]
                    and sd[i + 1][1] - sd[i][1] <= 5000 and sd[i][1] // BIN != sd[i + 1][1] // BIN)
    assert edge >= 2
    same = 0
    for n in t.want:
        if n.startswith("same"):
            by_pos = {}
            for k, (tn, pos, strand, _, _) in enumerate(t.want[n].sd):
                by_pos.setdefault(pos, []).append((tn, strand, bool(near[n][k])))
            same += sum(1 for v in by_pos.values() if len({x[0] for x in v}) > 1 and not any(x[2] for x in v))
            assert {x[2] for x in t.want[n].sd} == {"+", "-"}
    assert same >= 2
    counts = {len(t.want[n].sd) for n in t.want}
    assert {0, 1, 2} <= counts
    assert sum(1 for n in t.want if len(near[n]) > 0 and not near[n].any()) >= 3, "reads that lose every anchor"
    dup = [n for n in t.want if n.startswith("dup")]
    assert all(len({x[:3] for x in t.want[n].sd}) < len(t.want[n].sd) for n in dup) and len(dup) == 3


def test_pruned_equals_unpruned(ont):
    n_in, n_kept, n_redo = _check(ont, Run(ont, {}, os.path.join(ont.dir, "on.txt")), ont.base)
    assert n_kept * 2 <= n_in, "at least half of the anchors are dropped"
    assert n_redo == 3  # the reads with a duplicated key, and no other
    for n, want in ont.want.items():  # a read that lost every anchor: no chain, an unmapped record
        if want.sd and not ont.near(n).any():
            assert not want.cn and ont.base.sam.count(("\n%s\t4\t" % n).encode()) == 1


def test_everything_collides(ont):
    """64 bins: every anchor finds its own bin full -- nothing may be dropped by the table, the exact step drops the same anchors
    (in a class whose survivor capacity holds a whole read of this input: otherwise the reads would go to the unpruned sort)"""
    n_in, n_kept, n_redo = _check(ont, Run(ont, {"MM2AMD_PRUNE_BINS": "64", "MM2AMD_SORT_MIN_CLASS": "2"}, os.path.join(ont.dir, "bins.txt")), ont.base)
    assert n_kept * 2 <= n_in and n_redo == 3


def test_survivors_outgrow_the_capacity(ont):
    """a capacity of four survivors: every read with more goes to the unpruned sort"""
    r = Run(ont, {"MM2AMD_PRUNE_CAP": "4"}, os.path.join(ont.dir, "cap.txt"))
    n_in, n_kept, n_redo = _check(ont, r, ont.base)
    assert all(r.kp[n][1] == 1 for n in ont.want if n.startswith("loc")) and n_redo >= 33
    assert any(r.kp[n] == (int(ont.near(n).sum()), 0) and 0 < r.kp[n][0] <= 4 for n in ont.want if ont.want[n].sd), "and a read with fewer is pruned as before"


@pytest.mark.parametrize("min_class", [1, 2, 3, 4])
def test_every_lds_class(ont, min_class):
    n_in, n_kept, n_redo = _check(ont, Run(ont, {"MM2AMD_SORT_MIN_CLASS": str(min_class)}, os.path.join(ont.dir, "class%d.txt" % min_class)), ont.base)
    assert n_kept * 2 <= n_in and n_redo == 3


def test_pruned_read_in_pieces(ont):
    """a piece list made from the counts before pruning: pieces beyond the kept anchors are empty, the others cut the kept anchors"""
    assert max(int(ont.near(n).sum()) for n in ont.want) > 2 * 32
    n_in, n_kept, n_redo = _check(ont, Run(ont, {"MM2AMD_CHAIN_PIECE": "32"}, os.path.join(ont.dir, "piece.txt")), ont.base)
    assert n_kept * 2 <= n_in


OFF = {"rmq": (["-x", "lr:hqae"], None), "hpc": (["-x", "map-pb"], None), "min-score-10": (["-x", "map-ont", "-m", "10"], None), "sr-pairs": (["-x", "sr"], "pairs")}


@pytest.mark.parametrize("what", sorted(OFF))
def test_stays_off(what, planted, tmp_path):
    """where dropping isolated anchors is not exact (another chainer, pairs, spans that differ, a span that is a chain on its own) nothing is dropped"""
    args, inp = OFF[what]
    t = Truth(tgc._in_pairs(str(tmp_path / "in")) if inp else planted, args)
    base = Run(t, {"MM2AMD_ANCHOR_PRUNE": "0"}, os.path.join(str(tmp_path), "base.txt"))
    _check(t, Run(t, {}, os.path.join(str(tmp_path), "on.txt")), base, pruned=False)
    assert sum(len(r.cn) for r in t.want.values()) > 0
