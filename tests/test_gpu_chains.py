"""The device's chains, chain by chain: what chain_fill_kernel / chain_rmq_kernel / chain_rmq_wide_kernel / chain_backtrack_kernel and the
long-join re-chain produced for every read (MM2AMD_CHAIN_DUMP, minimap2_amd/csrc/chain_dump.hpp) against

  A. the reference binary's own CN lines (`minimap2_ref --print-qname --print-seeds`, map.c:326-330): per read, the sorted list of final chains;
  B. the reference's functions: the dump's parameter line against mm_set_opt / mm_mapopt_update and map.c:262-281, mg_lchain_dp / mg_lchain_rmq
     on the dumped sorted anchors against the dumped first pass (u[] in order, anchors word for word), map.c:283-289's question evaluated on
     the first pass, radix_sort_128x + mg_lchain_rmq(bw_long) against the dumped second pass;
  C. the same under every A/B switch of the chaining step: A and B hold, and the dumps' chains are identical across the switches.

Every comparison is exact equality, every read is compared, and every case asserts from the reference's output that it reaches its path.
The final SAM/PAF cannot see most of this: mm_set_parent / mm_select_sub / best_n drop the weak chains before anything is printed."""
import os
import subprocess
import sys
from collections import Counter

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import chainlib  # noqa: E402
import reflib  # noqa: E402
import synth  # noqa: E402

pytestmark = pytest.mark.gpu
REF_BIN = os.path.join(ROOT, "oracle", "_ref", "minimap2_ref")
EMU = os.environ.get("MM2AMD_EMU") == "1"
DROPIN = os.path.join(HERE, "_build", "dropin_emu" if EMU else "dropin_gpu")  # MM2AMD_EMU=1: tests/conftest.py

MM_F_SPLICE, MM_F_NO_LJOIN, MM_F_SR, MM_F_RMQ = 0x080, 0x400, 0x1000, 0x80000000  # minimap.h
U32 = np.uint64(0xffffffff)


# ---------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------
def _fasta(path):
    out = []
    for line in open(path, "rb"):
        if line.startswith(b">"):
            out.append([line[1:].split()[0].decode(), b""])
        else:
            out[-1][1] += line.strip()
    return [(n, s) for n, s in out]


def _write_reads(path, rds):
    with open(path, "wb") as f:
        for n, s in rds:
            f.write(b">" + n.encode() + b"\n" + s + b"\n")


def _in_ont(d):
    ref, rd, _, _ = synth.make("ont", d, 1 if EMU else 4, 40 if EMU else 150, 19)
    return ref, [rd]


def _in_weird(d):
    ref, rd = synth.make_weird(d)
    return ref, [rd]


def _in_repeats(d):
    ref, rd = synth.make_repeats(d)
    return ref, [rd]


def _in_tandem(d):
    os.makedirs(d, exist_ok=True)
    rng = np.random.default_rng(56)
    contig = chainlib.gen_tandem_array(rng)
    decoy = rng.integers(0, 4, 100000, dtype=np.uint8)
    rds = chainlib.gen_array_reads(rng, contig)
    synth.write_fasta(os.path.join(d, "ref.fa"), ["arr", "decoy"], [contig, decoy])
    _write_reads(os.path.join(d, "reads.fa"), rds[:3] if EMU else rds)
    return os.path.join(d, "ref.fa"), [os.path.join(d, "reads.fa")]


def _in_diverged(d):
    os.makedirs(d, exist_ok=True)
    rng = np.random.default_rng(55)
    contig = chainlib.gen_diverged_elements(rng)
    decoy = rng.integers(0, 4, 200000, dtype=np.uint8)
    reads = synth.gen_reads(rng, [contig], 40, 6000, 2000, 0.08)
    synth.write_fasta(os.path.join(d, "ref.fa"), ["elems", "decoy"], [contig, decoy])
    synth.write_fasta(os.path.join(d, "reads.fa"), ["rep%d" % i for i in range(len(reads))], reads[:10] if EMU else reads)
    return os.path.join(d, "ref.fa"), [os.path.join(d, "reads.fa")]


def _in_deep(d):
    """The deeper array: 20 copies of the 1 500-base element, reads that run from the left flank into the array, then 4 300 random bases, then a
    short error-free tail inside the array.  The tail's anchors on every diagonal but the best one have their predecessor more than 5 000 anchors
    back (the best diagonal's is found by the max_ii shortcut, lchain.c:189-200), so the default max_chain_iter decides whether they chain."""
    os.makedirs(d, exist_ok=True)
    n_copies, hole = 20, 4300
    rng = np.random.default_rng(57)
    contig = chainlib.gen_tandem_array(rng, n_copies=n_copies)
    decoy = rng.integers(0, 4, 100000, dtype=np.uint8)
    rds = []
    for i in range(2 if EMU else 6):
        st, tail = 28000 + 300 * i, 40 + 12 * i
        L = 30000 + (n_copies - 2) * 1500 + 700 - st
        body = synth.mutate_read(rng, contig[st:st + L - hole - tail], 0.03)
        r = np.concatenate([body, rng.integers(0, 4, hole - (len(body) - (L - hole - tail)), dtype=np.uint8), contig[st + L - tail:st + L]])
        if i % 2:
            r = synth.COMP[r[::-1]]
        rds.append(("deep%d" % i, synth.ACGT[r].tobytes()))
    synth.write_fasta(os.path.join(d, "ref.fa"), ["arr", "decoy"], [contig, decoy])
    _write_reads(os.path.join(d, "reads.fa"), rds)
    return os.path.join(d, "ref.fa"), [os.path.join(d, "reads.fa")]


def _in_duplicated(d):
    os.makedirs(d, exist_ok=True)
    rng = np.random.default_rng(56)
    contig = synth.gen_duplicated_reference(rng)
    decoy = rng.integers(0, 4, 200000, dtype=np.uint8)
    reads = synth.gen_reads(rng, [contig], 200, 9000, 3000, 0.08)
    synth.write_fasta(os.path.join(d, "ref.fa"), ["dup", "decoy"], [contig, decoy])
    synth.write_fasta(os.path.join(d, "reads.fa"), ["rep%d" % i for i in range(len(reads))], reads[:30] if EMU else reads)
    return os.path.join(d, "ref.fa"), [os.path.join(d, "reads.fa")]


def _in_hifi(d):
    ref, rd, _, _ = synth.make("hifi", d, 3, 12 if EMU else 80, 24)
    return ref, [rd]


def _in_contigs(d):  # the 100-300 kb queries of test_gpu_dropin.py::test_rmq_presets_identical: a deletion and an inversion
    os.makedirs(d, exist_ok=True)
    rng = np.random.default_rng(41)
    contigs = synth.gen_reference(rng, 3000000, 2)
    reads = synth.gen_reads(rng, contigs, 5, 250000, 30000, 0.02, min_len=100000)
    s = contigs[0][200000:600000].copy()
    s = np.concatenate([s[:100000], s[105000:250000], synth.COMP[s[250000:253000][::-1]], s[253000:]])
    reads.append(synth.mutate_read(rng, s, 0.01))
    synth.write_fasta(os.path.join(d, "ref.fa"), ["c1", "c2"], contigs)
    synth.write_fasta(os.path.join(d, "contigs.fa"), ["q%d" % i for i in range(len(reads))], reads[:1] if EMU else reads)
    return os.path.join(d, "ref.fa"), [os.path.join(d, "contigs.fa")]


def _in_cdna(d):
    ref, rd, _, _ = synth.make("cdna", d, 3, 40 if EMU else 200, 26)
    return ref, [rd]


def _in_pairs(d):
    ref, f1, f2, _ = synth.make_pairs(d)
    return ref, [f1, f2]


def _in_short(d):
    ref, rd = synth.make_short(d)
    return ref, [rd]


# ---------------------------------------------------------------------------------------------------------
# the reference side
# ---------------------------------------------------------------------------------------------------------
def _ref_run(args, ref, files):
    p = subprocess.run([REF_BIN] + list(args) + ["-t", "1", "--print-qname", "--print-seeds", ref] + list(files), stdout=subprocess.DEVNULL, stderr=subprocess.PIPE)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    return chainlib.ref_chain_blocks(p.stderr.decode())


def _n_cn(blocks):
    return sum(len(c) for r in blocks for c in r.cn)


def _chains_of(blocks):
    return [(r.name, sorted(r.cn)) for r in blocks]


def _lookback_depth(blocks, gap_ref):
    """the deepest look-back window of any read (lchain.c:172): anchors on the same target and strand at most gap_ref upstream, from the SD lines"""
    best = 0
    for r in blocks:
        groups = {}
        for t, pos, strand, _, _ in r.sd:
            groups.setdefault((t, strand), []).append(pos)
        for g in groups.values():
            a = np.array(g, dtype=np.int64)
            assert (np.diff(a) >= 0).all()
            best = max(best, int((np.arange(len(a)) - np.searchsorted(a, a - gap_ref, "left")).max()))
    return best


class Opts(object):
    """the chaining options of a command line: mm_set_opt + mm_mapopt_update of the compiled reference, then the command line's own settings (main.c)"""

    def __init__(self, ref_records, args):
        assert args[0] == "-x"
        m = reflib.RefMapper([s for _, s in ref_records], args[1], [n for n, _ in ref_records], cigar=False)
        mo, self.k = m.mo, int(m.io.k)
        rest, i = list(args[2:]), 0
        while i < len(rest):
            o = rest[i]
            if o == "--no-long-join":
                mo.flag |= MM_F_NO_LJOIN
                i += 1
                continue
            v = rest[i + 1]
            if o == "--max-chain-iter": mo.max_chain_iter = int(v)
            elif o == "--max-chain-skip": mo.max_chain_skip = int(v)
            elif o == "-n": mo.min_cnt = int(v)
            elif o == "-m": mo.min_chain_score = int(v)
            elif o == "-g": mo.max_gap = int(v)
            elif o == "-r":
                w = v.split(",")
                mo.bw = int(w[0])
                if len(w) > 1: mo.bw_long = int(w[1])
            else: raise AssertionError("option %s: not one this file knows how to mirror" % o)
            i += 2
        for f in ("flag", "bw", "bw_long", "max_gap", "max_gap_ref", "max_frag_len", "max_chain_skip", "max_chain_iter", "min_cnt", "min_chain_score", "rmq_size_cap",
                  "rmq_inner_dist", "rmq_rescue_size", "mid_occ"):
            setattr(self, f, int(getattr(mo, f)))
        self.rmq_rescue_ratio = np.float32(mo.rmq_rescue_ratio)
        self.pen_gap = float(np.float32(float(mo.chain_gap_scale) * 0.01 * self.k))  # map.c:273-274
        self.pen_skip = float(np.float32(float(mo.chain_skip_scale) * 0.01 * self.k))
        m.close()
        self.is_sr, self.is_splice, self.rmq = bool(self.flag & MM_F_SR), bool(self.flag & MM_F_SPLICE), bool(self.flag & MM_F_RMQ)

    def gaps(self, qlen):  # map.c:262-271
        gap_qry = max(qlen, self.max_gap) if self.is_sr else self.max_gap
        if self.max_gap_ref > 0: gap_ref = self.max_gap_ref
        elif self.max_frag_len > 0: gap_ref = max(self.max_frag_len - qlen, self.max_gap)
        else: gap_ref = self.max_gap
        return gap_ref, gap_qry

    def params(self, qlen, n_seg):  # chainlib.CHAIN_PARAMS
        gap_ref, gap_qry = self.gaps(qlen)
        return (gap_ref, gap_qry, self.bw, self.max_chain_skip, self.max_chain_iter, self.min_cnt, self.min_chain_score, self.pen_gap, self.pen_skip, int(self.is_splice), n_seg,
                int(self.rmq), self.rmq_inner_dist, self.rmq_size_cap, self.bw_long, self.mid_occ)

    def first_pass(self, inp, qlen, n_seg):  # map.c:275-281
        if self.rmq:
            return chainlib.ref_lchain_rmq(inp, self.max_gap, self.rmq_inner_dist, self.bw, self.max_chain_skip, self.rmq_size_cap, self.min_cnt, self.min_chain_score, self.pen_gap, self.pen_skip)
        gap_ref, gap_qry = self.gaps(qlen)
        return reflib.ref_lchain_dp(inp, gap_ref, gap_qry, self.bw, self.max_chain_skip, self.max_chain_iter, self.min_cnt, self.min_chain_score, self.pen_gap, self.pen_skip,
                                    int(self.is_splice), n_seg)

    def rechains(self, u, a, qlen, n_seg):  # map.c:283-285
        if not (self.bw_long > self.bw and (self.flag & (MM_F_SPLICE | MM_F_SR | MM_F_NO_LJOIN)) == 0 and n_seg == 1 and len(u) > 1):
            return False
        st, en = int(a[0][1] & U32), int(a[(int(u[0]) & 0xffffffff) - 1][1] & U32)
        st, en = st - (1 << 32) * (st >> 31), en - (1 << 32) * (en >> 31)
        return qlen - (en - st) > self.rmq_rescue_size or bool(np.float32(en - st) > np.float32(qlen) * self.rmq_rescue_ratio)

    def second_pass(self, a):  # map.c:287-291
        return chainlib.ref_lchain_rmq(reflib.ref_sort128(a), self.max_gap, self.rmq_inner_dist, self.bw_long, self.max_chain_skip, self.rmq_size_cap, self.min_cnt,
                                     self.min_chain_score, self.pen_gap, self.pen_skip)


# ---------------------------------------------------------------------------------------------------------
# the device side
# ---------------------------------------------------------------------------------------------------------
def _dump_run(args, ref, files, env, path):
    if os.path.exists(path):
        os.unlink(path)
    p = subprocess.run([DROPIN] + list(args) + ["-t", "4", "--stats", ref] + list(files), stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, env=dict(os.environ, MM2AMD_CHAIN_DUMP=path, **env))
    if p.returncode < 0 or p.returncode in (124, 134, 137, 139):  # killed by a signal: after a fault nothing more is started on the device
        pytest.exit("the mapper died (status %d) with %r: %s" % (p.returncode, env, p.stderr.decode()[-1500:]), returncode=3)
    assert p.returncode == 0, (env, p.stderr.decode()[-2000:])
    assert "backend=hip:gfx950" in p.stderr.decode(), p.stderr.decode()[-500:]
    return chainlib.chain_dump_blocks(open(path).read()) if os.path.exists(path) else {}


class ReadDump(object):
    """a read's blocks put in order: `first` / `second` are the blocks that hold the first pass's and the re-chain's chains (second: None without one)"""

    def __init__(self, name, blocks, times):
        n = Counter(b.key() for b in blocks)  # (a name that occurs several times in the input: the reads are copies of each other, and so must the blocks be)
        assert all(c == times for c in n.values()), (name, times, sorted(n.values()))
        seen, uniq = set(), []
        for b in blocks:
            if b.key() not in seen:
                seen.add(b.key())
                uniq.append(b)
        by = {}
        for b in uniq:
            by.setdefault((b.pass_no, b.side), []).append(b)
        assert all(len(v) == 1 for v in by.values()) and set(by) <= {(1, "dev"), (1, "host"), (2, "dev"), (2, "host")}, (name, sorted(by))
        assert (1, "dev") in by, "%s: no first-pass block" % name
        assert len(set((b.params, b.qlen) for b in uniq)) == 1, name
        dev1, host1, dev2, host2 = (by.get(k, [None])[0] for k in ((1, "dev"), (1, "host"), (2, "dev"), (2, "host")))
        self.name, self.qlen, self.params, self.inp = name, dev1.qlen, dev1.params, dev1.inp
        assert dev1.inp is not None
        if dev1.handed_back:
            assert host1 is not None and not host1.handed_back and np.array_equal(host1.inp, dev1.inp), "%s: handed back, and no host block with the same anchors" % name
            self.first = host1
        else:
            assert host1 is None, "%s: chained twice" % name
            self.first = dev1
        self.first_on_device = not dev1.handed_back
        self.rechained_on_device = dev2 is not None and not dev2.handed_back
        if self.rechained_on_device:
            assert host2 is None, "%s: re-chained twice" % name
            self.second = dev2
        else:
            assert dev2 is None or host2 is not None, "%s: the re-chain was handed back, and no host block" % name
            self.second = host2
        if host2 is not None and host2.inp is not None:
            assert np.array_equal(host2.inp, reflib.ref_sort128(self.first.a)), "%s: the host re-chain's input is not the sorted first pass" % name
        self.final = self.second if self.second is not None else self.first

    def content(self):
        return (self.inp.tobytes(), self.first.u.tobytes(), self.first.a.tobytes(), None if self.second is None else (self.second.u.tobytes(), self.second.a.tobytes()))


def _cn_tuples(block, tnames):
    out = []
    for c in block.chains():
        out.append(tuple((tnames[int(x) << 1 >> 33 & 0x7fffffff], int(np.int32(np.uint32(x & U32))), "+-"[int(x) >> 63], int(np.int32(np.uint32(y & U32))), int(y) >> 32 & 0xff) for x, y in c))
    return out


def _sd_tuples(inp, tnames):
    return [(tnames[int(x) << 1 >> 33 & 0x7fffffff], int(np.int32(np.uint32(x & U32))), "+-"[int(x) >> 63], int(np.int32(np.uint32(y & U32))), int(y) >> 32 & 0xff) for x, y in inp]


class Case(object):
    """one input and one command line: the reference's side is computed once, check() holds a run of ours against it"""

    def __init__(self, tmp_path, make_input, args):
        self.dir = str(tmp_path)
        self.ref, self.files = make_input(os.path.join(self.dir, "in"))
        self.args = list(args)
        self.want = _ref_run(self.args, self.ref, self.files)
        self.n_cn = _n_cn(self.want)
        assert self.n_cn > 0 and sum(len(r.cn) for r in self.want) > 0
        ref_records = _fasta(self.ref)
        self.tnames = [n for n, _ in ref_records]
        self.opts = Opts(ref_records, self.args)
        reads = [_fasta(f) for f in self.files]
        self.n_seg = len(reads)
        assert all(len(r) == len(reads[0]) for r in reads)
        self.qlen, self.times = {}, Counter()
        for k, (name, s) in enumerate(reads[0]):
            ql = sum(len(r[k][1]) for r in reads)
            assert self.qlen.setdefault(name, ql) == ql
            self.times[name] += 1
        self.want_by_name = {}
        for r in self.want:
            assert self.want_by_name.setdefault(r.name, r).cn == r.cn and self.want_by_name[r.name].sd == r.sd  # (copies of a read under one name)
        assert Counter(r.name for r in self.want) == Counter({n: c for n, c in self.times.items() if self.qlen[n] > 0})
        self.expect = {}   # name -> (first pass, re-chains?, second pass) from the reference's functions on the dumped anchors
        self.contents = None
        self.n_runs = 0

    def max_anchors(self):
        return max(len(r.sd) for r in self.want)

    def depth(self):
        return _lookback_depth(self.want, self.opts.gaps(max(self.qlen.values()))[0])

    def n_rechain_ref(self):
        """reads that satisfy map.c:283-289 on the reference's side (needs a check() before it: the first pass of the reference's function, held equal to the dump's)"""
        return sum(1 for e in self.expect.values() if e[2])

    def check(self, env):
        got = _dump_run(self.args, self.ref, self.files, env, os.path.join(self.dir, "chains.%d.txt" % self.n_runs))
        self.n_runs += 1
        assert set(got) == set(self.want_by_name), (env, sorted(set(got) ^ set(self.want_by_name))[:10])
        reads, o = {}, self.opts
        for name, blocks in got.items():
            rd = reads[name] = ReadDump(name, blocks, self.times[name])
            want = self.want_by_name[name]
            # B: identity
            assert rd.qlen == self.qlen[name], (env, name)
            assert rd.params == o.params(rd.qlen, self.n_seg), (env, name, rd.params, o.params(rd.qlen, self.n_seg))
            assert _sd_tuples(rd.inp, self.tnames) == want.sd, (env, name, "the anchors that entered chaining are not the reference's")
            # B: the reference's functions on the dumped anchors (computed once per read: the anchors are held equal across the runs below)
            if name not in self.expect:
                u1, a1 = o.first_pass(rd.inp, rd.qlen, self.n_seg)
                re = o.rechains(u1, a1, rd.qlen, self.n_seg)
                self.expect[name] = (rd.inp, (u1, a1), re, o.second_pass(a1) if re else None)
            inp0, (u1, a1), re, second = self.expect[name]
            assert np.array_equal(rd.inp, inp0), (env, name)
            assert np.array_equal(rd.first.u, u1), (env, name, "first pass: u[] differs from the reference function's", len(rd.first.u), len(u1))
            assert np.array_equal(rd.first.a, a1), (env, name, "first pass: chained anchors differ from the reference function's")
            assert (rd.second is not None) == re, (env, name, "re-chained: %s, map.c:283-289 says %s" % (rd.second is not None, re))
            if re:
                assert np.array_equal(rd.second.u, second[0]), (env, name, "second pass: u[] differs from the reference function's")
                assert np.array_equal(rd.second.a, second[1]), (env, name, "second pass: chained anchors differ from the reference function's")
            # A: the reference binary's CN lines
            assert sorted(_cn_tuples(rd.final, self.tnames)) == sorted(want.cn), (env, name, "final chains differ from the reference's CN lines")
        # C: identical across the switches
        contents = {n: r.content() for n, r in reads.items()}
        if self.contents is None:
            self.contents = contents
        assert contents == self.contents, (env, [n for n in contents if contents[n] != self.contents[n]][:10])
        return reads


FILL_SWITCHES = [{"MM2AMD_CHAIN_FILL_GLOBAL": "1"}, {"MM2AMD_CHAIN_RING": "128"}, {"MM2AMD_CHAIN_PIECE": "256"}, {"MM2AMD_CHAIN_PIECE": "1000"}]
LONG_JOIN_SWITCHES = [{"MM2AMD_RMQ_PIECE": "64"}, {"MM2AMD_RMQ_DENSE": "96", "MM2AMD_RMQ_PIECE": "64"}, {"MM2AMD_RMQ_RANK_MAX": "8"}, {"MM2AMD_LONG_JOIN_ON_HOST": "1"}]
BATCH_SWITCHES = [{"MM2AMD_SUBBATCH_READS": "3"}, {"MM2AMD_LANES": "1"}]
RMQ_SWITCHES = [{"MM2AMD_RMQ_PIECE": "64"}, {"MM2AMD_RMQ_DENSE": "96", "MM2AMD_RMQ_PIECE": "64"}, {"MM2AMD_RMQ_RANK_MAX": "8"}, {"MM2AMD_RMQ_ON_HOST": "1"}]


def _emu_few(switches, keep):
    """the emulator runs a 50 k-anchor read for minutes: under MM2AMD_EMU=1 the large inputs keep the switches named here"""
    return [s for s in switches if any(k in s for k in keep)] if EMU else switches


# ---------------------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(3600 if EMU else 600)
def test_plain_ont_reads(tmp_path):
    """the common path: almost every anchor isolated, one chain per read"""
    c = Case(tmp_path, _in_ont, ["-x", "map-ont"])
    c.check({})
    for env in FILL_SWITCHES + LONG_JOIN_SWITCHES + BATCH_SWITCHES:
        c.check(env)
    # (a floor, not a figure of merit: a 10 kb read with 12 % errors keeps about 0.88^15 = 15 % of its 2 x 10 000 / 11 minimizers, some 260 anchors, nearly
    # all of them chained; fewer than 100 CN lines per read would mean that the input has stopped mapping)
    assert c.n_cn > 100 * len(c.want)


@pytest.mark.timeout(3600 if EMU else 900)
@pytest.mark.parametrize("args", [["-x", "map-ont"], ["-x", "lr:hqae"], ["-x", "asm20"]], ids=lambda a: a[1])
def test_edge_case_reads(args, tmp_path):
    """make_weird: a 55 k-anchor read (pieces, the global sort), low-complexity islands, reads shorter than k (blocks without anchors), a name that
    occurs twice"""
    c = Case(tmp_path, _in_weird, args)
    assert c.max_anchors() > 4096 and c.max_anchors() > 1000  # pieces at the default length and at the small ones
    rmq = args[1] != "map-ont"
    if args[1] != "lr:hqae":
        assert c.n_cn >= 100000  # (this case alone compares 10^5 CN lines per run; the file's other inputs bring 10^4 to 2 x 10^5 each)
    rds = c.check({})
    if rmq:
        assert sum(1 for r in rds.values() if r.first_on_device and len(r.inp)) > 0
    if EMU:
        return  # (minutes per run on the emulator: the switches run on the GPU)
    for env in (RMQ_SWITCHES if rmq else FILL_SWITCHES + LONG_JOIN_SWITCHES) + BATCH_SWITCHES:
        rds = c.check(env)
        if "MM2AMD_RMQ_ON_HOST" in env:
            assert not any(r.first_on_device for r in rds.values())


REPEAT_INPUTS = {"tandem": _in_tandem, "diverged": _in_diverged, "repeats": _in_repeats}
CUTS = {"default": [], "iter200-skip5": ["--max-chain-iter", "200", "--max-chain-skip", "5"], "iter50": ["--max-chain-iter", "50"]}


# Where the lowered cuts change the reference's own result, measured with the reference alone on these inputs (reads whose sorted CN chains differ from the
# default cut's, long join on / off):   tandem array   iter200-skip5  0 / 0 of 12     iter50  0 / 12 of 12
#                                       60 elements    iter200-skip5  2 / 4 of 40     iter50  8 / 15 of 40
#                                       make_repeats   iter200-skip5  0 / 0 of 42     iter50  0 / 0 of 42
# On the tandem array the skip rule ends the inner loop long before 200 candidates, and what --max-chain-iter 50 changes in the first pass the re-chain by
# mg_lchain_rmq (map.c:283-292, no such cut) undoes; make_repeats' windows of up to 320 anchors are clamped, and the reference chains the same.  So the
# window is clamped in every lowered case (asserted), and that the clamp changes the reference's chains is asserted where the reference shows it.
CUT_CHANGES_CN = {("tandem", "iter50-no-long-join"), ("diverged", "iter200-skip5"), ("diverged", "iter50"), ("diverged", "iter200-skip5-no-long-join"), ("diverged", "iter50-no-long-join")}
CUT_CHANGES_FIRST_PASS = CUT_CHANGES_CN | {("tandem", "iter50")}


def _first_pass_differs(c, rds, max_iter, max_skip):
    """reads whose first pass, by the reference's mg_lchain_dp on the same anchors, is another one with this cut and skip limit"""
    o, n = c.opts, 0
    for r in rds.values():
        gap_ref, gap_qry = o.gaps(r.qlen)
        u, a = reflib.ref_lchain_dp(r.inp, gap_ref, gap_qry, o.bw, max_skip, max_iter, o.min_cnt, o.min_chain_score, o.pen_gap, o.pen_skip, int(o.is_splice), c.n_seg)
        n += not (np.array_equal(u, c.expect[r.name][1][0]) and np.array_equal(a, c.expect[r.name][1][1]))
    return n


@pytest.mark.timeout(3600 if EMU else 900)
@pytest.mark.parametrize("cut", list(CUTS) + [k + "-no-long-join" for k in CUTS if k != "default"])
@pytest.mark.parametrize("which", list(REPEAT_INPUTS))
def test_repeat_rich_reads(which, cut, tmp_path):
    """look-back beyond the LDS ring, the skip rule and the max_ii shortcut active, thousands of chains per read; with the lowered cuts max_chain_iter
    binds everywhere (lchain.c:173): every lowered case asserts that some window is deeper than the cut.  Whether the clamp then changes the reference's
    own chains is the reference's business (the table above CUT_CHANGES_CN): it is asserted for the cases where it does, and every lowered command
    line has a twin with --no-long-join, because the re-chain hides from the CN lines what the cut did to the first pass."""
    no_lj = cut.endswith("-no-long-join")
    base = ["--no-long-join"] if no_lj else []
    c = Case(tmp_path, REPEAT_INPUTS[which], ["-x", "map-ont"] + CUTS[cut.replace("-no-long-join", "")] + base)
    assert c.depth() > 256, "no read looks back beyond the ring"
    assert c.max_anchors() > 1000, "no read is cut into pieces of 1000"
    lowered = not cut.startswith("default")
    if lowered:
        assert c.depth() > c.opts.max_chain_iter
        cn_differs = _chains_of(c.want) != _chains_of(_ref_run(["-x", "map-ont"] + base, c.ref, c.files))
        print("%s %s: the reference's CN lines differ from the default cut's: %s" % (which, cut, cn_differs))
        if (which, cut) in CUT_CHANGES_CN and (not EMU or cut == "iter50-no-long-join"):  # (the emulator's runs take the first reads of an input only)
            assert cn_differs, "the lowered cut changes nothing in the reference's chains"
    rds = c.check({})
    if lowered:
        n = _first_pass_differs(c, rds, 5000, 25)
        print("%s %s: reads whose first pass differs from the default cut's by the reference's mg_lchain_dp: %d of %d" % (which, cut, n, len(rds)))
        if (which, cut) in CUT_CHANGES_FIRST_PASS and (not EMU or cut.startswith("iter50")):
            assert n > 0, "the lowered cut changes no read's first pass"
    switches = FILL_SWITCHES + BATCH_SWITCHES + ([] if no_lj else LONG_JOIN_SWITCHES)
    for env in _emu_few(switches, ["RING", "PIECE", "LONG_JOIN", "SUBBATCH"]):
        c.check(env)


@pytest.mark.timeout(3600 if EMU else 900)
@pytest.mark.parametrize("extra", [[], ["--no-long-join"]], ids=["default", "no-long-join"])
def test_deep_array_reaches_the_default_cut(extra, tmp_path):
    """max_chain_iter binding at its default of 5 000 (lchain.c:173; no other input of the suite reaches it: the deepest window elsewhere is 3 587).
    Preconditions, from the reference alone: a look-back window deeper than 5 000 anchors; the reference's first pass (mg_lchain_dp on its own
    anchors) differs between max_iter 5 000 and 1 000 000; and with --no-long-join the reference binary's CN lines differ between the two too.
    With the long join on, the reference's FINAL chains did not depend on the cut for any read of this family (96 reads, 12 seeds, holes of
    3.6-4.7 kb, tails of 35-600 bases tried on the host): the re-chain by mg_lchain_rmq keeps the same anchors either way.  So the default
    command line is held at the first pass (layer B, exact), and its twin without the long join carries the difference into layer A."""
    c = Case(tmp_path, _in_deep, ["-x", "map-ont"] + extra)
    assert c.opts.max_chain_iter == 5000 and c.depth() > 5000, c.depth()
    if extra:
        assert _chains_of(c.want) != _chains_of(_ref_run(c.args + ["--max-chain-iter", "1000000"], c.ref, c.files)), "the default cut changes nothing in the reference's chains"
    rds = c.check({})
    differ = _first_pass_differs(c, rds, 1000000, c.opts.max_chain_skip)
    assert differ > 0, "the default cut changes no read's first pass"
    for env in _emu_few(FILL_SWITCHES + BATCH_SWITCHES, []):
        c.check(env)


@pytest.mark.timeout(3600 if EMU else 900)
@pytest.mark.parametrize("extra", [[], ["-r", "500,20000"], ["--no-long-join"]], ids=["default", "r500-20000", "no-long-join"])
def test_long_join_on_the_device(extra, tmp_path):
    """the duplicated reference: every read has more than one chain; rechain_gather_kernel, the sort by reference position, chain_rmq_kernel with bw_long and
    the backtrack again -- and reads that decline the re-chain"""
    c = Case(tmp_path, _in_duplicated, ["-x", "map-ont"] + extra)
    rds = c.check({})
    if "--no-long-join" in extra:
        assert c.n_rechain_ref() == 0 and not any(r.second for r in rds.values())
    else:
        assert c.n_rechain_ref() >= 0.1 * len(rds), c.n_rechain_ref()
        assert sum(1 for r in rds.values() if r.rechained_on_device) > 0
    for env in LONG_JOIN_SWITCHES + BATCH_SWITCHES + _emu_few(FILL_SWITCHES, ["RING", "PIECE"]):
        rds = c.check(env)
        if "MM2AMD_LONG_JOIN_ON_HOST" in env:
            assert not any(r.rechained_on_device for r in rds.values())
            assert sum(1 for r in rds.values() if r.second is not None) == c.n_rechain_ref()


@pytest.mark.timeout(3600 if EMU else 900)
@pytest.mark.parametrize("preset", ["asm20", "lr:hqae", "asm5"])
@pytest.mark.parametrize("which", ["hifi", "contigs"])
def test_rmq_presets(which, preset, tmp_path):
    """chain_rmq_kernel as the primary chainer (MM_F_RMQ, map.c:275-277), the wide kernel for the long clusters, the host chainer as its A/B partner"""
    c = Case(tmp_path, _in_hifi if which == "hifi" else _in_contigs, ["-x", preset])
    rds = c.check({})
    assert sum(1 for r in rds.values() if r.first_on_device and len(r.inp)) > 0, "no read was chained by the kernel"
    for env in _emu_few(RMQ_SWITCHES + BATCH_SWITCHES, ["RMQ_ON_HOST", "RMQ_DENSE"] if which == "hifi" else ["RMQ_ON_HOST"]):
        rds = c.check(env)
        if "MM2AMD_RMQ_ON_HOST" in env:
            assert not any(r.first_on_device for r in rds.values())


@pytest.mark.timeout(3600 if EMU else 900)
@pytest.mark.parametrize("preset", ["asm20", "lr:hqae"])
def test_rmq_presets_hand_back(preset, tmp_path):
    """reads the RMQ kernel hands back to the host's tie-exact tree, under an RMQ preset on a repeat input.  The reference decides nothing here -- every read
    is compared whichever side chained it; the counts only show that both paths ran.  No read of make_repeats, the tandem array or the 60 elements is
    handed back on its own under asm20 / lr:hqae (measured: 0 of 42, 0 of 3 and 0 of 10 on the emulator; the number is printed), and no input that
    brings a tie in a range minimum was found for this file.  The hand-back is therefore forced with the mapper's own switch for it,
    MM2AMD_RMQ_DEV_MAX_ANCHORS, set to the median anchor count: half of the reads go through the device block marked handed-back and the host block
    of mapper.cpp, the other half through the kernel, and both must give the chains of the run without the switch."""
    c = Case(tmp_path, _in_repeats, ["-x", preset])
    rds = c.check({})
    assert sum(1 for r in rds.values() if r.first_on_device and len(r.inp)) > 0, "no read was chained by the kernel"
    print("%s: %d of %d reads handed back without the switch" % (preset, sum(1 for r in rds.values() if not r.first_on_device), len(rds)))
    median = sorted(len(r.sd) for r in c.want)[len(c.want) // 2]
    rds = c.check({"MM2AMD_RMQ_DEV_MAX_ANCHORS": str(median)})
    assert sum(1 for r in rds.values() if not r.first_on_device) > 0, "no read was handed back"
    assert sum(1 for r in rds.values() if r.first_on_device and len(r.inp)) > 0, "no read was chained by the kernel"
    for env in _emu_few(RMQ_SWITCHES + BATCH_SWITCHES, ["RMQ_ON_HOST", "RMQ_RANK"]):
        c.check(env)


@pytest.mark.timeout(3600 if EMU else 600)
def test_spliced_reads(tmp_path):
    """-x splice: is_cdna = 1 in the link score, max_drop = INT32_MAX in the backtrack (lchain.c:162)"""
    c = Case(tmp_path, _in_cdna, ["-x", "splice"])
    assert c.opts.is_splice
    c.check({})
    for env in FILL_SWITCHES + BATCH_SWITCHES:
        c.check(env)


@pytest.mark.timeout(3600 if EMU else 600)
def test_read_pairs(tmp_path):
    """-x sr with two files: n_seg = 2 (chain_fill_kernel<true, ...>, the segment-aware link score); the anchors' segment bits are in the dump's 64-bit y"""
    c = Case(tmp_path, _in_pairs, ["-x", "sr"])
    assert c.n_seg == 2 and c.opts.is_sr
    rds = c.check({})
    assert any(((r.inp[:, 1] >> np.uint64(48)) & np.uint64(0xff)).any() for r in rds.values() if len(r.inp)), "no anchor of a second segment"
    for env in FILL_SWITCHES + BATCH_SWITCHES:
        c.check(env)


@pytest.mark.timeout(3600 if EMU else 600)
def test_short_single_end_reads(tmp_path):
    """-x sr, one file: gap_qry = qlen for reads longer than max_gap (map.c:263-264), heap-ordered anchors going into chaining"""
    c = Case(tmp_path, _in_short, ["-x", "sr"])
    assert any(q > c.opts.max_gap for q in c.qlen.values())
    c.check({})
    for env in FILL_SWITCHES + BATCH_SWITCHES:
        c.check(env)


@pytest.mark.timeout(3600 if EMU else 900)
@pytest.mark.parametrize("extra", [["-n", "1", "-m", "10"], ["-n", "5", "-m", "200"], ["-g", "200"], ["-r", "50"]], ids=lambda e: "".join(e))
@pytest.mark.parametrize("which", ["ont", "diverged"])
def test_backtrack_and_distance_edges(which, extra, tmp_path):
    """min_cnt / min_chain_score at the edges of the backtrack (single-anchor chains with -n 1 -m 10), tight max_dist (-g) and bandwidth (-r)"""
    c = Case(tmp_path, _in_ont if which == "ont" else _in_diverged, ["-x", "map-ont"] + extra)
    if which == "diverged" or extra[0] == "-n" and extra[1] == "1":  # (the plain reads have one strong chain each: the other three settings leave the reference's chains as they are)
        assert _chains_of(c.want) != _chains_of(_ref_run(["-x", "map-ont"], c.ref, c.files)), "the option changes nothing in the reference's chains"
    rds = c.check({})
    if extra[0] == "-n" and extra[1] == "1":
        assert any((r.first.u & U32 == np.uint64(1)).any() for r in rds.values() if len(r.first.u)), "no single-anchor chain"
    for env in _emu_few(FILL_SWITCHES + BATCH_SWITCHES, ["RING", "PIECE", "SUBBATCH"]) + _emu_few(LONG_JOIN_SWITCHES, ["LONG_JOIN"]):
        c.check(env)


def test_dump_of_a_second_seeding_is_the_first_only(tmp_path):
    """-f x,y (map.c:293-316) seeds a sub-batch a second time: that call writes no blocks, so every read still has one first-pass block (the second
    seeding's chains are out of this file's scope, and no other case raises max_occ)"""
    ref, rd = synth.make_repeats(str(tmp_path / "in"))
    names = [n for n, _ in _fasta(rd)]
    got = _dump_run(["-x", "map-ont", "-f", "3,50"], ref, [rd], {}, str(tmp_path / "chains.txt"))
    assert set(got) == set(names)
    assert all(sum(1 for b in blocks if b.pass_no == 1 and b.side == "dev") == 1 for blocks in got.values())
