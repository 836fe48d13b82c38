"""seed_collect_kernel's probe rounds (kProbeDepth = 4 chunks of 64 minimizers in flight, hits compacted chunk by chunk) against the reference:
every read's rep_len and anchors from the device (MM2AMD_SEED_DUMP) against the reference's --print-seeds, every anchor's tandem flag
(MM2AMD_SEED_DUMP_FLAGS adds it to the device's lines; the reference prints none) against the flag worked out from the reference's minimizer
list as seed.c:47-48 does, and the mapping output.  The reads are built from the reference's own minimizer lists (mm_sketch) so that the
counts sit on the chunk and round boundaries, and run once with the per-bucket records (I.first) and once without them (MM2AMD_NO_FIRST_SLOT)."""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import reflib  # noqa: E402
from test_gpu_shortreads import DROPIN, REF_BIN, _run, _seed_blocks  # noqa: E402

pytestmark = pytest.mark.gpu

K = 4            # kProbeDepth (seed_chain.hip)
W_ONT, K_ONT = 10, 15  # map-ont's minimizers
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
COUNTS = [0, 1, 63, 64, 65, K * 64 - 1, K * 64, K * 64 + 1, 3 * K * 64]
N_COPIES, REPEAT_LEN = 50, 300


def _n_mz(seq):
    return len(reflib.ref_sketch(seq.tobytes() if isinstance(seq, np.ndarray) else seq, W_ONT, K_ONT))


def _tandem_pairs(seq):
    """indices i with equal hashes at minimizers i and i + 1 of the reference's list"""
    x = reflib.ref_sketch(seq, W_ONT, K_ONT)[:, 0] >> np.uint64(8)
    return set(np.flatnonzero(x[1:] == x[:-1]).tolist())


def _prefix_with_count(contig, rng, want, lo, hi):
    """an exact substring of contig[lo:hi] with exactly `want` minimizers in the reference's sketch"""
    if want == 1:  # a 15-mer that is a minimizer of the contig as well, so that the read's only seed hits
        y = reflib.ref_sketch(contig[lo:hi].tobytes(), W_ONT, K_ONT)[:, 1]
        end = lo + int(y[int(rng.integers(0, len(y)))] >> np.uint64(1) & np.uint64(0x7fffffff))
        return contig[end - K_ONT + 1:end + 1]
    for _ in range(200):
        s = int(rng.integers(lo, hi - 6 * (want + 64)))
        n = K_ONT - 1 if want == 0 else max(K_ONT, int(5.5 * want) - 150)
        while _n_mz(contig[s:s + n]) < want:
            n += 1
        if _n_mz(contig[s:s + n]) == want:
            return contig[s:s + n]
    raise AssertionError("no substring with %d minimizers" % want)


def _plant_tandem(contig, rng, start, index):
    """Overwrites 22 to 28 bases of `contig` with copies of a 7-mer, so that one to seven of its 15-mers occur twice, 7 bases apart: when such a 15-mer
    is a window's minimum, it is taken at both places, one after the other.  The array goes where minimizers `index` and `index + 1` of the read
    contig[start:] become that pair and neither has another equal neighbour: minimizer `index` then gets its tandem flag from the NEXT entry of the
    list alone and minimizer `index + 1` from the PREVIOUS one alone -- across a chunk boundary, from the other chunk.  Returns the place."""
    pos0 = start + int(reflib.ref_sketch(contig[start:start + 7 * (index + 64)].tobytes(), W_ONT, K_ONT)[index, 1] >> np.uint64(1) & np.uint64(0x7fffffff))
    for _ in range(40):
        unit = ACGT[rng.integers(0, 4, 7)]
        if len(set(unit.tolist())) < 3:
            continue
        for n in range(22, 29):
            for at in range(pos0 - 45, pos0 + 5):
                trial = contig.copy()
                trial[at:at + n] = np.tile(unit, 4)[:n]
                tp = _tandem_pairs(trial[start:at + n + 400].tobytes())
                if index in tp and index - 1 not in tp and index + 1 not in tp:
                    contig[:] = trial
                    return at
    raise AssertionError("no place for a pair of equal minimizers at %d | %d" % (index, index + 1))


def _repeat_in_chunk(flank, core, chunk):
    """flank[:n] + core + flank[n:n + 300], n chosen so that the minimizers that lie wholly in `core` -- the read's only frequent seeds -- all have
    places in chunk `chunk` of the first round, away from its ends"""
    for n in range(int(5.5 * (64 * chunk + 10)), int(5.5 * (64 * chunk + 50))):
        read = flank[:n].tobytes() + core.tobytes() + flank[n:n + 300].tobytes()
        end = reflib.ref_sketch(read, W_ONT, K_ONT)[:, 1] >> np.uint64(1) & np.uint64(0x7fffffff)
        inside = np.flatnonzero((end >= n + K_ONT - 1) & (end < n + len(core)))
        if len(inside) and inside.min() >= 64 * chunk + 4 and inside.max() < 64 * chunk + 60:
            return read
    raise AssertionError("no place for the core in chunk %d" % chunk)


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("seed_collect"))
    rng = np.random.default_rng(2025)
    contigs = [ACGT[rng.integers(0, 4, 50000)].copy() for _ in range(4)]
    # a repeat family: 50 copies of a 300 b element whose 36 b core is exact and whose flanks differ by 15 % from copy to copy.  The core's handful of
    # minimizers occur 50 times; they are few enough (under 2e-4 of the distinct minimizers) that the reference's mid_occ stays at its floor of 10
    elem = ACGT[rng.integers(0, 4, REPEAT_LEN)]
    core = slice(REPEAT_LEN // 2 - 18, REPEAT_LEN // 2 + 18)
    rep_at = []
    for c in range(N_COPIES):
        ci, at = 1 + c % 3, 2000 + (c // 3) * 2500 + int(rng.integers(0, 500))
        e = elem.copy()
        m = rng.random(REPEAT_LEN) < 0.15
        m[core] = False
        e[m] = ACGT[rng.integers(0, 4, int(m.sum()))]
        contigs[ci][at:at + REPEAT_LEN] = e
        rep_at.append((ci, at))
    # the tandem read: two equal neighbouring minimizers across the first chunk boundary (63 | 64) and across the round boundary (K * 64 - 1 | K * 64)
    t_start = 1000
    c0 = contigs[0]
    at1 = _plant_tandem(c0, rng, t_start, 63)
    at2 = _plant_tandem(c0, rng, t_start, K * 64 - 1)
    tandem_read = c0[t_start:at2 + 28 + 900].tobytes()
    tp = _tandem_pairs(tandem_read)
    assert {63, K * 64 - 1} <= tp and not {62, 64, K * 64 - 2, K * 64} & tp, (at1, at2, sorted(tp))
    # reads by minimizer count, exact substrings of repeat-free sequence: every minimizer hits once
    reads = [("cnt%d" % n, _prefix_with_count(c0, rng, n, 10000, 50000).tobytes()) for n in COUNTS]
    for (name, s), n in zip(reads, COUNTS):
        assert _n_mz(s) == n, name
    reads.append(("tandem", tandem_read))
    reads.append(("nohit", ACGT[rng.integers(0, 4, 3000)].tobytes()))
    ci, at = rep_at[7]
    reads.append(("repeat", contigs[ci][at - 1500:at + REPEAT_LEN + 1500].tobytes()))        # unique | one copy of the family | unique
    ci, at = rep_at[9]
    reads.append(("repeat_edge", contigs[ci][at + 20:at + REPEAT_LEN + 700].tobytes()))      # starts inside a copy: the streak of frequent seeds begins the read
    # two cores 400 unmatched bases apart between unique flanks: one streak of frequent seeds long enough for occ_dist to keep one of them (the heap)
    c3 = contigs[3]
    reads.append(("repeat_streak", b"".join([c3[40000:40800].tobytes(), elem[core].tobytes(), ACGT[rng.integers(0, 4, 400)].tobytes(), elem[core].tobytes(), c3[40800:41600].tobytes()])))
    # the family's core as the only frequent seeds of a read, in chunk 1 and in chunk 3 of the first round: n_high comes from those chunks alone
    reads.append(("repeat_chunk1", _repeat_in_chunk(c0[5000:7500], elem[core], 1)))
    reads.append(("repeat_chunk3", _repeat_in_chunk(c0[7500:10000], elem[core], 3)))
    reads.append(("one_base", b"A"))
    ref_fa, rd_fa = os.path.join(tmp, "ref.fa"), os.path.join(tmp, "reads.fa")
    open(ref_fa, "w").write("".join(">ctg%d\n%s\n" % (i + 1, c.tobytes().decode()) for i, c in enumerate(contigs)))
    open(rd_fa, "w").write("".join(">%s\n%s\n" % (nm, s.decode()) for nm, s in reads))
    # read pairs for -x sr: the second mate's seeds carry SD_SEG1
    comp = {65: 84, 67: 71, 71: 67, 84: 65}
    p1, p2 = os.path.join(tmp, "r1.fa"), os.path.join(tmp, "r2.fa")
    with open(p1, "w") as f1, open(p2, "w") as f2:
        for j, (ci, st, l1, l2, ins) in enumerate([(0, 20000, 150, 150, 400), (3, 31000, 150, 120, 300), (rep_at[3][0], rep_at[3][1] - 100, 150, 150, 450)]):
            c = contigs[ci]
            f1.write(">pair%d/1\n%s\n" % (j, c[st:st + l1].tobytes().decode()))
            f2.write(">pair%d/2\n%s\n" % (j, bytes(comp[b] for b in c[st + ins - l2:st + ins].tobytes()[::-1]).decode()))
    return {"ref": ref_fa, "reads": rd_fa, "names": [nm for nm, _ in reads], "seqs": dict(reads), "p1": p1, "p2": p2, "tmp": tmp}


def _ref_seed_lines(args, files):
    p = subprocess.run([REF_BIN] + args + ["-t", "1", "--print-qname", "--print-seeds"] + files, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE)
    assert p.returncode == 0, p.stderr.decode()[-1000:]
    return p.stderr.decode().split("\n")


def _dev_seed_lines(args, files, dump, env):
    if os.path.exists(dump):
        os.remove(dump)
    p = subprocess.run([DROPIN] + args + ["-t", "4"] + files, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, env=dict(os.environ, MM2AMD_SEED_DUMP=dump, **env))
    assert p.returncode == 0, p.stderr.decode()[-1000:]
    return open(dump).read().split("\n")


@pytest.fixture(scope="module")
def want_long(case):
    return _seed_blocks(_ref_seed_lines(["-x", "map-ont"], [case["ref"], case["reads"]]))


ENVS = [{}, {"MM2AMD_NO_FIRST_SLOT": "1"}]
ENV_IDS = ["bucket_records", "no_bucket_records"]


@pytest.fixture(scope="module", params=ENVS, ids=ENV_IDS)
def got_long(case, request):
    """the device's blocks, with the tandem flag as a last column of every SD line"""
    env = dict(request.param, MM2AMD_SEED_DUMP_FLAGS="1")
    return _seed_blocks(_dev_seed_lines(["-x", "map-ont"], [case["ref"], case["reads"]], os.path.join(case["tmp"], "seeds_%d.txt" % len(request.param)), env))


def test_the_reads_are_what_the_cases_need(case, want_long):
    """The counts.  What decides where a read's chunks and rounds end is its number of minimizers, which the reference's mm_sketch gives and the fixture
    asserts; the reference's --print-seeds shows the minimizers that hit, one group of anchors each, and for these exact substrings of unique sequence
    every one hits (a read's windows are windows of the contig), so the same counts are asserted from its lines here."""
    assert set(want_long) == set(case["names"])
    for n in COUNTS:
        blk = want_long["cnt%d" % n]
        assert blk[0].startswith("RS\t")
        n_hit = len(set(l.split("\t")[4] for l in blk[1:]))  # distinct query positions among the SD lines: the read's minimizers that hit
        assert n_hit == n, (n, n_hit)
    assert want_long["nohit"] == ["RS\t0"] and want_long["one_base"] == ["RS\t0"]
    for nm in ("repeat", "repeat_edge", "repeat_streak", "repeat_chunk1", "repeat_chunk3"):
        assert int(want_long[nm][0].split("\t")[1]) > 0, nm  # rep_len: seeds above mid_occ were filtered
    assert len(want_long["tandem"]) > K * 64


def test_seeds_match_print_seeds(case, want_long, got_long):
    assert set(got_long) == set(want_long)
    bad = [k for k in case["names"] if want_long[k] != [l.rsplit("\t", 1)[0] if l.startswith("SD\t") else l for l in got_long[k]]]
    assert not bad, bad


def test_tandem_flags_match_the_reference(case, got_long):
    """MM_SEED_TANDEM of every anchor: set when the seed's minimizer has the hash of the one before or after it in the read's list (seed.c:47-48).
    An anchor's query position names its minimizer (map.c:188-196: the last base of the k-mer, counted from the read's other end on the reverse
    strand)."""
    n_set = {}
    for nm in case["names"]:
        seq = case["seqs"][nm]
        mz = reflib.ref_sketch(seq, W_ONT, K_ONT)
        h = mz[:, 0] >> np.uint64(8)
        assert len(h) == 0 or np.unique(h, return_counts=True)[1].max() <= 10  # (mid_occ: the query-side filter leaves the list as it is)
        eq = h[1:] == h[:-1]
        tandem = np.concatenate([eq, [False]]) | np.concatenate([[False], eq])
        at = {int(e): i for i, e in enumerate(mz[:, 1] >> np.uint64(1) & np.uint64(0x7fffffff))}
        n_set[nm] = 0
        for l in got_long[nm][1:]:
            f = l.split("\t")
            qpos, span, flag = int(f[4]), int(f[5]), int(f[7])
            i = at[qpos if f[3] == "+" else len(seq) + span - 2 - qpos]
            assert flag == int(tandem[i]), (nm, i, l)
            n_set[nm] += flag
    assert n_set["tandem"] >= 4, n_set  # minimizers 63 | 64 and K * 64 - 1 | K * 64 hit, and carry the flag


@pytest.mark.parametrize("env", ENVS, ids=ENV_IDS)
def test_pair_seeds_match_print_seeds(case, env):
    """-x sr pairs: a fragment's two minimizer lists joined, the second mate's seeds marked SD_SEG1.  The reference prints a QR line per mate and the device
    one per fragment, so the RS / SD blocks are compared without their names."""
    files = [case["ref"], case["p1"], case["p2"]]
    def blocks(lines):  # one block per fragment, from its RS line on; the lanes write their fragments in the order they finish
        out = []
        for l in lines:
            if l.startswith("RS\t"):
                out.append([l])
            elif l.startswith("SD\t"):
                out[-1].append(l)
        return sorted(out)
    want = blocks(_ref_seed_lines(["-x", "sr"], files))
    got = blocks(_dev_seed_lines(["-x", "sr"], files, os.path.join(case["tmp"], "pairs_%d.txt" % len(env)), env))
    assert len(want) == 3 and sum(len(b) for b in want) > 30
    assert got == want


@pytest.mark.parametrize("env", ENVS, ids=ENV_IDS)
def test_mapping_output_matches(case, env, monkeypatch):
    """the PAF records with CIGARs, end to end (the tandem flag decides which anchors may end a gap fill, align.c:804; these reads do not depend on
    that choice, which is why test_tandem_flags_match_the_reference reads the flags themselves)"""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    args = ["-x", "map-ont", "-c"]
    assert _run([REF_BIN, "-t", "4"] + args + [case["ref"], case["reads"]]) == _run([DROPIN, "-t", "4"] + args + [case["ref"], case["reads"]])
