"""=/X CIGARs on the device (cigar_eqx_kernel, MM_F_EQX): the cases of tests/test_gpu_eqx.py (hardware) and tests/test_eqx_emu.py (the kernel's own
source under the wave emulator).  Judges, never the code under test: the UNMODIFIED reference's mm_update_extra with is_eqx = 1
(reflib.ref_update_extra(..., eqx=True), oracle/ref_align_shim.c) for regions, the reference binary's --eqx for mapped reads."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import rec_text_cases as R  # noqa: E402
import reflib  # noqa: E402
import synth  # noqa: E402
import test_gpu_regions as G  # noqa: E402  (_sv_reads; its own cases are GPU-marked)
import test_gpu_update_extra as T  # noqa: E402  (random_region)

HAVE_REFALIGN = os.path.exists(reflib.REFALIGN_SO)
HAVE_BIN = os.path.exists(reflib.REF_BIN)
MAT = reflib.ts_mat(2, 4)
Q, E = 4, 2
OP_COUNTS = [1, 2, 3, 8, 40, 150, 600]
N_RANDOM = 500
# what the random set must hold, counted on the REFERENCE's output (regions with an X; regions relabelled in place).  The reference alone gives
# 339 / 161 (log_gap = 1) and 343 / 157 (log_gap = 0) with the seeds below (tests/test_eqx_emu.py asserts it without the device)
MIN_SPLIT, MIN_INPLACE = 100, 20


# ---------------------------------------------------------------------------------------------------------
# 1. regions through update_extra_batch(..., eqx=True)
# ---------------------------------------------------------------------------------------------------------
def build(rng, ops, p_mis=0.0, mis_at=()):
    """a region of one window from (op, len) pairs: random sequences, match columns unequal with probability p_mis and at the listed match columns
    (counted over all matches)"""
    tlen = sum(l for o, l in ops if o in (0, 2, 3))
    t = rng.integers(0, 4, tlen, dtype=np.uint8)
    q, tp, col = [], 0, 0
    for o, l in ops:
        if o == 0:
            seg = t[tp:tp + l].copy()
            mask = rng.random(l) < p_mis
            for c in mis_at:
                if col <= c < col + l:
                    mask[c - col] = True
            seg[mask] = (seg[mask] + rng.integers(1, 4, int(mask.sum()), dtype=np.uint8)) % 4
            q.append(seg)
            tp, col = tp + l, col + l
        elif o == 1:
            q.append(rng.integers(0, 4, l, dtype=np.uint8))
        else:
            tp += l
    q = np.concatenate(q) if q else np.zeros(0, dtype=np.uint8)
    return q.tobytes(), t.tobytes(), [[l << 4 | o for o, l in ops]]


def alternating(n, mlen):
    """n operations: matches of mlen columns with a short insertion or deletion between them (an even n: one deletion is followed by a skip)"""
    gaps = [(1, 1), (2, 1), (1, 2), (2, 2)]
    ops = []
    for i in range(n - 1 + n % 2):
        ops.append((0, mlen) if i % 2 == 0 else gaps[(i // 2) % 4])
    if n % 2 == 0:
        ops[1] = (2, 1)
        ops.insert(2, (3, 30))
    assert len(ops) == n
    return ops


SINGLE_LENGTHS = [1, 63, 64, 65, 127, 128, 129, 200]
COUNTED = (255, 256, 257)


def directed_jobs():
    """[(label, job)]"""
    rng = np.random.default_rng(43)
    out = [("identity", (b"\0\1\2", b"\0\1\2", [[3 << 4]])), ("all-mismatch", (b"\0\1\2", b"\3\3\3", [[3 << 4]])), ("one-inside", (b"\0\1\2\3", b"\0\1\1\3", [[4 << 4]]))]
    for L in SINGLE_LENGTHS:
        for c in sorted({0, 62, 63, 64, 65, L - 1}):
            if c < L:
                out.append(("single %d, column %d" % (L, c), build(rng, [(0, L)], mis_at=[c])))
    out.append(("run 62..66", build(rng, [(0, 200)], mis_at=[62, 63, 64, 65, 66])))
    out.append(("N columns", (bytes([0, 4, 4, 1, 2, 3]), bytes([0, 4, 0, 1, 2, 3]), [[6 << 4]])))
    out.append(("leading insertion", build(rng, [(1, 3), (0, 20)], mis_at=[2, 10])))
    out.append(("leading deletion", build(rng, [(2, 3), (0, 20)], mis_at=[2, 10])))
    out.append(("I D N between", build(rng, [(0, 10), (1, 2), (0, 10), (2, 3), (0, 10), (3, 50), (0, 10)], mis_at=[5, 15, 25, 35])))
    for n in COUNTED:
        out.append(("%d operations" % n, build(rng, alternating(n, 8), p_mis=0.2)))
    out.append(("7000 operations", build(rng, alternating(6999, 10), p_mis=0.1)))
    return out


_CASES = {}


def kernel_cases(log_gap):
    """(labels, jobs, the reference's =/X results, the reference's plain results): computed once per log_gap"""
    if log_gap not in _CASES:
        rng = np.random.default_rng(41 + log_gap)
        jobs = [T.random_region(rng, int(rng.choice(OP_COUNTS)), int(rng.choice([1, 2, 4])), float(rng.choice([0.0, 0.03, 0.1])), float(rng.choice([0.0, 0.02, 0.1])))
                for _ in range(N_RANDOM)]
        labels = ["random %d" % i for i in range(N_RANDOM)]
        for lb, j in directed_jobs():
            labels.append(lb), jobs.append(j)
        eqx = [reflib.ref_update_extra(q, t, p, MAT, Q, E, log_gap, eqx=True) for q, t, p in jobs]
        plain = [reflib.ref_update_extra(q, t, p, MAT, Q, E, log_gap) for q, t, p in jobs]
        _CASES[log_gap] = (labels, jobs, eqx, plain)
    return _CASES[log_gap]


def reference_shapes(log_gap):
    """what the REFERENCE's output holds, for the cases' own assertions"""
    labels, jobs, eqx, plain = kernel_cases(log_gap)
    ops = [[c & 0xf for c in w[0]] for w in eqx]
    by = dict(zip(labels, range(len(labels))))
    return dict(n_split=sum(8 in o for o in ops[:N_RANDOM]), n_inplace=sum(7 in o and 8 not in o for o in ops[:N_RANDOM]),
                run=eqx[by["run 62..66"]][0], all_mismatch=eqx[by["all-mismatch"]][0], n_columns=eqx[by["N columns"]][0],
                counted=[len(plain[by["%d operations" % n]][0]) for n in COUNTED], between=ops[by["I D N between"]],
                big_in=len(jobs[by["7000 operations"]][2][0]), big_out=len(eqx[by["7000 operations"]][0]),
                shifts=(eqx[by["leading insertion"]][5], eqx[by["leading deletion"]][6]))


def check_reference_shapes(log_gap):
    s = reference_shapes(log_gap)
    assert s["n_split"] > MIN_SPLIT and s["n_inplace"] > MIN_INPLACE, s  # the random set takes both paths
    assert s["run"] == (62 << 4 | 7, 5 << 4 | 8, 133 << 4 | 7)           # one 5X, not cut at a 64-column step
    assert s["all_mismatch"] == (3 << 4 | 7,)                             # the in-place quirk
    assert s["n_columns"] == (2 << 4 | 7, 1 << 4 | 8, 3 << 4 | 7)         # N against N is =, N against A is X
    assert s["counted"] == list(COUNTED)                                  # (nothing slid away: the kernel sees 255, 256 and 257 operations)
    assert {1, 2, 3, 7, 8} <= set(s["between"])
    assert s["big_in"] <= 7168 < s["big_out"], s
    assert s["shifts"] == (3, 3)


def check_kernel(mm, log_gap):
    labels, jobs, want, plain = kernel_cases(log_gap)
    check_reference_shapes(log_gap)
    got = mm.update_extra_batch(jobs, MAT, Q, E, log_gap, eqx=True)
    for i, lb in enumerate(labels):
        assert got[i] == want[i], "%s (%d operations in %d windows): %r != %r" % (lb, sum(len(p) for p in jobs[i][2]), len(jobs[i][2]), got[i], want[i])
    got = mm.update_extra_batch(jobs, MAT, Q, E, log_gap)  # without eqx: as before
    for i, lb in enumerate(labels):
        assert got[i] == plain[i], "%s without eqx: %r != %r" % (lb, got[i], plain[i])


def check_sizing(mm):
    """the sizing call's counts are the real call's; a pool one word short: ENOMEM, counts filled, nothing written"""
    labels, jobs, want, _ = kernel_cases(1)
    jobs, want = jobs[N_RANDOM - 40:], want[N_RANDOM - 40:]  # forty random regions and the directed ones
    n = len(jobs)
    arr, keep, _ = mm.fin_jobs(jobs)
    call = mm.lib().mm2amd_update_extra_eqx_batch
    sized = (mm.FinRes * n)()
    assert call(n, arr, bytes(MAT), Q, E, 1, sized, None, 0) == 0
    counts = [r.n_cigar for r in sized]
    assert counts == [len(w[0]) for w in want]
    total = sum(counts)
    GUARD = 0xA5A5A5A5
    pool = (C.c_uint32 * (total + 1))(*([GUARD] * (total + 1)))
    res = (mm.FinRes * n)()
    assert call(n, arr, bytes(MAT), Q, E, 1, res, pool, total) == 0
    assert [r.n_cigar for r in res] == counts and [r.cigar_off for r in res] == [r.cigar_off for r in sized]
    assert pool[total] == GUARD
    for i in range(n):
        assert tuple(pool[res[i].cigar_off:res[i].cigar_off + res[i].n_cigar]) == want[i][0]
    short = (C.c_uint32 * total)(*([GUARD] * total))  # room for total - 1 words, then the guard word
    res = (mm.FinRes * n)()
    assert call(n, arr, bytes(MAT), Q, E, 1, res, short, total - 1) == mm.ENOMEM
    assert [r.n_cigar for r in res] == counts
    assert all(w == GUARD for w in short)
    del keep


# ---------------------------------------------------------------------------------------------------------
# 2. mapped reads against the reference binary
# ---------------------------------------------------------------------------------------------------------
MAPPED_CASES = [  # (name, the binary's options, preset, Aligner arguments)
    ("c", ["-c", "--eqx"], "map-ont", dict(extra_flags=R.F_OUT_CG)),
    ("a", ["-a", "--eqx"], "map-ont", dict(sam=True)),
    ("c_cs", ["-c", "--eqx", "--cs"], "map-ont", dict(extra_flags=R.F_OUT_CG | R.F_OUT_CS)),
    ("a_MD", ["-a", "--eqx", "--MD"], "map-ont", dict(sam=True, extra_flags=R.F_OUT_MD)),
    ("hifi_c", ["-c", "--eqx"], "map-hifi", dict(extra_flags=R.F_OUT_CG)),
]


def mapped_run(mm, refs, names, batch_of, preset, kw, eqx):
    """one Aligner, one batch: (device text, host writer's text, packed hit records, last_stats, profile)"""
    al = mm.Aligner(refs, preset=preset, names=names, n_threads=4, eqx=eqx, **kw)
    try:
        mm.profile_enable(True)  # (also clears what earlier runs accumulated)
        al.stage(batch_of(mm))
        n_reg, reg, rep_len = al.run(raw=True)
        try:
            st, prof = al.last_stats(), mm.profile_get()
            need = mm.lib().mm2amd_pack_regs(len(n_reg), n_reg, reg, None, 0)
            assert need >= 0
            buf = C.create_string_buffer(max(int(need), 1))
            assert mm.lib().mm2amd_pack_regs(len(n_reg), n_reg, reg, buf, need) == need
            dev = al.format_raw(n_reg, reg, rep_len, device=True)
            host = al.format_raw(n_reg, reg, rep_len)
        finally:
            al.free_raw(n_reg, reg)
        return dev, host, buf.raw[:need], st, prof
    finally:
        mm.profile_enable(False)
        al.close()


def eqx_launches(prof):
    return sum(v["launches"] for k, v in prof.items() if k.startswith("cigar_eqx_kernel"))


def check_routes(mm, monkeypatch, want, refs, names, batch_of, preset, kw, min_host=0):
    """--eqx on the device route: the binary's text, the reads where they are without --eqx, the kernel launched; MM2AMD_DEVICE_EQX=0: the same text and
    records from the host's rounds"""
    monkeypatch.delenv("MM2AMD_DEVICE_EQX", raising=False)
    dev, host, packed, st, prof = mapped_run(mm, refs, names, batch_of, preset, kw, True)
    assert dev == want, R.first_difference(dev, want)
    assert host == want
    _, _, _, st_plain, prof_plain = mapped_run(mm, refs, names, batch_of, preset, kw, False)
    # Z-drop hand-backs do not depend on the flag: the routing with --eqx is the routing without it
    assert st["n_region_reads_dev"] == st_plain["n_region_reads_dev"] > 0, (st["n_region_reads_dev"], st_plain["n_region_reads_dev"])
    assert st["n_region_reads_host"] == st_plain["n_region_reads_host"] >= min_host
    assert eqx_launches(prof) > 0 and eqx_launches(prof_plain) == 0
    monkeypatch.setenv("MM2AMD_DEVICE_EQX", "0")
    dev0, host0, packed0, st0, prof0 = mapped_run(mm, refs, names, batch_of, preset, kw, True)
    assert dev0 == want and host0 == want
    assert st0["n_region_reads_dev"] == 0 and eqx_launches(prof0) == 0
    assert packed0 == packed  # the two routes' hit records byte by byte, mm_extra_t::capacity included
    return st


def check_mapped(mm, monkeypatch, mapped, case):
    ref_fa, reads_fq, refs, names, rds = mapped
    _, opts, preset, kw = case
    want = R.binary_text(ref_fa, reads_fq, opts, preset=preset)
    assert b"X" in want and b"=" in want
    check_routes(mm, monkeypatch, want, refs, names, lambda m: R.batch_with_quality(m, rds), preset, kw)


# ---------------------------------------------------------------------------------------------------------
# 3. hand-backs, 4. short reads
# ---------------------------------------------------------------------------------------------------------
HANDBACK_SEED = 52  # chosen on a run without --eqx: 3 of the 16 reads need the host's rounds, 13 stay on the device route


def handback_inputs(outdir):
    rng = np.random.default_rng(HANDBACK_SEED)
    contigs = synth.gen_reference(rng, 800000, 2)
    reads = G._sv_reads(rng, contigs, 8, 0.08) + synth.gen_reads(rng, contigs, 8, 4000, 1000, 0.08)
    refs, names = [synth.ACGT[c].tobytes() for c in contigs], ["chr1", "chr2"]
    rds = [(b"read%d" % i, synth.ACGT[r].tobytes()) for i, r in enumerate(reads)]
    ref_fa, reads_fa = os.path.join(outdir, "ref.fa"), os.path.join(outdir, "reads.fa")
    synth.write_fasta(ref_fa, names, contigs)
    with open(reads_fa, "wb") as f:
        for nm, s in rds:
            f.write(b">" + nm + b"\n" + s + b"\n")
    return ref_fa, reads_fa, refs, names, rds


def check_handbacks(mm, monkeypatch, outdir):
    ref_fa, reads_fa, refs, names, rds = handback_inputs(outdir)
    want = R.binary_text(ref_fa, reads_fa, ["-a", "--eqx"])
    st = check_routes(mm, monkeypatch, want, refs, names, lambda m: m.Batch(rds), "map-ont", dict(sam=True), min_host=1)
    assert st["n_region_reads_host"] >= 1 and st["n_region_reads_dev"] >= 1, st


def short_inputs(outdir, n_pairs=64):
    rng = np.random.default_rng(57)
    contigs = synth.gen_reference(rng, 400000, 2)
    pairs = []
    for k in range(n_pairs):
        c = contigs[k % 2]
        ins = int(rng.integers(320, 600))
        st = int(rng.integers(0, len(c) - ins))
        a, b = c[st:st + 150].copy(), synth.COMP[c[st + ins - 150:st + ins][::-1]]
        for s in (a, b):  # ~1 % substitutions; every fourth pair is exact (its CIGARs are relabelled in place)
            if k % 4:
                m = rng.random(len(s)) < 0.012
                s[m] = (s[m] + rng.integers(1, 4, int(m.sum()), dtype=np.uint8)) % 4
        if k % 8 == 5:  # a small deletion in the first mate
            a = np.concatenate([a[:70], a[74:], c[st + 150:st + 154]])
        if rng.random() < 0.5:
            a, b = b, a
        pairs.append((b"pair%d" % k, synth.ACGT[a].tobytes(), synth.ACGT[b].tobytes()))
    refs, names = [synth.ACGT[c].tobytes() for c in contigs], ["chr1", "chr2"]
    ref_fa, f1, f2 = (os.path.join(outdir, n) for n in ("ref.fa", "r1.fa", "r2.fa"))
    synth.write_fasta(ref_fa, names, contigs)
    for path, which in ((f1, 1), (f2, 2)):
        with open(path, "wb") as f:
            for p in pairs:
                f.write(b">" + p[0] + b"/%d\n" % which + p[which] + b"\n")
    return ref_fa, f1, f2, refs, names, pairs


def check_short(mm, monkeypatch, outdir):
    ref_fa, f1, f2, refs, names, pairs = short_inputs(outdir)
    out = subprocess.run([reflib.REF_BIN, "-x", "sr", "-t", "2", "-a", "--eqx", ref_fa, f1, f2], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, check=True).stdout
    want = b"".join(ln + b"\n" for ln in out.split(b"\n") if ln and not ln.startswith(b"@"))
    cig = [ln.split(b"\t")[5] for ln in want.split(b"\n") if ln]
    assert any(b"X" in c for c in cig) and any(c == b"150=" for c in cig)  # both verdicts are in the REFERENCE's text
    check_routes(mm, monkeypatch, want, refs, names, lambda m: m.Batch(pairs), "sr", dict(sam=True))
