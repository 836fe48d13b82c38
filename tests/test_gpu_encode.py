"""encode_kernel behind mm2amd_encode_batch (the mapper's launch shape: a small persistent grid over the batch's 16-byte words) against a numpy
restatement of the nt4 table and its complement: every byte of both strands of every unit, and the bytes around each unit's block."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

_env_blocks = os.environ.get("MM2AMD_ENCODE_BLOCKS", "")
GRID_BLOCKS = int(_env_blocks) if _env_blocks.isdigit() and 0 < int(_env_blocks) <= 4096 else 64  # kEncodeBlocks, or what an A/B run asks for (seed_chain.hip)
BLOCK_THREADS = 256

# seq_nt4_table of the reference (sketch.c:9-26), restated: A/a 0, C/c 1, G/g 2, T/t/U/u 3, everything else 4
NT4 = np.full(256, 4, dtype=np.uint8)
for _c, _v in (("A", 0), ("C", 1), ("G", 2), ("T", 3), ("U", 3)):
    NT4[ord(_c)] = NT4[ord(_c.lower())] = _v
COMP = np.array([3, 2, 1, 0, 4], dtype=np.uint8)
ALPHABET = np.frombuffer(b"ACGTUacgtuNnRYKMSWBDHVrykmswbdhv\xc3", dtype=np.uint8)  # the full set, IUPAC letters and one byte >= 128


def _seq(rng, n, plain=False):
    if plain:
        return np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, n)].tobytes()
    return ALPHABET[rng.integers(0, ALPHABET.size, n)].tobytes()


def _units(r):
    return (r[0],) + ((r[1],) if len(r[1]) else ()) if isinstance(r, tuple) else (r,)


def _check(reads, lo=0, hi=None):
    """reads[lo:hi] encoded as a sub-batch of `reads`: their blocks hold the codes, every other byte of the pool is untouched"""
    import minimap2_amd as mm
    hi = len(reads) if hi is None else hi
    pool, unit_off = mm.encode_batch(reads, lo, hi) if (lo, hi) != (0, len(reads)) else mm.encode_batch(reads)
    units = [u for r in reads for u in _units(r)]
    assert len(unit_off) == len(units) + 1 and [int(b - a) for a, b in zip(unit_off, unit_off[1:])] == [len(u) for u in units]
    u_lo, u_hi = sum(len(_units(r)) for r in reads[:lo]), sum(len(_units(r)) for r in reads[:hi])
    want = np.full(2 * int(unit_off[-1]) + 32, 0xff, dtype=np.uint8)
    for u, o in list(zip(units, unit_off))[u_lo:u_hi]:
        f = NT4[np.frombuffer(u, dtype=np.uint8)]
        o = 16 + 2 * int(o)
        want[o:o + len(u)] = f
        want[o + len(u):o + 2 * len(u)] = COMP[f][::-1]
    assert pool.shape == want.shape
    for u, o in zip(units, unit_off):  # unit by unit first, so that a failure names the unit: both strands, and the byte on either side of the block
        lo, hi = 16 + 2 * int(o), 16 + 2 * int(o) + 2 * len(u)
        assert np.array_equal(pool[lo - 1:hi + 1], want[lo - 1:hi + 1]), (len(u), int(o), np.flatnonzero(pool[lo - 1:hi + 1] != want[lo - 1:hi + 1])[:8])
    assert np.array_equal(pool, want)  # (the guards included: nothing before the first block or after the last)


def test_every_alignment_and_every_character():
    rng = np.random.default_rng(11)
    lens = [1, 15, 16, 17, 31, 33, 255, 256, 257, 4097]
    # back to back, the starts fall at 0, 1, 16, 32, 49, 80, 113, 368, 624, 881: alignments 0, 1 and 9 of 16 only; a run of 17-base reads
    # behind them walks a start through all 16
    reads = [_seq(rng, n) for n in lens + [17] * 16]
    starts = np.cumsum([0] + [len(r) for r in reads])[:-1]
    assert set(int(s) % 16 for s in starts) == set(range(16))
    assert set(b"".join(reads)) == set(ALPHABET.tobytes())
    _check(reads)


def test_fewer_words_than_threads():
    rng = np.random.default_rng(12)
    reads = [_seq(rng, n) for n in (5, 0, 40, 3, 0, 0, 90)]  # 9 words for 16 384 lanes; empty reads in front of, between and behind the others
    assert sum(len(r) for r in reads) // 16 < GRID_BLOCKS * BLOCK_THREADS
    _check(reads)
    _check([b"", b""])


def test_more_reads_than_blocks():
    rng = np.random.default_rng(13)
    lens = rng.integers(0, 400, 100 * GRID_BLOCKS)
    lens[::97] = 0
    reads = [_seq(rng, int(n)) for n in lens]  # ~1.3 MB: more words than one pass of the grid takes (kEncodeDepth = 4 words per lane), several reads per word at places
    assert len(reads) > GRID_BLOCKS and sum(len(r) for r in reads) // 16 > 4 * GRID_BLOCKS * BLOCK_THREADS
    _check(reads)


def test_pairs():
    rng = np.random.default_rng(14)
    reads = [(_seq(rng, 150), _seq(rng, 1)), (_seq(rng, 1), _seq(rng, 149)), (_seq(rng, 100), _seq(rng, 151)), _seq(rng, 77), (_seq(rng, 33), _seq(rng, 250))]
    _check(reads)


def test_one_read():
    rng = np.random.default_rng(15)
    _check([_seq(rng, 1)])
    _check([_seq(rng, 10001)])


def test_sub_batches_that_start_anywhere():
    """A mapper lane launches the kernel on reads [lo, hi) of the batch, with the batch's offsets: the range's first word starts at any of the
    16 alignments, and the blocks' 1 KiB-aligned split begins before it."""
    rng = np.random.default_rng(16)
    reads = [_seq(rng, n) for n in [1000] + [17] * 16 + [300, 0, 5000, 33]]
    starts = np.cumsum([0] + [len(r) for r in reads])
    for lo in range(1, 18):  # the sub-batch's first byte at 1000 + 17 * (lo - 1): every alignment of 16
        _check(reads, lo, len(reads))
    assert set(int(starts[lo]) % 16 for lo in range(1, 18)) == set(range(16))
    _check(reads, 3, 5)      # ends inside a word as well, two words in all
    _check(reads, 18, 19)    # an empty range (one empty read)
    _check(reads, 7, 7)
    pairs = [(_seq(rng, 150), _seq(rng, 1)), (_seq(rng, 101), _seq(rng, 151)), _seq(rng, 77), (_seq(rng, 33), _seq(rng, 250)), (_seq(rng, 2000), _seq(rng, 1999))]
    _check(pairs, 1, 4)
    _check(pairs, 2, 5)
