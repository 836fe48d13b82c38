"""Helpers of tests/test_gpu_chains.py: the binding of the reference's mg_lchain_rmq, the parsers of the reference's QR / SD / CN blocks
(--print-qname --print-seeds) and of MM2AMD_CHAIN_DUMP (minimap2_amd/csrc/chain_dump.hpp), and the generators of the two repeat inputs
that tests/test_gpu_aligner.py builds inline (the same bytes, given the same generator state)."""
import ctypes as C

import numpy as np

from reflib import _libc, ref
from synth import ACGT, COMP, mutate_read


def ref_lchain_rmq(a, max_dist, max_dist_inner, bw, max_chn_skip, cap_rmq_size, min_cnt, min_sc, pen_gap, pen_skip):
    """mg_lchain_rmq (lchain.c:250) -> (u array, compacted anchors (n,2))"""
    R = ref()
    R.mg_lchain_rmq.restype = C.c_void_p
    R.mg_lchain_rmq.argtypes = [C.c_int] * 7 + [C.c_float, C.c_float, C.c_int64, C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_void_p), C.c_void_p]
    a = np.ascontiguousarray(a, dtype=np.uint64)
    n = a.shape[0]
    if n == 0:
        return np.zeros(0, np.uint64), np.zeros((0, 2), np.uint64)
    mem = _libc.malloc(a.nbytes)
    C.memmove(mem, a.ctypes.data, a.nbytes)
    n_u = C.c_int(0)
    u = C.c_void_p()
    b = R.mg_lchain_rmq(max_dist, max_dist_inner, bw, max_chn_skip, cap_rmq_size, min_cnt, min_sc, pen_gap, pen_skip, n, mem, C.byref(n_u), C.byref(u), None)
    if n_u.value == 0:
        return np.zeros(0, np.uint64), np.zeros((0, 2), np.uint64)
    uu = np.ctypeslib.as_array(C.cast(u, C.POINTER(C.c_uint64)), shape=(n_u.value,)).copy()
    na = int((uu & np.uint64(0xffffffff)).sum())
    bb = np.ctypeslib.as_array(C.cast(b, C.POINTER(C.c_uint64)), shape=(na, 2)).copy()
    _libc.free(u); _libc.free(b)
    return uu, bb


class RefRead(object):
    """one QR block of the reference: sd = [(target, target position, strand, query position, span)], cn = the chains, each a tuple of such tuples"""
    __slots__ = ("name", "sd", "cn")

    def __init__(self, name):
        self.name, self.sd, self.cn = name, [], []


def ref_chain_blocks(text):
    """the reference's stderr under --print-qname --print-seeds -> [RefRead], in the order printed (a name may occur more than once)"""
    out, cur, chain, last_j = [], None, None, None

    def close():
        if chain:
            cur.cn.append(tuple(chain))

    for l in text.split("\n"):
        f = l.split("\t")
        if f[0] == "QR":
            close()
            cur, chain, last_j = RefRead(f[1]), None, None
            out.append(cur)
        elif f[0] == "SD":
            cur.sd.append((f[1], int(f[2]), f[3], int(f[4]), int(f[5])))
        elif f[0] == "CN":
            if f[1] != last_j:
                close()
                chain, last_j = [], f[1]
            chain.append((f[2], int(f[3]), f[4], int(f[5]), int(f[6])))
    close()
    return out


class ChainBlock(object):
    """one block of MM2AMD_CHAIN_DUMP (minimap2_amd/csrc/chain_dump.hpp): inp = the sorted anchors that went in ((n, 2) uint64, None if not recorded),
    u = score << 32 | count per chain, a = the chained anchors ((n, 2) uint64)"""
    __slots__ = ("name", "qlen", "pass_no", "side", "handed_back", "params", "inp", "u", "a")

    def key(self):
        return (self.name, self.qlen, self.pass_no, self.side, self.handed_back, self.params, None if self.inp is None else self.inp.tobytes(), self.u.tobytes(), self.a.tobytes())

    def chains(self):
        """the chains as lists of (x, y) rows"""
        out, off = [], 0
        for w in self.u:
            c = int(w) & 0xffffffff
            out.append(self.a[off:off + c])
            off += c
        assert off == len(self.a)
        return out


CHAIN_PARAMS = ("gap_ref", "gap_qry", "bw", "max_chain_skip", "max_chain_iter", "min_cnt", "min_chain_score", "chn_pen_gap", "chn_pen_skip", "is_cdna", "n_seg", "rmq",
                "rmq_inner_dist", "rmq_size_cap", "bw_long", "mid_occ")


def _hex_words(field, n_words):
    w = np.array([int(t, 16) for t in field.split(" ")] if field else [], dtype=np.uint64)
    assert len(w) == n_words, (len(w), n_words)
    return w


def chain_dump_blocks(text):
    """MM2AMD_CHAIN_DUMP's text -> {read name: [ChainBlock]}; the blocks of a file come in any order (lanes, sub-batches), every block must be complete"""
    out, cur, stage = {}, None, 0
    for l in text.split("\n"):
        if not l:
            continue
        f = l.split("\t")
        if f[0] == "CH":
            assert stage == 0 and len(f) == 6 and f[4] in ("dev", "host") and f[5] in ("chained", "handed-back"), l[:200]
            cur = ChainBlock()
            cur.name, cur.qlen, cur.pass_no, cur.side, cur.handed_back = f[1], int(f[2]), int(f[3]), f[4], f[5] == "handed-back"
            stage = 1
        elif f[0] == "PR":
            assert stage == 1 and len(f) == 1 + len(CHAIN_PARAMS), l[:200]
            cur.params = tuple(float.fromhex(v) if k.startswith("chn_pen") else int(v) for k, v in zip(CHAIN_PARAMS, f[1:]))
            stage = 2
        elif f[0] == "IN":
            assert stage == 2, l[:200]
            cur.inp = None if f[1] == "-" else _hex_words(f[2], 2 * int(f[1])).reshape(-1, 2)
            stage = 3
        elif f[0] == "U":
            assert stage == 3, l[:200]
            cur.u = _hex_words(f[2], int(f[1]))
            stage = 4
        elif f[0] == "A":
            assert stage == 4, l[:200]
            cur.a = _hex_words(f[2], 2 * int(f[1])).reshape(-1, 2)
            assert int((cur.u & np.uint64(0xffffffff)).sum()) == len(cur.a)
            stage = 5
        elif f[0] == "END":
            assert stage == 5, l[:200]
            out.setdefault(cur.name, []).append(cur)
            stage = 0
        else:
            raise AssertionError("unexpected line in the chain dump: %r" % l[:200])
    assert stage == 0, "the chain dump ends inside a block"
    return out


def gen_diverged_elements(rng, n_elem=60, elem_len=1500, div=0.03):
    """a contig with n_elem diverged copies of one element between random spacers of 200-3000 bases: thousands of anchors per read,
    equal-x ties, high-occurrence seeds"""
    elem = rng.integers(0, 4, elem_len, dtype=np.uint8)
    parts = []
    for c in range(n_elem):
        e = elem.copy()
        mut = rng.random(len(e)) < div
        e[mut] = (e[mut] + rng.integers(1, 4, int(mut.sum()), dtype=np.uint8)) % 4
        parts += [rng.integers(0, 4, int(rng.integers(200, 3000)), dtype=np.uint8), e]
    return np.concatenate(parts)


def gen_tandem_array(rng, n_copies=8, elem_len=1500, div=0.01, flank=30000):
    """a contig with a tandem array of n_copies near-identical copies of one element between two random flanks"""
    elem = rng.integers(0, 4, elem_len, dtype=np.uint8)
    copies = []
    for c in range(n_copies):
        e = elem.copy()
        mut = rng.random(len(e)) < div
        e[mut] = (e[mut] + rng.integers(1, 4, int(mut.sum()), dtype=np.uint8)) % 4
        copies.append(e)
    return np.concatenate([rng.integers(0, 4, flank, dtype=np.uint8)] + copies + [rng.integers(0, 4, flank, dtype=np.uint8)])


def gen_array_reads(rng, contig, n=12, start=24000, step=500, length=16000, grow=300, err=0.03):
    """n reads across the array of gen_tandem_array, every second one from the reverse strand -> [(name, ASCII bytes)]"""
    rds = []
    for i in range(n):
        st = start + step * i
        r = mutate_read(rng, contig[st:st + length + grow * i], err)
        if i % 2:
            r = COMP[r[::-1]]
        rds.append(("arr%d" % i, ACGT[r].tobytes()))
    return rds
