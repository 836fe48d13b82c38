"""A reader of minimap2's index file format (.mmi, magic MMI\\2), for tests: splits a file into its parts and a part into header, names,
per-bucket n / p / size / pairs, and the packed sequence S.  The layout of one part:

    "MMI\\2" | w k b n_seq flag (5 x u32) | n_seq x (l:u8, name[l], len:u32) | 2^b x (n:u32, p[n]:u64, size:u32, size x (key:u64, value:u64)) | S[(sum_len+7)/8]:u32

S is absent when flag & 2 (MM_I_NO_SEQ).  key = hash >> b << 1 | single; value = the position of a single occurrence, start_p << 32 | count
otherwise.  Everything is little endian; the 8-byte items are not aligned."""
import numpy as np

MAGIC = b"MMI\2"
NO_SEQ = 2


class Part(object):
    __slots__ = ("w", "k", "b", "n_seq", "flag", "names", "lens", "n", "p", "size", "keys", "vals", "S", "start", "end", "sec_start", "sec_end",
                 "bucket_off")

    @property
    def header(self):
        return (self.w, self.k, self.b, self.n_seq, self.flag)

    def sorted_pairs(self, bk):
        """bucket bk's (keys, values), by ascending key"""
        o = np.argsort(self.keys[bk], kind="stable")
        return self.keys[bk][o], self.vals[bk][o]

    def flat(self):
        """(hashes, positions) of every minimizer in the part, sorted by (hash, position): the content, whatever the order in the file"""
        hs, ps = [], []
        for bk in range(1 << self.b):
            k, v, p = self.keys[bk], self.vals[bk], self.p[bk]
            if not len(k):
                continue
            h = (k >> np.uint64(1)) << np.uint64(self.b) | np.uint64(bk)
            single = (k & np.uint64(1)) == 1
            hs.append(h[single]), ps.append(v[single])
            for hh, vv in zip(h[~single], v[~single]):
                st, cnt = int(vv) >> 32, int(vv) & 0xffffffff
                hs.append(np.full(cnt, hh, np.uint64)), ps.append(p[st:st + cnt])
        if not hs:
            return np.zeros(0, np.uint64), np.zeros(0, np.uint64)
        h, p = np.concatenate(hs), np.concatenate(ps)
        o = np.lexsort((p, h))
        return h[o], p[o]


def parse_part(buf, off=0):
    """buf: the file as bytes / a uint8 array; off: where the part starts.  Raises ValueError on a file that ends early."""
    a = np.frombuffer(buf, np.uint8) if not isinstance(buf, np.ndarray) else buf
    if a[off:off + 4].tobytes() != MAGIC:
        raise ValueError("bad magic")

    def u32(at, n=1):
        if at + 4 * n > len(a):
            raise ValueError("truncated")
        return np.frombuffer(a[at:at + 4 * n].tobytes(), "<u4")

    def u64(at, n):
        if at + 8 * n > len(a):
            raise ValueError("truncated")
        return np.frombuffer(a[at:at + 8 * n].tobytes(), "<u8")

    P = Part()
    P.start = off
    P.w, P.k, P.b, P.n_seq, P.flag = (int(x) for x in u32(off + 4, 5))
    at = off + 24
    P.names, P.lens = [], []
    for _ in range(P.n_seq):
        l = int(a[at])
        P.names.append(a[at + 1:at + 1 + l].tobytes())
        P.lens.append(int(u32(at + 1 + l)[0]))
        at += 5 + l
    P.sec_start = at
    P.n, P.p, P.size, P.keys, P.vals, P.bucket_off = [], [], [], [], [], []
    for _ in range(1 << P.b):
        P.bucket_off.append(at)
        n = int(u32(at)[0])
        P.n.append(n), P.p.append(u64(at + 4, n))
        at += 4 + 8 * n
        size = int(u32(at)[0])
        kv = u64(at + 4, 2 * size)
        P.size.append(size), P.keys.append(kv[0::2]), P.vals.append(kv[1::2])
        at += 4 + 16 * size
    P.sec_end = at
    if P.flag & NO_SEQ:
        P.S = None
    else:
        nw = (sum(P.lens) + 7) // 8
        P.S = u32(at, nw)
        at += 4 * nw
    P.end = at
    return P


def parse_file(fn):
    """every part of the file, in order"""
    buf = np.fromfile(fn, np.uint8)
    parts, off = [], 0
    while off < len(buf):
        parts.append(parse_part(buf, off))
        off = parts[-1].end
    return parts
