"""Large raw streams for the long-stream decoder's tests, built without
compressing gigabytes.

The reference compresses every 64 KiB block of its input on its own
(src/compress.rs:99-127), so a stream is its header followed by the
compressed bodies of its blocks:

    varint(total) + body[b0] + body[b1] + ... == O.compress(blk[b0] + blk[b1] + ...)

A Pool compresses each of its blocks once.  A Stream is an index array into
the pool, chosen by a seeded RNG so that no two neighbours are the same
block, and an optional partial last block (the tail: dlen % 65536 != 0).
Every pool block and every tail carries a unique 8-byte stamp, so output
that lands one piece off, or in another stream, differs from what is
expected.  The expected output is the pool plus the index array: a GPU test
rebuilds it on the device slice by slice instead of holding gigabytes on
the host.

Block kinds: text from tests/golden/corpus; incompressible bytes (one 64 KiB
literal, so chains run through literal bytes across segment and
super-segment boundaries); zeros and short runs (dense small copies: the
most hops per segment); noise of 2-4 symbols.

tests/test_long_streams_cpu.py checks the construction against O.compress
and that every shape below reaches the plan geometry it is there for;
tests/test_gpu_long_streams.py decodes them.
"""
import random
import struct

import numpy as np

import foreign
import oracle_lib as O

BLOCK = 1 << 16
KINDS = ("text", "random", "zeros", "runs", "noise")
MIB = 1 << 20

_TEXT = None


def corpus_text():
    """Every text-like corpus file, concatenated (no jpeg, no pdf)."""
    global _TEXT
    if _TEXT is None:
        names = ["alice29.txt", "asyoulik.txt", "lcet10.txt", "plrabn12.txt",
                 "html", "urls.10K", "geo.protodata", "kppkn.gtb",
                 "Mark.Twain-Tom.Sawyer.txt"]
        _TEXT = np.frombuffer(b"".join((O.CORPUS / n).read_bytes()
                                       for n in names), dtype=np.uint8)
    return _TEXT


def make_block(kind, rng, n=BLOCK):
    """n bytes of one kind (uint8 array), not yet stamped."""
    if kind == "text":
        t = corpus_text()
        o = int(rng.integers(0, len(t) - n + 1))
        return t[o:o + n].copy()
    if kind == "random":
        return rng.integers(0, 256, n, dtype=np.uint8)
    if kind == "zeros":
        return np.zeros(n, dtype=np.uint8)
    if kind == "runs":
        vals = rng.integers(0, 256, n // 4 + 1, dtype=np.uint8)
        lens = rng.integers(4, 13, n // 4 + 1)
        return np.repeat(vals, lens)[:n].copy()
    if kind == "noise":
        sym = rng.integers(0, 256, int(rng.integers(2, 5)), dtype=np.uint8)
        return rng.choice(sym, n)
    raise ValueError(kind)


def stamp(blk, value):
    """A unique 8-byte counter at the front (or all of a shorter block)."""
    s = np.frombuffer(struct.pack("<Q", value), dtype=np.uint8)
    k = min(8, len(blk))
    blk[:k] = s[:k]
    return blk


def body(raw):
    """O.compress(raw) without its header."""
    c = O.compress(bytes(raw))
    return c[len(foreign.varint(len(raw))):]


class Pool:
    """counts[kind] distinct 64 KiB blocks: raw[P, 65536] and their bodies."""

    def __init__(self, counts, seed, stamp0=1 << 48):
        rng = np.random.default_rng(seed)
        self.kinds = [k for k in KINDS for _ in range(counts.get(k, 0))]
        self.raw = np.empty((len(self.kinds), BLOCK), dtype=np.uint8)
        self.bodies = []
        for i, k in enumerate(self.kinds):
            self.raw[i] = stamp(make_block(k, rng), stamp0 + i)
            self.bodies.append(body(self.raw[i]))
        self.blen = np.array([len(b) for b in self.bodies], dtype=np.int64)
        self.of_kind = {k: np.array([i for i, x in enumerate(self.kinds)
                                     if x == k], dtype=np.int64)
                        for k in KINDS}
        self._tails = stamp0 + (1 << 40)

    def order(self, rng, n, weights):
        """n block indices, kinds drawn by weights {kind: w}, no two
        neighbours the same block."""
        ks = [k for k in KINDS if weights.get(k, 0) > 0]
        w = np.array([weights[k] for k in ks], dtype=np.float64)
        kind = rng.choice(len(ks), n, p=w / w.sum())
        idx = np.empty(n, dtype=np.int64)
        for j, k in enumerate(ks):
            m = kind == j
            idx[m] = rng.choice(self.of_kind[k], int(m.sum()))
        while True:
            same = np.flatnonzero(idx[1:] == idx[:-1]) + 1
            if not same.size:
                return idx
            for j, k in enumerate(ks):
                m = same[kind[same] == j]
                idx[m] = rng.choice(self.of_kind[k], m.size)

    def tail(self, kind, n, rng):
        """A partial block of n bytes with a stamp of its own."""
        self._tails += 1
        return stamp(make_block(kind, rng, n), self._tails)

    def stream(self, idx, tail=None):
        return Stream(self, idx, tail)


class Stream:
    """varint(dlen) + pool bodies[idx] + the tail's body."""

    def __init__(self, pool, idx, tail=None):
        self.pool = pool
        self.idx = np.asarray(idx, dtype=np.int64)
        self.tail = (np.zeros(0, dtype=np.uint8) if tail is None
                     else np.asarray(tail, dtype=np.uint8))
        self.tail_body = body(self.tail) if len(self.tail) else b""
        self.dlen = len(self.idx) * BLOCK + len(self.tail)
        self.header = foreign.varint(self.dlen)
        self.in_len = (len(self.header) + int(pool.blen[self.idx].sum()) +
                       len(self.tail_body))

    def bytes(self, header=None):
        b = self.pool.bodies
        return b"".join([self.header if header is None else header] +
                        [b[i] for i in self.idx] + [self.tail_body])

    def expected(self):
        """The output on the host (small streams only)."""
        return self.pool.raw[self.idx].tobytes() + self.tail.tobytes()

    def block_offset(self, k):
        """Compressed offset of block k's body."""
        return (len(self.header) +
                int(self.pool.blen[self.idx[:k]].sum()))


def prefix_blocks(pool, idx, target):
    """The fewest leading blocks of idx whose bodies reach `target` bytes."""
    c = np.cumsum(pool.blen[idx])
    k = int(np.searchsorted(c, target)) + 1
    assert k <= len(idx), "order too short for the target"
    return k


# ---------------------------------------------------------------------
# the shapes of tests/test_gpu_long_streams.py
# ---------------------------------------------------------------------
POOL_COUNTS = {"text": 96, "random": 24, "zeros": 24, "runs": 48,
               "noise": 32}
MIX = {"text": 4, "random": 1, "zeros": 2, "runs": 2, "noise": 2}
# the format's limits: mostly runs and text, input just above 1 GiB
LIMIT_MIX = {"text": 7, "random": 1, "zeros": 11, "runs": 1}

_POOL = None


def pool():
    global _POOL
    if _POOL is None:
        _POOL = Pool(POOL_COUNTS, seed=20261016)
    return _POOL


# Lone streams (snapmi_decompress_stream): name -> (compressed bytes, the
# forced (seg_log2, scan_segs) or None for the library's own choice).  The
# geometry each reaches is pinned by test_long_streams_cpu.py.
LADDER = {
    "scan8": (6 * MIB, None),          # 1 KiB, scan 8, nsuper3 2
    "scan16": (20 * MIB, None),        # 1 KiB, scan 16
    "scan32": (40 * MIB, None),        # 1 KiB, scan 32
    "under256": (250 * MIB, None),     # 1 KiB, scan 64, nsuper3 63
    "over256": (262 * MIB, None),      # 4 KiB by size, nsuper3 17
    "4k-small": (40 * MIB, (12, 0)),   # 4 KiB, scan 8, nsuper3 3
    "spread3x2": (300 * MIB, (10, 0)),  # 1 KiB, nsuper3 75: two spread3 wgs
}
_LADDER_ORDER = None


def ladder(name):
    """Ladder shape `name`: a prefix of one order of the pool, with a tail."""
    global _LADDER_ORDER
    p = pool()
    if _LADDER_ORDER is None:
        _LADDER_ORDER = p.order(np.random.default_rng(1), 40000, MIX)
    target, _ = LADDER[name]
    k = prefix_blocks(p, _LADDER_ORDER, target)
    rng = np.random.default_rng(k)
    return p.stream(_LADDER_ORDER[:k],
                    p.tail("text", int(rng.integers(1, BLOCK)), rng))


LIMIT_BLOCKS = (1 << 16) - 1
_LIMIT_ORDER = None


def limit(tail):
    """dlen = 2^32 - 65536 (65535 pieces, tail False) or 2^32 - 1 (a
    65535-byte tail)."""
    global _LIMIT_ORDER
    p = pool()
    if _LIMIT_ORDER is None:
        _LIMIT_ORDER = p.order(np.random.default_rng(2), LIMIT_BLOCKS,
                               LIMIT_MIX)
    rng = np.random.default_rng(3)
    return p.stream(_LIMIT_ORDER,
                    p.tail("text", BLOCK - 1, rng) if tail else None)


def mixed(seed, nblocks, weights=MIX, tail_len=None, tail_kind="text"):
    """A stream of nblocks pool blocks (and a tail of tail_len bytes)."""
    p = pool()
    rng = np.random.default_rng(seed)
    idx = p.order(rng, nblocks, weights) if nblocks else []
    t = p.tail(tail_kind, tail_len, rng) if tail_len else None
    return p.stream(idx, t)


def long_stream_rule(in_len, dlen, min_len=32 << 10):
    """long_stream_rule of csrc/snapmi_streamplan.hpp
    (test_streamplan_cpu.py holds the two against each other)."""
    sane = dlen // 22 <= in_len and 2 * dlen >= 3 * BLOCK
    return sane and in_len >= min_len and (2 * dlen >= 3 * in_len or
                                           in_len >= (256 << 10))


def batch_long(seed, count, lo=33 << 10, hi=80 << 10):
    """`count` long streams (long_stream_rule) of lo..hi compressed bytes:
    1-4 blocks of mixed kinds and a tail of a random kind and length, each
    stream distinct by its tail's stamp."""
    p = pool()
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < count:
        nb = int(rng.integers(1, 5))
        idx = p.order(rng, nb, MIX)
        base = int(p.blen[idx].sum())
        if base + 8 > hi:
            continue
        tk = KINDS[int(rng.integers(0, len(KINDS)))]
        tl = int(rng.integers(1, BLOCK))
        st = p.stream(idx, p.tail(tk, tl, rng))
        if lo <= st.in_len <= hi and long_stream_rule(st.in_len, st.dlen):
            out.append(st)
    return out


def exact_long(seed, count, in_len=32 << 10):
    """`count` long streams of exactly in_len compressed bytes (the rule's
    minimum by default): two blocks of zeros and an incompressible
    tail whose length sets the size."""
    p = pool()
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < count:
        idx = p.order(rng, 2, {"zeros": 1})
        base = len(foreign.varint(2 * BLOCK + 1)) + int(p.blen[idx].sum())
        n = in_len - base - 3   # a literal of 257..65536 bytes: 3 header bytes
        assert 256 < n <= BLOCK
        st = p.stream(idx, p.tail("random", n, rng))
        if st.in_len != in_len:   # (the encoder found a match in the noise)
            continue
        assert long_stream_rule(st.in_len, st.dlen)
        out.append(st)
    return out


def short_streams(seed, count):
    """(stream, data) pairs under the long-stream rule: text of 0 .. 20 000
    bytes, stamped."""
    rng = np.random.default_rng(seed)
    t = corpus_text()
    out = []
    for i in range(count):
        n = int(rng.choice([0, 1, 7, 60, 300, 1500, 5000,
                            int(rng.integers(1, 20000))]))
        o = int(rng.integers(0, len(t) - n))
        d = bytes(stamp(t[o:o + n].copy(), (1 << 56) + seed * 100000 + i))
        out.append((O.compress(d), d))
    return out


# ---------------------------------------------------------------------
# foreign streams: copy-4 elements and literals of a MiB and more
# ---------------------------------------------------------------------
def foreign_long(seed, lit_lens=(1 << 20, (1 << 20) + 12345, (1 << 24) + 7)):
    """(stream, expected) of literals of lit_lens bytes (3 and 4 length
    bytes) with copy-4 elements behind each that reach back across pieces,
    and copy-2 runs between: no encoder here writes any of it, and the
    pieces of such a stream are not independent."""
    rng = random.Random(seed)
    nrng = np.random.default_rng(seed)
    body_, out = bytearray(), bytearray()
    for n in lit_lens:
        data = nrng.integers(0, 256, n, dtype=np.uint8).tobytes()
        body_ += foreign.lit(data, 4 if n > (1 << 24) else None)
        out += data
        for _ in range(300):
            length = rng.randrange(1, 65)
            off = rng.choice([rng.randrange(1, 65),
                              rng.randrange(65536, len(out) + 1)])
            body_ += foreign.copy(off, length, 4)
            for _ in range(length):
                out.append(out[-off])
        for _ in range(200):
            length = rng.randrange(1, 65)
            off = rng.randrange(1, 65536)
            body_ += foreign.copy(off, length, 2)
            for _ in range(length):
                out.append(out[-off])
    return foreign.varint(len(out)) + bytes(body_), bytes(out)


# ---------------------------------------------------------------------
# batches of tests/test_gpu_long_streams.py: (Stream or bytes, cap) items
# ---------------------------------------------------------------------
def _items(streams, shorts, seed):
    items = [(s, s.dlen) for s in streams] + [(c, len(d)) for c, d in shorts]
    random.Random(seed).shuffle(items)
    return items


def _natural(seed, target):
    """Long streams of a few MiB whose compressed bytes total `target`
    (within a block and a tail)."""
    rng = np.random.default_rng(seed)
    out, total = [], 0
    while total < target - 40 * MIB:
        st = mixed(seed * 1000 + len(out), int(rng.integers(40, 200)),
                   tail_len=int(rng.integers(1, BLOCK)))
        out.append(st)
        total += st.in_len
    p = pool()
    idx = p.order(rng, 4000, MIX)
    k = prefix_blocks(p, idx, target - total - 8)
    out.append(p.stream(idx[:k]))
    return out


_BATCHES = {}


def batch_items(name):
    """The batch `name`: a list of (Stream or stream bytes, output cap)."""
    if name in _BATCHES:
        return _BATCHES[name]
    if name in ("long4096", "long4097"):
        # exactly kBatchLongMaxL long streams (the pieces path), and one more
        # (k_long_plan's list overflows: a wavefront per stream)
        items = _items(batch_long(11, 4096 if name == "long4096" else 4097),
                       short_streams(12, 1500), 1)
    elif name in ("n16384", "n16385"):
        # kBatchLongMaxN streams (the last batch that looks for long ones)
        # and one more
        n = 16384 if name == "n16384" else 16385
        items = _items(batch_long(13, 300), short_streams(14, n - 300), 2)
    elif name == "mixed":
        # at forced 1 KiB segments: a stream of more than 64 level-3 blocks,
        # a thousand long streams of the rule's minimum size, corrupt and
        # truncated long streams, long streams whose buffer is a byte short
        streams = [ladder("spread3x2")] + exact_long(15, 1000)
        bad = []
        for j, st in enumerate(batch_long(16, 24)):
            comp, cap = mutate(st, ["last_block", "two_blocks", "cut",
                                    "hdr+1", "hdr-1", "hdr+65536"][j % 6])
            if j % 4 == 3:
                comp = comp[:len(comp) // 2]
            bad.append((comp, cap))
        items = _items(streams, short_streams(18, 200), 3)
        items += bad
        items += [(st, st.dlen - 1) for st in batch_long(17, 6)]
        random.Random(4).shuffle(items)
    elif name in ("under256", "over256"):
        # no forced geometry: long bytes just under / over 256 MiB
        target = (256 * MIB - 2 * MIB if name == "under256"
                  else 256 * MIB + MIB)
        items = _items(_natural(5 if name == "under256" else 6, target),
                       short_streams(19, 300), 5)
    else:
        raise KeyError(name)
    _BATCHES[name] = items
    return items


# ---------------------------------------------------------------------
# errors at scale: mutations of valid streams
# ---------------------------------------------------------------------
def copy_elements(b):
    """Positions of the copy elements of a body (a stream without header)."""
    p, out = 0, []
    while p < len(b):
        tag = b[p]
        if tag & 3 == 0:
            n6 = tag >> 2
            if n6 >= 60:
                nb = n6 - 59
                n = int.from_bytes(b[p + 1:p + 1 + nb], "little") + 1
                p += 1 + nb + n
            else:
                p += 2 + n6
        else:
            out.append(p)
            p += 1 + {1: 1, 2: 2, 3: 4}[tag & 3]
    return out


def _zero_offset(comp, st, k, last=True):
    """Sets the offset of a copy in block k's body (the tail for k ==
    len(st.idx)) to 0: Offset(0, d) there."""
    b = (st.tail_body if k == len(st.idx)
         else st.pool.bodies[st.idx[k]])
    cps = copy_elements(b)
    assert cps, "a block without copies"
    p = st.block_offset(k) + cps[-1 if last else len(cps) // 2]
    nb = {1: 1, 2: 2, 3: 4}[comp[p] & 3]
    if comp[p] & 3 == 1:
        comp[p] &= 0x1F
    comp[p + 1:p + 1 + nb] = bytes(nb)


def _with_copies(st, ks):
    for k in ks:
        if st.pool.kinds[st.idx[k]] != "random":
            return k
    raise AssertionError("no block with copies")


def mutate(st, name):
    """(stream bytes, cap) of error case `name` made from stream st."""
    comp = bytearray(st.bytes())
    cap = st.dlen
    if name == "last_block":        # in the last block (the tail if any)
        _zero_offset(comp, st, len(st.idx) if len(st.tail) else
                     _with_copies(st, range(len(st.idx) - 1, -1, -1)))
    elif name == "two_blocks":      # one early, one late: the first wins
        n = len(st.idx)
        _zero_offset(comp, st, _with_copies(st, range(n - 2, -1, -1)))
        _zero_offset(comp, st, _with_copies(st, range(0, n)), last=False)
    elif name.startswith("hdr"):    # the header announces +-1, +-65536
        cap = st.dlen + int(name[3:])
        comp = bytearray(foreign.varint(cap)) + comp[len(st.header):]
    elif name == "cut":             # the last element cut short
        comp = comp[:-1]
    else:
        raise KeyError(name)
    return bytes(comp), cap


ERROR_CASES = ["last_block", "two_blocks", "hdr+1", "hdr-1", "hdr+65536",
               "hdr-65536", "cut", "beyond2g"]
BEYOND = (1 << 15) + 22          # the corrupt block of beyond2g: > 2 GiB in


def error_case(name, materialize=True):
    """(stream bytes or None, cap, output offset of the corrupt block or
    of the stream's end) of error case `name`: 128 MiB of output, or for
    beyond2g a stream of runs whose corrupt block starts past 2^31."""
    if name == "beyond2g":
        p = pool()
        rng = np.random.default_rng(31)
        idx = p.order(rng, BEYOND + 20, {"zeros": 1})
        idx[BEYOND] = p.of_kind["text"][0]
        st = p.stream(idx)
        if not materialize:
            return None, st.dlen, BEYOND * BLOCK
        comp = bytearray(st.bytes())
        _zero_offset(comp, st, BEYOND)
        return bytes(comp), st.dlen, BEYOND * BLOCK
    st = mixed(30, 2048, tail_len=5000)
    if not materialize:
        return None, st.dlen, st.dlen
    comp, cap = mutate(st, name)
    return comp, cap, st.dlen
