"""bi_build (csrc/snapmi_blockindex.hpp) in a few lines of Python - the
sequential walk that snapmi_build_block_index must reproduce on every route -
and the streams its tests share: oracle streams of the sizes where the block
count changes, and the unaligned, corrupt and missized shapes."""
import random

import blockindex_ref as B
import foreign

BLOCK = B.BLOCK
BUILT, UNALIGNED, CORRUPT, MISSIZED = 1, 2, 3, 4


def elem_step(s, p, out):
    """Hop over the element at p: (p, out) behind it, or None when it does
    not fit.  Reads the tag and a literal's length bytes only."""
    tag = s[p]
    kind = tag & 3
    if kind == 0:
        n6 = tag >> 2
        length, hd = n6 + 1, 1
        if n6 >= 60:
            nb = n6 - 59
            if p + 1 + nb > len(s):
                return None
            length = int.from_bytes(s[p + 1:p + 1 + nb], "little") + 1
            hd = 1 + nb
        if len(s) - (p + hd) < length:
            return None
        return p + hd + length, out + length
    cnb = {1: 1, 2: 2, 3: 4}[kind]
    if p + 1 + cnb > len(s):
        return None
    return p + 1 + cnb, out + (4 + ((tag >> 2) & 7) if kind == 1
                               else 1 + (tag >> 2))


def build(stream, dlen):
    """(status, entries) of `stream`, which the caller says announces dlen."""
    n = B.entries(dlen)
    zero = [0] * n
    hdr, announced = B.header(stream)
    if hdr == 0:
        return CORRUPT, zero
    if announced != dlen:
        return MISSIZED, zero
    if dlen == 0:
        return (BUILT, [hdr]) if len(stream) == hdr else (CORRUPT, zero)
    if dlen <= BLOCK:
        return BUILT, [hdr, len(stream)]
    e = [hdr] + [None] * (n - 2) + [len(stream)]
    p, out = hdr, 0
    while p < len(stream):
        if out % BLOCK == 0 and 0 < out < dlen:
            e[out // BLOCK] = p
        step = elem_step(stream, p, out)
        if step is None or step[1] > dlen:
            return CORRUPT, zero
        p, out = step
    if p != len(stream) or out != dlen:
        return CORRUPT, zero
    if None in e:
        return UNALIGNED, zero
    return BUILT, e


SIZES = [0, 1, 1000, 65535, 65536, 65537, 131072, 200000, 196608]


def inputs(text):
    """The inputs of the oracle batch: `text` (at least 200 000 bytes) cut to
    SIZES, and 70 000 random bytes - whose stream opens every block with a
    literal that has length bytes."""
    assert len(text) >= 200000
    return [text[:n] for n in SIZES] + [random.Random(1).randbytes(70000)]


def foreign_aligned():
    """Two blocks, the second opening with a copy that reaches 100 bytes back
    into the first: aligned, though its second piece cannot decode alone.
    (stream, entries)"""
    rng = random.Random(5)
    first = rng.randbytes(65536)
    rest = rng.randbytes(3000)
    body0 = foreign.lit(first)
    body1 = foreign.copy(100, 64, 2) + foreign.lit(rest)
    hdr = foreign.varint(65536 + 64 + 3000)
    stream = hdr + body0 + body1
    return stream, [len(hdr), len(hdr) + len(body0), len(stream)]


def unaligned():
    """{name: (stream, dlen)}: whole chains with an element across a multiple
    of 64 KiB."""
    rng = random.Random(7)
    out = {}
    out["one literal of 100 000"] = (
        foreign.varint(100000) + foreign.lit(rng.randbytes(100000)), 100000)
    d = 65530 + 64 + 3000
    out["copy of 64 from output 65 530"] = (
        foreign.varint(d) + foreign.lit(rng.randbytes(65530))
        + foreign.copy(100, 64, 2) + foreign.lit(rng.randbytes(3000)), d)
    d = 1000 + 140000 + 500
    out["literal of 140 000 over two boundaries"] = (
        foreign.varint(d) + foreign.lit(rng.randbytes(1000))
        + foreign.lit(rng.randbytes(140000))
        + foreign.lit(rng.randbytes(500)), d)
    return out


def corrupt(base):
    """{name: (stream, dlen the header announces / the host believes)} from
    `base`, a valid stream of two blocks and more: every one is CORRUPT."""
    hdr, dlen = B.header(base)
    body = base[hdr:]
    rng = random.Random(9)
    lit70k = foreign.lit(rng.randbytes(70000))
    out = {}
    out["cut in the middle of an element"] = (
        foreign.varint(71000) + lit70k + foreign.lit(rng.randbytes(1000))[:-10],
        71000)
    out["one trailing byte too many"] = (base + b"\x00", dlen)
    out["header announces dlen + 1"] = (B.varint(dlen + 1) + body, dlen + 1)
    out["header announces dlen - 1"] = (B.varint(dlen - 1) + body, dlen - 1)
    out["a literal whose length passes the end"] = (
        foreign.varint(100000) + lit70k
        + bytes([63 << 2]) + (2**31).to_bytes(4, "little") + rng.randbytes(50),
        100000)
    out["in_len == 0"] = (b"", 100000)
    out["an 11-byte varint"] = (b"\x80" * 10 + b"\x01" + body, dlen)
    return out
