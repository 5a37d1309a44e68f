"""The block index of raw streams (csrc/snapmi_blockindex.hpp) in a few lines
of Python, and the index a compressed stream must come with, from the oracle:
the tests of the indexed batch calls compare against these."""
BLOCK = 65536


def varint(n):
    out = bytearray()
    while n >= 0x80:
        out.append((n & 0x7F) | 0x80)
        n >>= 7
    out.append(n)
    return bytes(out)


def entries(length):
    return -(-length // BLOCK) + 1


def header(stream):
    """(bytes of the varint, its value) or (0, 0) when there is none."""
    v = 0
    for k, b in enumerate(stream[:10]):
        v |= (b & 0x7F) << (7 * k)
        if b < 0x80:
            v &= (1 << 64) - 1
            return (k + 1, v) if v <= 0xFFFFFFFF else (0, 0)
    return 0, 0


def indexed(stream, cap, index, first, nxt, index_entries):
    """The rule: is `stream`, which owns index[first:nxt], indexed?"""
    if nxt > index_entries or first > nxt or nxt - first < 3:
        return False
    e = index[first:nxt]
    hdr, dlen = header(stream)
    return (hdr != 0 and dlen <= cap and len(e) == entries(dlen)
            and e[0] == hdr and e[-1] == len(stream)
            and all(a < b for a, b in zip(e, e[1:])))


def piece(e, dlen, k):
    """(in_off, in_len, out_off, out_len) of piece k."""
    return (e[k], e[k + 1] - e[k], k * BLOCK,
            min((k + 1) * BLOCK, dlen) - k * BLOCK)


def block_streams(data):
    """The oracle's stream of every 64 KiB block of data, without its own
    varint."""
    import oracle_lib as O
    out = []
    for k in range(0, len(data), BLOCK):
        blk = data[k:k + BLOCK]
        out.append(O.compress(blk)[len(varint(len(blk))):])
    return out


def expected_index(data):
    """The entries of the compressed stream of `data`: the varint's length,
    then the running sum of the blocks' compressed lengths (an empty input:
    the one entry 1)."""
    e = [len(varint(len(data)))]
    for b in block_streams(data):
        e.append(e[-1] + len(b))
    return e
