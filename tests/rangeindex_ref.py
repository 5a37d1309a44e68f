"""The range-read rules of csrc/snapmi_blockindex.hpp in a few lines of
Python (blocks a range touches, edge blocks and their rooms, the local index
rule, the span an edge block hands over), and what a range read must answer:
the CPU test compares the header against these, the GPU tests the call."""
import blockindex_ref as B

BLOCK = B.BLOCK
U64 = 1 << 64
E_ARGUMENT = 101


def blocks(off, n):
    """(count, first block) the range [off, off + n) touches; count 0 for an
    empty range and for one whose end passes 2^64."""
    k0 = off // BLOCK
    if n == 0 or off + n >= U64:
        # (off + n == 2^64 wraps to 0 in the header's arithmetic as well)
        return 0, k0
    return (off + n - 1) // BLOCK - k0 + 1, k0


def edge(off, n, k):
    """Is touched block k cut by the range?"""
    return k * BLOCK < off or (k + 1) * BLOCK > off + n


def edges(off, n):
    cnt, k0 = blocks(off, n)
    if cnt == 0:
        return 0
    if cnt == 1:
        return int(edge(off, n, k0))
    return int(edge(off, n, k0)) + int(edge(off, n, k0 + cnt - 1))


def edge_slot(off, n, k):
    k0 = off // BLOCK
    return int(k != k0 and edge(off, n, k0))


def span(off, n, k):
    """(from, to, bytes): room bytes [from, from + bytes) of touched block k
    go to byte `to` of the range's buffer."""
    lo = max(k * BLOCK, off)
    hi = min((k + 1) * BLOCK, off + n)
    return lo - k * BLOCK, lo - off, hi - lo


def pieces(offs, lens):
    return min(sum(blocks(o, n)[0] for o, n in zip(offs, lens)), U64 - 1)


def stream_usable(in_len, hdr, dlen, index, first, nxt, total):
    if nxt > total or first > nxt or nxt - first != B.entries(dlen):
        return False
    return index[first] == hdr and index[nxt - 1] == in_len


def first_bad_block(e, in_len, off, n):
    cnt, k0 = blocks(off, n)
    for k in range(k0, k0 + cnt):
        if not (e[k] < e[k + 1] <= in_len):
            return k
    return None


def room_groups(offs, lens, scratch_bytes):
    """Groups of consecutive ranges whose edge rooms fit the scratch."""
    cap = scratch_bytes // BLOCK
    out, cur, rooms = [], [], 0
    for r, (o, n) in enumerate(zip(offs, lens)):
        e = edges(o, n)
        if cur and rooms + e > cap:
            out.append(cur)
            cur, rooms = [], 0
        cur.append(r)
        rooms += e
    if cur:
        out.append(cur)
    return out


def expect(streams, index, first, ranges, decode_piece, header_error,
           whole=None):
    """What snapmi_decompress_ranges_indexed answers for `ranges` (stream,
    off, len) when the device arrays equal the host's: per range (bytes or
    None, (kind, a, b, c)).  streams: compressed bytes; index / first: the
    flat index and first[] as lists; decode_piece(stream bytes) -> (bytes or
    None, error tuple) is the oracle on varint(room) || piece;
    header_error(stream) -> error tuple or None; whole[s]: the stream's
    output when known (the slices are then checked against the pieces)."""
    total = len(index)
    out = []
    for s, off, n in ranges:
        if s >= len(streams):
            out.append((None, (E_ARGUMENT, s, len(streams), 0)))
            continue
        st = streams[s]
        hdr, dlen = (0, 0)
        if len(st):
            he = header_error(st)
            if he is not None:
                out.append((None, he))
                continue
            hdr, dlen = B.header(st)
        if off + n >= U64 or off + n > dlen:
            out.append((None, (E_ARGUMENT, off, n, dlen)))
            continue
        if n == 0:
            out.append((b"", (0, 0, 0, 0)))
            continue
        cnt, k0 = blocks(off, n)
        f0, f1 = first[s], first[s + 1]
        if not stream_usable(len(st), hdr, dlen, index, f0, f1, total):
            out.append((None, (E_ARGUMENT, s, k0, 0)))
            continue
        e = index[f0:f1]
        buf, err = bytearray(), None
        for k in range(k0, k0 + cnt):
            if not (e[k] < e[k + 1] <= len(st)):
                err = (E_ARGUMENT, s, k, 0)
                break
            in_off, in_len, out_off, out_len = B.piece(e, dlen, k)
            data, perr = decode_piece(
                B.varint(out_len) + st[in_off:in_off + in_len], out_len)
            if data is None:
                err = perr
                break
            assert len(data) == out_len
            a, _, m = span(off, n, k)
            buf += data[a:a + m]
        if err is not None:
            out.append((None, err))
            continue
        assert len(buf) == n
        if whole is not None and whole[s] is not None:
            assert bytes(buf) == whole[s][off:off + n]
        out.append((bytes(buf), (0, 0, 0, 0)))
    return out
