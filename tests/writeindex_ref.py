"""The range-write rules of csrc/snapmi_blockindex.hpp (bi_write_*) in a few
lines of Python - the host's checks, the touched blocks of a write list, the
covered / edge rule, the splice - and what snapmi_write_ranges_indexed must
answer, from the oracle: the CPU test compares the header against these, the
GPU tests the call."""
import blockindex_ref as B
import rangeindex_ref as R

BLOCK = B.BLOCK
U64 = 1 << 64
E_ARGUMENT, BUFFER_TOO_SMALL = 101, 2
OK = (0, 0, 0, 0)
WRAPS, NO_STREAM, ORDER = 1, 2, 3
SLOT, ROOM = 76496, BLOCK           # scratch per touched block / edge block
FLOOR = SLOT + ROOM                 # of "write_scratch_bytes"


def check(writes, n):
    """What is wrong with the list of (stream, off, len), and where: (0, None)
    or (WRAPS / NO_STREAM / ORDER, index of the write).  Empty writes are not
    looked at."""
    prev = None
    for w, (s, off, ln) in enumerate(writes):
        if ln == 0:
            continue
        if off + ln >= U64:
            return WRAPS, w
        if s >= n:
            return NO_STREAM, w
        if prev is not None and (s, off) < prev:
            return ORDER, w
        prev = (s, off + ln)
    return 0, None


def touched(writes):
    """The touched blocks of a checked list, in order: (stream, block, index
    of its first write, edge).  A block two writes share counts once."""
    out = []
    for w, (s, off, ln) in enumerate(writes):
        cnt, k0 = R.blocks(off, ln)
        for k in range(k0, k0 + cnt):
            if out and out[-1][:2] == (s, k):
                continue
            out.append((s, k, w, R.edge(off, ln, k)))
    return out


def blocks(writes):
    """snapmi_write_blocks of any list (the walk of bi_write_touch)."""
    total, last = 0, None
    for s, off, ln in writes:
        cnt, k0 = R.blocks(off, ln)
        if cnt == 0:
            continue
        if last == (s, k0):
            cnt -= 1
        last = (s, (off + ln - 1) // BLOCK)
        total += cnt
    return min(total, U64 - 1)


def splice(e, tk, tsize, hdr_new):
    """The new entries of a stream with old entries e whose touched blocks tk
    (ascending) compress to tsize."""
    new = dict(zip(tk, tsize))
    out = [hdr_new]
    for k in range(len(e) - 1):
        out.append(out[-1] + new.get(k, e[k + 1] - e[k]))
    return out


def groups(writes, scratch_bytes):
    """The groups of touched streams (lists of stream numbers) whose slots and
    rooms fit the scratch."""
    per = {}
    for s, _, _, edge in touched([w for w in writes if w[2]]):
        per.setdefault(s, [0, 0])
        per[s][0] += 1
        per[s][1] += int(edge)
    out, cur, used = [], [], 0
    for s in sorted(per):
        need = per[s][0] * SLOT + per[s][1] * ROOM
        if cur and used + need > scratch_bytes:
            out.append(cur)
            cur, used = [], 0
        cur.append(s)
        used += need
    if cur:
        out.append(cur)
    return out


def patched(data, writes):
    buf = bytearray(data)
    for off, b in writes:
        buf[off:off + len(b)] = b
    return bytes(buf)


def expect(streams, index, first, writes, caps, compress, decode_piece,
           header_error):
    """What snapmi_write_ranges_indexed answers: per stream (new stream bytes
    or None, new entries, (kind, a, b, c)) - None with OK for a stream no
    write names - and the new flat index.  streams: compressed bytes; index /
    first: the flat index and first[] as lists; writes: the checked list of
    (stream, off, bytes); caps[i]: the output capacity; compress(bytes): the
    oracle; decode_piece(stream bytes, room) -> (bytes or None, error tuple):
    the oracle on varint(room) || piece; header_error(stream) -> error tuple
    or None."""
    total = len(index)
    writes = [w for w in writes if len(w[2])]
    res = []
    new_index = list(index)
    for s, st in enumerate(streams):
        mine = [(off, b) for t, off, b in writes if t == s]
        if not mine:
            res.append((None, None, OK))
            continue
        hdr, dlen = 0, 0
        err = None
        if len(st):
            err = header_error(st)
            if err is None:
                hdr, dlen = B.header(st)
        if err is None:
            for off, b in mine:
                if off + len(b) > dlen:
                    err = (E_ARGUMENT, off, len(b), dlen)
                    break
        f0 = f1 = 0
        if err is None:
            f0, f1 = first[s], first[s + 1]
            if not R.stream_usable(len(st), hdr, dlen, index, f0, f1, total):
                err = (E_ARGUMENT, s, 0, 0)
        if err is None:
            e = index[f0:f1]
            for k in range(len(e) - 1):
                if not (e[k] < e[k + 1] <= len(st)):
                    err = (E_ARGUMENT, s, k, 0)
                    break
        tk, tsize, body = [], [], {}
        if err is None:
            for _, k, _, edge in touched([(s, o, len(b)) for o, b in mine]):
                in_off, in_len, out_off, out_len = B.piece(e, dlen, k)
                if edge:
                    blk, perr = decode_piece(
                        B.varint(out_len) + st[in_off:in_off + in_len],
                        out_len)
                    if blk is None:
                        err = perr
                        break
                    blk = bytearray(blk)
                else:
                    blk = bytearray(out_len)
                for off, b in mine:
                    cnt, k0 = R.blocks(off, len(b))
                    if k0 <= k < k0 + cnt:
                        a, to, m = R.span(off, len(b), k)
                        blk[a:a + m] = b[to:to + m]
                z = compress(bytes(blk))[len(B.varint(out_len)):]
                tk.append(k)
                tsize.append(len(z))
                body[k] = z
        if err is None:
            ne = splice(e, tk, tsize, len(B.varint(dlen)))
            if ne[-1] > caps[s]:
                err = (BUFFER_TOO_SMALL, caps[s], ne[-1], 0)
        if err is not None:
            res.append((None, None, err))
            continue
        out = B.varint(dlen) + b"".join(
            body[k] if k in body else st[e[k]:e[k + 1]]
            for k in range(len(e) - 1))
        assert len(out) == ne[-1]
        new_index[f0:f1] = ne
        res.append((out, ne, OK))
    return res, new_index


class Case:
    """The streams of the write tests (those of the range reads): text cut to
    0, 1 000, 65 536, 131 072 and 200 000 bytes, 70 000 random bytes, and a
    two-block foreign stream whose second block opens with a copy that
    reaches into the first."""

    def __init__(self):
        import random

        import foreign
        import oracle_lib as O
        text = (O.CORPUS / "alice29.txt").read_bytes() * 2
        self.inputs = [b"", text[:1000], text[:65536], text[1000:1000 + 131072],
                       text[:200000], random.Random(1).randbytes(70000)]
        self.comps = [O.compress(d) for d in self.inputs]
        self.index = [B.expected_index(d) for d in self.inputs]
        rng = random.Random(5)
        block0, rest = rng.randbytes(65536), rng.randbytes(3000)
        body0 = foreign.lit(block0)
        body1 = foreign.copy(100, 64, 2) + foreign.lit(rest)
        hdr = foreign.varint(65536 + 64 + 3000)
        self.comps.append(hdr + body0 + body1)
        self.index.append([len(hdr), len(hdr) + len(body0),
                           len(self.comps[-1])])
        self.FOREIGN = 6
        self.whole = [O.decompress(c) for c in self.comps]
        assert self.whole[:6] == self.inputs and len(self.whole[6]) == 68600
        self.first = [0]
        for idx in self.index:
            self.first.append(self.first[-1] + len(idx))
        self.flat = [e for idx in self.index for e in idx]
        self.n = len(self.comps)

    def with_index(self, s, idx):
        """(flat, first) with stream s's entries replaced (same count)."""
        assert len(idx) == len(self.index[s])
        flat = list(self.flat)
        flat[self.first[s]:self.first[s + 1]] = idx
        return flat, list(self.first)


def decode_piece(stream, room):
    import oracle_lib as O
    try:
        return O.decompress(stream, room), OK
    except O.SnapError as e:
        return None, (e.kind, e.a, e.b, e.c)


def header_error(stream):
    import oracle_lib as O
    try:
        O.decompress_len(stream)
        return None
    except O.SnapError as e:
        return (e.kind, e.a, e.b, e.c)


def shapes(dlen, rng):
    """The write shapes of the tests that a stream of dlen bytes holds: lists
    of (off, bytes), each list one call's writes into the stream."""
    def rnd(n):
        return rng.randbytes(n)
    out = []
    for off in (0, 65535, 65536, dlen - 1):
        if 0 <= off < dlen:
            out.append([(off, rnd(1))])
    if dlen >= 65546:
        out.append([(65530, rnd(16))])
        out.append([(100, rnd(2)), (300, rnd(2)), (65535, rnd(2))])
    if dlen >= 131072:
        out.append([(65536, rnd(65536))])
    if dlen >= 141000:
        out.append([(1000, rnd(140000))])
    if dlen:
        out.append([(0, rnd(dlen))])
        out.append([(0, bytes(min(dlen, 70000)))])           # zeros: shrinks
        out.append([(dlen // 3, rnd(min(dlen - dlen // 3, 3000)))])  # grows
    return out
