"""The append rules of csrc/snapmi_blockindex.hpp (bi_append_*) in a few lines
of Python - the host's checks, the layout of the new index, the tail and the
new blocks, the splice - and what snapmi_append_indexed must answer, from the
oracle: the CPU test compares the header against these, the GPU tests the
call."""
import blockindex_ref as B
import rangeindex_ref as R

BLOCK = B.BLOCK
U64 = 1 << 64
LIMIT = (1 << 31) - 1
E_ARGUMENT, BUFFER_TOO_SMALL, TOO_BIG = 101, 2, 1
MAX_INPUT = 0xFFFFFFFF
OK = (0, 0, 0, 0)
WRAPS, TOO_MANY = 1, 2
SLOT, ROOM = 76496, BLOCK           # scratch per new block / tail
FLOOR = SLOT + ROOM                 # of "write_scratch_bytes"

# the old lengths and the appends of the tests: around a block's end on
# either side, no tail (0, 65536, 131072), more than one new block
OLD_LENS = [0, 1, 127, 65535, 65536, 65537, 131072, 200000]
APPENDS = [0, 1, 2, 65535, 65536, 65537, 200000]


def entries(dlen, add):
    return B.entries(dlen + add)


def full(dlen):
    return dlen // BLOCK


def tail(dlen):
    return dlen % BLOCK


def fill(dlen, add):
    return min(add, BLOCK - tail(dlen)) if tail(dlen) else 0


def blocks(dlen, add):
    return -(-(dlen + add) // BLOCK) - full(dlen) if add else 0


def block(dlen, add, j):
    """New block j: (room, off, len, in_len) - source bytes [off, off + len)
    go into it; room: behind the tail, the compressor reads in_len bytes."""
    if tail(dlen) and j == 0:
        return (True, 0, fill(dlen, add), tail(dlen) + fill(dlen, add))
    off = fill(dlen, add) + (j - 1 if tail(dlen) else j) * BLOCK
    ln = min(add - off, BLOCK)
    return (False, off, ln, ln)


def check(out_lens, app_lens, index_entries):
    """(code, bad stream, new entries, new blocks) of the host's lists."""
    e = b = 0
    for i, (d, a) in enumerate(zip(out_lens, app_lens)):
        if d + a >= U64:
            return WRAPS, i, 0, 0
        e = min(e + entries(d, a), U64 - 1)
        b = min(b + blocks(d, a), U64 - 1)
    if len(out_lens) + index_entries + e + b > LIMIT:
        return TOO_MANY, 0, e, b
    return 0, 0, e, b


def new_first(out_lens, app_lens):
    out = [0]
    for d, a in zip(out_lens, app_lens):
        out.append(out[-1] + entries(d, a))
    return out


def splice(e, kf, nsize, hdr_new):
    """The new entries of a stream with old entries e whose kf full blocks
    are kept and whose new blocks compress to nsize."""
    out = [hdr_new]
    for k in range(kf):
        out.append(out[-1] + e[k + 1] - e[k])
    for z in nsize:
        out.append(out[-1] + z)
    return out


def groups(old_lens, app_lens, scratch_bytes):
    """The groups of named streams (lists of stream numbers) whose slots and
    rooms fit the scratch."""
    out, cur, used = [], [], 0
    for s, (d, a) in enumerate(zip(old_lens, app_lens)):
        if not a:
            continue
        need = blocks(d, a) * SLOT + (ROOM if tail(d) else 0)
        if cur and used + need > scratch_bytes:
            out.append(cur)
            cur, used = [], 0
        cur.append(s)
        used += need
    if cur:
        out.append(cur)
    return out


def counters(old_lens, appends, res):
    """Info "append_blocks", "append_blocks_decoded", "append_streams_ok",
    "append_streams_failed" of a call."""
    named = [s for s, b in enumerate(appends) if len(b)]
    failed = sum(1 for s in named if res[s][0] is None)
    return (sum(blocks(old_lens[s], len(appends[s])) for s in named),
            sum(1 for s in named if tail(old_lens[s])),
            len(named) - failed, failed)


def expect(streams, index, first, old_lens, appends, caps, compress,
           decode_piece, header_error):
    """What snapmi_append_indexed answers: per stream (new stream bytes or
    None, new entries, (kind, a, b, c)) - None with OK for a stream nobody
    names - and the new first[] and the new flat index.  streams: compressed
    bytes; index / first: the flat index and first[] as lists; old_lens: the
    host's copy of what the headers announce; appends[i]: the bytes appended
    to stream i (empty: not named); caps[i]: the output capacity;
    compress(bytes): the oracle; decode_piece(stream bytes, room) -> (bytes
    or None, error tuple): the oracle on varint(room) || piece;
    header_error(stream) -> error tuple or None."""
    total = len(index)
    nf = new_first(old_lens, [len(b) for b in appends])
    res, new_index = [], []
    for s, st in enumerate(streams):
        cnt = nf[s + 1] - nf[s]
        add = appends[s]
        if not add:
            f0, f1 = first[s], first[s + 1]
            keep = f0 <= f1 <= total and f1 - f0 == cnt
            ne = list(index[f0:f1]) if keep else [0] * cnt
            new_index += ne
            res.append((None, ne, OK))
            continue
        hdr, dlen = 0, 0
        err = None
        if len(st):
            err = header_error(st)
            if err is None:
                hdr, dlen = B.header(st)
        if err is None and dlen != old_lens[s]:
            err = (E_ARGUMENT, s, dlen, old_lens[s])
        if err is None and dlen + len(add) > MAX_INPUT:
            err = (TOO_BIG, dlen + len(add), MAX_INPUT, 0)
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
        body = []
        if err is None:
            kf = full(dlen)
            for j in range(blocks(dlen, len(add))):
                room, off, ln, in_len = block(dlen, len(add), j)
                blk = b""
                if room:
                    blk, perr = decode_piece(
                        B.varint(tail(dlen)) + st[e[kf]:e[kf + 1]], tail(dlen))
                    if blk is None:
                        err = perr
                        break
                blk += add[off:off + ln]
                assert len(blk) == in_len
                body.append(compress(blk)[len(B.varint(in_len)):])
        if err is None:
            ne = splice(e, kf, [len(z) for z in body],
                        len(B.varint(dlen + len(add))))
            assert len(ne) == cnt
            if ne[-1] > caps[s]:
                err = (BUFFER_TOO_SMALL, caps[s], ne[-1], 0)
        if err is not None:
            new_index += [0] * cnt
            res.append((None, [0] * cnt, err))
            continue
        out = B.varint(dlen + len(add)) + st[e[0]:e[kf]] + b"".join(body)
        assert len(out) == ne[-1]
        new_index += ne
        res.append((out, ne, OK))
    assert len(new_index) == nf[-1]
    return res, nf, new_index


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


def text(n, at=0):
    """n bytes of corpus text from offset `at`."""
    import oracle_lib as O
    data = (O.CORPUS / "alice29.txt").read_bytes()
    data = data * (-(-(at + n) // len(data)) + 1)
    return data[at:at + n]


class Case:
    """The streams of the append tests: text cut to every length of OLD_LENS,
    with the oracle's streams and index of them."""

    def __init__(self, lens=OLD_LENS):
        import oracle_lib as O
        self.inputs = [text(n, 1000 * i) for i, n in enumerate(lens)]
        self.old_lens = list(lens)
        self.comps = [O.compress(d) for d in self.inputs]
        self.index = [B.expected_index(d) for d in self.inputs]
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
