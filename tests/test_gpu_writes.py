"""GPU suite: range writes of indexed raw streams
(snapmi_write_ranges_indexed).

A stream that succeeds must be, byte for byte, varint(dlen) followed per
block by the oracle's stream of the patched block or by the old bytes - for
the oracle's own streams that is O.compress(patched data) with
B.expected_index(patched data) - and a stream that fails has the error
include/snapmi.h names and a buffer nobody wrote to (writeindex_ref.expect is
that contract in Python).  The streams, the writes' sources and every output
sit between guard bands (gpu_buffers.Slab) that are checked after every call,
and the outputs are filled with the guard byte, so a byte written behind a
stream's new length shows as well."""
import ctypes as C
import random

import pytest
import torch

import blockindex_ref as B
import oracle_lib as O
import writeindex_ref as W
from gpu_buffers import GUARD, Slab, read_errs, u64

pytestmark = pytest.mark.gpu

OK = W.OK
SLACK = 37  # bytes of capacity behind the length a stream is expected to take


@pytest.fixture(scope="module", autouse=True)
def _gpu(built):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.fixture(scope="module")
def case():
    return W.Case()


class Call:
    """The device side of one call: streams, index, write sources and outputs
    in slabs.  writes: (stream, off, bytes), as the caller hands them."""

    def __init__(self, case, writes, flat=None, first=None, comps=None,
                 caps=None, seed=0):
        self.case, self.writes = case, writes
        self.comps = case.comps if comps is None else comps
        self.flat = case.flat if flat is None else flat
        self.first = case.first if first is None else first
        n = len(self.comps)
        if caps is None:
            # what the model says each stream takes, and a little more
            res, _ = self.model([1 << 40] * n)
            caps = [len(r[0]) + SLACK if r[0] is not None
                    else len(c) + 1000 for r, c in zip(res, self.comps)]
        self.caps = caps
        self.src = Slab([len(c) for c in self.comps], seed + 1, self.comps)
        self.in_lens = u64([len(c) for c in self.comps])
        self.d_first = u64(self.first)
        self.d_index = u64(self.flat + [7] * 4)  # (never read: behind it)
        self.wsrc = Slab([max(len(w[2]), 1) for w in writes] or [1], seed + 2,
                         [w[2] for w in writes])
        self.w_ptrs = [int(p) for p in self.wsrc.d_ptrs.cpu().tolist()]
        self.out = Slab(caps, seed)
        self.out_lens = torch.full((n,), -7, dtype=torch.int64, device="cuda")
        self.errs = torch.full((32 * n,), 0x77, dtype=torch.uint8,
                               device="cuda")
        self.new_index = torch.full((len(self.flat) + 4,), -7,
                                    dtype=torch.int64, device="cuda")

    def model(self, caps=None):
        return W.expect(self.comps, self.flat, self.first, self.writes,
                        self.caps if caps is None else caps, O.compress,
                        W.decode_piece, W.header_error)

    def enqueue(self, ctx):
        from rust_snappy_amd import raw
        raw.write_ranges_indexed(
            ctx, self.src.d_ptrs, self.in_lens, self.d_first, self.d_index,
            [w[0] for w in self.writes], [w[1] for w in self.writes],
            [len(w[2]) for w in self.writes], self.w_ptrs[:len(self.writes)],
            self.out.d_ptrs, self.out.d_caps, self.out_lens, self.errs,
            self.new_index, index_entries=len(self.flat))

    def untouched(self, what):
        """Nothing the call may write has been written."""
        self.out.assert_guards(what)
        assert bool((self.out.data == GUARD).all()), what
        assert set(self.out_lens.cpu().tolist()) == {-7}, what
        assert bool((self.errs == 0x77).all()), what
        assert set(self.new_index.cpu().tolist()) == {-7}, what

    def results(self, what):
        for slab in (self.out, self.src, self.wsrc):
            slab.assert_guards(what)
        for i, c in enumerate(self.comps):  # the streams are only read
            assert self.src.bytes(i, len(c)) == c, (what, i)
        for i, w in enumerate(self.writes):
            assert self.wsrc.bytes(i, len(w[2])) == w[2], (what, i)
        lens = self.out_lens.cpu().tolist()
        errs = read_errs(self.errs)
        index = [x & (2**64 - 1) for x in self.new_index.cpu().tolist()]
        return lens, errs, index

    def check(self, what, index=True):
        lens, errs, new_index = self.results(what)
        want, want_index = self.model()
        for i, (wbytes, wentries, werr) in enumerate(want):
            key = (what, i)
            print(key, lens[i], errs[i], werr)
            assert errs[i] == werr, key
            n = 0 if wbytes is None else len(wbytes)
            assert lens[i] == n, key
            assert self.out.bytes(i, n) == (wbytes or b""), key
            # exactly [0, new length) is written - nothing for a stream that
            # failed or that no write names
            rest = self.out.bytes(i, self.caps[i])[n:]
            assert rest == bytes([GUARD]) * len(rest), key
        if index:
            assert new_index[:len(self.flat)] == want_index, what
            assert new_index[len(self.flat):] == [2**64 - 7] * 4, what
        return lens, errs, new_index, want

    def counters(self, ctx, want):
        named = [w for w in self.writes if len(w[2])]
        lists = [(w[0], w[1], len(w[2])) for w in named]
        t = W.touched(lists)
        assert ctx.info("write_blocks") == len(t) == W.blocks(lists)
        assert ctx.info("write_blocks_decoded") == sum(q[3] for q in t)
        streams = {w[0] for w in named}
        failed = sum(1 for s in streams if want[s][0] is None)
        assert ctx.info("write_streams_failed") == failed
        assert ctx.info("write_streams_ok") == len(streams) - failed


def run(ctx, case, writes, what, **kw):
    c = Call(case, writes, **kw)
    torch.cuda.synchronize()  # the buffers are filled
    c.enqueue(ctx)
    ctx.synchronize()
    res = c.check(what)
    c.counters(ctx, res[3])
    return c, res


# --------------------------------------------------------------- 1. exact
@pytest.mark.parametrize("s", [1, 2, 3, 4, 5])
def test_exact_bytes_of_every_shape(ctx, case, s):
    """Every write shape the stream holds, a call each: the new stream is the
    oracle's stream of the patched data and the new entries are its index."""
    rng = random.Random(100 + s)
    data = case.inputs[s]
    shapes = W.shapes(len(data), rng)
    if len(data) >= 300:  # the old bytes again: the new stream is the old one
        shapes.append([(100, data[100:300])])
    for j, ws in enumerate(shapes):
        what = f"stream {s} shape {j} off {ws[0][0]} len {len(ws[0][1])}"
        c, (lens, errs, index, want) = run(
            ctx, case, [(s, off, b) for off, b in ws], what, seed=j)
        new = W.patched(data, ws)
        stream = O.compress(new)
        assert errs[s] == OK and lens[s] == len(stream), what
        assert c.out.bytes(s, lens[s]) == stream, what
        assert index[case.first[s]:case.first[s + 1]] == \
            B.expected_index(new), what


def test_aligned_block_is_not_decoded(ctx, case):
    blk = random.Random(7).randbytes(65536)
    run(ctx, case, [(4, 65536, blk)], "aligned block")
    assert ctx.info("write_blocks") == 1
    assert ctx.info("write_blocks_decoded") == 0
    run(ctx, case, [(4, 1000, bytes(140000))], "edge, covered, edge")
    assert ctx.info("write_blocks") == 3
    assert ctx.info("write_blocks_decoded") == 2


# --------------------------------------------------------------- 2. mixed
def mixed(case):
    rng = random.Random(22)
    d = case.inputs
    return [(1, 0, rng.randbytes(10)), (1, 500, b"x" * 100), (1, 999, b"!"),
            (3, 65530, rng.randbytes(16)), (3, 131071, b"z"),
            (4, 100, b"ab"), (4, 300, b"cd"), (4, 65535, b"ef"),
            (4, 70000, b""),                              # ignored
            (4, 131072, d[4][:68928]),                    # to the end
            (5, 0, bytes(70000)),
            (case.FOREIGN, 10, b"block 0 alone")]


def test_mixed_batch_and_reading_it_back(ctx, case):
    """Several writes into several streams; streams 0 and 2 are named by no
    write: buffer untouched, length 0, kind 0, entries copied.  Then the new
    streams with the new index through the indexed decode and the range reads
    against the patched data."""
    from rust_snappy_amd import batch
    writes = mixed(case)
    c, (lens, errs, index, want) = run(ctx, case, writes, "mixed")
    for s in (0, 2):
        assert (lens[s], errs[s]) == (0, OK)
        assert c.out.bytes(s, c.caps[s]) == bytes([GUARD]) * c.caps[s]
        assert index[case.first[s]:case.first[s + 1]] == case.index[s]
    assert all(e == OK for e in errs)
    new = [W.patched(case.whole[s], [(o, b) for t, o, b in writes if t == s])
           for s in range(case.n)]
    for s in (1, 3, 4, 5):
        assert c.out.bytes(s, lens[s]) == O.compress(new[s]), s
    # ... and through the batch wrapper: the merged streams decode to the
    # patched data, whole and by ranges
    src = batch.StreamBatch.from_bytes(case.comps, torch.device("cuda"))
    merged, new_idx, werrs = batch.write_ranges(
        ctx, src, (u64(case.first), u64(case.flat)), writes)
    assert [tuple(e) for e in werrs] == [OK] * case.n
    assert [x & (2**64 - 1) for x in new_idx[1].cpu().tolist()] == \
        index[:len(case.flat)]
    for s in range(case.n):
        assert merged.stream_bytes(s) == (
            c.out.bytes(s, lens[s]) if lens[s] else case.comps[s]), s
    # (the foreign stream's block 1 still copies from block 0: decoded whole
    # it gives what those bytes now decode to; its pieces cannot)
    dst, dlens, derrs = batch.decompress(ctx, merged, index=new_idx)
    for s in range(case.FOREIGN):
        assert derrs[s] == OK and dst.stream_bytes(s, dlens[s]) == new[s], s
    ranges = [(1, 0, 1000), (3, 65000, 2000), (3, 0, 131072),
              (4, 0, 200000), (4, 65530, 10), (4, 131000, 69000),
              (5, 69999, 1), (2, 100, 300), (case.FOREIGN, 0, 100)]
    got, rerrs = batch.read_ranges(ctx, merged, new_idx, ranges)
    assert [tuple(e) for e in rerrs] == [OK] * len(ranges)
    assert got == [new[s][o:o + n] for s, o, n in ranges]


# --------------------------------------------------------------- 3. failures
GOOD = [(1, 10, b"good"), (5, 65530, b"across the boundary")]


def corrupt_block_1(case):
    """Stream 4 with the first element of block 1 turned into a copy that
    reaches behind the start of its piece."""
    c = bytearray(case.comps[4])
    e1 = case.index[4][1]
    c[e1:e1 + 3] = b"\xfe\xff\xff"  # copy-2, 64 bytes, offset 65535
    return bytes(c)


def failing(case):
    """name -> (writes, keywords of Call, stream, its error or None)."""
    idx4, n4 = case.index[4], len(case.comps[4])
    out = {}
    out["off+len = dlen+1"] = ([(4, 199999, b"ab")], {}, 4,
                               (101, 199999, 2, 200000))
    out["the empty stream"] = ([(0, 0, b"a")], {}, 0, (101, 0, 1, 0))
    bad = list(case.comps)
    bad[3] = b"\xff" * 11 + bad[3][11:]
    out["no header"] = ([(3, 5, b"a")], dict(comps=bad), 3,
                        W.header_error(bad[3]))
    flat, first = case.with_index(4, idx4[:3] + [idx4[2]] + idx4[4:])
    out["not increasing at an untouched block"] = (
        [(4, 5, b"a")], dict(flat=flat, first=first), 4, (101, 4, 2, 0))
    flat, first = case.with_index(4, idx4[:2] + [n4 + 1000] + idx4[3:])
    out["an entry above in_len"] = (
        [(4, 5, b"a")], dict(flat=flat, first=first), 4, (101, 4, 1, 0))
    first = list(case.first)
    first[5] -= 1  # stream 4 one entry short, stream 5 one too many
    out["wrong entry count"] = (
        [(4, 5, b"a")], dict(first=first), 4, (101, 4, 0, 0))
    first = [f + len(case.flat) - 3 for f in case.first]
    out["first beyond index_entries"] = (
        [(4, 5, b"a")], dict(first=first), 4, (101, 4, 0, 0))
    bad = list(case.comps)
    bad[4] = corrupt_block_1(case)
    out["corrupt byte in a touched edge block"] = (
        [(4, 70000, b"a")], dict(comps=bad), 4, None)
    return out


FAILURES = ["off+len = dlen+1", "the empty stream", "no header",
            "not increasing at an untouched block", "an entry above in_len",
            "wrong entry count", "first beyond index_entries",
            "corrupt byte in a touched edge block"]


@pytest.mark.parametrize("name", FAILURES)
def test_failures(ctx, case, name):
    """A failed stream: exact fields, length 0, not one byte of its buffer
    written, its old entries in the new index - and the good streams beside
    it are exact."""
    cases = failing(case)
    assert sorted(cases) == sorted(FAILURES)
    ws, kw, s, err = cases[name]
    writes = sorted(GOOD + ws, key=lambda w: (w[0], w[1]))
    prefix_sum = "first" not in kw
    c = Call(case, writes, **kw)
    torch.cuda.synchronize()
    c.enqueue(ctx)
    ctx.synchronize()
    lens, errs, index, want = c.check(name, index=prefix_sum)
    c.counters(ctx, want)
    if err is None:  # the piece's error, from the oracle on varint || piece
        comp, e = c.comps[s], c.flat[case.first[s]:case.first[s + 1]]
        room = min(65536, 200000 - 65536)
        _, err = W.decode_piece(B.varint(room) + comp[e[1]:e[2]], room)
        assert err[0] not in (0, 101)
    assert (lens[s], errs[s]) == (0, err), (name, errs[s])
    if name == "first beyond index_entries":
        # every touched stream has lost its index; nothing else is promised
        assert [errs[t] for t in (1, 5)] == [(101, 1, 0, 0), (101, 5, 0, 0)]
        return
    if name == "wrong entry count":
        assert errs[5] == (101, 5, 0, 0) and errs[1] == OK
        return
    for t in (1, 5):  # the good streams beside it
        assert errs[t] == OK and lens[t] == len(want[t][0]), (name, t)
        new = W.patched(case.inputs[t],
                        [(o, b) for u, o, b in writes if u == t])
        assert c.out.bytes(t, lens[t]) == O.compress(new), (name, t)
    f0, f1 = c.first[s], c.first[s + 1]
    assert index[f0:f1] == c.flat[f0:f1], name  # its old entries


def test_cap_one_below_and_exact(ctx, case):
    writes = sorted(GOOD + [(4, 70000, random.Random(3).randbytes(3000))],
                    key=lambda w: (w[0], w[1]))
    res, _ = W.expect(case.comps, case.flat, case.first, writes,
                      [1 << 40] * case.n, O.compress, W.decode_piece,
                      W.header_error)
    need = [len(r[0]) if r[0] is not None else 64 for r in res]
    assert need[4] > len(case.comps[4])  # random bytes into text: it grows
    c, (lens, errs, _, _) = run(ctx, case, writes, "exact caps", caps=need)
    assert [errs[s] for s in (1, 4, 5)] == [OK] * 3 and lens[4] == need[4]
    short = list(need)
    short[4] -= 1
    c, (lens, errs, index, _) = run(ctx, case, writes, "cap one below",
                                    caps=short, seed=4)
    assert (lens[4], errs[4]) == (0, (2, need[4] - 1, need[4], 0))
    assert errs[1] == errs[5] == OK
    assert index[case.first[4]:case.first[5]] == case.index[4]


# --------------------------------------------------------------- 4. foreign
def test_foreign_stream(ctx, case):
    """Block 1 opens with a copy that reaches into block 0: a write into it
    fails with its piece's error; a write into block 0 alone succeeds, and
    the old bytes of block 1 follow the new block 0."""
    F = case.FOREIGN
    comp, e = case.comps[F], case.index[F]
    c, (lens, errs, _, _) = run(ctx, case, [(F, 65536 + 10, b"into block 1")],
                                "foreign block 1")
    _, perr = W.decode_piece(B.varint(3064) + comp[e[1]:e[2]], 3064)
    assert perr[0] not in (0, 101) and (lens[F], errs[F]) == (0, perr)
    new0 = W.patched(case.whole[F][:65536], [(100, b"into block 0")])
    c, (lens, errs, index, _) = run(ctx, case, [(F, 100, b"into block 0")],
                                    "foreign block 0")
    z = O.compress(new0)[3:]
    want = B.varint(68600) + z + comp[e[1]:e[2]]
    assert errs[F] == OK and c.out.bytes(F, lens[F]) == want
    assert index[case.first[F]:case.first[F + 1]] == [3, 3 + len(z),
                                                       len(want)]


# --------------------------------------------------------------- 5. refusals
def test_host_checks_enqueue_nothing(ctx, case):
    """Unsorted, overlapping, stream == n, a wrapping write and a NULL
    required pointer are SNAPMI_E_ARGUMENT before anything is enqueued: every
    output keeps its fill.  m == 0 and all-empty writes are OK and enqueue
    nothing either."""
    from rust_snappy_amd import _lib
    c = Call(case, [(4, 100, b"ab"), (4, 300, b"cd")], seed=5)
    torch.cuda.synchronize()
    L = _lib.of(ctx)
    a, b = c.w_ptrs[:2]

    def call(streams, offs, lens, srcs=(a, b), **null):
        m = len(streams)
        arg = dict(
            in_ptrs=c.src.d_ptrs.data_ptr(), in_lens=c.in_lens.data_ptr(),
            first=c.d_first.data_ptr(), index=c.d_index.data_ptr(),
            stream=(C.c_uint32 * max(m, 1))(*streams),
            off=(C.c_uint64 * max(m, 1))(*offs),
            len=(C.c_uint64 * max(m, 1))(*lens),
            src=(C.c_uint64 * max(m, 1))(*srcs[:m]),
            out_ptrs=c.out.d_ptrs.data_ptr(), out_caps=c.out.d_caps.data_ptr(),
            out_lens=c.out_lens.data_ptr(), new_index=c.new_index.data_ptr())
        arg.update(null)
        return L.snapmi_write_ranges_indexed(
            ctx._h, arg["in_ptrs"], arg["in_lens"], case.n, arg["first"],
            arg["index"], len(c.flat), arg["stream"], arg["off"], arg["len"],
            arg["src"], m, arg["out_ptrs"], arg["out_caps"], arg["out_lens"],
            c.errs.data_ptr(), arg["new_index"])

    refused = {
        "unsorted": ([4, 4], [300, 100], [2, 2]),
        "unsorted streams": ([4, 3], [100, 100], [2, 2]),
        "overlapping": ([4, 4], [100, 101], [2, 2]),
        "stream == n": ([4, case.n], [100, 0], [2, 2]),
        "off + len wraps": ([4, 4], [100, 2**64 - 1], [2, 1]),
        "m = 2^31": None,
    }
    for what, lists in refused.items():
        if lists is None:
            m = 1 << 31
            rc = L.snapmi_write_ranges_indexed(
                ctx._h, c.src.d_ptrs.data_ptr(), c.in_lens.data_ptr(), case.n,
                c.d_first.data_ptr(), c.d_index.data_ptr(), len(c.flat),
                (C.c_uint32 * 2)(4, 4), (C.c_uint64 * 2)(100, 300),
                (C.c_uint64 * 2)(2, 2), (C.c_uint64 * 2)(a, b), m,
                c.out.d_ptrs.data_ptr(), c.out.d_caps.data_ptr(),
                c.out_lens.data_ptr(), c.errs.data_ptr(),
                c.new_index.data_ptr())
        else:
            rc = call(*lists)
        assert rc == 101, what
        ctx.synchronize()
        c.untouched(what)
    for name in ("in_ptrs", "in_lens", "first", "index", "stream", "off",
                 "len", "src", "out_ptrs", "out_caps", "out_lens",
                 "new_index"):
        assert call([4, 4], [100, 300], [2, 2], **{name: None}) == 101, name
        ctx.synchronize()
        c.untouched(name + " NULL")
    # touched blocks at the limit: n + index_entries + blocks = 2^31
    blocks = (1 << 31) - case.n - len(c.flat)
    assert call([4], [0], [blocks * 65536]) == 101
    ctx.synchronize()
    c.untouched("blocks at the limit")
    # nothing to do is OK, and nothing is done: m == 0, every write empty
    # (an empty write is not looked at: its stream, offset and source may be
    # anything)
    assert call([], [], []) == 0
    assert call([99, 4], [2**64 - 1, 5], [0, 0], srcs=(0, 0)) == 0
    ctx.synchronize()
    c.untouched("nothing to do")
    assert ctx.info("write_blocks") == 0
    assert ctx.info("write_streams_ok") == ctx.info("write_streams_failed") == 0
    # ... and the context serves the call itself afterwards
    c.enqueue(ctx)
    ctx.synchronize()
    c.check("after the refusals")


# --------------------------------------------------------------- 6. scale
def test_long_stream_strides(ctx):
    """One stream of 1 100 blocks.  Writes into blocks 0, 1023, 1024 and 1099
    and one that covers blocks 300 .. 599 and cuts 299 and 600: more touched
    blocks than the 256 a stride of k_write_sizes sums, more blocks than the
    64 a stride of k_write_plan checks, more splice jobs than one wavefront
    takes."""
    pattern = bytes(range(256)) * 4
    data = pattern * (1100 * 64)
    comp = O.compress(data)
    index = B.expected_index(data)
    assert len(index) == 1101 and len(comp) < (4 << 20)
    other = bytes(reversed(pattern)) * (300 * 64 + 1)
    ws = [(5, b"first block"), (299 * 65536 + 65000, other[:536 + 300 * 65536 + 7]),
          (1023 * 65536 + 65527, b"ends 1023"),
          (1024 * 65536, b"opens 1024"), (len(data) - 3, b"end")]
    new = W.patched(data, ws)
    stream, entries = O.compress(new), B.expected_index(new)

    class One:
        comps, flat, first, n = [comp], index, [0, len(index)], 1
    writes = [(0, o, b) for o, b in ws]
    c = Call(One, writes, caps=[len(stream) + SLACK])
    torch.cuda.synchronize()
    c.enqueue(ctx)
    ctx.synchronize()
    lens, errs, got_index = c.results("1 100 blocks")
    assert errs[0] == OK and lens[0] == len(stream)
    assert c.out.bytes(0, lens[0]) == stream
    assert got_index[:1101] == entries
    rest = c.out.bytes(0, c.caps[0])[lens[0]:]
    assert rest == bytes([GUARD]) * SLACK
    t = W.touched([(0, o, len(b)) for o, b in ws])
    assert len(t) == 1 + 302 + 2 + 1 and ctx.info("write_blocks") == len(t)
    assert ctx.info("write_blocks_decoded") == sum(q[3] for q in t) == 6
    assert ctx.info("write_streams_ok") == 1


def test_more_touched_streams_than_one_stride_of_the_job_scan(ctx):
    """1 100 indexed streams of one to three blocks, a small write into each
    but stream 1 025, the write into stream 1 024 behind its end: 1 099
    touched streams in one group, so k_write_jobs walks a second stride of its
    scan, whose first stream (the group's 1 025th) failed and has no jobs."""
    text = (O.CORPUS / "alice29.txt").read_bytes() * 2
    pay = [text[:3000], text[500:500 + 70000], text[7:7 + 150000],
           random.Random(4).randbytes(70000)]
    comp = [O.compress(d) for d in pay]
    index = [B.expected_index(d) for d in pay]
    n = 1100

    class Many:
        comps = [comp[i % 4] for i in range(n)]
        flat = [e for i in range(n) for e in index[i % 4]]
        first = [0]
    for i in range(n):
        Many.first.append(Many.first[-1] + len(index[i % 4]))
    rng = random.Random(1100)
    writes = []
    for i in range(n):
        d = len(pay[i % 4])
        if i == 1024:
            writes.append((i, d + 3, b"no"))
        elif i != 1025:
            m = rng.randrange(1, 40)
            writes.append((i, rng.randrange(0, d - m), rng.randbytes(m)))
    lists = [(s, o, len(b)) for s, o, b in writes]
    assert W.groups(lists, 1 << 30) == [[i for i in range(n) if i != 1025]]
    c, (lens, errs, new_index, want) = run(ctx, Many, writes, "1 100 streams")
    d = len(pay[1024 % 4])
    assert (lens[1024], errs[1024]) == (0, (101, d + 3, 2, d))
    assert (lens[1025], errs[1025]) == (0, OK)
    assert sum(1 for e in errs if e != OK) == 1
    for i in (0, 1023, 1026, n - 1):
        new = W.patched(pay[i % 4], [(o, b) for s, o, b in writes if s == i])
        assert c.out.bytes(i, lens[i]) == O.compress(new), i
        assert new_index[Many.first[i]:Many.first[i + 1]] == \
            B.expected_index(new), i


def test_groups_at_the_floor(ctx, case):
    """The mixed batch with "write_scratch_bytes" at its floor: one group per
    touched stream (a stream that exceeds the floor alone is a group of its
    own), the same results."""
    writes = mixed(case)
    lists = [(s, o, len(b)) for s, o, b in writes]
    assert W.groups(lists, 1 << 30) == [[1, 3, 4, 5, 6]]
    assert W.groups(lists, W.FLOOR) == [[1], [3], [4], [5], [6]]
    _, plain = run(ctx, case, writes, "one group")
    ctx.set_option("write_scratch_bytes", W.FLOOR)
    try:
        _, grouped = run(ctx, case, writes, "a group per stream", seed=3)
        with pytest.raises(Exception):
            ctx.set_option("write_scratch_bytes", W.FLOOR - 1)
    finally:
        ctx.set_option("write_scratch_bytes", 1 << 30)
    assert grouped[:3] == plain[:3]


# --------------------------------------------------------------- 7. ordering
@pytest.mark.parametrize("library", ["test", "product"])
def test_enqueued_behind_compress(built, case, library):
    """compress_batch_indexed and the writes into what it is still writing,
    enqueued back to back on a fresh context: the streams, their lengths and
    the index reach the second call through device memory only; one
    synchronize at the end.  "scratch_bytes" behind the call covers its
    compress slots and rooms."""
    import rust_snappy_amd as R_
    from rust_snappy_amd import raw
    S = torch.cuda.Stream()
    lib = R_._lib.load_product() if library == "product" else None
    ctx = R_.raw.Context(0, stream=S.cuda_stream, lib=lib)
    try:
        with torch.cuda.stream(S):
            inputs = case.inputs
            n = len(inputs)
            src = Slab([max(len(d), 1) for d in inputs], 11, inputs)
            lens = torch.tensor([len(d) for d in inputs], dtype=torch.int64)
            dst = Slab([O.max_compress_len(len(d)) for d in inputs], 12)
            comp_lens = torch.full((n,), -7, dtype=torch.int64, device="cuda")
            entries = raw.block_index_entries([len(d) for d in inputs])
            first = torch.full((n + 1,), -7, dtype=torch.int64, device="cuda")
            index = torch.full((entries,), -7, dtype=torch.int64,
                               device="cuda")
            writes = [w for w in mixed(case) if w[0] != case.FOREIGN]
            wsrc = Slab([max(len(w[2]), 1) for w in writes], 13,
                        [w[2] for w in writes])
            new = [W.patched(inputs[s],
                             [(o, b) for t, o, b in writes if t == s])
                   for s in range(n)]
            want = [O.compress(d) for d in new]
            out = Slab([len(w) + SLACK for w in want], 14)
            out_lens = torch.full((n,), -7, dtype=torch.int64, device="cuda")
            errs = torch.full((32 * n,), 0x77, dtype=torch.uint8,
                              device="cuda")
            new_index = torch.full((entries,), -7, dtype=torch.int64,
                                   device="cuda")
            d_lens = lens.cuda()
            w_ptrs = [int(p) for p in wsrc.d_ptrs.cpu().tolist()]
            S.synchronize()
            before = ctx.info("scratch_bytes")
            raw.compress_batch(ctx, src.d_ptrs, d_lens, dst.d_ptrs,
                               dst.d_caps, comp_lens, None, host_in_lens=lens,
                               index_first=first, index=index,
                               index_cap=entries)
            between = ctx.info("scratch_bytes")
            raw.write_ranges_indexed(
                ctx, dst.d_ptrs, comp_lens, first, index,
                [w[0] for w in writes], [w[1] for w in writes],
                [len(w[2]) for w in writes], w_ptrs, out.d_ptrs, out.d_caps,
                out_lens, errs, new_index, index_entries=entries)
            after = ctx.info("scratch_bytes")
            ctx.synchronize()  # the one wait
            for slab in (out, dst, wsrc, src):
                slab.assert_guards("behind compress")
            got = out_lens.cpu().tolist()
            es = read_errs(errs)
            t = W.touched([(w[0], w[1], len(w[2])) for w in writes if w[2]])
            touched_streams = {q[0] for q in t}
            flat = []
            for s in range(n):
                if s in touched_streams:
                    assert (got[s], es[s]) == (len(want[s]), OK), (s, es[s])
                    assert out.bytes(s, got[s]) == want[s], s
                    flat += B.expected_index(new[s])
                else:
                    assert (got[s], es[s]) == (0, OK), s
                    flat += case.index[s]
            assert new_index.cpu().tolist() == flat
            rooms = sum(q[3] for q in t)
            assert between >= before
            assert after - between >= len(t) * W.SLOT + rooms * W.ROOM, (
                before, between, after)
            assert ctx.info("write_streams_ok") == len(touched_streams)
    finally:
        ctx.close()
