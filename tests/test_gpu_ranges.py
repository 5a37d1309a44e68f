"""GPU suite: range reads of indexed raw streams
(snapmi_decompress_ranges_indexed).

Every range must give bytes [off, off + len) of the oracle's decode of the
whole stream, or fail as include/snapmi.h says (rangeindex_ref.expect is that
contract in Python; a piece's error is the oracle's on varint(room) || piece
bytes, kind and fields).  The streams and every output sit between guard
bands (gpu_buffers.Slab) that are checked after every call; a failed range's
own buffer is unspecified and not compared."""
import random

import numpy as np
import pytest
import torch

import blockindex_ref as B
import foreign
import oracle_lib as O
import rangeindex_ref as R
from gpu_buffers import Slab, read_errs, u64

pytestmark = pytest.mark.gpu

OK = (0, 0, 0, 0)
U64 = 1 << 64
FLOOR = 128 << 10


@pytest.fixture(scope="module", autouse=True)
def _gpu(built):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _foreign():
    """Two blocks; the second opens with a copy that reaches 100 bytes back
    into the first: its piece cannot decode alone."""
    rng = random.Random(5)
    first = rng.randbytes(65536)
    rest = rng.randbytes(3000)
    body0 = foreign.lit(first)
    body1 = foreign.copy(100, 64, 2) + foreign.lit(rest)
    hdr = foreign.varint(65536 + 64 + 3000)
    stream = hdr + body0 + body1
    return stream, [len(hdr), len(hdr) + len(body0), len(stream)]


class Case:
    def __init__(self):
        text = (O.CORPUS / "alice29.txt").read_bytes() * 2  # (152 089 B)
        self.inputs = [b"", text[:1000], text[:65536], text[1000:1000 + 131072],
                       text[:200000], random.Random(1).randbytes(70000)]
        self.comps = [O.compress(d) for d in self.inputs]
        self.index = [B.expected_index(d) for d in self.inputs]
        fs, fi = _foreign()
        self.comps.append(fs)
        self.index.append(fi)
        self.FOREIGN = 6
        self.whole = [O.decompress(c) for c in self.comps]
        assert self.whole[:6] == self.inputs and len(self.whole[6]) == 68600
        assert [len(d) for d in self.inputs] == [0, 1000, 65536, 131072,
                                                 200000, 70000]
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


@pytest.fixture(scope="module")
def case():
    return Case()


def decode_piece(stream, room):
    try:
        return O.decompress(stream, room), OK
    except O.SnapError as e:
        return None, (e.kind, e.a, e.b, e.c)


def header_error(stream):
    try:
        O.decompress_len(stream)
        return None
    except O.SnapError as e:
        return (e.kind, e.a, e.b, e.c)


def room_of(n):
    return n if n <= (1 << 22) else 16


class Call:
    """The device side of one call: streams, index and outputs in slabs."""

    def __init__(self, case, ranges, flat=None, first=None, dev_lens=None,
                 seed=0, comps=None):
        self.case, self.ranges = case, ranges
        self.comps = case.comps if comps is None else comps
        self.flat = case.flat if flat is None else flat
        self.first = case.first if first is None else first
        self.src = Slab([len(c) for c in self.comps], seed + 1, self.comps)
        self.in_lens = u64([len(c) for c in self.comps])
        self.d_first = u64(self.first)
        self.d_index = u64(self.flat + [7] * 4)  # (never read: behind it)
        self.offs = [r[1] for r in ranges]
        self.lens = [r[2] for r in ranges]
        dl = self.lens if dev_lens is None else dev_lens
        self.out = Slab([room_of(n) for n in dl], seed)
        self.d_stream = torch.tensor([r[0] for r in ranges],
                                     dtype=torch.int64).to(torch.int32).cuda()
        self.d_off, self.d_len = u64(self.offs), u64(dl)
        m = len(ranges)
        self.got = torch.full((m,), -7, dtype=torch.int64, device="cuda")
        self.errs = torch.full((32 * m,), 0x77, dtype=torch.uint8,
                               device="cuda")

    def enqueue(self, ctx):
        from rust_snappy_amd import raw
        raw.decompress_ranges_indexed(
            ctx, self.src.d_ptrs, self.in_lens, self.d_first, self.d_index,
            self.d_stream, self.d_off, self.d_len, self.offs, self.lens,
            self.out.d_ptrs, self.got, self.errs,
            index_entries=len(self.flat))

    def reset(self):
        self.out.refill()
        self.got.fill_(-7)
        self.errs.fill_(0x77)

    def results(self, what):
        self.out.assert_guards(what)
        self.src.assert_guards(what)
        for i, c in enumerate(self.comps):  # the streams are only read
            assert self.src.bytes(i, len(c)) == c, (what, i)
        got = self.got.cpu().numpy().tolist()
        errs = read_errs(self.errs)
        data = [self.out.bytes(r, got[r]) for r in range(len(got))]
        return got, errs, data

    def want(self):
        return R.expect(self.comps, self.flat, self.first, self.ranges,
                        decode_piece, header_error, self.case.whole
                        if self.comps is self.case.comps else None)

    def check(self, what, want=None, skip=()):
        got, errs, data = self.results(what)
        want = self.want() if want is None else want
        for r, (wbytes, werr) in enumerate(want):
            if r in skip:
                continue
            key = (what, r, self.ranges[r])
            print(key, got[r], errs[r], werr)
            assert errs[r] == werr, key
            if wbytes is None:
                assert got[r] == 0, key
            else:
                s, off, n = self.ranges[r]
                assert got[r] == n == len(wbytes), key
                assert data[r] == wbytes, key
                if self.comps is self.case.comps:
                    assert wbytes == self.case.whole[s][off:off + n], key
        return got, errs, data


def run(ctx, case, ranges, what, **kw):
    c = Call(case, ranges, **kw)
    c.enqueue(ctx)
    ctx.synchronize()
    res = c.check(what)
    from rust_snappy_amd import raw
    want = c.want()
    assert ctx.info("range_pieces") == raw.range_pieces(c.offs, c.lens)
    if "dev_lens" not in kw:
        failed = sum(1 for w in want if w[0] is None)
        assert ctx.info("range_ranges_failed") == failed
        assert ctx.info("range_ranges_ok") == len(want) - failed
    return c, res


def shapes(case):
    out = []
    for s, w in enumerate(case.whole):
        d = len(w)
        out += [(s, 0, d), (s, d, 0), (s, 0, d + 1), (s, U64 - 1, 1),
                (s, U64 - 1, 0), (s, 1, U64 - 1)]
        if d:
            out += [(s, 0, 1), (s, d - 1, 1)]
        if d >= 400:
            out += [(s, 100, 300)]
        if d >= 65537:
            out += [(s, 65535, 2)]
        if d >= 131072:
            out += [(s, 65536, 65536)]
    out += [(4, 1000, 189000), (case.n, 0, 1), (case.n, 0, 0),
            (2**32 - 1, 5, 5),
            (1, 10, 20), (1, 500, 100),            # two ranges in one block
            (case.FOREIGN, 100, 1000),             # block 0 alone: succeeds
            (case.FOREIGN, 65536, 100),            # block 1: its piece fails
            (case.FOREIGN, 65000, 1000)]
    return out


def test_every_shape(ctx, case):
    ranges = shapes(case)
    c, (got, errs, _) = run(ctx, case, ranges, "shapes")
    by = dict(zip(ranges, zip(got, errs)))
    F = case.FOREIGN
    assert by[(F, 100, 1000)] == (1000, OK)
    assert by[(F, 0, 68600)][0] == 0 and by[(F, 0, 68600)][1][0] not in (0, 101)
    assert by[(F, 65536, 100)][1] == by[(F, 0, 68600)][1]
    assert by[(4, 1000, 189000)] == (189000, OK)
    assert by[(0, 0, 0)] == (0, OK)
    assert by[(4, 0, 200001)][1] == (101, 0, 200001, 200000)
    assert by[(4, U64 - 1, 1)][1] == (101, U64 - 1, 1, 200000)
    assert by[(case.n, 0, 1)][1] == (101, case.n, case.n, 0)
    # m == 0 enqueues nothing
    from rust_snappy_amd import raw
    empty = torch.zeros(0, dtype=torch.int64, device="cuda")
    raw.decompress_ranges_indexed(
        ctx, c.src.d_ptrs, c.in_lens, c.d_first, c.d_index,
        empty.to(torch.int32), empty, empty, [], [], empty, empty, None,
        index_entries=len(c.flat))
    ctx.synchronize()


def sixty_four(case):
    rng = random.Random(64)
    ranges = []
    for _ in range(64):
        off = rng.randrange(0, 200000)
        n = rng.choice([1, 17, 4096, 65536, 70000, 131072])
        ranges.append((4, off, min(n, 200000 - off)))
    ranges[5] = (4, 65536, 65536)
    ranges[9] = (4, 0, 200000)
    rng.shuffle(ranges)
    return ranges


def test_sixty_four_ranges_and_grouping(ctx, case):
    """64 ranges of one stream in shuffled order; with the scratch at its
    floor (two rooms) the same call runs in many groups and gives the same
    bytes, lengths and errors."""
    ranges = sixty_four(case)
    offs, lens = [r[1] for r in ranges], [r[2] for r in ranges]
    assert len(R.room_groups(offs, lens, 1 << 30)) == 1
    assert len(R.room_groups(offs, lens, FLOOR)) > 20
    _, plain = run(ctx, case, ranges, "64 ranges")
    assert all(e == OK for e in plain[1])
    ctx.set_option("range_scratch_bytes", FLOOR)
    try:
        _, grouped = run(ctx, case, ranges, "64 ranges, many groups", seed=3)
        with pytest.raises(Exception):
            ctx.set_option("range_scratch_bytes", FLOOR - 1)
    finally:
        ctx.set_option("range_scratch_bytes", 1 << 30)
    assert grouped == plain


def two_thousand(case):
    """2 051 ranges over streams 1 .. 5 in shuffled order: most of a few
    hundred bytes inside one block, some across a block boundary, some a whole
    block; then one of length 0 and, at index 1 024, one that starts behind
    its stream's end."""
    rng = random.Random(2051)
    ranges = []
    for r in range(2051):
        if r % 10 == 8:    # across a boundary
            s = rng.choice([3, 4, 5])
            d = len(case.whole[s])
            b = 65536 * rng.randrange(1, (d + 65535) // 65536)
            off = b - rng.randrange(1, 300)
            ranges.append((s, off, b - off + rng.randrange(1, min(300, d - b))))
        elif r % 10 == 9:  # a whole block
            s = rng.choice([2, 3, 4])
            k = rng.randrange(len(case.whole[s]) // 65536)
            ranges.append((s, 65536 * k, 65536))
        else:
            s = rng.choice([1, 2, 3, 4, 5])
            d = len(case.whole[s])
            k = rng.randrange((d + 65535) // 65536)
            lo, hi = 65536 * k, min(65536 * (k + 1), d)
            n = rng.randrange(100, 600)
            ranges.append((s, rng.randrange(lo, hi - n), n))
    rng.shuffle(ranges)
    ranges[77] = (4, 1234, 0)
    ranges[1024] = (4, 200001, 10)
    return ranges


def test_more_ranges_than_one_workgroup_scans(ctx, case):
    """2 051 ranges in one group: k_range_scan_a / _c run on three workgroups
    (the last with three ranges), k_range_scan_b scans three pairs of totals,
    and the range that fails stands first in the second workgroup.  With the
    scratch at its floor the same call runs in a thousand groups of one
    workgroup each and gives the same bytes, lengths and errors."""
    ranges = two_thousand(case)
    offs, lens = [r[1] for r in ranges], [r[2] for r in ranges]
    assert len(R.room_groups(offs, lens, 1 << 30)) == 1
    assert len(R.room_groups(offs, lens, FLOOR)) > 500
    _, plain = run(ctx, case, ranges, "2051 ranges")
    got, errs, _ = plain
    assert errs[1024] == (101, 200001, 10, 200000) and got[1024] == 0
    assert (got[77], errs[77]) == (0, OK)
    assert sum(1 for e in errs if e != OK) == 1
    ctx.set_option("range_scratch_bytes", FLOOR)
    try:
        _, grouped = run(ctx, case, ranges, "2051 ranges, many groups", seed=3)
    finally:
        ctx.set_option("range_scratch_bytes", 1 << 30)
    assert grouped == plain


HOSTILE = ["swapped", "mid_element", "beyond", "last_beyond", "count",
           "first_garbage", "zero_index"]


@pytest.mark.parametrize("how", HOSTILE)
def test_hostile_index(ctx, case, how):
    """Stream 4 (four blocks) gets a hostile index - or everything does, for
    first[] -; the ranges the damage reaches fail as specified, every other
    range of the call is exact, the bands are intact."""
    s = 4
    good = case.index[s]
    flat, first = case.with_index(s, good)
    rng = random.Random(HOSTILE.index(how))
    if how == "swapped":
        flat, first = case.with_index(s, [good[0], good[2], good[1]] + good[3:])
    elif how == "mid_element":
        flat, first = case.with_index(
            s, [good[0]] + [x + 1 for x in good[1:-1]] + [good[-1]])
    elif how == "beyond":
        flat, first = case.with_index(
            s, good[:2] + [len(case.comps[s]) + 1000] + good[3:])
    elif how == "last_beyond":
        flat, first = case.with_index(s, good[:-1] + [good[-1] + 2**33])
    elif how == "count":
        first[s + 1] -= 1  # stream 4 one entry short, stream 5 one too many
    elif how == "first_garbage":
        first = [rng.getrandbits(64) for _ in first]
    elif how == "zero_index":
        flat, first = case.with_index(s, [0] * len(good))
    ranges = [(s, 0, 200000), (s, 10, 100), (s, 65536, 65536),
              (s, 70000, 10), (s, 131072, 68928), (s, 199999, 1),
              (s, 1000, 189000), (s, 200000, 0),
              (3, 0, 131072), (3, 65535, 2), (1, 0, 1000), (5, 69999, 1),
              (5, 0, 70000), (2, 0, 65536), (0, 0, 0),
              (case.FOREIGN, 7, 7)]
    c = Call(case, ranges, flat=flat, first=first)
    want = c.want()
    failed = [r for r, w in enumerate(want) if w[0] is None]
    passed = [r for r, w in enumerate(want) if w[0] is not None]
    # the damage reaches some ranges of the call and spares others
    assert failed and passed, (failed, passed)
    if how in ("swapped", "beyond"):
        assert want[2][1] == (101, s, 1, 0)       # block 1's entries
        assert want[5][0] is not None              # block 3 is untouched
    if how in ("last_beyond", "zero_index", "count"):
        assert want[1][1] == (101, s, 0, 0) and want[4][1] == (101, s, 2, 0)
        assert want[8][0] is not None
    if how == "mid_element":
        assert want[1][0] is None and want[1][1][0] not in (0, 101)
    c.enqueue(ctx)
    ctx.synchronize()
    c.check(how, want)


def test_device_ranges_larger_than_the_hosts_copies(ctx, case):
    """d_range_len above h_range_len.  A length no stream holds fails its own
    range and takes no slots; a modest lie that asks for a piece more than
    the host sized fails where the slots run out - here the last range.
    Every other range is exact and nothing is written outside the buffers
    (which have the DEVICE lengths: the bands prove it)."""
    ranges = [(4, 0, 100), (3, 65535, 2), (4, 70000, 1000), (1, 0, 1000),
              (4, 65000, 100)]
    dev = [100, 2, 1 << 40, 1000, 70000]
    c = Call(case, ranges, dev_lens=dev)
    c.enqueue(ctx)
    ctx.synchronize()
    want = c.want()
    got, errs, data = c.check("device lens larger", want, skip=(2, 4))
    assert got[2] == 0 and errs[2] == (101, 70000, 1 << 40, 200000)
    # slots: first slot, pieces asked, pieces sized
    assert got[4] == 0 and errs[4] == (101, 4, 3, 6), errs[4]
    assert ctx.info("range_ranges_failed") == 2
    # ... and the same lie in front: the ranges that still fit are exact
    ranges = [(4, 65000, 100), (4, 0, 100), (1, 0, 1000)]
    c = Call(case, ranges, dev_lens=[1000, 100, 1000])
    c.enqueue(ctx)
    ctx.synchronize()
    got, errs, data = c.results("device lens larger, in front")
    assert (got[0], errs[0]) == (1000, OK)
    assert data[0] == case.whole[4][65000:66000]
    assert (got[1], errs[1]) == (100, OK) and data[1] == case.whole[4][:100]
    assert got[2] == 0 and errs[2] == (101, 3, 1, 3), errs[2]


def test_refused_calls_enqueue_nothing(ctx, case):
    """What the entry point refuses before its first launch: a NULL host
    copy, m at 2^31, n + index_entries + pieces at 2^31.  Each is
    SNAPMI_E_ARGUMENT and leaves got, errs and the outputs as they were.
    (Straight through ctypes: the wrapper always builds both host arrays.
    Every refusal comes before the host arrays are read, so the short ones
    given with m = 2^31 are never indexed.)"""
    import ctypes as C
    from rust_snappy_amd import _lib
    ranges = [(4, 1000, 189000), (1, 10, 20)]
    c = Call(case, ranges, seed=5)
    L = _lib.of(ctx)
    h_off = (C.c_uint64 * 2)(*c.offs)
    h_len = (C.c_uint64 * 2)(*c.lens)
    LIMIT = 1 << 31
    pieces = R.pieces(c.offs, c.lens)
    assert pieces == 4

    def call(off=h_off, ln=h_len, m=2, entries=len(c.flat)):
        return L.snapmi_decompress_ranges_indexed(
            ctx._h, c.src.d_ptrs.data_ptr(), c.in_lens.data_ptr(), case.n,
            c.d_first.data_ptr(), c.d_index.data_ptr(), entries,
            c.d_stream.data_ptr(), c.d_off.data_ptr(), c.d_len.data_ptr(),
            off, ln, c.out.d_ptrs.data_ptr(), c.got.data_ptr(),
            c.errs.data_ptr(), m)

    huge = (C.c_uint64 * 2)(0, 0), (C.c_uint64 * 2)(LIMIT * 65536, 0)
    refused = {
        "h_range_off NULL": dict(off=None),
        "h_range_len NULL": dict(ln=None),
        "both NULL": dict(off=None, ln=None),
        "m = 2^31": dict(m=LIMIT),
        "n + entries + pieces = 2^31":
            dict(entries=LIMIT - case.n - pieces),
        "pieces = 2^31": dict(off=huge[0], ln=huge[1]),
    }
    for what, kw in refused.items():
        assert call(**kw) == 101, what
        ctx.synchronize()
        c.out.assert_guards(what)
        assert bool((c.out.data == 0xA5).all()), what
        assert c.got.cpu().tolist() == [-7, -7], what
        assert bool((c.errs == 0x77).all()), what
    # one below the limit is not refused for its size (entries at or behind
    # the streams' own are never read), and the call itself is served
    assert call(entries=LIMIT - case.n - pieces - 1) == 0
    ctx.synchronize()
    c.check("entries one below the limit")
    c.reset()
    assert call() == 0
    ctx.synchronize()
    c.check("after the refusals")


def test_read_ranges_sizes_its_buffers_from_the_streams(ctx, case):
    """batch.read_ranges: a range that does not fit its stream gets no
    buffer - a length of 200 GiB is the range's own
    SNAPMI_E_ARGUMENT, not an allocation failure - and the ranges beside it
    are served."""
    from rust_snappy_amd import batch
    src = batch.StreamBatch.from_bytes(case.comps, torch.device("cuda"))
    index = (u64(case.first), u64(case.flat))
    ranges = [(4, 1000, 189000), (4, 0, 200001), (1, 10, 200 << 30),
              (case.n, 0, 1 << 20), (0, 0, 0), (1, 10, 20), (4, U64 - 1, 1)]
    data, errs = batch.read_ranges(ctx, src, index, ranges)
    assert [tuple(e) for e in errs] == [
        OK, (101, 0, 200001, 200000), (101, 10, 200 << 30, 1000),
        (101, case.n, case.n, 0), OK, OK, (101, U64 - 1, 1, 200000)]
    assert data == [case.whole[4][1000:190000], b"", b"", b"", b"",
                    case.whole[1][10:30], b""]


# ------------------------------------------------------------------ ordering
def make_context(library, stream):
    import rust_snappy_amd as R_
    lib = R_._lib.load_product() if library == "product" else None
    return R_.raw.Context(0, stream=stream.cuda_stream, lib=lib)


ORDER_RANGES = [(4, 1000, 189000), (3, 65536, 65536), (1, 10, 20),
                (5, 69999, 1), (2, 0, 65536), (4, 65535, 2), (0, 0, 0),
                (4, 0, 200001)]


@pytest.mark.parametrize("library", ["test", "product"])
def test_enqueued_behind_compress(built, case, library):
    """compress_batch_indexed and the range reads of what it is still
    writing, enqueued back to back on one context: the streams, their
    lengths and the index reach the second call through device memory only;
    one synchronize at the end."""
    from rust_snappy_amd import raw
    S = torch.cuda.Stream()
    ctx = make_context(library, S)
    try:
        with torch.cuda.stream(S):
            inputs = case.inputs
            n = len(inputs)
            src = Slab([max(len(d), 1) for d in inputs], 11, inputs)
            lens = torch.tensor([len(d) for d in inputs], dtype=torch.int64)
            dst = Slab([O.max_compress_len(len(d)) for d in inputs], 12)
            out_lens = torch.full((n,), -7, dtype=torch.int64, device="cuda")
            entries = raw.block_index_entries([len(d) for d in inputs])
            first = torch.full((n + 1,), -7, dtype=torch.int64, device="cuda")
            index = torch.full((entries,), -7, dtype=torch.int64,
                               device="cuda")
            ranges = [r for r in ORDER_RANGES]
            offs, rl = [r[1] for r in ranges], [r[2] for r in ranges]
            out = Slab([room_of(x) for x in rl], 13)
            m = len(ranges)
            got = torch.full((m,), -7, dtype=torch.int64, device="cuda")
            errs = torch.full((32 * m,), 0x77, dtype=torch.uint8,
                              device="cuda")
            d_stream = torch.tensor([r[0] for r in ranges],
                                    dtype=torch.int32).cuda()
            d_lens, d_off, d_len = lens.cuda(), u64(offs), u64(rl)
            S.synchronize()
            raw.compress_batch(ctx, src.d_ptrs, d_lens, dst.d_ptrs,
                               dst.d_caps, out_lens, None, host_in_lens=lens,
                               index_first=first, index=index,
                               index_cap=entries)
            raw.decompress_ranges_indexed(
                ctx, dst.d_ptrs, out_lens, first, index, d_stream, d_off,
                d_len, offs, rl, out.d_ptrs, got, errs,
                index_entries=entries)
            ctx.synchronize()
            out.assert_guards("behind compress")
            dst.assert_guards("behind compress")
            got = got.cpu().numpy().tolist()
            es = read_errs(errs)
            for r, (s, off, ln) in enumerate(ranges):
                if off + ln <= len(inputs[s]):
                    assert (got[r], es[r]) == (ln, OK), (r, got[r], es[r])
                    assert out.bytes(r, ln) == inputs[s][off:off + ln], r
                else:
                    assert got[r] == 0
                    assert es[r] == (101, off, ln, len(inputs[s]))
    finally:
        ctx.close()


@pytest.mark.parametrize("library", ["test", "product"])
def test_graph_capture_and_replay(built, case, library):
    """One call captured into a graph (a linear chain) behind an eager call
    of the same size, replayed over reset outputs, then over an index made
    hostile in place."""
    S = torch.cuda.Stream()
    ctx = make_context(library, S)
    try:
        with torch.cuda.stream(S):
            ranges = ORDER_RANGES + [(case.FOREIGN, 65536, 100)]
            c = Call(case, ranges, seed=21)
            S.synchronize()
            c.enqueue(ctx)  # the scratch grows here
            S.synchronize()
            eager = c.check("eager")
            c.reset()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=S):
                c.enqueue(ctx)
            c.reset()
            g.replay()
            S.synchronize()
            assert c.check("replay") == eager
            # the same buffers, stream 4's entries 1 and 2 swapped in place
            flat, _ = case.with_index(
                4, [case.index[4][0], case.index[4][2], case.index[4][1]]
                + case.index[4][3:])
            c.flat = flat
            c.d_index.copy_(u64(flat + [7] * 4))
            c.reset()
            g.replay()
            S.synchronize()
            want = c.want()
            assert want[0][0] is None and want[1][0] is not None
            c.check("replay over a hostile index", want)
    finally:
        ctx.close()
