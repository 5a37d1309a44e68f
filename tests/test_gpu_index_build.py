"""GPU suite: the block index of streams that came without one
(snapmi_build_block_index).

Every stream's verdict and entries must be bi_build's
(csrc/snapmi_blockindex.hpp; indexbuild_ref.build is that rule in Python),
whichever route produced them - the parallel scan, the sequential walker - and
whatever the streams beside it hold.  Streams, d_index_first, the index and
the verdicts sit between guard bands (gpu_buffers.Slab) that are checked after
every call; the index is poisoned before it, and four poisoned entries behind
d_index_first[n] must stay so."""
import functools

import numpy as np
import pytest
import torch

import blockindex_ref as B
import indexbuild_ref as IB
import oracle_lib as O
from gpu_buffers import GUARD, Slab, u64

pytestmark = pytest.mark.gpu

POISON = 0x7777777777777777
EXTRA = 4  # poisoned entries behind d_index_first[n]
E_ARGUMENT = 101


@pytest.fixture(scope="module", autouse=True)
def _gpu(built):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.fixture(scope="module")
def tctx(_gpu):
    import rust_snappy_amd as R
    c = R.raw.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def pctx(_gpu):
    import rust_snappy_amd as R
    c = R.raw.Context(0, lib=R._lib.load_product())
    yield c
    c.close()


class Case:
    """The streams of the suite, made once."""

    def __init__(self):
        alice = (O.CORPUS / "alice29.txt").read_bytes()
        self.text = (alice * 7)[:1 << 20]
        # 1: the oracle's streams, the block counts around every edge, the
        # random stream (a literal with length bytes at every block start)
        # and 1 MiB of text (16 blocks, both table levels of the scan)
        self.inputs = IB.inputs(self.text) + [self.text]
        self.oracle = [O.compress(d) for d in self.inputs]
        self.expected = [B.expected_index(d) for d in self.inputs]
        self.foreign, self.foreign_index = IB.foreign_aligned()
        self.unaligned = IB.unaligned()
        self.base = self.oracle[IB.SIZES.index(200000)]
        self.corrupt = IB.corrupt(self.base)
        # the neighbours of the hostile streams: one stream per kind
        self.beside = [self.oracle[i] for i in (2, 5, 7, 9)]


@pytest.fixture(scope="module")
def case():
    return Case()


reference = functools.lru_cache(maxsize=None)(IB.build)


def announced(stream):
    hdr, dlen = B.header(stream)
    return dlen if hdr else 0


class Words:
    """Arrays of 64-bit words inside the buffers of a Slab, each at the first
    multiple of 8 inside its buffer; what is left of the buffer in front and
    behind belongs to the guards."""

    def __init__(self, counts, seed):
        self.counts = [int(c) for c in counts]
        self.slab = Slab([8 * c + 8 for c in self.counts], seed)
        base = self.slab.data.data_ptr()
        assert base % 8 == 0
        self.at = [(int(o) + 7) // 8 * 8 for o in self.slab.offs]
        self.ptrs = [base + a for a in self.at]
        img = self.slab.image()
        for a, c in zip(self.at, self.counts):
            img[a:a + 8 * c] = np.frombuffer(
                np.full(c, POISON, dtype=np.uint64).tobytes(), dtype=np.uint8)
        self.slab.data.copy_(torch.from_numpy(img))

    def fetch(self, what):
        self.slab.assert_guards(what)
        host = self.slab.host
        out = []
        for o, cap, a, c in zip(self.slab.offs, self.slab.caps, self.at,
                                self.counts):
            o = int(o)
            pad = np.concatenate([host[o:a], host[a + 8 * c:o + cap]])
            assert bool((pad == GUARD).all()), what
            out.append([int(v) for v in
                        np.frombuffer(host[a:a + 8 * c].tobytes(),
                                      dtype=np.uint64)])
        return out


class Call:
    """One call: the streams as the device holds them, what the host believes
    (h_in, h_out: default the truth), and everything the call may write."""

    def __init__(self, streams, h_in=None, h_out=None, dev_lens=None, seed=0,
                 with_status=True):
        self.streams = [bytes(s) for s in streams]
        n = self.n = len(streams)
        self.dev_lens = [len(s) for s in streams] if dev_lens is None \
            else list(dev_lens)
        self.h_in = list(self.dev_lens) if h_in is None else list(h_in)
        self.h_out = [announced(s) for s in streams] if h_out is None \
            else list(h_out)
        self.counts = [B.entries(d) for d in self.h_out]
        self.entries = sum(self.counts)
        self.src = Slab([len(s) for s in self.streams], seed + 1,
                        self.streams)
        self.in_lens = u64(self.dev_lens)
        self.words = Words([n + 1, self.entries + EXTRA], seed + 2)
        self.status = Slab([n], seed + 3) if with_status else None
        torch.cuda.synchronize()

    def enqueue(self, ctx, index_cap=None):
        from rust_snappy_amd import raw
        return ctx._L.snapmi_build_block_index(
            ctx._h, self.src.d_ptrs.data_ptr(), self.in_lens.data_ptr(),
            raw._u64_array(self.h_in), raw._u64_array(self.h_out), self.n,
            self.words.ptrs[0], self.words.ptrs[1],
            self.entries + EXTRA if index_cap is None else index_cap,
            self.status_ptr())

    def status_ptr(self):
        if self.status is None:
            return None
        return self.status.data.data_ptr() + int(self.status.offs[0])

    def want(self):
        """(verdict, entries) per stream."""
        out = []
        for s, dl, hi, ho in zip(self.streams, self.dev_lens, self.h_in,
                                 self.h_out):
            if dl != hi:
                out.append((IB.MISSIZED, [0] * B.entries(ho)))
            else:
                out.append(reference(s[:dl], ho))
        return out

    def results(self, what):
        """(first, per-stream entries, verdicts or None) after the guards,
        the poison behind the index and the streams themselves."""
        self.src.assert_guards(what)
        for i, s in enumerate(self.streams):  # the streams are only read
            assert self.src.bytes(i, len(s)) == s, (what, i)
        first, flat = self.words.fetch(what)
        assert flat[self.entries:] == [POISON] * EXTRA, what
        verdicts = None
        if self.status is not None:
            self.status.assert_guards(what)
            verdicts = list(self.status.bytes(0, self.n))
        want_first = [0]
        for c in self.counts:
            want_first.append(want_first[-1] + c)
        assert first == want_first, what
        per = [flat[a:b] for a, b in zip(first, first[1:])]
        return first, per, verdicts

    def check(self, ctx, what, want=None):
        first, per, verdicts = self.results(what)
        want = self.want() if want is None else want
        for i, (st, e) in enumerate(want):
            key = (what, i, len(self.streams[i]), self.h_out[i])
            assert per[i] == e, key
            if verdicts is not None:
                assert verdicts[i] == st, key
        counts = [sum(1 for st, _ in want if st == k) for k in (1, 2, 3, 4)]
        got = [ctx.info("index_build_" + k) for k in
               ("built", "unaligned", "corrupt", "missized")]
        assert got == counts, (what, got, counts)
        return per, verdicts


def run(ctx, streams, what, **kw):
    c = Call(streams, **kw)
    assert c.enqueue(ctx) == 0, ctx._L.snapmi_last_error(ctx._h)
    ctx.synchronize()
    return c, c.check(ctx, what)


def multi_block(call):
    return sum(1 for d in call.h_out if d > 65536)


# ------------------------------------------------------------------ 1, 2, 3
@pytest.mark.parametrize("library", ["test", "product"])
def test_oracle_streams(tctx, pctx, case, library):
    ctx = tctx if library == "test" else pctx
    c, (per, verdicts) = run(ctx, case.oracle, "oracle streams")
    assert per == case.expected
    assert verdicts == [IB.BUILT] * len(case.oracle)
    assert len(case.expected[-1]) == 17
    assert ctx.info("index_build_walked") == 0


def test_this_librarys_own_index(tctx, case):
    """compress_batch_indexed on the same inputs, then the index built from
    its outputs: equal entry for entry."""
    from rust_snappy_amd import batch
    src = batch.StreamBatch.from_bytes(case.inputs, torch.device("cuda"))
    done, first, index = batch.compress(tctx, src, want_index=True)
    streams = [done.stream_bytes(i) for i in range(done.n)]
    c, (per, verdicts) = run(tctx, streams, "own streams", seed=20)
    wrote_first = [int(v) for v in first.cpu().tolist()]
    wrote = [int(v) for v in index.cpu().tolist()]
    assert [wrote[a:b] for a, b in zip(wrote_first, wrote_first[1:])] == per
    assert verdicts == [IB.BUILT] * len(streams)


def test_foreign_aligned_stream(tctx, case):
    """A copy at the head of block 1 that reaches into block 0: BUILT - the
    builder does not look at offsets - and the indexed decoder, which does,
    hands the stream back and still gives the oracle's bytes."""
    from rust_snappy_amd import batch
    streams = [case.oracle[5], case.foreign, case.oracle[2]]
    c, (per, verdicts) = run(tctx, streams, "foreign", seed=30)
    assert per[1] == case.foreign_index and verdicts[1] == IB.BUILT
    src = batch.StreamBatch.from_bytes(streams, torch.device("cuda"))
    first = [0]
    for p in per:
        first.append(first[-1] + len(p))
    flat = [e for p in per for e in p]
    out, lens, errs = batch.decompress(tctx, src, index=(u64(first), u64(flat)))
    for i, s in enumerate(streams):
        assert errs[i][0] == 0
        assert out.stream_bytes(i, lens[i]) == O.decompress(s), i
    assert tctx.info("index_streams_fallback") == 1
    assert tctx.info("index_streams_pieced") == 1


# ------------------------------------------------------------------ 4, 5, 6
def hostile_batch(case, shapes):
    """The hostile streams of `shapes`, each between the neighbours."""
    streams, h_out, where = [], [], {}
    for k, (name, (s, dlen)) in enumerate(shapes.items()):
        b = case.beside[k % len(case.beside)]
        streams += [b, s]
        h_out += [announced(b), dlen]
        where[name] = len(streams) - 1
    streams.append(case.beside[0])
    h_out.append(announced(case.beside[0]))
    return streams, h_out, where


def test_unaligned_streams(tctx, case):
    streams, h_out, where = hostile_batch(case, case.unaligned)
    c, (per, verdicts) = run(tctx, streams, "unaligned", h_out=h_out, seed=40)
    assert len(where) == 3
    for name, i in where.items():
        assert verdicts[i] == IB.UNALIGNED, name
        assert per[i] == [0] * B.entries(h_out[i]), name
        assert verdicts[i - 1] == verdicts[i + 1] == IB.BUILT, name
    assert tctx.info("index_build_walked") == 0


def test_corrupt_streams(tctx, case):
    streams, h_out, where = hostile_batch(case, case.corrupt)
    c, (per, verdicts) = run(tctx, streams, "corrupt", h_out=h_out, seed=50)
    assert len(where) == 7
    for name, i in where.items():
        assert verdicts[i] == IB.CORRUPT, name
        assert per[i] == [0] * B.entries(h_out[i]), name
        assert verdicts[i - 1] == verdicts[i + 1] == IB.BUILT, name
    # every one of them fell through the scan to the walker, nothing else
    assert tctx.info("index_build_walked") == 7


def test_host_copies_that_lie(tctx, case):
    """A wrong h_out_lens with the same and with another block count, and
    h_in_lens off by one either way: MISSIZED, zeros inside exactly the
    entries the host sized, the neighbours exact."""
    o = case.oracle
    streams = [o[2], o[7], o[5], o[6], o[9], o[7], o[3], o[6], o[10]]
    h_out = [announced(s) for s in streams]
    h_in = [len(s) for s in streams]
    assert h_out[1] == 200000 and h_out[3] == 131072
    h_out[1] = 200001             # 4 blocks either way
    h_out[3] = 131073             # 3 blocks where the stream has 2
    h_in[5] += 1
    h_in[7] -= 1
    c, (per, verdicts) = run(tctx, streams, "lies", h_in=h_in, h_out=h_out,
                             dev_lens=[len(s) for s in streams], seed=60)
    assert [len(p) for p in per] == [B.entries(d) for d in h_out]
    for i in range(len(streams)):
        lied = i in (1, 3, 5, 7)
        assert verdicts[i] == (IB.MISSIZED if lied else IB.BUILT), i
        if lied:
            assert per[i] == [0] * B.entries(h_out[i]), i
    assert len(per[3]) == 4
    assert tctx.info("index_build_missized") == 4


# ------------------------------------------------------------------ 7
def test_arguments_and_bounds(tctx, case):
    streams = [case.oracle[k] for k in (7, 2, 5)]
    c = Call(streams, seed=70)
    # index_cap one short: refused, nothing enqueued, nothing written
    assert c.enqueue(tctx, index_cap=c.entries - 1) == E_ARGUMENT
    tctx.synchronize()
    first, flat = c.words.fetch("cap one short")
    assert first == [POISON] * 4 and flat == [POISON] * (c.entries + EXTRA)
    c.status.assert_guards("cap one short")
    assert bool((c.status.data == GUARD).all())
    c.src.assert_guards("cap one short")
    # NULL host arrays (straight through ctypes)
    from rust_snappy_amd import raw
    L = tctx._L
    good_in, good_out = raw._u64_array(c.h_in), raw._u64_array(c.h_out)
    for h_in, h_out in ((None, good_out), (good_in, None), (None, None)):
        rc = L.snapmi_build_block_index(
            tctx._h, c.src.d_ptrs.data_ptr(), c.in_lens.data_ptr(), h_in,
            h_out, c.n, c.words.ptrs[0], c.words.ptrs[1], c.entries + EXTRA,
            c.status_ptr())
        assert rc == E_ARGUMENT
    tctx.synchronize()
    first, flat = c.words.fetch("NULL host arrays")
    assert first == [POISON] * 4 and flat == [POISON] * (c.entries + EXTRA)
    # exactly enough room is enough
    assert c.enqueue(tctx, index_cap=c.entries) == 0
    tctx.synchronize()
    c.check(tctx, "exact cap")
    # n == 0 writes first[0] = 0 and nothing else
    z = Call([], seed=71)
    assert z.enqueue(tctx) == 0
    tctx.synchronize()
    first, flat = z.words.fetch("n == 0")
    assert first == [0] and flat == [POISON] * EXTRA
    # one-block streams only: no scan, no walker
    small = [case.oracle[k] for k in (0, 1, 2, 3, 4)] + [b"\x00\x00",
                                                          b"\xff" * 12]
    s, (per, verdicts) = run(tctx, small, "one-block streams", seed=72)
    assert verdicts == [1, 1, 1, 1, 1, IB.CORRUPT, IB.CORRUPT]
    assert per[0] == [1] and per[5] == [0] and per[6] == [0]
    assert tctx.info("index_build_walked") == 0
    # d_status == NULL
    run(tctx, streams, "no status", seed=73, with_status=False)


# ------------------------------------------------------------------ 8
def batches(case):
    u, hu, _ = hostile_batch(case, case.unaligned)
    k, hk, wk = hostile_batch(case, case.corrupt)
    return {"oracle": (case.oracle, None, set()),
            "unaligned": (u, hu, set()),
            "corrupt": (k, hk, set(wk.values()))}


@pytest.mark.parametrize("which", ["oracle", "unaligned", "corrupt"])
def test_routes_agree(tctx, case, which):
    """Scan then walker (0), the walker alone (1): the same entries and
    verdicts.  The scan alone (2): the streams it gives up on - the corrupt
    ones and no others - come back CORRUPT."""
    streams, h_out, fell = batches(case)[which]
    try:
        seen = {}
        for route in (0, 1, 2):
            tctx.set_test_option("index_build_route", route)
            c, seen[route] = run(tctx, streams, f"{which}, route {route}",
                                 h_out=h_out, seed=80 + route)
            walked = tctx.info("index_build_walked")
            if route == 0:
                assert walked == len(fell)
            elif route == 1:
                assert walked == multi_block(c) > 0
            else:
                assert walked == 0
        assert seen[0] == seen[1] == seen[2]
        want = c.want()
        assert {i for i, (st, _) in enumerate(want)
                if st == IB.CORRUPT and c.h_out[i] > 65536} == fell
    finally:
        tctx.set_test_option("index_build_route", 0)


def test_groups(tctx, case):
    """The scan route in groups of two streams - which reuse the tables and,
    from the third group on, a staging slot an earlier copy has read - gives
    what one group gives."""
    _, one = run(tctx, case.oracle, "one group", seed=90)
    try:
        tctx.set_test_option("index_build_group_streams", 2)
        _, many = run(tctx, case.oracle, "groups of two", seed=91)
    finally:
        tctx.set_test_option("index_build_group_streams", 4096)
    assert many == one


# ------------------------------------------------------------------ 9
def test_end_to_end(tctx, case):
    """batch.build_index, then range reads and the indexed decode through
    what it built."""
    from rust_snappy_amd import batch
    src = batch.StreamBatch.from_bytes(case.oracle, torch.device("cuda"))
    first, index, status = batch.build_index(tctx, src)
    assert status == [IB.BUILT] * src.n
    assert [int(v) for v in index.cpu().tolist()] == [
        e for idx in case.expected for e in idx]
    ranges = []
    for s, d in enumerate(case.inputs):
        n = len(d)
        if n >= 8192:
            ranges.append((s, 4096, 4096))
        if n > 66100:
            ranges.append((s, 65000, 1100))   # across a boundary
        ranges.append((s, 0, n))              # the whole stream
    data, errs = batch.read_ranges(tctx, src, (first, index), ranges)
    for (s, off, n), got, err in zip(ranges, data, errs):
        assert tuple(err) == (0, 0, 0, 0), (s, off, n, err)
        assert got == case.inputs[s][off:off + n], (s, off, n)
    out, lens, errs = batch.decompress(tctx, src, index=(first, index))
    for i, d in enumerate(case.inputs):
        assert errs[i][0] == 0 and out.stream_bytes(i, lens[i]) == d, i
    assert tctx.info("index_streams_pieced") == sum(
        1 for d in case.inputs if len(d) > 65536)
    assert tctx.info("index_streams_fallback") == 0
    # lengths the caller already has give the same index
    first2, index2, status2 = batch.build_index(
        tctx, src, out_lens=[len(d) for d in case.inputs])
    assert torch.equal(first2, first) and torch.equal(index2, index)


# ------------------------------------------------------------------ 10
def test_back_to_back_calls(case):
    """Two builds of different batches enqueued on one context with no wait
    between them, one synchronize; then a larger batch, which grows the
    context's buffers."""
    import rust_snappy_amd as R
    ctx = R.raw.Context(0)
    try:
        u, hu, _ = hostile_batch(case, case.unaligned)
        a = Call(case.oracle[4:10], seed=100)
        b = Call(u, h_out=hu, seed=101)
        assert a.enqueue(ctx) == 0
        assert b.enqueue(ctx) == 0
        ctx.synchronize()
        # (the counters are the last call's)
        first, per, verdicts = a.results("first of two")
        assert [(v, e) for v, e in zip(verdicts, per)] == a.want()
        b.check(ctx, "second of two")
        k, hk, _ = hostile_batch(case, case.corrupt)
        big = Call(case.oracle + k + u, h_out=[announced(s) for s in
                                               case.oracle] + hk + hu,
                   seed=102)
        assert big.enqueue(ctx) == 0
        ctx.synchronize()
        big.check(ctx, "a larger batch")
    finally:
        ctx.close()
