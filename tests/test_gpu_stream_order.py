"""GPU suite: the stream-ordering contract of the device-resident API
(section 3 of include/snapmi.h; DESIGN.md 4.2a "what is ordered by what").

Every other GPU test makes one call, waits and compares: the state a context
keeps across calls (ticket, lane tables and epochs, grow-only scratch, the side
stream and its fork / join events, the host-posted ratio and token words, the
indexed decoder's gate) only ever sees an idle device.  Here calls are
enqueued back to back with ONE wait at the end of a pipeline:

  1. six compress batches (small, large, small, larger, tiny, large - two of
     them grow the scratch while earlier calls are in flight) on every
     compressor configuration, forward and in reverse, plain and indexed;
  2. alternating incompressible / text batches with the ratio hint live,
     pipelined and with a wait after every call: the bytes are the oracle's
     whichever match finder the hint picked;
  3. six decode batches, a sequence of indexed calls between which the gate
     changes state (all pieced / some handed back / nothing indexed / fewer
     than three entries / all pieced), and three snapmi_decompress_stream
     calls, all without a wait in between;
  4. a context on the caller's stream: inputs produced on that stream,
     compress chained into decompress through d_out_lens, one wait on the
     caller's stream - and the calls return while a hold keeps that stream busy;
  5. snapmi_decompress_batch and snapmi_decompress_batch_indexed captured
     into a graph and replayed over buffers whose content changes.

Every result is compared with the oracle (bytes, lengths, error variant and
fields); decode results also with the unindexed call made eagerly on a second
context; outputs lie between guard bands."""
import random
import time

import numpy as np
import pytest
import torch

import blockindex_ref as B
import foreign
import kats
import oracle_lib as O
from gpu_buffers import Slab, hostile, read_errs, u64

pytestmark = pytest.mark.gpu

LENGTHS = [0, 1, 200, 300, 600, 1500, 4096, 8193, 65536, 65537, 131077,
           200000]
SMALL = LENGTHS[:8]
KINDS = ("text", "zeros", "noise")
OK = (0, 0, 0, 0)


@pytest.fixture(scope="module", autouse=True)
def _gpu(built):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


# ------------------------------------------------------------------ the data
_TEXT = []
_COMP = {}


def data(kind, n, salt=0):
    if not _TEXT:
        t = (O.CORPUS / "alice29.txt").read_bytes()
        _TEXT.append(t * 3)
    if kind == "text":
        return _TEXT[0][7 + 13 * salt:7 + 13 * salt + n]
    if kind == "zeros":
        return bytes(n)
    return random.Random(n * 31 + salt).randbytes(n)


def comp(d):
    """(the oracle's stream, its block index) of d, computed once."""
    if d not in _COMP:
        _COMP[d] = (O.compress(d), B.expected_index(d))
    return _COMP[d]


def small(count, salt):
    """count streams of the short lengths, kinds and lengths rotating."""
    return [(KINDS[(k + salt) % 3], SMALL[(k * 3 + salt) % len(SMALL)])
            for k in range(count)]


# small, large, small, larger, tiny, large
SPECS = [
    small(9, 0) + [("text", 65536), ("zeros", 65537), ("noise", 1500)],
    [("text", 200000), ("zeros", 200000), ("noise", 131077),
     ("text", 131077), ("noise", 65537), ("zeros", 65536), ("text", 65537)]
    + small(17, 1),
    small(12, 2) + [("noise", 65536), ("text", 8193)],
    [("text", 200000), ("noise", 200000), ("zeros", 200000),
     ("text", 131077), ("zeros", 131077), ("noise", 131077), ("text", 65537),
     ("noise", 65537), ("zeros", 65537), ("text", 65536)] + small(26, 3),
    [(k, n) for k, n in small(24, 4) if n <= 1500][:12],
    [("noise", 200000), ("text", 200000), ("zeros", 131077),
     ("text", 131077), ("noise", 65537), ("text", 65536), ("zeros", 65536)]
    + small(13, 5),
]


class CBatch:
    """A compress batch and what the oracle says of it.  short: the index of
    a stream whose capacity is a byte short (or None)."""

    def __init__(self, spec, salt, short=None):
        self.datas = [data(k, n, salt) for k, n in spec]
        self.caps = [O.max_compress_len(len(d)) for d in self.datas]
        self.want, self.index = [], []
        for i, d in enumerate(self.datas):
            c, idx = comp(d)
            if i == short:
                self.caps[i] -= 1
                with pytest.raises(O.SnapError) as e:
                    O.compress(d, self.caps[i])
                e = e.value
                self.want.append((0, (e.kind, e.a, e.b, e.c), b""))
                self.index.append([0] * len(idx))
            else:
                self.want.append((len(c), OK, c))
                self.index.append(idx)
        self.first = [0]
        for idx in self.index:
            self.first.append(self.first[-1] + len(idx))
        self.flat = [e for idx in self.index for e in idx]
        self.blocks = sum(-(-len(d) // 65536) for d in self.datas)
        self.total = sum(len(d) for d in self.datas)


@pytest.fixture(scope="module")
def cbatches():
    out = [CBatch(s, k, short=6 if k == 3 else None)
           for k, s in enumerate(SPECS)]
    assert [12 <= len(b.datas) <= 36 for b in out] == [True] * 6
    assert max(b.total for b in out) <= 3 << 19
    # two of them need more scratch than any batch in front of them, beyond
    # the eighth of slack a buffer is given
    assert out[1].blocks > 2 * out[0].blocks
    assert out[3].blocks > out[1].blocks * 5 // 4 + 1
    assert len(out[3].datas[6]) == 65537
    return out


class CBufs:
    """The tensors of one compress call, its own, filled before the
    pipeline's first call."""

    def __init__(self, b, seed):
        n = len(b.datas)
        self.b = b
        self.src = Slab([max(len(d), 1) for d in b.datas], seed + 1, b.datas)
        self.h_lens = torch.tensor([len(d) for d in b.datas],
                                   dtype=torch.int64)
        self.d_lens = self.h_lens.cuda()
        self.dst = Slab(b.caps, seed)
        self.out_lens = torch.full((n,), -7, dtype=torch.int64, device="cuda")
        self.errs = torch.full((32 * n,), 0xEE, dtype=torch.uint8,
                               device="cuda")
        self.first = torch.full((n + 1,), -7, dtype=torch.int64,
                                device="cuda")
        self.index = torch.full((len(b.flat) + 8,), -7, dtype=torch.int64,
                                device="cuda")

    def enqueue(self, ctx, indexed):
        from rust_snappy_amd import raw
        kw = {}
        if indexed:
            kw = dict(index_first=self.first, index=self.index,
                      index_cap=len(self.b.flat))
        raw.compress_batch(ctx, self.src.d_ptrs, self.d_lens, self.dst.d_ptrs,
                           self.dst.d_caps, self.out_lens, self.errs,
                           host_in_lens=self.h_lens, **kw)

    def check(self, indexed, what):
        b = self.b
        self.dst.assert_guards(what)
        lens = self.out_lens.cpu().tolist()
        errs = read_errs(self.errs)
        for i, (n, err, c) in enumerate(b.want):
            assert (lens[i], errs[i]) == (n, err), (what, i, lens[i], errs[i])
            assert self.dst.bytes(i, lens[i]) == c, (what, i, len(b.datas[i]))
        first, index = self.first.cpu().tolist(), self.index.cpu().tolist()
        if indexed:
            assert first == b.first, what
            assert index[:len(b.flat)] == b.flat, what
            assert index[len(b.flat):] == [-7] * 8, what
        else:
            assert set(first) | set(index) == {-7}, what


def compress_pipeline(ctx, batches, order, indexed, what):
    """The batches in `order`, back to back, one wait at the end.  Returns
    the context's scratch bytes behind every enqueue."""
    bufs = [CBufs(batches[k], 10 * k + indexed) for k in order]
    torch.cuda.synchronize()  # the buffers are filled
    trace = [ctx.info("scratch_bytes")]
    for u in bufs:
        u.enqueue(ctx, indexed)
        trace.append(ctx.info("scratch_bytes"))
    ctx.synchronize()  # the one wait
    for k, u in zip(order, bufs):
        u.check(indexed, f"{what} batch {k}")
    return trace


# ------------------------------------------------ 1. pipelined compress
def test_pipelined_compress_every_route(cctx, cbatches):
    """Six batches back to back with host lengths given and one wait, on
    every compressor configuration; then in reverse, with the scratch at its
    final size; then both again through snapmi_compress_batch_indexed.  The
    batch scratch is handed back first (release_scratch, a product option),
    so that the forward pipeline's second and fourth batch each find buffers
    too small and grow them - free and allocate behind a wait for the
    stream - while the calls in front of them are in flight."""
    cctx.set_option("release_scratch", 1)
    cctx.synchronize()
    cctx.set_option("release_scratch", 0)
    fwd, rev = list(range(6)), list(range(5, -1, -1))
    trace = compress_pipeline(cctx, cbatches, fwd, 0, "forward")
    grown = [k for k in range(1, 6) if trace[k + 1] > trace[k]]
    assert trace[2] > trace[1] and trace[4] > trace[3], (trace, grown)
    # (in reverse the buffers are at their final size - but for the token
    # pool of the "_spill" configurations, which grows behind a batch that
    # spilled)
    compress_pipeline(cctx, cbatches, rev, 0, "reverse")
    compress_pipeline(cctx, cbatches, fwd, 1, "indexed forward")
    compress_pipeline(cctx, cbatches, rev, 1, "indexed reverse")


# ------------------------------------------------ 2. the ratio hint
@pytest.fixture(scope="module")
def hint_batches():
    def spec(kind):
        return [(kind, 200000), (kind, 131077), (kind, 65537),
                (kind, 65536)] + [(kind, n) for n in SMALL]
    out = [CBatch(spec("noise"), 6), CBatch(spec("text"), 7)]
    assert all(b.blocks >= 8 and len(b.datas) == 12 for b in out)
    return out


@pytest.mark.parametrize("library", ["test", "product"])
def test_ratio_hint_does_not_change_the_bytes(built, hint_batches, library):
    """Default routing with lane_min_blocks 4: batches of eight blocks and
    more post their ratio (k_post_ratio) and the next batch's match finder is
    chosen by what the host happens to read (match_kernel 2).  Incompressible
    and text batches alternate, eight calls: pipelined the hint is stale or
    half written, with a wait after every call it is the last batch's - the
    bytes are the oracle's either way."""
    import rust_snappy_amd as R
    lib = R._lib.load_product() if library == "product" else None
    for waits in (False, True):
        with R.raw.Context(0, lib=lib) as ctx:
            ctx.set_option("lane_min_blocks", 4)
            bufs = [CBufs(hint_batches[k % 2], k) for k in range(8)]
            torch.cuda.synchronize()
            kernels = []
            for u in bufs:
                u.enqueue(ctx, 0)
                kernels.append(ctx.last_kernel())
                if waits:
                    ctx.synchronize()
            ctx.synchronize()
            for k, u in enumerate(bufs):
                u.check(0, f"call {k} waits={waits} kernels={kernels}")


# ------------------------------------------------ decode batches
def oracle_decode(c, cap):
    try:
        out = O.decompress(c, cap)
        return len(out), OK, out
    except O.SnapError as e:
        return 0, (e.kind, e.a, e.b, e.c), b""


def flipped(c, idx, rng):
    """One flipped byte behind the header."""
    p = rng.randrange(idx[0] + 1, len(c))
    return c[:p] + bytes([c[p] ^ 0x5A]) + c[p + 1:]


def broken_piece(c, idx):
    """A copy with offset zero where the second block begins: that piece
    fails for certain (the length of the stream stays)."""
    return c[:idx[1]] + foreign.copy(0, 8, 2) + c[idx[1] + 3:]


class DBatch:
    """Compressed streams, capacities, the index handed in with them
    (entries per stream; None: the unindexed call) and the oracle's result
    for every stream."""

    def __init__(self, comps, caps, index=None, entries=None):
        self.comps, self.caps, self.index = comps, caps, index
        self.want = [oracle_decode(c, cap) for c, cap in zip(comps, caps)]
        if index is not None:
            self.first = [0]
            for idx in index:
                self.first.append(self.first[-1] + len(idx))
            self.flat = [e for idx in index for e in idx]
            self.entries = self.first[-1] if entries is None else entries

    def passing(self):
        """Streams whose entries pass the rule of the header."""
        return [i for i, (c, cap) in enumerate(zip(self.comps, self.caps))
                if B.indexed(c, cap, self.flat, self.first[i],
                             self.first[i + 1], self.entries)]


def good(cb, skip=()):
    keep = [i for i in range(len(cb.datas)) if i not in skip]
    return ([comp(cb.datas[i])[0] for i in keep],
            [len(cb.datas[i]) for i in keep],
            [comp(cb.datas[i])[1] for i in keep])


def with_damage(cb, rng, indexed, kat_copies=1):
    """The streams of a compress batch plus: the reference's error vectors
    (a few bytes each; kat_copies times), a flipped byte, a truncated stream,
    a capacity a byte short, a piece that cannot decode - each with its TRUE
    index when indexed."""
    comps, caps, index = good(cb)
    long_ones = [i for i, c in enumerate(caps) if c > 65536]
    a, b, c, d = (long_ones + long_ones)[:4]
    comps.append(flipped(comps[a], index[a], rng))
    caps.append(caps[a])
    index.append(index[a])
    cut = rng.randrange(index[b][0] + 1, len(comps[b]))
    comps.append(comps[b][:cut])
    caps.append(caps[b])
    index.append(index[b])
    comps.append(comps[c])
    caps.append(caps[c] - 1)
    index.append(index[c])
    comps.append(broken_piece(comps[d], index[d]))
    caps.append(caps[d])
    index.append(index[d])
    for _, stream, _, _ in kats.ERROR_KATS * kat_copies:
        comps.append(stream)
        caps.append(64)
        index.append([1, max(len(stream) // 2, 2), len(stream)])
    return DBatch(comps, caps, index if indexed else None)


@pytest.fixture(scope="module")
def dbatches(cbatches):
    """The six batches of the pipeline as decode batches, the damage in the
    large ones.  The plain launch's only scratch is the order of the streams,
    four bytes each: the second and the fourth batch carry the error vectors
    several times over (91 and 187 streams), so that this buffer too is
    outgrown twice inside the pipeline."""
    rng = random.Random(3)
    out = []
    for k, cb in enumerate(cbatches):
        if k in (1, 3, 5):
            out.append(with_damage(cb, rng, False, {1: 3, 3: 7, 5: 1}[k]))
        elif k == 4:
            comps, caps, _ = good(cb)
            out.append(DBatch(comps + [s[1] for s in kats.ERROR_KATS],
                              caps + [64] * len(kats.ERROR_KATS)))
        else:
            out.append(DBatch(*good(cb)[:2]))
    return out


@pytest.fixture(scope="module")
def ibatches(cbatches):
    """Indexed calls between which the gate changes state: A all long
    streams pieced, B some pieces fail and their streams are handed back
    (and streams that are not indexed, errors, a short capacity beside
    them), C every index hostile - nothing indexed, D fewer than three
    entries - the plain launch."""
    rng = random.Random(4)
    a = DBatch(*good(cbatches[5]))
    b = with_damage(cbatches[1], rng, True)
    long_ones = [i for i, c in enumerate(b.caps[:len(cbatches[1].datas)])
                 if c > 65536]
    idx = list(b.index)
    for i, how in zip(long_ones, ("mid_element", "plus1", "swapped")):
        idx[i] = hostile(idx[i], len(b.comps[i]), how, rng, idx[0])
    b = DBatch(b.comps, b.caps, idx)
    comps, caps, index = good(cbatches[3], skip=(6,))
    bad = [hostile(e, len(c), ("equal", "random", "last_short", "none")[i % 4],
                   rng, index[0]) for i, (e, c) in enumerate(zip(index, comps))]
    c = DBatch(comps, caps, bad)
    comps, caps, index = good(cbatches[0])
    d = DBatch(comps, caps, index, entries=2)
    n_long = sum(1 for x in a.caps if x > 65536)
    assert len(a.passing()) == n_long >= 4
    assert len(b.passing()) >= 4 and not c.passing() and not d.passing()
    return {"A": a, "B": b, "C": c, "D": d}


class DBufs:
    """The tensors of one decode call.  room: bytes the input slab gives
    every stream (default: what this batch needs); phys: the real sizes of
    the output buffers (default: the capacities the call is told)."""

    def __init__(self, b, seed, room=None, phys=None):
        n = len(b.comps)
        self.src = Slab(room or [max(len(c), 1) for c in b.comps], seed + 1)
        self.dst = Slab(phys or b.caps, seed)
        self.in_lens = torch.zeros(n, dtype=torch.int64, device="cuda")
        self.d_caps = torch.zeros(n, dtype=torch.int64, device="cuda")
        self.out_lens = torch.zeros(n, dtype=torch.int64, device="cuda")
        self.errs = torch.zeros(32 * n, dtype=torch.uint8, device="cuda")
        self.first = self.index = None
        if b.index is not None:
            self.first = u64(b.first)
            self.index = u64(b.flat + [0])
        self.load(b)
        self.reset()

    def load(self, b):
        """Batch b into the same device memory, in place."""
        self.b = b
        self.src.refill(b.comps)
        self.in_lens.copy_(torch.tensor([len(c) for c in b.comps]))
        self.d_caps.copy_(torch.tensor(b.caps))
        if self.index is not None:
            assert len(b.flat) + 1 == self.index.numel()
            assert self.first.cpu().tolist() == b.first
            self.index.copy_(u64(b.flat + [0]))

    def reset(self):
        self.dst.refill()
        self.out_lens.fill_(-7)
        self.errs.fill_(0xEE)

    def enqueue(self, ctx):
        from rust_snappy_amd import raw
        kw = {}
        if self.index is not None:
            kw = dict(index_first=self.first, index=self.index,
                      index_entries=self.b.entries)
        raw.decompress_batch(ctx, self.src.d_ptrs, self.in_lens,
                             self.dst.d_ptrs, self.d_caps, self.out_lens,
                             self.errs, **kw)

    def results(self, what):
        """[(length, error, bytes)] behind a wait; the guard bands whole."""
        self.dst.assert_guards(what)
        lens = self.out_lens.cpu().tolist()
        errs = read_errs(self.errs)
        return [(lens[i], errs[i], self.dst.bytes(i, lens[i]))
                for i in range(len(lens))]

    def check(self, what, eager=None):
        got = self.results(what)
        for i, w in enumerate(self.b.want):
            assert got[i][:2] == w[:2], (what, i, got[i][:2], w[:2])
            assert got[i][2] == w[2], (what, i)
            if eager is not None:
                assert got[i] == eager[i], (what, i, got[i][:2], eager[i][:2])


def eager_unindexed(ctx2, b, seed=77):
    """The unindexed call on a second context, waited for."""
    u = DBufs(DBatch(b.comps, b.caps), seed)
    torch.cuda.synchronize()
    u.enqueue(ctx2)
    ctx2.synchronize()
    return u.results("eager")


def context_like(request, lib_of):
    """A fresh context of the kind the `ctx` fixture's parameter names."""
    import rust_snappy_amd as R
    kind = request.node.callspec.params["ctx"]
    if kind == "product":
        return R.raw.Context(0, lib=lib_of._L)
    c = R.raw.Context(0)
    c.set_option("decode_kernel", {"dec3": 3, "dec2": 2}[kind])
    return c


# ------------------------------------------------ 3. pipelined decode
def test_pipelined_decode(request, ctx, dbatches, ibatches):
    """batch_long_streams 0: snapmi_decompress_batch only enqueues.  The six
    batches back to back, then the indexed calls A B C D A and again in
    reverse, one wait per direction - on a fresh context of the fixture's
    kind, so that its buffers grow inside the pipeline; every result against
    the oracle and against the unindexed call made eagerly on a second
    context (the fixture's own)."""
    ctx.set_option("batch_long_streams", 0)
    pipe = context_like(request, ctx)
    try:
        pipe.set_option("batch_long_streams", 0)
        eager = [eager_unindexed(ctx, b) for b in dbatches]
        ieager = {k: eager_unindexed(ctx, b) for k, b in ibatches.items()}
        for direction in (1, -1):
            order = list(range(6))[::direction]
            names = ["A", "B", "C", "D", "A"][::direction]
            bufs = [DBufs(dbatches[k], 10 * k) for k in order]
            ibufs = [DBufs(ibatches[k], 5 + j) for j, k in enumerate(names)]
            torch.cuda.synchronize()
            trace = [pipe.info("scratch_bytes")]
            for u in bufs + ibufs:
                u.enqueue(pipe)
                trace.append(pipe.info("scratch_bytes"))
            pipe.synchronize()  # the one wait
            for k, u in zip(order, bufs):
                u.check(f"batch {k} direction {direction}", eager[k])
            for j, (k, u) in enumerate(zip(names, ibufs)):
                u.check(f"indexed {k} at {j} direction {direction}",
                        ieager[k])
            if direction == 1:  # a fresh context: buffers grew on the way
                assert trace[2] > trace[1] and trace[4] > trace[3], trace
            else:
                assert trace[-1] == trace[0], trace
    finally:
        pipe.close()
        ctx.set_option("batch_long_streams", 1)


def test_pipelined_decompress_stream(request, ctx):
    """Three snapmi_decompress_stream calls back to back into different
    outputs: pieces, the sequential path (a corrupt block), pieces again."""
    from rust_snappy_amd import raw
    text, zeros = data("text", 200000), data("zeros", 200000)
    c0, i0 = comp(text)
    c2, _ = comp(zeros)
    streams = [(c0, len(text)), (broken_piece(c0, i0), len(text)),
               (c2, len(zeros))]
    pipe = context_like(request, ctx)
    try:
        src = Slab([len(c) for c, _ in streams], 1, [c for c, _ in streams])
        dst = Slab([cap for _, cap in streams], 2)
        out_lens = torch.full((3,), -7, dtype=torch.int64, device="cuda")
        errs = torch.full((96,), 0xEE, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        for i, (c, cap) in enumerate(streams):
            o, p = int(src.offs[i]), int(dst.offs[i])
            raw.decompress_stream(pipe, src.data[o:o + len(c)], len(c),
                                  dst.data[p:p + cap], out_lens[i:i + 1],
                                  errs[32 * i:32 * i + 32])
        pipe.synchronize()
        assert raw.stream_decode_path(pipe) == 0  # the last one: pieces
        dst.assert_guards("decompress_stream")
        lens, es = out_lens.cpu().tolist(), read_errs(errs)
        eager = eager_unindexed(ctx, DBatch([c for c, _ in streams],
                                            [cap for _, cap in streams]))
        for i, (c, cap) in enumerate(streams):
            want = oracle_decode(c, cap)
            got = (lens[i], es[i], dst.bytes(i, lens[i]))
            assert got[:2] == want[:2] and got[2] == want[2], (i, got[:2])
            assert got == eager[i], i
        assert es[1][0] != 0 and es[0] == es[2] == OK
    finally:
        pipe.close()


def test_scratch_bytes_counts_every_call_and_contexts_close(built):
    """"scratch_bytes" sums what the context has given memory to, and
    snapmi_ctx_destroy frees exactly that.  On a fresh context, one call each
    of indexed decode, range reads, the device index build and a batch with a
    long stream: after each the figure has risen by at least what the call
    must hold, from the shapes alone -
      indexed decode  T * 73 + E * 4: a descriptor slot (40 + 32 + 1 bytes)
                      per stream and per index entry, an owner word per entry;
      range reads     a 64 KiB room per cut block of a range;
      index build     (3n + 1) * 8 + 5n: the lengths both ways and first[],
                      the walk list and the states;
      long stream     2n modes, and a descriptor slot for each of the long
                      stream's dlen / 64 KiB + 2 pieces.
    Every result against the oracle; then the context closes, and two more
    are made and closed."""
    import indexbuild_ref as IB
    import long_streams as LS
    import rangeindex_ref as RR
    import rust_snappy_amd as R
    from rust_snappy_amd import raw
    datas = [data("text", 3 * 65536, salt) for salt in (1, 2, 3)]
    n = len(datas)
    batch = DBatch([comp(d)[0] for d in datas], [len(d) for d in datas],
                   [comp(d)[1] for d in datas])
    E, T = batch.entries, n + batch.entries
    assert E == 4 * n and batch.passing() == [0, 1, 2]
    c = R.raw.Context(0)
    try:
        trace = [c.info("scratch_bytes")]
        # ---- indexed decode
        u = DBufs(batch, 31)
        torch.cuda.synchronize()
        u.enqueue(c)
        c.synchronize()
        trace.append(c.info("scratch_bytes"))
        u.check("indexed decode")
        assert c.info("index_streams_pieced") == n
        assert trace[1] - trace[0] >= T * 73 + E * 4, trace

        # ---- range reads: both edges of every range inside a block
        ranges = [(0, 100, 70000), (1, 65537, 131070), (2, 65535, 65538)]
        offs, lens = [r[1] for r in ranges], [r[2] for r in ranges]
        rooms = sum(RR.edges(o, ln) for o, ln in zip(offs, lens))
        assert rooms == 2 * len(ranges)
        out = Slab(lens, 32)
        got = torch.full((3,), -7, dtype=torch.int64, device="cuda")
        rerrs = torch.full((96,), 0x77, dtype=torch.uint8, device="cuda")
        d_stream = torch.tensor([r[0] for r in ranges],
                                dtype=torch.int32).cuda()
        d_off, d_len = u64(offs), u64(lens)
        torch.cuda.synchronize()
        raw.decompress_ranges_indexed(c, u.src.d_ptrs, u.in_lens, u.first,
                                      u.index, d_stream, d_off, d_len, offs,
                                      lens, out.d_ptrs, got, rerrs,
                                      index_entries=E)
        c.synchronize()
        trace.append(c.info("scratch_bytes"))
        out.assert_guards("range reads")
        assert got.cpu().tolist() == lens and read_errs(rerrs) == [OK] * 3
        for i, (s, o, ln) in enumerate(ranges):
            assert out.bytes(i, ln) == datas[s][o:o + ln], i
        assert c.info("range_ranges_ok") == 3
        assert trace[2] - trace[1] >= rooms * 65536, trace

        # ---- the index of the same streams, built on the device
        h_in, h_out = [len(s) for s in batch.comps], batch.caps
        first = torch.full((n + 1,), -7, dtype=torch.int64, device="cuda")
        index = torch.full((E,), -7, dtype=torch.int64, device="cuda")
        status = torch.full((n,), 0x77, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        raw.build_block_index(c, u.src.d_ptrs, u.in_lens, h_in, h_out, first,
                              index, status)
        c.synchronize()
        trace.append(c.info("scratch_bytes"))
        want = [IB.build(s, d) for s, d in zip(batch.comps, batch.caps)]
        assert status.cpu().tolist() == [w[0] for w in want] == [IB.BUILT] * n
        assert first.cpu().tolist() == batch.first
        assert index.cpu().tolist() == batch.flat == \
            [e for w in want for e in w[1]]
        assert trace[3] - trace[2] >= (3 * n + 1) * 8 + 5 * n, trace

        # ---- a small batch with one long stream (200 KiB of text)
        st = LS.mixed(20261019, 3, {"text": 1}, tail_len=8192)
        assert st.dlen == 200 << 10
        assert LS.long_stream_rule(st.in_len, st.dlen)
        shorts = [comp(data("text", k, 4))[0] for k in (300, 4096, 8193)]
        lb = DBatch([st.bytes()] + shorts, [st.dlen, 300, 4096, 8193])
        assert lb.want[0][2] == st.expected()
        v = DBufs(lb, 33)
        torch.cuda.synchronize()
        v.enqueue(c)
        c.synchronize()
        trace.append(c.info("scratch_bytes"))
        v.check("long stream in a batch")
        pieces = st.dlen // 65536 + 2
        assert trace[4] - trace[3] >= 2 * len(lb.comps) + pieces * 73, trace
    finally:
        c.close()
    for _ in range(2):
        again = R.raw.Context(0)
        assert again.info("scratch_bytes") == trace[0]  # (the ticket alone)
        again.close()


# ------------------------------------------------ 4. the caller's stream
def make_context(library, stream):
    import rust_snappy_amd as R
    lib = R._lib.load_product() if library == "product" else None
    return R.raw.Context(0, stream=stream.cuda_stream, lib=lib)


@pytest.mark.parametrize("library", ["test", "product"])
def test_callers_stream_chain(built, cbatches, library):
    """A context on a torch stream S: the inputs are produced on S (a
    non_blocking copy from pinned memory, then a device-side clone),
    compress is chained into decompress - which takes its in_lens from the
    compress call's d_out_lens and its inputs from the compress outputs -
    and the only wait is S.synchronize().  Destroying the context leaves S
    usable."""
    from rust_snappy_amd import raw
    b = cbatches[1]
    n = len(b.datas)
    S = torch.cuda.Stream()
    ctx = make_context(library, S)
    assert ctx.stream == S.cuda_stream
    ctx.set_option("batch_long_streams", 0)
    offs = np.cumsum([0] + [len(d) + 5 for d in b.datas])
    pinned = torch.empty(int(offs[-1]), dtype=torch.uint8).pin_memory()
    pinned.numpy()[:] = GUARD_BYTE
    for o, d in zip(offs, b.datas):
        pinned.numpy()[o:o + len(d)] = np.frombuffer(d, dtype=np.uint8)
    h_lens = torch.tensor([len(d) for d in b.datas], dtype=torch.int64)
    full = [O.max_compress_len(len(d)) for d in b.datas]
    with torch.cuda.stream(S):
        mid = Slab(full, 1)
        out = Slab([len(d) for d in b.datas], 2)
        d_lens = h_lens.cuda()
        c_lens = torch.full((n,), -7, dtype=torch.int64, device="cuda")
        c_errs = torch.full((32 * n,), 0xEE, dtype=torch.uint8, device="cuda")
        o_lens = torch.full((n,), -7, dtype=torch.int64, device="cuda")
        o_errs = torch.full((32 * n,), 0xEE, dtype=torch.uint8, device="cuda")
        h_ptrs = torch.from_numpy(offs[:-1].astype(np.int64)).pin_memory()
        # the inputs, on S, with no wait behind them
        staged = pinned.to("cuda", non_blocking=True)
        src = staged.clone()
        in_ptrs = h_ptrs.to("cuda", non_blocking=True) + src.data_ptr()
        raw.compress_batch(ctx, in_ptrs, d_lens, mid.d_ptrs, mid.d_caps,
                           c_lens, c_errs, host_in_lens=h_lens)
        raw.decompress_batch(ctx, mid.d_ptrs, c_lens, out.d_ptrs, out.d_caps,
                             o_lens, o_errs)
    S.synchronize()  # the only wait
    with torch.cuda.stream(S):
        mid.assert_guards("compressed")
        out.assert_guards("round trip")
        assert c_lens.cpu().tolist() == [len(comp(d)[0]) for d in b.datas]
        assert o_lens.cpu().tolist() == [len(d) for d in b.datas]
        assert read_errs(c_errs) == read_errs(o_errs) == [OK] * n
    for i, d in enumerate(b.datas):
        assert mid.bytes(i, len(comp(d)[0])) == comp(d)[0], i
        assert out.bytes(i, len(d)) == d, i
    ctx.close()
    with torch.cuda.stream(S):
        x = torch.arange(1000, device="cuda").sum()
    S.synchronize()
    assert int(x) == 499500 and S.query()


GUARD_BYTE = 0xA5
HOLD_FLOOR_MS = 250.0


def hold(S, ms, rate):
    """Keeps S busy for about ms milliseconds (rate: _sleep cycles per ms)."""
    with torch.cuda.stream(S):
        torch.cuda._sleep(int(ms * rate))


def sleep_rate(S):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(
        enable_timing=True)
    with torch.cuda.stream(S):
        torch.cuda._sleep(1000)  # (loads the kernel)
        a.record(S)
        torch.cuda._sleep(4_000_000)
        b.record(S)
    S.synchronize()
    return 4_000_000 / a.elapsed_time(b)


@pytest.mark.parametrize("library", ["test", "product"])
def test_calls_return_while_the_stream_is_held(built, cbatches, library):
    """The four batch calls only enqueue: with S held busy, each of
    snapmi_compress_batch (host lengths given), _compress_batch_indexed,
    _decompress_batch (batch_long_streams 0) and _decompress_batch_indexed
    returns, and S.query() is still False behind the last of them.  The
    scratch is warm (the same calls ran once before), so nothing grows.

    The hold is sized by measurement: the four enqueues are timed three
    times on the idle, warmed context, and the hold is 20x the slowest of
    them, at least HOLD_FLOOR_MS.  Measured on an MI355X, this library and
    its parent commit's alike (the library did not change): the four
    enqueues take 0.24 ms on the idle context and 0.13 ms behind the hold,
    which was asked to last 250 ms and lasted 248-250 ms - a thousand times
    the enqueue.  snapmi_decompress_stream is called behind a second hold and only
    its results are asserted (its descriptor goes up by a pageable
    hipMemcpyAsync; what was observed - it returns after 0.1 ms with the
    stream still busy - is noted in DESIGN.md 4.2a)."""
    from rust_snappy_amd import raw
    cb = cbatches[5]
    db = DBatch(*good(cb))
    S = torch.cuda.Stream()
    ctx = make_context(library, S)
    ctx.set_option("batch_long_streams", 0)
    try:
        with torch.cuda.stream(S):
            rate = sleep_rate(S)

            def four(seed):
                bufs = [CBufs(cb, seed), CBufs(cb, seed + 1),
                        DBufs(DBatch(db.comps, db.caps), seed + 2),
                        DBufs(db, seed + 3)]
                S.synchronize()
                return bufs

            def enqueue(bufs):
                t0 = time.perf_counter()
                bufs[0].enqueue(ctx, 0)
                bufs[1].enqueue(ctx, 1)
                bufs[2].enqueue(ctx)
                bufs[3].enqueue(ctx)
                return (time.perf_counter() - t0) * 1e3

            def check(bufs, what):
                S.synchronize()
                bufs[0].check(0, what)
                bufs[1].check(1, what)
                bufs[2].check(what)
                bufs[3].check(what)

            warm = four(0)
            enqueue(warm)
            check(warm, "warm-up")
            idle_ms = 0.0
            for k in range(3):
                bufs = four(10 * k)
                idle_ms = max(idle_ms, enqueue(bufs))
                S.synchronize()
            hold_ms = max(20 * idle_ms, HOLD_FLOOR_MS)
            bufs = four(50)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(
                enable_timing=True)
            a.record(S)
            hold(S, hold_ms, rate)
            b.record(S)
            held_ms = enqueue(bufs)
            busy = not S.query()
            check(bufs, "behind the hold")
            lasted = a.elapsed_time(b)
            print(f"\n[{library}] four enqueues idle {idle_ms:.3f} ms, held "
                  f"{held_ms:.3f} ms; hold asked {hold_ms:.0f} ms, lasted "
                  f"{lasted:.0f} ms")
            assert lasted >= 20 * idle_ms, (lasted, idle_ms)
            assert busy, (idle_ms, held_ms, hold_ms, lasted)

            # snapmi_decompress_stream: results only
            c, _ = comp(cb.datas[1])
            d_in = torch.from_numpy(np.frombuffer(c, dtype=np.uint8).copy()
                                    ).cuda()
            dst = Slab([len(cb.datas[1])], 9)
            out_len = torch.full((1,), -7, dtype=torch.int64, device="cuda")
            err = torch.full((32,), 0xEE, dtype=torch.uint8, device="cuda")
            raw.decompress_stream(ctx, d_in, len(c), dst.data[
                int(dst.offs[0]):int(dst.offs[0]) + dst.caps[0]], out_len, err)
            S.synchronize()  # warm
            dst.refill()
            out_len.fill_(-7)
            S.synchronize()
            hold(S, HOLD_FLOOR_MS, rate)
            t0 = time.perf_counter()
            raw.decompress_stream(ctx, d_in, len(c), dst.data[
                int(dst.offs[0]):int(dst.offs[0]) + dst.caps[0]], out_len, err)
            took = (time.perf_counter() - t0) * 1e3
            print(f"[{library}] decompress_stream behind a hold of "
                  f"{HOLD_FLOOR_MS:.0f} ms: returned after {took:.3f} ms, "
                  f"stream still busy: {not S.query()}")
            S.synchronize()
            dst.assert_guards("decompress_stream")
            assert out_len.cpu().tolist() == [len(cb.datas[1])]
            assert read_errs(err) == [OK]
            assert dst.bytes(0, dst.caps[0]) == cb.datas[1]
    finally:
        ctx.close()


# ------------------------------------------------ 5. graphs
GRAPH_SPEC = [("text", 200000), ("zeros", 200000), ("noise", 131077),
              ("text", 131077), ("zeros", 65537), ("text", 65536),
              ("noise", 8193), ("text", 4096), ("zeros", 1500),
              ("noise", 600), ("text", 300), ("zeros", 200), ("noise", 1),
              ("text", 0)]


@pytest.fixture(scope="module")
def gbatches():
    """A: every long stream indexed.  B, same n and first[]: stream 0 has a
    piece that cannot decode (handed back, then an error), stream 2's last
    entry is short, stream 3 has a flipped byte, stream 8 is truncated,
    stream 4's capacity is a byte short.  C, other bytes: no index passes."""
    rng = random.Random(8)
    datas = [data(k, n) for k, n in GRAPH_SPEC]
    comps = [comp(d)[0] for d in datas]
    caps = [len(d) for d in datas]
    index = [comp(d)[1] for d in datas]
    a = DBatch(comps, caps, index)
    bc, bcaps, bidx = list(comps), list(caps), list(index)
    bc[0] = broken_piece(comps[0], index[0])
    bidx[2] = hostile(index[2], len(comps[2]), "last_short", rng, index[0])
    bc[3] = flipped(comps[3], index[3], rng)
    bc[8] = comps[8][:len(comps[8]) - 3]
    bcaps[4] -= 1
    b = DBatch(bc, bcaps, bidx)
    datas = [data(k, n, 1) for k, n in GRAPH_SPEC]
    c = DBatch([comp(d)[0] for d in datas], caps,
               [hostile(comp(d)[1], len(comp(d)[0]), "equal", rng, index[0])
                for d in datas])
    assert a.first == b.first == c.first
    assert a.passing() == [0, 1, 2, 3, 4] and not c.passing()
    assert b.passing() == [0, 1, 3]
    assert b.want[0][1] != OK and b.want[4][1] != OK and b.want[8][1] != OK
    room = [max(len(x.comps[i]) for x in (a, b, c)) or 1
            for i in range(len(caps))]
    return {"A": a, "B": b, "C": c, "room": room, "phys": caps}


@pytest.mark.parametrize("library", ["test", "product"])
@pytest.mark.parametrize("call", ["plain", "indexed"])
def test_graph_capture_and_replay(built, gbatches, ibatches, call, library):
    """snapmi_decompress_batch (batch_long_streams at its default of 1: under
    capture it skips its look at the batch by itself, returns OK and waits
    for nothing - a wait would end the capture with an error) and
    snapmi_decompress_batch_indexed, each captured with torch.cuda.graph on
    the context's stream behind one eager run of the identical call, then
    replayed: over A; over B and over C written into the same buffers; over
    A behind eager indexed calls that advance the context's sequence number
    and rewrite the gate; twice with no wait in between.  The outputs are
    reset before every replay and the guard bands checked behind it.  The
    frozen sequence number of the captured launches must not let a gate
    word left by an earlier replay, or by the eager calls, open a launch
    over descriptors of another run: results are the oracle's and the eager
    unindexed call's on a second context every time."""
    import rust_snappy_amd as R
    A, Bb, C = gbatches["A"], gbatches["B"], gbatches["C"]
    S = torch.cuda.Stream()
    ctx = make_context(library, S)
    second = R.raw.Context(0, lib=ctx._L)
    second.set_option("batch_long_streams", 0)
    try:
        eager = {k: eager_unindexed(second, gbatches[k]) for k in "ABC"}
        with torch.cuda.stream(S):
            src = A if call == "indexed" else DBatch(A.comps, A.caps)
            u = DBufs(src, 1, room=gbatches["room"], phys=gbatches["phys"])

            def load(b):
                u.load(b if call == "indexed" else DBatch(b.comps, b.caps))
                u.reset()

            others = [DBufs(ibatches["C"], 3), DBufs(ibatches["B"], 4)]
            S.synchronize()
            u.enqueue(ctx)  # the identical call, eagerly: the scratch grows
            S.synchronize()
            u.check("eager", eager["A"])
            if call == "indexed":
                assert ctx.info("index_streams_pieced") == 5
                assert ctx.info("index_streams_fallback") == 0
            u.reset()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=S):
                u.enqueue(ctx)
            for step, k in enumerate("ABC"):
                load(gbatches[k])
                g.replay()
                S.synchronize()
                u.check(f"replay over {k}", eager[k])
            # eager indexed calls of other batches on the same context:
            # nothing indexed, then streams pieced and streams handed back
            for o in others:
                o.enqueue(ctx)
                S.synchronize()
                o.check("eager between replays")
                n_pass = len(o.b.passing())
                pieced = ctx.info("index_streams_pieced")
                fallback = ctx.info("index_streams_fallback")
                assert pieced + fallback == n_pass, (pieced, fallback, n_pass)
                if n_pass:
                    assert pieced >= 1 and fallback >= 1, (pieced, fallback)
            load(A)
            g.replay()
            S.synchronize()
            u.check("replay over A behind eager calls", eager["A"])
            # ... over B, whose handed-back streams need the launch behind
            # the gate that the eager calls have just rewritten
            load(Bb)
            g.replay()
            S.synchronize()
            u.check("replay over B behind eager calls", eager["B"])
            load(A)
            g.replay()
            g.replay()
            S.synchronize()
            u.check("two replays, no wait between", eager["A"])
    finally:
        ctx.close()
        second.close()
