"""GPU suite: no result depends on what the context's scratch held.

A context reuses about sixty grow-only buffers as the call before left them,
and a buffer that grows comes back from the allocator holding anything - in
practice zeros, which hide a kernel that reads a word before this call has
written it.  DESIGN.md 4.2b says which buffers are scratch (every word a call
reads was written earlier in the same call) and which keep state; the test
build's option "scratch_fill" (include/snapmi_test.h) sets every scratch
buffer - device, pinned, the host pipe's slots - and every new allocation to a
byte of the test's choice.

The procedure of every case, on one context (under_fills):
  1. a dirtying call of the same entry point on other data, with at least
     twice the streams and blocks: every buffer the case needs exists and
     holds another batch's values;
  2. the case, checked, with nothing filled (leftovers);
  3. "scratch_fill" 0x00, 0xFF, 0xA5 in turn, the case checked behind each;
  4. behind every setting "scratch_fill_seen" == "scratch_fill_buffers" > 0:
     the knob did what it says.
Once per family the case also runs on a NEW context with "scratch_fill" 0xFF
set before its first call: every buffer is born filled (the growth path).

Every assertion is byte or integer equality with the oracle or the models of
the other suites (oracle_lib, indexed_store and the models it composes,
crc_ref, foreign, kats, long_streams), through their helpers where those have
guard bands.  No tolerances.  The parameters of the ctx / cctx fixtures that
run the shipped library have no such knob: they raise TestOnlyOption at the
first setting and are skipped by conftest's hook.

Left out: the pooled contexts of the libsnappy seam (snapmi_seam.hip) cannot
be reached by a context option; the scalar calls below run the same run_one
path on a context of their own."""
import contextlib
import itertools
import random

import numpy as np
import pytest
import torch

import crc_ref
import foreign
import kats
import long_streams as LS
import oracle_lib as O
from conftest import set_scan_geometry

pytestmark = pytest.mark.gpu

OK = (0, 0, 0, 0)
BYTES = (0x00, 0xFF, 0xA5)
_memo = {}


def memo(key, make):
    if key not in _memo:
        _memo[key] = make()
    return _memo[key]


# ------------------------------------------------------------------ the knob
def fill(ctx, byte):
    """Set the knob and see that it did what it says."""
    ctx.set_test_option("scratch_fill", byte)
    n, seen = ctx.info("scratch_fill_buffers"), ctx.info("scratch_fill_seen")
    assert seen == n > 0, (hex(byte), seen, n)
    assert ctx.info("scratch_fill_bytes") >= n


def under_fills(ctx, dirty, case):
    """The procedure above; case(what) runs the case and checks everything it
    returns."""
    ctx.set_test_option("scratch_fill", -1)   # (the shipped library: skipped)
    try:
        dirty()
        case("leftovers")
        for b in BYTES:
            fill(ctx, b)
            case(f"filled {b:#04x}")
    finally:
        ctx.set_test_option("scratch_fill", -1)


@contextlib.contextmanager
def born_filled(options=(), test_options=()):
    """A new context of the test build whose every buffer is born holding
    0xFF."""
    import rust_snappy_amd as R
    c = R.raw.Context(0)
    try:
        for k, v in options:
            c.set_option(k, v)
        for k, v in test_options:
            c.set_test_option(k, v)
        fill(c, 0xFF)   # (the ticket of snapmi_ctx_create is there already)
        yield c
    finally:
        c.close()


LANES = (("compress_mode", 1), ("lane_min_blocks", 1), ("lane_coresident", 0),
         ("match_kernel", 0))


@pytest.fixture(scope="module", autouse=True)
def _gpu(built):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.fixture(scope="module")
def own(built):
    """A context of the test build that serves only this file: the host
    memory calls, the scalar calls."""
    import rust_snappy_amd as R
    c = R.raw.Context(0)
    yield c
    c.close()


# ------------------------------------------------------------ raw compress
LENGTHS = [0, 1, 17, 200, 255, 256, 700, 1023, 1024, 2047, 2048, 8192, 8193,
           65535, 65536, 65537, 131073, 200000]
FILES = ["alice29.txt", "asyoulik.txt", "html", "lcet10.txt", "plrabn12.txt",
         "urls.10K", "geo.protodata", "kppkn.gtb", "paper-100k.pdf",
         "fireworks.jpeg"]


def text():
    return memo("text", lambda: b"".join(
        (O.CORPUS / n).read_bytes()
        for n in ("alice29.txt", "lcet10.txt", "plrabn12.txt")))


def blocks_of(datas):
    return sum((len(d) + 65535) // 65536 for d in datas)


def compress_inputs():
    def make():
        t, rng = text(), random.Random(41)
        datas = []
        for n in LENGTHS:
            datas += [t[11:11 + n], bytes(rng.choices(b"ab", k=n)), bytes(n)]
        datas.append((O.CORPUS / "fireworks.jpeg").read_bytes()[:70000])
        for name in FILES:
            datas.append((O.CORPUS / name).read_bytes())
            if blocks_of(datas) > 70:
                break
        assert blocks_of(datas) > 64   # two segments in "lanes_segmented"
        return datas
    return memo("compress_inputs", make)


def compress_dirt():
    """Other data, twice the streams and blocks."""
    return memo("compress_dirt", lambda: (
        [d[::-1] for d in compress_inputs()] +
        [d[1:] + b"\x5a" for d in compress_inputs()]))


def compressed():
    return memo("compressed", lambda: [O.compress(d)
                                       for d in compress_inputs()])


def compress_case(ctx, spill=False):
    from test_gpu_bounds import encode_guarded
    datas, want = compress_inputs(), compressed()

    def case(what):
        if spill:   # the pool grows behind a batch that spilled: start over
            ctx.set_option("token_pool_pct", 1)
        dst, lens, errs = encode_guarded(ctx, datas, 7, False)
        assert errs == [OK] * len(datas), what
        assert [int(x) for x in lens] == [len(c) for c in want], what
        for i, c in enumerate(want):
            assert dst.bytes(i, len(c)) == c, (what, i, len(datas[i]))
    return case


def compress_dirty(ctx):
    from test_gpu_bounds import encode_guarded
    return lambda: encode_guarded(ctx, compress_dirt(), 9, False)


def test_raw_compress(cctx, request):
    """Every route of the compressor: the planner's arrays, the ticket, the
    scheduler's lists, token pages and counts, the spill list, the slots."""
    name = request.node.callspec.params["cctx"]
    spill = name.endswith("_spill")
    under_fills(cctx, compress_dirty(cctx), compress_case(cctx, spill))
    if name in ("lanes_spill", "spans_match_spill"):
        assert cctx.info("token_blocks_spilled") > 0


def test_raw_compress_reallocating(built):
    """release_scratch 1 and a wait behind every call: each call's token
    scratch is a new allocation, born filled - and all of it is given back,
    the token counts and the scheduler's lists included."""
    import rust_snappy_amd as R
    c = R.raw.Context(0)
    try:
        for k, v in LANES:
            c.set_option(k, v)
        c.set_option("release_scratch", 1)
        case = compress_case(c)

        def released(what):
            case(what)   # (encode_guarded ends with ctx.synchronize())
            assert c.info("token_scratch_bytes") == 0, what
        under_fills(c, compress_dirty(c), released)
        # the window kernel's scheduler lists are given back as well
        before = c.info("scratch_bytes")
        c.set_option("compress_mode", 0)
        c.set_option("small_batch_kernel", 0)
        c.set_option("span_schedule", 2)
        c.set_test_option("scratch_fill", 0xA5)
        released("scheduled window kernel")
        assert c.last_kernel() == "k_compress_spans"
        assert c.info("scratch_bytes") <= before
    finally:
        c.close()


def test_raw_compress_born_filled(built):
    with born_filled(LANES + (("lane_segment_blocks", 64),)) as c:
        compress_case(c)("born filled, lanes")
    with born_filled() as c:
        compress_case(c)("born filled, default route")


# ---------------------------------------------------------- raw decompress
def decode_inputs():
    """(streams, capacities): the compress case's streams, foreign streams,
    the error KATs, single-byte corruptions, capacities one byte short."""
    def make():
        comps = list(compressed())
        caps = [len(d) for d in compress_inputs()]
        for c, d in foreign.cases()[:5]:
            comps.append(c)
            caps.append(len(d))
        for _, data, _, bad_header in kats.ERROR_KATS:
            comps.append(data)
            caps.append(1024 if bad_header else O.decompress_len(data))
        rng = random.Random(17)
        good = [i for i, d in enumerate(compress_inputs()) if len(d) >= 17]
        for _ in range(20):
            i = rng.choice(good)
            b = bytearray(compressed()[i])
            b[rng.randrange(len(b))] ^= 1 << rng.randrange(8)
            comps.append(bytes(b))
            caps.append(len(compress_inputs()[i]))
        for i in rng.sample(good, 6):
            comps.append(compressed()[i])
            caps.append(len(compress_inputs()[i]) - 1)
        return comps, caps
    return memo("decode_inputs", make)


def decode_verdicts():
    """The oracle's bytes or error fields, once."""
    def make():
        out = []
        for m, cap in zip(*decode_inputs()):
            try:
                out.append((O.decompress(m, cap), OK))
            except O.SnapError as oe:
                out.append((None, (oe.kind, oe.a, oe.b, oe.c)))
        return out
    return memo("decode_verdicts", make)


def decode_dirt():
    return memo("decode_dirt", lambda: [O.compress(d)
                                        for d in compress_dirt()])


def decode_case(ctx):
    from test_gpu_bounds import decode_guarded
    comps, caps = decode_inputs()
    want = decode_verdicts()
    assert sum(e != OK for _, e in want) >= len(kats.ERROR_KATS) + 6

    def case(what):
        dst, lens, errs = decode_guarded(ctx, comps, caps, 3, False)
        for i, (w, e) in enumerate(want):
            assert errs[i] == e, (what, i, errs[i], e)
            if w is not None:
                assert int(lens[i]) == len(w), (what, i)
                assert dst.bytes(i, len(w)) == w, (what, i)
    return case


def decode_dirty(ctx):
    from test_gpu_bounds import decode_guarded
    dirt = decode_dirt()
    caps = [len(d) for d in compress_dirt()]
    return lambda: decode_guarded(ctx, dirt, caps, 5, False)


def test_raw_decompress(ctx):
    under_fills(ctx, decode_dirty(ctx), decode_case(ctx))


def test_raw_decompress_many_streams_per_workgroup(ctx):
    """decode_many_min lowered: k_decompress_streams3_many, sixteen streams
    of the sorted order per workgroup."""
    ctx.set_test_option("decode_many_min", 8)
    try:
        under_fills(ctx, decode_dirty(ctx), decode_case(ctx))
    finally:
        ctx.set_test_option("decode_many_min", 1 << 20)


def test_raw_decompress_born_filled(built):
    with born_filled() as c:
        decode_case(c)("born filled")
    with born_filled(test_options=(("decode_many_min", 8),)) as c:
        decode_case(c)("born filled, many per workgroup")


# ------------------------------------------------------------- long streams
LONG = ("scan8", "scan16")   # the two smallest of the ladder
GEOMETRIES = [pytest.param((10, 0), id="1k"), pytest.param((12, 16),
                                                            id="4k-16")]


def ladder(name):
    """(a tail is stamped with a running number: one Stream per name)"""
    return memo(("ladder", name), lambda: LS.ladder(name))


@pytest.fixture(scope="module")
def dpool():
    return torch.from_numpy(LS.pool().raw).cuda()


def lone_case(ctx, st, dpool):
    from rust_snappy_amd import raw
    from test_gpu_long_streams import assert_output, decode_lone
    comp = memo(("lone", id(st)), st.bytes)

    def case(what):
        slab, out, n, e, _ = decode_lone(ctx, comp, st.dlen)
        assert e == OK and n == st.dlen, (what, e, n)
        assert_output(out, st, dpool)
        # the parallel scan decoded it, not the sequential decoder
        assert raw.stream_decode_path(ctx) == 0, what
    return case


@pytest.mark.parametrize("geom", GEOMETRIES)
def test_long_streams_alone(ctx, dpool, geom):
    from test_gpu_long_streams import decode_lone
    ctx.set_test_option("scratch_fill", -1)
    set_scan_geometry(ctx, geom)
    try:
        for name in LONG:
            st = ladder(name)
            # (other data of twice the blocks)
            other = LS.mixed(77, 2 * len(st.idx), tail_len=4321)
            under_fills(ctx,
                        lambda: decode_lone(ctx, other.bytes(), other.dlen),
                        lone_case(ctx, st, dpool))
    finally:
        set_scan_geometry(ctx, None)


def batch_of(streams, shorts, seed):
    """(Stream or stream bytes, output capacity) items, shuffled."""
    items = [(s, s.dlen) for s in streams] + [(c, len(d)) for c, d in shorts]
    random.Random(seed).shuffle(items)
    return items


def long_batch():
    return memo("long_batch", lambda: batch_of(
        [ladder(n) for n in LONG], LS.short_streams(23, 40), 6))


def long_batch_dirt():
    def make():
        a, b = (ladder(n) for n in LONG)
        return batch_of([LS.mixed(78, 2 * len(a.idx), tail_len=99),
                         LS.mixed(79, 2 * len(b.idx), tail_len=7),
                         LS.mixed(80, 3), LS.mixed(81, 5, tail_len=65535)],
                        LS.short_streams(24, 80), 7)
    return memo("long_batch_dirt", make)


def long_batch_case(ctx):
    from test_gpu_long_streams import check_batch
    items = long_batch()

    def case(what):
        lens, errs = check_batch(ctx, items, 60)
        assert errs == [OK] * len(items), what
    return case


@pytest.mark.parametrize("geom", GEOMETRIES)
def test_long_streams_in_a_batch(ctx, geom):
    """... beside forty small streams: k_long_plan's list and count, the
    modes of both launches, the side launch's order buffer."""
    from test_gpu_long_streams import decode_batch
    ctx.set_test_option("scratch_fill", -1)
    set_scan_geometry(ctx, geom)
    try:
        dirt = long_batch_dirt()
        under_fills(ctx,
                    lambda: decode_batch(ctx, [s.bytes() if isinstance(
                        s, LS.Stream) else s for s, _ in dirt],
                        [c for _, c in dirt], 61),
                    long_batch_case(ctx))
    finally:
        set_scan_geometry(ctx, None)


def test_long_streams_born_filled(dpool):
    with born_filled() as c:
        lone_case(c, ladder("scan8"), dpool)("born filled, alone")
    with born_filled() as c:
        long_batch_case(c)("born filled, batch")


# ---------------------------------------------------------- the indexed family
@pytest.fixture(scope="module")
def played_fail():
    import indexed_store as S
    return S.play(S.SCENARIO_FAIL)


def filling(ctx):
    """run_chain's before_call: the next of the three bytes in front of every
    call - indexed compress, indexed decode, range reads, writes (the failing
    ones too), appends, build_block_index, each on freshly filled scratch."""
    turn = itertools.cycle(BYTES)
    return lambda: fill(ctx, next(turn))


@pytest.mark.parametrize("ctx", ["dec3"], indirect=True)
def test_indexed_chain_on_the_default_route(ctx, played_fail):
    from test_gpu_indexed_store import kernel_of, run_chain
    try:
        run_chain(ctx, played_fail, kernel_of("dec3"),
                  before_call=filling(ctx))
    finally:
        ctx.set_test_option("scratch_fill", -1)


@pytest.mark.parametrize("cctx", ["lanes", "lanes_spill", "coresident"],
                         indirect=True)
def test_indexed_chain_on_the_token_path(cctx, played_fail, request):
    from test_gpu_indexed_store import SPILLS, kernel_of, run_chain
    name = request.node.callspec.params["cctx"]
    try:
        run_chain(cctx, played_fail, kernel_of(name), spills=name in SPILLS,
                  before_call=filling(cctx))
    finally:
        cctx.set_test_option("scratch_fill", -1)


def test_indexed_chain_born_filled(played_fail):
    from test_gpu_indexed_store import kernel_of, run_chain
    with born_filled() as c:
        run_chain(c, played_fail, kernel_of("dec3"))
    with born_filled(LANES) as c:
        run_chain(c, played_fail, kernel_of("lanes"))


# ----------------------------------------------------- frames on the device
IDENT = b"\xff\x06\x00\x00sNaPpY"


def frame_text():
    """About 300 KB whose 64 KiB chunks are text, stored (a stretch that does
    not compress) and text again."""
    def make():
        t = text()
        d = (t[5000:105000] + random.Random(29).randbytes(140000) +
             t[200000:260001])
        f = O.frame_compress(d)
        types = chunk_types(f)
        assert 0 in types and 1 in types, types
        return d, f
    return memo("frame_text", make)


def chunk_types(f):
    r, out = 0, []
    while r < len(f):
        n = int.from_bytes(f[r + 1:r + 4], "little")
        if f[r] <= 1:
            out.append(f[r])
        r += 4 + n
    return out


def mixed_chunks():
    """The same text cut by the caller into chunks of mixed sizes: (lens, the
    framed stream the oracle gives chunk by chunk)."""
    def make():
        d, _ = frame_text()
        rng, lens, o = random.Random(31), [], 0
        while o < len(d):
            n = min(rng.choice([1, 17, 300, 4096, 40000, 65535, 65536]),
                    len(d) - o)
            lens.append(n)
            o += n
        want, o = IDENT, 0
        for n in lens:
            want += O.frame_compress(d[o:o + n])[10:]
            o += n
        assert {0, 1} <= set(chunk_types(want))
        return lens, want
    return memo("mixed_chunks", make)


def dev(b):
    return torch.frombuffer(bytearray(b or b"\0"), dtype=torch.uint8).cuda()


def frame_compress_case(ctx):
    from rust_snappy_amd import frame
    d, want = frame_text()
    lens, want_mixed = mixed_chunks()
    d_in = dev(d)

    def case(what):
        torch.cuda.synchronize()
        for want_index in (False, True):
            out, n, index = frame.compress_device(ctx, d_in, want_index)
            assert out[:n].cpu().numpy().tobytes() == want, (what, want_index)
            if want_index:
                from test_gpu_frame_nowait import chunk_offsets
                assert index.cpu().tolist() == chunk_offsets(want) + \
                    [len(want)], what
        out, n = frame.compress_chunks_device(ctx, d_in, lens)
        assert out[:n].cpu().numpy().tobytes() == want_mixed, what
    return case


def frame_dirt():
    def make():
        t = text()
        d = t[300000:700000] + random.Random(30).randbytes(200000)
        return d, O.frame_compress(d)
    return memo("frame_dirt", make)


def test_frame_compress(ctx):
    from rust_snappy_amd import frame
    other = dev(frame_dirt()[0])

    def dirty():
        torch.cuda.synchronize()
        frame.compress_device(ctx, other, True)
    under_fills(ctx, dirty, frame_compress_case(ctx))


@contextlib.contextmanager
def front(ctx, which):
    """The parallel walk for streams of this size, or the library's own
    choice (the sequential walk)."""
    if which == "parallel":
        ctx.set_test_option("frame_walk_segment", 128 << 10)
        ctx.set_option("frame_parallel_walk_min", 0)
    try:
        yield
    finally:
        ctx.set_test_option("frame_walk_segment", 32 << 20)
        ctx.set_option("frame_parallel_walk_min", 4 << 20)


def frame_decode_case(ctx):
    """The three fronts of a lone decode, and the no-wait decode whose table
    is sized by the caller's bound: the pad behind the chunks the stream has
    is scratch the call writes itself."""
    from rust_snappy_amd import frame
    from gpu_buffers import u64
    from test_gpu_frame_nowait import Bufs, NO_WAIT, call, chunk_offsets
    streams = [frame_text(), (frame_text()[0], mixed_chunks()[1])]

    def nowait(what, d, f, bound, index=None, want_front=None):
        b = Bufs(f, len(d), 11)
        idx = u64(index) if index is not None else None
        torch.cuda.synchronize()
        assert call(ctx, b, bound, idx, NO_WAIT) == 0, what
        ctx.synchronize()
        assert b.result(what) == (len(d), OK, d), (what, bound)
        if want_front is not None:
            assert ctx.info("frame_nowait_front") == want_front, what

    def case(what):
        for k, (d, f) in enumerate(streams):
            key = (what, k)
            d_in = dev(f)
            offs = chunk_offsets(f)
            index = u64(offs + [len(f)])
            torch.cuda.synchronize()
            for which in ("index", "walk", "parallel"):
                with front(ctx, which):
                    out, n = frame.decompress_device(
                        ctx, d_in, len(f), index if which == "index" else None)
                assert out[:n].cpu().numpy().tobytes() == d, (key, which)
            exact = len(offs)
            nowait(key, d, f, exact, offs + [len(f)], want_front=1)
            nowait(key, d, f, exact, want_front=3)
            nowait(key, d, f, 4 * exact, want_front=3)
            # (the parallel walk keeps 32 candidates a segment: it decides
            # the stream of 64 KiB chunks, and may hand the one of tiny
            # chunks to the sequential walk)
            with front(ctx, "parallel"):
                nowait(key, d, f, 4 * exact, want_front=2 if k == 0 else None)
    return case


def test_frame_decode_fronts(ctx):
    from rust_snappy_amd import frame
    d, f = frame_dirt()
    other = dev(f)

    def dirty():
        torch.cuda.synchronize()
        for which in ("walk", "parallel"):
            with front(ctx, which):
                frame.decompress_device(ctx, other, len(f))
    under_fills(ctx, dirty, frame_decode_case(ctx))


def frame_batch():
    """Sixty streams to compress; the good and malformed streams of
    tests/test_gpu_frame_batch.py to decode, with the oracle's verdicts."""
    def make():
        import test_gpu_frame_batch as FB
        t, rng = text(), random.Random(37)
        datas = FB.batch_inputs()
        while len(datas) < 60:
            n = rng.randrange(150000)
            o = rng.randrange(len(t) - n)
            datas.append(t[o:o + n])
        streams, origs = FB.mixed_batch()
        assert len(streams) >= 60
        return (datas, [O.frame_compress(d) for d in datas], streams, origs,
                [FB.oracle_verdict(s) for s in streams])
    return memo("frame_batch", make)


def frame_batch_case(ctx):
    import test_gpu_frame_batch as FB
    from rust_snappy_amd import batch, frame
    datas, want, streams, origs, verdicts = frame_batch()
    cap = 1 << 18

    def case(what):
        src = batch.StreamBatch.from_bytes(datas)
        dst, lens, errs = frame.compress_many(ctx, src)
        for i, w in enumerate(want):
            assert errs[i] == OK, (what, i, errs[i])
            assert dst.stream_bytes(i, lens[i]) == w, (what, i)
        src = batch.StreamBatch.from_bytes(streams)
        dst, lens, errs = frame.decompress_many(ctx, src,
                                                caps=[cap] * len(streams))
        failed = 0
        for i, (w, oe) in enumerate(verdicts):
            got = dst.stream_bytes(i, lens[i])
            if origs[i] is not None:
                assert (errs[i], got) == (OK, origs[i]), (what, i)
            elif oe is None:
                assert (errs[i], got) == (OK, w), (what, i)
            else:
                FB.assert_oracle_error(errs[i], oe, streams[i])
                failed += 1
        assert failed >= 20, what
    return case


def test_frame_batches(ctx):
    from rust_snappy_amd import batch, frame
    datas, want, _, _, _ = frame_batch()

    def dirty():
        more = [d[::-1] for d in datas] + [d[3:] + b"\1\2\3" for d in datas]
        src = batch.StreamBatch.from_bytes(more)
        frame.compress_many(ctx, src)
        src = batch.StreamBatch.from_bytes([w + w[10:] for w in want] + want)
        frame.decompress_many(ctx, src)
    under_fills(ctx, dirty, frame_batch_case(ctx))


def test_frames_born_filled(built):
    with born_filled() as c:
        frame_compress_case(c)("born filled")
    with born_filled() as c:
        frame_decode_case(c)("born filled")
    with born_filled() as c:
        frame_batch_case(c)("born filled")


# --------------------------------------------------------------- host memory
def host_frame_inputs():
    def make():
        data = b"".join(d for _, d in O.corpus_round())[:3_000_001]
        nch = (len(data) + 65535) // 65536
        lens = np.full(nch, 65536, dtype=np.uint32)
        lens[-1] = len(data) - (nch - 1) * 65536
        return data, lens, O.frame_compress(data)
    return memo("host_frame_inputs", make)


class HostMem:
    """n bytes of host memory, pageable or pinned, behind guard bytes."""

    def __init__(self, n, pinned, fill=None):
        from rust_snappy_amd import frame
        self.n, self.pin = n, frame.HostBuffer(n + 128) if pinned else None
        self.array = self.pin.array if pinned else np.empty(n + 128, np.uint8)
        self.array[:] = 0xC7
        if fill is not None:
            self.array[64:64 + n] = np.frombuffer(fill, dtype=np.uint8)
        self.ptr = self.array.ctypes.data + 64

    def bytes(self, n):
        return self.array[64:64 + n].tobytes()

    def assert_guards(self, n, what):
        assert (self.array[:64] == 0xC7).all(), what
        assert (self.array[64 + n:] == 0xC7).all(), what

    def close(self):
        self.array = None
        if self.pin:
            self.pin.close()


def host_frame_case(ctx, pinned):
    """snapmi_frame_encode_host / _decode_host with slices small enough that
    all three slots of the pipe carry one."""
    import ctypes as C
    from rust_snappy_amd import _lib
    L = _lib.of(ctx)
    data, lens, want = host_frame_inputs()
    nch = len(lens)
    cap = L.snapmi_frame_encode_bound(len(data), nch)

    def case(what):
        h_in = HostMem(len(data), pinned, data)
        h_out = HostMem(cap, pinned)
        # (the decoder takes whole chunks: room for 64 KiB each)
        h_back = HostMem(nch * 65536, pinned)
        try:
            written = C.c_size_t(0)
            rc = L.snapmi_frame_encode_host(
                ctx._h, C.c_void_p(h_in.ptr), lens.ctypes.data_as(C.c_void_p),
                nch, 0, C.c_void_p(h_out.ptr), cap, C.byref(written))
            assert rc == 0 and written.value == len(want), (what, rc)
            assert h_out.bytes(len(want)) == want, what
            h_out.assert_guards(len(want), what)
            stale = (C.c_uint8 * 10)()
            consumed = C.c_size_t(0)
            err = _lib.SnapmiError()
            rc = L.snapmi_frame_decode_host(
                ctx._h, C.c_void_p(h_out.ptr), len(want), 2, stale,
                C.c_void_p(h_back.ptr), nch * 65536, C.byref(written),
                C.byref(consumed), C.byref(err))
            assert (rc, written.value, consumed.value) == \
                (0, len(data), len(want)), (what, rc)
            assert (err.kind, err.a, err.b, err.c) == OK, what
            assert h_back.bytes(len(data)) == data, what
            h_back.assert_guards(len(data), what)
        finally:
            for h in (h_in, h_out, h_back):
                h.close()
    return case


@contextlib.contextmanager
def small_slices(ctx):
    ctx.set_option("host_encode_slice", 1 << 20)        # three slices
    ctx.set_option("host_decode_slice_chunks", 16)      # three slices
    try:
        yield
    finally:
        ctx.set_option("host_encode_slice", 2048 << 20)
        ctx.set_option("host_decode_slice_chunks", 8192)


@pytest.mark.parametrize("pinned", [False, True], ids=["pageable", "pinned"])
def test_host_frame_calls(own, pinned):
    from rust_snappy_amd import frame
    data, lens, _ = host_frame_inputs()
    other = bytearray((data + data)[::-1])
    more = np.concatenate([lens[::-1], lens[::-1]])
    with small_slices(own):
        under_fills(own, lambda: frame.encode_host(own, other, more),
                    host_frame_case(own, pinned))


def host_raw_case(ctx, pinned):
    import test_gpu_host_batch as HB
    datas, comps = HB.inputs(), HB.oracle_compressed()

    def case(what):
        lens, errs, outs = HB.run(ctx, True, datas,
                                  [O.max_compress_len(len(d)) for d in datas],
                                  pinned)
        assert errs == [OK] * len(datas), what
        assert outs == comps, what
        lens, errs, outs = HB.run(ctx, False, comps, [len(d) for d in datas],
                                  pinned, seed=2)
        assert errs == [OK] * len(datas), what
        assert outs == datas, what
        assert ctx.info("host_batch_slices") >= 3, what
    return case


def host_frame_batch_case(ctx, pinned):
    import test_gpu_frame_host_batch as FHB
    from rust_snappy_amd import frame
    datas, framed = FHB.inputs(), FHB.framed()
    pairs = FHB.decode_pairs()

    def case(what):
        lens, errs, outs = FHB.run(ctx, True, datas,
                                   [frame.frame_max_len(len(d))
                                    for d in datas], pinned)
        assert errs == [OK] * len(datas), what
        assert outs == framed, what
        assert ctx.info("host_batch_slices") >= 3, what
        lens, errs, outs = FHB.run(ctx, False, [f for f, _ in pairs],
                                   [len(d) for _, d in pairs], pinned, seed=2)
        assert errs == [OK] * len(pairs), what
        assert outs == [d for _, d in pairs], what
    return case


@pytest.mark.parametrize("pinned", [False, True], ids=["pageable", "pinned"])
def test_host_batch_calls(own, pinned):
    """snapmi_[frame_]compress_batch_host / _decompress_batch_host
    (raw.compress_many, frame.compress_many_host and their decoders are
    wrappers of these) from guarded pageable and pinned buffers."""
    import test_gpu_host_batch as HB
    import test_gpu_frame_host_batch as FHB
    own.set_option("host_batch_slice", 256 << 10)
    try:
        dirt = [d[::-1] for d in HB.inputs()] * 2

        def dirty():
            HB.run(own, True, dirt, [O.max_compress_len(len(d))
                                     for d in dirt], pinned)
            fr = FHB.framed()
            FHB.run(own, False, fr + fr, [len(d) for d in FHB.inputs()] * 2,
                    pinned)
        raw_case = host_raw_case(own, pinned)
        frame_case = host_frame_batch_case(own, pinned)
        under_fills(own, dirty,
                    lambda what: (raw_case(what), frame_case(what)))
    finally:
        own.set_option("host_batch_slice", 16 << 20)


def test_host_wrappers(own):
    """... and through the Python wrappers the issue names, once filled."""
    import test_gpu_host_batch as HB
    import test_gpu_frame_host_batch as FHB
    from rust_snappy_amd import frame, raw
    own.set_option("host_batch_slice", 256 << 10)
    try:
        def case(what):
            outs, errs = raw.compress_many(HB.inputs(), own)
            assert errs == [None] * len(outs), what
            assert outs == HB.oracle_compressed(), what
            outs, errs = raw.decompress_many(outs, own)
            assert (outs, errs) == (HB.inputs(), [None] * len(outs)), what
            fr = frame.compress_many_host(FHB.inputs(), own)
            assert fr == FHB.framed(), what
            assert frame.decompress_many_host(fr, own) == FHB.inputs(), what
        under_fills(own, lambda: raw.compress_many(
            [d[::-1] for d in HB.inputs()] * 2, own), case)
    finally:
        own.set_option("host_batch_slice", 16 << 20)


def test_host_memory_born_filled(built):
    with born_filled((("host_encode_slice", 1 << 20),
                      ("host_decode_slice_chunks", 16))) as c:
        host_frame_case(c, True)("born filled")
    with born_filled((("host_batch_slice", 256 << 10),)) as c:
        host_raw_case(c, False)("born filled")
        host_frame_batch_case(c, True)("born filled")


# ------------------------------------------------------------------------ CRC
CRC_SIZES = [0, 1, 100, 65536, 65537, 131073, 700_000, 4 << 20]
CRC_BLOCK = 4096


def crc_buffer(n):
    """(bytes, crc_ref's masked CRC32C of them).  4 KiB blocks, each a stamp
    of its number and one body of random bytes: no two segments of a buffer
    are equal, and crc_ref's bit-by-bit loop runs over a few KiB only - the
    blocks are joined by its combine()."""
    def make():
        body = random.Random(43).randbytes(CRC_BLOCK - 8)
        crc_body = crc_ref.crc32c(body)
        out, crc, k = [], crc_ref.crc32c(b""), 0
        while len(out) * CRC_BLOCK < n:
            left = n - len(out) * CRC_BLOCK
            stamp = (k + (n << 20)).to_bytes(8, "little")
            if left >= CRC_BLOCK:
                blk = stamp + body
                c = crc_ref.combine(crc_ref.crc32c(stamp), crc_body,
                                    len(body))
            else:
                blk = (stamp + body)[:left]
                c = crc_ref.crc32c(blk)
            crc = crc_ref.combine(crc, c, len(blk))
            out.append(blk)
            k += 1
        return b"".join(out), crc_ref.mask(crc)
    return memo(("crc", n), make)


def test_crc_buffer_model():
    """The joined CRC is the bit-by-bit one (a size the loop can afford)."""
    b, c = crc_buffer(3 * CRC_BLOCK + 77)
    assert c == crc_ref.crc32c_masked(b) == O.crc32c_masked(b)


def crc_case(ctx):
    from rust_snappy_amd import frame
    bufs = [crc_buffer(n) for n in CRC_SIZES]
    held = [dev(b)[:len(b)] for b, _ in bufs]

    def case(what):
        got = frame.crc32c_masked_many(ctx, held)
        assert got == [c for _, c in bufs], what
    return case


def test_crc(ctx):
    from rust_snappy_amd import frame
    other = [dev(random.Random(k).randbytes(n))
             for k, n in enumerate([3, 70000, 140000, 1_500_000, 9 << 20] * 2
                                   + [5] * 8)]
    under_fills(ctx, lambda: frame.crc32c_masked_many(ctx, other),
                crc_case(ctx))


def test_crc_born_filled(built):
    with born_filled() as c:
        crc_case(c)("born filled")


# --------------------------------------------------------------- scalar calls
SCALAR = [0, 100, 300, 5000, 200000]


def scalar_case(ctx):
    from rust_snappy_amd import raw
    enc, dec = raw.Encoder(ctx), raw.Decoder(ctx)
    datas = [text()[13:13 + n] for n in SCALAR]
    want = memo("scalar", lambda: [O.compress(d) for d in datas])

    def case(what):
        for d, w in zip(datas, want):
            assert enc.compress_vec(d) == w, (what, len(d))
            assert dec.decompress_vec(w) == d, (what, len(d))
    return case


def test_scalar_calls(built):
    import rust_snappy_amd as R
    c = R.raw.Context(0)
    try:
        enc, dec = R.raw.Encoder(c), R.raw.Decoder(c)
        big = text()[400000:800000]

        def dirty():
            assert dec.decompress_vec(enc.compress_vec(big)) == big
        under_fills(c, dirty, scalar_case(c))
    finally:
        c.close()
    with born_filled() as c:
        scalar_case(c)("born filled")
