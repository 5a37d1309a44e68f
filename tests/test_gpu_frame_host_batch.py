"""GPU suite of the host-memory frame batch calls
(snapmi_frame_compress_batch_host / snapmi_frame_decompress_batch_host,
frame.compress_many_host / decompress_many_host): stream i of a batch is
exactly what the device batch calls and the one-stream calls give for it
alone - the oracle's framed bytes, its reader's verdict and the bytes it had
delivered by then -, no stream affects another, nothing is written outside
[0, out_len) of any buffer, and a slice of well-formed streams is decoded from
the host's chunk list with the same results as by the device's walk."""
import ctypes as C
import random

import numpy as np
import pytest
import torch

import oracle_lib as O
from test_frame_host_batch_cpu import Delivered, IDENT, chunk
from test_gpu_frame_batch import assert_oracle_error
from test_gpu_host_batch import Arena, errs_of, memo, text

pytestmark = pytest.mark.gpu

OK = (0, 0, 0, 0)
BUFFER_TOO_SMALL = 2
E_ARGUMENT = 101
UNEXPECTED_EOF = 64
LENGTHS = [0, 1, 15, 16, 17, 255, 256, 1023, 8192, 65535, 65536, 65537,
           131072, 131073]
DEFAULT_SLICE = 16 << 20


def inputs():
    """The lengths at which the codec and the chunking change path, as text,
    one stream that does not compress (stored chunks) and one of five
    chunks; 1 MB."""
    def make():
        t = text()
        datas = [t[7:7 + n] for n in LENGTHS]
        datas.append(random.Random(3).randbytes(70_000))
        datas.append(t[1000:301_000])
        return datas
    return memo("fhb_inputs", make)


def framed():
    return memo("fhb_framed", lambda: [O.frame_compress(d) for d in inputs()])


def decode_pairs():
    """(framed, original): the oracle's forms of inputs() and streams with
    chunks the reader skips - skippable, padding, a repeated identifier."""
    def make():
        pairs = list(zip(framed(), inputs()))
        d = inputs()[9]
        f = framed()[9]
        pairs.append((IDENT + chunk(0x80, b"xyz") + chunk(0xFE, b"pp")
                      + f[10:] + IDENT, d))
        pairs.append((f + f, d + d))
        pairs.append((IDENT + IDENT + chunk(0xFD, b"") + chunk(0xFE, b"\0" * 40),
                      b""))
        pairs.append((f + chunk(0x99, b"q" * 5000) + framed()[13][10:],
                      d + inputs()[13]))
        return pairs
    return memo("fhb_pairs", make)


def run(ctx, compress, streams, caps, pinned=False, seed=1, lens_only=False):
    """One host frame batch call from guarded buffers: (lens, errs, bytes
    delivered per stream), after checking that exactly [0, len) of every
    output buffer changed (guard bands of 96 bytes around every buffer) and
    nothing of the inputs."""
    from rust_snappy_amd import frame
    src = Arena([len(s) for s in streams], seed, pinned, fill=streams)
    dst = Arena(caps, seed + 100, pinned)
    try:
        lens, errs = frame.batch_host(
            ctx, compress, src.ptrs, [len(s) for s in streams],
            None if lens_only else dst.ptrs, None if lens_only else caps)
        errs = errs_of(errs)
        lens = [int(x) for x in lens]
        if lens_only:
            outs = [b""] * len(streams)
        else:
            for i in range(len(streams)):
                assert lens[i] <= caps[i], i
            outs = [dst.bytes(i, lens[i]) for i in range(len(streams))]
        dst.assert_only(outs)
        src.assert_only([None] * len(streams))
        return lens, errs, outs
    finally:
        src.close()
        dst.close()


def device_decode(ctx, streams, caps):
    """snapmi_frame_decompress_batch on a device copy: (lens, errs, bytes)."""
    from rust_snappy_amd import batch, frame
    src = batch.StreamBatch.from_bytes(streams)
    dst, lens, errs = frame.decompress_many(ctx, src, caps=caps)
    return ([int(x) for x in lens], errs,
            [dst.stream_bytes(i, lens[i]) for i in range(len(streams))])


@pytest.fixture(scope="module")
def tctx(built):
    """A context of the test build, for the test options."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import rust_snappy_amd as R
    c = R.raw.Context(0)
    yield c
    c.close()


def encode_alone(ctx, d):
    from rust_snappy_amd import frame
    lens = [min(65536, len(d) - o) for o in range(0, len(d), 65536)]
    return frame.encode_host(ctx, bytearray(d), lens)


@pytest.mark.parametrize("slice_bytes", [64 << 10, DEFAULT_SLICE])
@pytest.mark.parametrize("cctx", ["product", "spans", "lanes", "small_tables",
                                  "product-lanes"], indirect=True)
def test_compress_equals_oracle_and_the_one_stream_call(cctx, slice_bytes):
    from rust_snappy_amd import frame
    datas, want = inputs(), framed()
    cctx.set_option("host_batch_slice", slice_bytes)
    caps = [frame.frame_max_len(len(d)) for d in datas]
    lens, errs, outs = run(cctx, True, datas, caps)
    if slice_bytes == 64 << 10:
        # slices end inside the list, the long stream is a slice of its own
        assert cctx.info("host_batch_slices") >= 8
    else:
        assert cctx.info("host_batch_slices") == 1
    assert cctx.info("host_batch_h2d_bytes") >= sum(len(d) for d in datas)
    for i, d in enumerate(datas):
        assert errs[i] == OK, (i, errs[i])
        assert outs[i] == want[i], (i, len(d))
        if d and slice_bytes == DEFAULT_SLICE:
            assert encode_alone(cctx, d) == outs[i], i
    assert outs[0] == b""        # no identifier for an empty input
    cctx.set_option("host_batch_slice", DEFAULT_SLICE)


@pytest.mark.parametrize("pinned", [False, True])
@pytest.mark.parametrize("pack_to_host", [0, 1])
@pytest.mark.parametrize("direct_min", [4096, 1 << 20])
def test_compress_copy_routes(tctx, pinned, pack_to_host, direct_min):
    from rust_snappy_amd import frame
    datas, want = inputs(), framed()
    tctx.set_option("host_batch_slice", 256 << 10)
    tctx.set_test_option("host_batch_pack_to_host", pack_to_host)
    tctx.set_test_option("host_batch_direct_min", direct_min)
    try:
        caps = [frame.frame_max_len(len(d)) for d in datas]
        lens, errs, outs = run(tctx, True, datas, caps, pinned=pinned, seed=5)
        assert errs == [OK] * len(datas) and outs == want
        back = run(tctx, False, want, [len(d) for d in datas], pinned=pinned,
                   seed=6)
        assert back[1] == [OK] * len(datas) and back[2] == datas
        assert tctx.info("host_batch_listed_slices") == \
            tctx.info("host_batch_slices") >= 2
    finally:
        tctx.set_test_option("host_batch_pack_to_host", 1)
        tctx.set_test_option("host_batch_direct_min", 1 << 20)
        tctx.set_option("host_batch_slice", DEFAULT_SLICE)


@pytest.mark.parametrize("slice_bytes", [64 << 10, DEFAULT_SLICE])
def test_decompress_equals_the_device_call(ctx, slice_bytes):
    pairs = decode_pairs()
    ctx.set_option("host_batch_slice", slice_bytes)
    streams = [f for f, _ in pairs]
    caps = [len(d) for _, d in pairs]
    lens, errs, outs = run(ctx, False, streams, caps, seed=2)
    # every stream is well-formed: no slice falls back to the device's walk
    slices = ctx.info("host_batch_slices")
    assert slices >= (5 if slice_bytes == 64 << 10 else 1)
    assert ctx.info("host_batch_listed_slices") == slices
    for i, (f, d) in enumerate(pairs):
        assert (errs[i], outs[i]) == (OK, d), (i, errs[i])
    assert device_decode(ctx, streams, caps) == (lens, errs, outs)
    # room to spare changes nothing
    roomy = [c + 1000 for c in caps]
    assert run(ctx, False, streams, roomy, seed=3) == (lens, errs, outs)
    ctx.set_option("host_batch_slice", DEFAULT_SLICE)


@pytest.mark.parametrize("pinned", [False, True])
def test_listed_and_walked_decode_agree(tctx, pinned):
    pairs = decode_pairs()
    streams = [f for f, _ in pairs]
    caps = [len(d) for _, d in pairs]
    res = {}
    try:
        for slice_bytes in (64 << 10, DEFAULT_SLICE):
            tctx.set_option("host_batch_slice", slice_bytes)
            for listed in (0, 1):
                tctx.set_test_option("host_batch_listed", listed)
                res[slice_bytes, listed] = run(tctx, False, streams, caps,
                                               pinned=pinned, seed=7)
                slices = tctx.info("host_batch_slices")
                assert tctx.info("host_batch_listed_slices") == \
                    (slices if listed else 0)
    finally:
        tctx.set_test_option("host_batch_listed", 1)
        tctx.set_option("host_batch_slice", DEFAULT_SLICE)
    first = res[64 << 10, 0]
    assert first[1] == [OK] * len(pairs) and first[2] == [d for _, d in pairs]
    assert all(r == first for r in res.values())


def error_batch():
    """Good streams interleaved with every way a stream can fail: (streams,
    original of a good stream or None)."""
    def make():
        t = text()
        three = t[5000:5000 + 150_000]
        f3 = O.frame_compress(three)
        hops = []
        r = 10
        while r < len(f3):
            hops.append(r)
            r += 4 + int.from_bytes(f3[r + 1:r + 4], "little")
        assert len(hops) == 3
        crc_bad = bytearray(f3)
        crc_bad[hops[1] + 4] ^= 0x55          # checksum of the second chunk
        payload_bad = bytearray(f3)
        payload_bad[hops[1] + 8 + 40] ^= 0xFF  # corrupt raw payload
        for k in range(41, 48):
            payload_bad[hops[1] + 8 + k] = 0xFF
        crc = b"\x11\x22\x33\x44"
        bad = [
            b"\xff\x06\x00\x00sNaPpX",                    # bad identifier
            b"\x00\x05\x00\x00abcde",                     # no identifier
            f3 + b"\x02\x01\x00\x00a",                    # unsupported type
            f3[:hops[1]] + b"\x00\xff\xff\xff",           # over-long chunk
            bytes(crc_bad), bytes(payload_bad),
            f3[:-5],                                      # cut-off last chunk
            IDENT + chunk(0, b"\xff\xff", crc),           # the stale-buffer
            f3 + chunk(0, b"\x80" * 6, crc),              # rule, three ways
            IDENT + chunk(0x80, b"\xbb" * 4 + b"\x01" + b"\xbb" * 5)
            + chunk(0, b"\x80" * 4, crc),
            f3 + chunk(0, b"\x81\x80\x04" + b"a" * 9, crc) + f3[10:],
        ]
        goods = inputs()
        streams, origs = [], []
        for k, s in enumerate(bad):
            g = goods[(3 * k + 5) % len(goods)]
            streams += [O.frame_compress(g), s]
            origs += [g, None]
        streams.append(framed()[10])
        origs.append(goods[10])
        return streams, origs
    return memo("fhb_errors", make)


def oracle_results():
    def make():
        D = Delivered()
        return [D(s) for s in error_batch()[0]]
    return memo("fhb_oracle", make)


@pytest.mark.parametrize("slice_bytes", [64 << 10, DEFAULT_SLICE])
def test_errors_stay_in_their_stream(ctx, slice_bytes):
    streams, origs = error_batch()
    caps = [1 << 19] * len(streams)
    ctx.set_option("host_batch_slice", slice_bytes)
    lens, errs, outs = run(ctx, False, streams, caps, seed=8)
    slices = ctx.info("host_batch_slices")
    listed = ctx.info("host_batch_listed_slices")
    kinds = set()
    for i, s in enumerate(streams):
        got, data, oe = oracle_results()[i]
        assert (lens[i], outs[i]) == (got, data), i
        if origs[i] is not None:
            assert (errs[i], outs[i]) == (OK, origs[i]), i
        else:
            assert oe is not None, i
            assert_oracle_error(errs[i], O.SnapError(*oe), s)
            kinds.add(errs[i][0])
    # StreamHeaderMismatch, StreamHeader, UnsupportedChunkType / Length,
    # Checksum, a raw decoder error, the cut-off, Header, TooBig-or-length
    assert {11, 10, 12, 13, 14, UNEXPECTED_EOF, 4} <= kinds, kinds
    assert any(origs[i] is None and lens[i] > 0 for i in range(len(streams)))
    assert device_decode(ctx, streams, caps) == (lens, errs, outs)
    # a slice that holds a malformed stream is walked by the device
    if slice_bytes == DEFAULT_SLICE:
        assert (slices, listed) == (1, 0)
    else:
        assert 0 < listed < slices
    ctx.set_option("host_batch_slice", DEFAULT_SLICE)


def test_capacity_one_short(ctx):
    from rust_snappy_amd import batch, frame
    datas, fr = inputs(), framed()
    ctx.set_option("host_batch_slice", 256 << 10)
    want = [frame.frame_max_len(len(d)) for d in datas]
    caps = [w - 1 if len(d) and i % 3 == 1 else w
            for i, (d, w) in enumerate(zip(datas, want))]
    lens, errs, outs = run(ctx, True, datas, caps, seed=9)
    short = 0
    for i, d in enumerate(datas):
        if caps[i] < want[i]:
            short += 1
            assert errs[i] == (BUFFER_TOO_SMALL, caps[i], want[i], 0), i
            assert lens[i] == 0
        else:
            assert (errs[i], outs[i]) == (OK, fr[i]), i
    assert short >= 5
    # (run() has checked that a refused stream's buffer is untouched)
    streams, origs = error_batch()
    streams = fr + streams
    full = [len(d) for d in datas] + [1 << 19] * len(origs)
    caps = [c - 1 if c and i % 3 == 1 and i < len(datas) else c
            for i, c in enumerate(full)]
    lens, errs, outs = run(ctx, False, streams, caps, seed=10)
    short = 0
    for i, d in enumerate(datas):
        if caps[i] < full[i]:
            short += 1
            assert errs[i] == (BUFFER_TOO_SMALL, caps[i], full[i], 0), i
            assert lens[i] == 0
        else:
            assert (errs[i], outs[i]) == (OK, d), i
    assert short >= 5
    assert device_decode(ctx, streams, caps) == (lens, errs, outs)
    # lengths only: the device call's lengths, on the error streams too
    hl, he, _ = run(ctx, False, streams, caps, seed=11, lens_only=True)
    src = batch.StreamBatch.from_bytes(streams)
    dl = torch.zeros(src.n, dtype=torch.int64, device="cuda")
    de = torch.zeros(32 * src.n, dtype=torch.uint8, device="cuda")
    frame.decompress_many_ptrs(ctx, src.d_ptrs, src.d_lens, None, None, dl, de)
    ctx.synchronize()
    assert hl == [int(x) for x in dl.cpu().numpy()]
    assert he == batch.read_errors(de)
    assert hl[:len(datas)] == [len(d) for d in datas]
    ctx.set_option("host_batch_slice", DEFAULT_SLICE)


def test_edges_and_reuse_of_the_context(ctx):
    from rust_snappy_amd import _lib, batch, frame, raw
    L = _lib.of(ctx)
    ctx.set_option("host_batch_slice", 64 << 10)
    datas, fr = inputs(), framed()
    calls = (L.snapmi_frame_compress_batch_host,
             L.snapmi_frame_decompress_batch_host)
    # n == 0 does nothing, whatever the pointers
    for f in calls:
        assert f(ctx._h, None, None, None, None, None, None, 0) == 0
    # NULL arguments
    src = Arena([len(datas[4])], 11, fill=[datas[4]])
    dst = Arena([64], 12)
    in_lens = np.array([len(datas[4])], dtype=np.uint64)
    out_lens = np.array([99], dtype=np.uint64)
    caps = np.array([64], dtype=np.uint64)
    null = np.zeros(1, dtype=np.uint64)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    for f in calls:
        for args in ((None, p(in_lens), p(dst.ptrs), p(caps), p(out_lens)),
                     (p(src.ptrs), None, p(dst.ptrs), p(caps), p(out_lens)),
                     (p(src.ptrs), p(in_lens), p(dst.ptrs), None, p(out_lens)),
                     (p(src.ptrs), p(in_lens), p(dst.ptrs), p(caps), None),
                     (p(null), p(in_lens), p(dst.ptrs), p(caps), p(out_lens)),
                     (p(src.ptrs), p(in_lens), p(null), p(caps), p(out_lens))):
            assert f(ctx._h, *args, None, 1) == E_ARGUMENT
    # (only decompress has a lengths-only form)
    assert calls[0](ctx._h, p(src.ptrs), p(in_lens), None, None, p(out_lens),
                    None, 1) == E_ARGUMENT
    assert out_lens[0] == 99
    dst.assert_only([None])
    src.close()
    dst.close()
    # all-empty inputs, one stream, h_errs NULL (run() passes errors; here not)
    lens, errs, outs = run(ctx, True, [b""] * 5, [0, 10, 0, 3, 0], seed=12)
    assert (lens, errs, outs) == ([0] * 5, [OK] * 5, [b""] * 5)
    lens, errs, outs = run(ctx, False, [b""] * 5, [0, 10, 0, 3, 0], seed=12)
    assert (lens, errs, outs) == ([0] * 5, [OK] * 5, [b""] * 5)
    assert run(ctx, True, [datas[12]], [frame.frame_max_len(131072)],
               seed=13)[2] == [fr[12]]
    assert run(ctx, False, [fr[12]], [131072], seed=13)[2] == [datas[12]]
    # 3 000 streams of 1 byte
    ones = [bytes([i & 255]) for i in range(3000)]
    lens, errs, outs = run(ctx, True, ones, [frame.frame_max_len(1)] * 3000,
                           seed=14)
    assert errs == [OK] * 3000
    assert outs == memo("fhb_ones", lambda: [O.frame_compress(b) for b in ones])
    lens, errs, back = run(ctx, False, outs, [1] * 3000, seed=15)
    assert errs == [OK] * 3000 and back == ones
    # one context across raw-host, frame-host and device calls in turn
    rcaps = [raw.max_compress_len(len(d)) for d in datas]
    rl, re_ = raw.batch_host(ctx, True, *host_ptrs(datas), *out_slab(rcaps))
    assert [int(e["kind"]) for e in re_] == [0] * len(datas)
    fcaps = [frame.frame_max_len(len(d)) for d in datas]
    assert run(ctx, True, datas, fcaps, seed=16)[2] == fr
    sb = batch.StreamBatch.from_bytes(datas)
    dst_b, lens_b, errs_b = frame.compress_many(ctx, sb)
    for i in range(len(datas)):
        assert errs_b[i] == OK and dst_b.stream_bytes(i, lens_b[i]) == fr[i]
    assert run(ctx, False, fr, [len(d) for d in datas], seed=17)[2] == datas
    rl2, _ = raw.batch_host(ctx, True, *host_ptrs(datas), *out_slab(rcaps))
    assert list(rl2) == list(rl)
    ctx.set_option("host_batch_slice", DEFAULT_SLICE)


_keep = []


def host_ptrs(datas):
    views = [np.frombuffer(d, dtype=np.uint8) if d else None for d in datas]
    _keep.append(views)
    return ([v.ctypes.data if v is not None else 0 for v in views],
            [len(d) for d in datas])


def out_slab(caps):
    offs = np.concatenate([[0], np.cumsum(caps)]).astype(np.uint64)
    slab = np.empty(int(offs[-1]) + 1, dtype=np.uint8)
    _keep.append(slab)
    return offs[:-1] + np.uint64(slab.ctypes.data), caps


def test_python_round_trip_and_error_display(ctx):
    import rust_snappy_amd as R
    from rust_snappy_amd import frame
    datas, fr = inputs(), framed()
    ctx.set_option("host_batch_slice", 1 << 20)
    got = frame.compress_many_host(datas, ctx)
    assert got == fr
    views = [memoryview(c) if i % 2 else bytearray(c)
             for i, c in enumerate(got)]
    assert frame.decompress_many_host(views, ctx) == datas
    lens, errs = frame.decoded_lens_host(fr, ctx)
    assert [int(x) for x in lens] == [len(d) for d in datas]
    assert not errs["kind"].any()
    streams, origs = error_batch()
    res = frame.decompress_many_host(streams, ctx, caps=[1 << 19] * len(origs))
    for i, s in enumerate(streams):
        n, data, oe = oracle_results()[i]
        if origs[i] is not None:
            assert res[i] == origs[i]
        else:
            assert isinstance(res[i], R.Error) and res[i].partial == data
    # the reference's text (src/error.rs:298-303, :327-332)
    assert res[3].display() == ("snappy: corrupt input (expected stream "
                                "header but got unexpected chunk type byte 0)")
    e = res[9]
    assert e.variant == "Checksum" and e.display() == (
        "snappy: corrupt input (bad checksum; expected: "
        f"{e.fields['expected']}, got: {e.fields['got']})")
    assert e.fields["got"] == O.crc32c_masked(
        text()[5000 + 65536:5000 + 131072])
    ctx.set_option("host_batch_slice", DEFAULT_SLICE)
