"""GPU suite of the batched frame calls (snapmi_frame_compress_batch /
snapmi_frame_decompress_batch, frame.compress_many / decompress_many): every
stream of a batch is exactly what the one-stream call gives for it alone -
bytes equal to the oracle's write::FrameEncoder, lengths, errors and the
valid prefix equal to snapmi_frame_decompress of that stream, and nothing
written outside any output buffer."""
import ctypes as C
import random

import numpy as np
import pytest
import torch

import kats
import oracle_lib as O
from test_gpu_bounds import Guarded

pytestmark = pytest.mark.gpu

IDENT = b"\xff\x06\x00\x00sNaPpY"
OK = (0, 0, 0, 0)
BUFFER_TOO_SMALL = 2
UNEXPECTED_EOF = 64          # SNAPMI_E_UNEXPECTED_EOF (the oracle says -1)
# errors that only decoding a chunk's payload brings out
DECODE_STAGE = {"HeaderMismatch", "Literal", "CopyRead", "CopyWrite", "Offset",
                "Checksum"}
CORPUS = ["html", "urls.10K", "fireworks.jpeg", "paper-100k.pdf", "html_x_4",
          "alice29.txt", "asyoulik.txt", "lcet10.txt", "plrabn12.txt",
          "geo.protodata", "kppkn.gtb", "Mark.Twain-Tom.Sawyer.txt"]


def text():
    return b"".join((O.CORPUS / n).read_bytes()
                    for n in ("alice29.txt", "lcet10.txt", "plrabn12.txt"))


def batch_inputs(seed=7):
    t = text()
    datas = [(O.CORPUS / n).read_bytes() for n in CORPUS]
    datas += [b"", b"\x00", t[:65535], t[:65536], t[:65537],
              kats.RANDOM1, kats.RANDOM2, kats.RANDOM3, kats.RANDOM4,
              b"a" * 65536, b""]
    rng = random.Random(seed)
    for k in range(10):
        n = rng.randrange(300_000)
        if k % 3 == 0:
            datas.append(rng.randbytes(n))
        else:
            o = rng.randrange(len(t) - n)
            datas.append(t[o:o + n])
    return datas


def chunk(ty, body, crc=b""):
    n = len(crc) + len(body)
    return bytes([ty, n & 255, (n >> 8) & 255, n >> 16]) + crc + body


def ptr(t):
    return C.c_void_p(t.data_ptr())


def single_decode(ctx, s, cap, lengths_only=False):
    """snapmi_frame_decompress of one stream: (length, error, bytes)."""
    from rust_snappy_amd import _lib, batch
    d_in = torch.frombuffer(bytearray(s + b"\0"), dtype=torch.uint8).cuda()
    out = torch.empty(max(cap, 16), dtype=torch.uint8, device="cuda")
    out_len = torch.zeros(1, dtype=torch.int64, device="cuda")
    err = torch.zeros(32, dtype=torch.uint8, device="cuda")
    rc = _lib.of(ctx).snapmi_frame_decompress(
        ctx._h, ptr(d_in), len(s), None if lengths_only else ptr(out), cap,
        ptr(out_len), ptr(err), None, 0)
    assert rc == 0
    ctx.synchronize()
    n = int(out_len.item())
    return n, batch.read_errors(err)[0], out[:n].cpu().numpy().tobytes()


def oracle_verdict(s):
    """(bytes, None) or (None, SnapError) of the oracle's FrameDecoder."""
    try:
        return O.frame_decompress(s, 1 << 20), None
    except O.SnapError as oe:
        return None, oe


def declared_len(s):
    """What the data chunks of a structurally sound stream say they hold: a
    stored chunk's payload, the varint in front of a compressed one."""
    pos, total = 0, 0
    while pos < len(s):
        ty, n = s[pos], int.from_bytes(s[pos + 1:pos + 4], "little")
        body = s[pos + 8:pos + 4 + n]
        if ty == 1:
            total += len(body)
        elif ty == 0:
            v = shift = 0
            for b in body:
                v |= (b & 0x7F) << shift
                shift += 7
                if b < 0x80:
                    break
            total += v
        pos += 4 + n
    return total


def assert_oracle_error(got, oe, s):
    if oe.kind == -1:
        assert got[0] == UNEXPECTED_EOF, (got, oe)
    elif O.KIND_NAMES[oe.kind] == "StreamHeaderMismatch":
        assert got[0] == oe.kind, (got, oe)   # fields: the single call's
    else:
        assert got == (oe.kind, oe.a, oe.b, oe.c), (got, oe)


@pytest.mark.parametrize("cctx", ["product", "lanes", "lanes_segmented",
                                  "spans", "small_tables", "lanes_spill",
                                  "product-lanes"], indirect=True)
def test_compress_many_bytes_equal_oracle(cctx):
    from rust_snappy_amd import batch, frame
    datas = batch_inputs()
    src = batch.StreamBatch.from_bytes(datas)
    dst, lens, errs = frame.compress_many(cctx, src)
    for i, d in enumerate(datas):
        assert errs[i] == OK, (i, errs[i])
        assert dst.stream_bytes(i, lens[i]) == O.frame_compress(d), \
            (i, len(d))


@pytest.mark.parametrize("cctx", ["lanes_segmented"], indirect=True)
def test_compress_many_segments_fall_inside_streams(cctx):
    """Segments of 64 chunks over the batch's chunk list: a segment boundary
    falls inside a stream, whose base offset comes from an earlier segment."""
    from rust_snappy_amd import batch, frame
    t = text()
    rng = random.Random(11)
    datas, chunks, inside = [], 0, 0
    while chunks < 300:
        n = rng.randrange(1, 5 * 65536)
        o = rng.randrange(len(t) - n)
        k = (n + 65535) // 65536
        inside += chunks // 64 != (chunks + k - 1) // 64
        chunks += k
        datas.append(t[o:o + n])
        if len(datas) % 7 == 3:
            datas.append(b"")
    assert inside >= 3
    src = batch.StreamBatch.from_bytes(datas)
    dst, lens, errs = frame.compress_many(cctx, src)
    for i, d in enumerate(datas):
        assert errs[i] == OK, i
        assert dst.stream_bytes(i, lens[i]) == O.frame_compress(d), i


def test_decompress_many_round_trip_equals_single_calls(ctx):
    from rust_snappy_amd import batch, frame
    datas = batch_inputs(seed=8)
    framed = [O.frame_compress(d) for d in datas]
    src = batch.StreamBatch.from_bytes(framed)
    dst, lens, errs = frame.decompress_many(ctx, src)
    for i, d in enumerate(datas):
        got = dst.stream_bytes(i, lens[i])
        assert errs[i] == OK, (i, errs[i])
        assert got == d == O.frame_decompress(framed[i]), i
        assert single_decode(ctx, framed[i], len(d)) == \
            (int(lens[i]), errs[i], got), i


def error_streams():
    """Every stream of test_frame_decoder_errors and the short-varint streams
    of test_frame_short_varint_reads_the_stale_scratch_buffer, plus errors
    behind good chunks (a valid prefix)."""
    html = (O.CORPUS / "html").read_bytes()
    good = O.frame_compress(html)
    out = [b"123", b"\x00\x05\x00\x00abcde", b"\xff\x06\x00\x00sNaPpX",
           b"\xff\x05\x00\x00sNaPp", IDENT + b"\x02\x01\x00\x00a",
           IDENT + b"\x00\xff\xff\xff", IDENT + b"\x00\x03\x00\x00abc"]
    bad = bytearray(good)
    bad[10 + 4] ^= 0x55
    out.append(bytes(bad))                              # checksum
    bad = bytearray(good)
    bad[10 + 8 + 3 + 5] ^= 0xFF
    out.append(bytes(bad))                              # corrupt payload
    rng = random.Random(5)
    for _ in range(12):
        bad = bytearray(good)
        bad[10 + 8 + rng.randrange(3, 2000)] ^= 1 << rng.randrange(8)
        out.append(bytes(bad))
    out.append(good[:-5])                               # truncated
    # skippable, padding and a repeated identifier are skipped
    out.append(IDENT + b"\x80\x03\x00\x00xyz" + b"\xfe\x02\x00\x00pp"
               + good[10:] + IDENT)
    out.append(good + good[10:])
    # errors behind good chunks: the bytes in front are the stream's output
    out.append(good + good[10:40])
    out.append(good + b"\x02\x01\x00\x00a")
    out.append(good + b"\xff\x06\x00\x00sNaPpZ")
    crc = b"\x11\x22\x33\x44"
    skip = lambda body: chunk(0x80, body)  # noqa: E731
    out += [
        IDENT + chunk(0, b"\xff\xff", crc),
        IDENT + chunk(0, b"", crc),
        IDENT + skip(b"\xaa" * 5 + b"\x7f" + b"\xaa" * 4)
        + chunk(0, b"\xff" * 5, crc),
        IDENT + skip(b"\xbb" * 4 + b"\x01" + b"\xbb" * 5)
        + chunk(0, b"\x80" * 4, crc),
        good + chunk(0, b"\x80" * 6, crc),
        IDENT + skip(b"\xcc" * 10) + chunk(0, b"\x80" * 4, crc),
        IDENT + skip(b"\xdd" * 5 + b"\x03" + b"\xdd" * 4)
        + chunk(1, b"x" * 20, O.crc32c_masked(b"x" * 20).to_bytes(4, "little"))
        + chunk(0, b"\x80" * 5, crc),
    ]
    return out


def mixed_batch():
    """error streams interleaved with good ones: (streams, originals of the
    good ones or None)"""
    goods = [(O.CORPUS / n).read_bytes()[:90000] for n in CORPUS]
    streams, origs = [], []
    for k, s in enumerate(error_streams()):
        g = goods[k % len(goods)]
        streams += [O.frame_compress(g), s]
        origs += [g, None]
    return streams, origs


def test_errors_stay_in_their_stream(ctx):
    from rust_snappy_amd import batch, frame
    streams, origs = mixed_batch()
    cap = 1 << 18
    src = batch.StreamBatch.from_bytes(streams)
    dst, lens, errs = frame.decompress_many(ctx, src, caps=[cap] * len(streams))
    kinds = set()
    for i, s in enumerate(streams):
        got = dst.stream_bytes(i, lens[i])
        assert single_decode(ctx, s, cap) == (int(lens[i]), errs[i], got), i
        want, oe = oracle_verdict(s)
        if origs[i] is not None:
            assert (errs[i], got) == (OK, origs[i]), i
        elif oe is None:
            assert (errs[i], got) == (OK, want), i
        else:
            assert_oracle_error(errs[i], oe, s)
            kinds.add(errs[i][0])
    # every kind the list is made of (Header, Empty, TooBig, Checksum, ...)
    assert {3, 4, 1, 10, 11, 12, 13, 14, UNEXPECTED_EOF} <= kinds, kinds
    # some failing streams deliver the good chunks in front of the error
    assert any(origs[i] is None and errs[i] != OK and lens[i] > 0
               for i in range(len(streams)))


def test_lengths_only_equals_single_calls(ctx):
    from rust_snappy_amd import batch, frame
    streams, origs = mixed_batch()
    src = batch.StreamBatch.from_bytes(streams)
    lens = torch.zeros(src.n, dtype=torch.int64, device="cuda")
    errs = torch.zeros(32 * src.n, dtype=torch.uint8, device="cuda")
    frame.decompress_many_ptrs(ctx, src.d_ptrs, src.d_lens, None, None, lens,
                               errs)
    ctx.synchronize()
    lens, errs = lens.cpu().numpy(), batch.read_errors(errs)
    for i, s in enumerate(streams):
        n, e, _ = single_decode(ctx, s, 0, lengths_only=True)
        assert (int(lens[i]), errs[i]) == (n, e), i
        if origs[i] is not None:
            assert (int(lens[i]), errs[i]) == (len(origs[i]), OK)
        # the oracle's verdict, as far as a call that decodes nothing can
        # reach it: what the raw decoder or a checksum would find stays unseen
        # (every stream here has one defect at the most)
        want, oe = oracle_verdict(s)
        if oe is None:
            assert (int(lens[i]), errs[i]) == (len(want), OK), i
        elif errs[i] != OK:
            assert_oracle_error(errs[i], oe, s)
        else:
            assert O.KIND_NAMES[oe.kind] in DECODE_STAGE, (i, oe)
            assert int(lens[i]) == declared_len(s), i


@pytest.mark.parametrize("aligned", [True, False])
def test_compress_cap_one_short_and_guards(ctx, aligned):
    from rust_snappy_amd import batch, frame
    datas = batch_inputs(seed=9)
    want = [frame.frame_max_len(len(d)) for d in datas]
    caps = [w - 1 if len(d) and i % 3 == 1 else w
            for i, (d, w) in enumerate(zip(datas, want))]
    gin = Guarded([len(d) for d in datas], seed=1, aligned=False, fill=datas)
    gout = Guarded(caps, seed=2, aligned=aligned)
    before = gout.fetch().copy()
    n = len(datas)
    lens = torch.zeros(n, dtype=torch.int64, device="cuda")
    errs = torch.zeros(32 * n, dtype=torch.uint8, device="cuda")
    # (no host copy of the lengths: the blocking fetch)
    frame.compress_many_ptrs(ctx, gin.d_ptrs, gin.d_caps, gout.d_ptrs,
                             gout.d_caps, lens, errs)
    ctx.synchronize()
    gout.assert_guards("frame compress batch")
    lens, errs = lens.cpu().numpy(), batch.read_errors(errs)
    refused = 0
    for i, d in enumerate(datas):
        o = int(gout.offs[i])
        if caps[i] < want[i]:
            refused += 1
            assert errs[i] == (BUFFER_TOO_SMALL, caps[i], want[i], 0), i
            assert lens[i] == 0
            assert (gout.host[o:o + caps[i]] == before[o:o + caps[i]]).all()
        else:
            assert errs[i] == OK, i
            assert gout.bytes(i, lens[i]) == O.frame_compress(d), i
    assert refused >= 5


@pytest.mark.parametrize("aligned", [True, False])
def test_decompress_cap_one_short_and_guards(ctx, aligned):
    from rust_snappy_amd import batch, frame
    datas = batch_inputs(seed=10)
    streams = [O.frame_compress(d) for d in datas]
    caps = [len(d) - 1 if len(d) and i % 3 == 1 else len(d)
            for i, d in enumerate(datas)]
    bad, _ = mixed_batch()
    streams += bad
    caps += [1 << 18] * len(bad)
    gin = Guarded([len(s) for s in streams], seed=3, aligned=False,
                  fill=streams)
    gout = Guarded(caps, seed=4, aligned=aligned)
    before = gout.fetch().copy()
    n = len(streams)
    lens = torch.zeros(n, dtype=torch.int64, device="cuda")
    errs = torch.zeros(32 * n, dtype=torch.uint8, device="cuda")
    frame.decompress_many_ptrs(ctx, gin.d_ptrs, gin.d_caps, gout.d_ptrs,
                               gout.d_caps, lens, errs)
    ctx.synchronize()
    gout.assert_guards("frame decompress batch")
    lens, errs = lens.cpu().numpy(), batch.read_errors(errs)
    short = 0
    for i, s in enumerate(streams):
        got = gout.bytes(i, lens[i])
        if i < len(datas) and caps[i] < len(datas[i]):
            short += 1
            o = int(gout.offs[i])
            assert errs[i] == (BUFFER_TOO_SMALL, caps[i], len(datas[i]), 0)
            assert lens[i] == 0
            assert (gout.host[o:o + caps[i]] == before[o:o + caps[i]]).all()
        elif i < len(datas):
            assert (errs[i], got) == (OK, datas[i]), i
        else:
            want, oe = oracle_verdict(s)
            if oe is None:
                assert (errs[i], got) == (OK, want), i
            else:
                assert_oracle_error(errs[i], oe, s)
        assert single_decode(ctx, s, caps[i]) == (int(lens[i]), errs[i], got)
    assert short >= 5


def test_shapes(ctx):
    from rust_snappy_amd import batch, frame
    # n = 0: nothing to do, nothing enqueued
    e = torch.zeros(0, dtype=torch.int64, device="cuda")
    frame.compress_many_ptrs(ctx, e, e, e, e, e, None,
                             host_in_lens=torch.zeros(0, dtype=torch.int64))
    frame.decompress_many_ptrs(ctx, e, e, e, e, e, None)
    ctx.synchronize()
    # n = 1
    html = (O.CORPUS / "html").read_bytes()
    dst, lens, errs = frame.compress_many(
        ctx, batch.StreamBatch.from_bytes([html]))
    f = dst.stream_bytes(0, lens[0])
    assert errs == [OK] and f == O.frame_compress(html)
    back, blens, berrs = frame.decompress_many(
        ctx, batch.StreamBatch.from_bytes([f]))
    assert berrs == [OK] and back.stream_bytes(0, blens[0]) == html
    # 10 000 streams of 200 bytes to 4 KiB in one call each way
    t = text()
    rng = random.Random(12)
    datas = []
    for _ in range(10_000):
        n = rng.randrange(200, 4097)
        o = rng.randrange(len(t) - n)
        datas.append(t[o:o + n])
    dst, lens, errs = frame.compress_many(ctx, batch.StreamBatch.from_bytes(
        datas))
    assert all(e == OK for e in errs)
    framed = [dst.stream_bytes(i, lens[i]) for i in range(len(datas))]
    assert framed == [O.frame_compress(d) for d in datas]
    back, blens, berrs = frame.decompress_many(
        ctx, batch.StreamBatch.from_bytes(framed))
    assert all(e == OK for e in berrs)
    assert np.array_equal(blens, [len(d) for d in datas])
    host = back.data.cpu().numpy()
    for i, d in enumerate(datas):
        o = int(back.offsets[i])
        assert host[o:o + len(d)].tobytes() == d, i
