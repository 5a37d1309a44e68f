"""The no-wait framed decode on the GPU: snapmi_frame_decompress_ex with
SNAPMI_FRAME_NO_WAIT (include/snapmi.h).  The caller bounds the data chunks,
the call only enqueues, and while the bound holds the length, the error and
the bytes are those of the same call without the flag - whatever the side
index contains, however generous the bound.  Every flagged call here is
compared with the unflagged call on a second context and, where the stream is
valid, with the oracle; outputs lie between guard bands."""
import ctypes as C
import math
import random
import struct
import time

import numpy as np
import pytest
import torch

import oracle_lib as O
from gpu_buffers import Slab, read_errs, u64
from test_gpu_stream_order import (HOLD_FLOOR_MS, hold, make_context,
                                   sleep_rate)

pytestmark = pytest.mark.gpu

NO_WAIT, CONTINUATION = 4, 1
OK = (0, 0, 0, 0)
E_ARGUMENT, UNEXPECTED_EOF, BUFFER_TOO_SMALL = 101, 64, 2
INDEX, PARALLEL, WALK, EXCEEDED = 1, 2, 3, 4
IDENT = b"\xff\x06\x00\x00sNaPpY"
SIZES = [0, 1, 65535, 65536, 65537, 131077, 200000]
KINDS = ("text", "zeros", "noise")

_TEXT = []


def data(kind, n, salt=0):
    if kind == "zeros":
        return bytes(n)
    if kind == "noise":
        return random.Random(1000 * salt + n).randbytes(n)
    if not _TEXT:
        _TEXT.append((O.CORPUS / "alice29.txt").read_bytes()
                     + (O.CORPUS / "asyoulik.txt").read_bytes())
    t = _TEXT[0]
    o = (7919 * salt) % 1000
    return (t[o:] * (n // len(t) + 2))[:n]


def chunk(ty, body, crc=b""):
    n = len(crc) + len(body)
    return bytes([ty, n & 255, (n >> 8) & 255, n >> 16]) + crc + body


def chunk_offsets(s, continuation=False):
    """Header offsets of the data chunks of a well-formed stream."""
    r, out = 0, []
    while r < len(s):
        ty, n = s[r], int.from_bytes(s[r + 1:r + 4], "little")
        if ty <= 1:
            out.append(r)
        r += 4 + n
    assert r == len(s)
    return out


def with_foreign_chunks(f):
    """A skippable chunk, a padding chunk and a repeated identifier between
    the data chunks of f (the construction of test_frame_index_host)."""
    offs = chunk_offsets(f) + [len(f)]
    first = offs[1] - offs[0]
    return (f[:10] + bytes([0x80, 3, 0, 0, 1, 2, 3]) + f[10:10 + first]
            + bytes([0xFE, 2, 0, 0, 9, 9]) + f[:10] + f[10 + first:])


# --------------------------------------------------------------- the harness
class Bufs:
    """One decode's device buffers: the stream, an output of exactly `cap`
    bytes between guard bands, the length and the error record."""

    def __init__(self, s, cap, seed=0, room=None):
        self.cap = int(cap)
        self.d_in = torch.zeros(max(room or len(s), 1), dtype=torch.uint8,
                                device="cuda")
        self.load(s)
        self.slab = Slab([self.cap], seed)
        o = int(self.slab.offs[0])
        self.out = self.slab.data[o:o + self.cap]
        self.out_len = torch.full((1,), -7, dtype=torch.int64, device="cuda")
        self.err = torch.full((32,), 0xEE, dtype=torch.uint8, device="cuda")

    def load(self, s):
        self.s = bytes(s)
        if len(s):
            self.d_in[:len(s)].copy_(torch.frombuffer(bytearray(s),
                                                      dtype=torch.uint8))

    def reset(self):
        self.slab.refill()
        self.out_len.fill_(-7)
        self.err.fill_(0xEE)

    def result(self, what, has_out=True):
        """(length, error, bytes) behind a wait; the bands are clean."""
        self.slab.assert_guards(what)
        n = int(self.out_len.item())
        e = read_errs(self.err)[0]
        got = self.slab.bytes(0, n) if has_out else None
        if not has_out:  # lengths only: nothing at all is written
            assert self.slab.bytes(0, self.cap) == bytes([0xA5]) * self.cap
        return n, e, got


def call(ctx, b, n_chunks, index=None, flags=0, stale=None, has_out=True,
         cap=None):
    """snapmi_frame_decompress_ex as it is; returns the status."""
    st = (C.c_uint8 * 10)(*stale) if stale is not None else None
    return ctx._L.snapmi_frame_decompress_ex(
        ctx._h, C.c_void_p(b.d_in.data_ptr()) if len(b.s) else None,
        len(b.s), C.c_void_p(b.out.data_ptr()) if has_out else None,
        b.cap if cap is None else cap, C.c_void_p(b.out_len.data_ptr()),
        C.c_void_p(b.err.data_ptr()),
        C.c_void_p(index.data_ptr()) if index is not None else None,
        int(n_chunks), flags, st)


class Pair:
    """The context under test and a second one for the unflagged call, both
    on one torch stream (so torch's copies are ordered with the calls)."""

    def __init__(self, library):
        self.S = torch.cuda.Stream()
        self.ctx = make_context(library, self.S)
        self.second = make_context(library, self.S)
        self._ref = {}

    def close(self):
        self.ctx.close()
        self.second.close()

    def reference(self, s, cap, flags=0, stale=None, has_out=True):
        """The unflagged call without an index (an index never changes its
        result), once per stream and capacity."""
        key = (s, cap, flags, bytes(stale or b""), has_out)
        if key not in self._ref:
            b = Bufs(s, cap, 5)
            assert call(self.second, b, 0, None, flags, stale, has_out) == 0
            self.S.synchronize()
            self._ref[key] = b.result("unflagged", has_out)
        return self._ref[key]

    def flagged(self, s, cap, bound, index=None, flags=0, stale=None,
                has_out=True, seed=1, ctx=None):
        """One flagged call: (length, error, bytes, front)."""
        ctx = ctx or self.ctx
        b = Bufs(s, cap, seed)
        idx = u64(index) if index is not None else None
        if idx is not None:
            assert idx.numel() == bound + 1
        rc = call(ctx, b, bound, idx, flags | NO_WAIT, stale, has_out)
        assert rc == 0, (rc, bound)
        self.S.synchronize()
        n, e, got = b.result(f"flagged, bound {bound}", has_out)
        return n, e, got, ctx.info("frame_nowait_front")

    def same(self, s, cap, bound, index=None, front=None, **kw):
        """The flagged call gives what the unflagged one gives."""
        want = self.reference(s, cap, kw.get("flags", 0), kw.get("stale"),
                              kw.get("has_out", True))
        got = self.flagged(s, cap, bound, index, **kw)
        assert got[:3] == want, (bound, got[:2], want[:2], got[3])
        if front is not None:
            assert got[3] == front, (bound, got[3], front)
        return got


@pytest.fixture(scope="module", params=["test", "product"])
def pair(request, built):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    p = Pair(request.param)
    with torch.cuda.stream(p.S):
        yield p
    p.close()


_FRAMED = {}


def framed(kind, n):
    if (kind, n) not in _FRAMED:
        d = data(kind, n)
        _FRAMED[kind, n] = (d, O.frame_compress(d))
    return _FRAMED[kind, n]


# ------------------------------------------------------------------ streams
def test_info_before_the_first_flagged_call(built):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import rust_snappy_amd as R
    for lib in (None, R._lib.load_product()):
        c = R.raw.Context(0, lib=lib)
        assert c.info("frame_nowait_front") == -1
        c.close()


@pytest.mark.parametrize("kind", KINDS)
def test_valid_streams_bound_and_index(pair, kind):
    """Every size: index with the exact count (front 1), no index with the
    exact bound and with 1, 5 and 1000 to spare (front 3: these streams are
    shorter than frame_parallel_walk_min)."""
    for n in SIZES:
        d, f = framed(kind, n)
        offs = chunk_offsets(f)
        exact = len(offs)
        assert exact == (n + 65535) // 65536
        assert pair.reference(f, n) == (n, OK, d)
        pair.same(f, n, exact, offs + [len(f)],
                  front=INDEX if f else WALK)  # (b"": no identifier)
        for spare in (0, 1, 5, 1000):
            pair.same(f, n, exact + spare, None, front=WALK)
        # an index padded to a generous bound does not tile: the walk
        pair.same(f, n, exact + 5, offs + [len(f)] * 6, front=WALK)


def test_no_chunks_at_all(pair):
    for s, flags, front in ((b"", 0, WALK), (IDENT, 0, INDEX),
                            (b"", CONTINUATION, INDEX)):
        assert pair.reference(s, 0, flags) == (0, OK, b"")
        pair.same(s, 0, 0, None, front=WALK, flags=flags)
        pair.same(s, 0, 0, [len(s)], front=front, flags=flags)
        pair.same(s, 0, 7, None, front=WALK, flags=flags)


@pytest.mark.parametrize("piece", [1, 17, 300, 65536])
def test_streams_cut_by_the_caller(pair, piece):
    """snapmi_frame_compress_chunks: chunks of 1, 17, 300 and 65536 bytes."""
    from rust_snappy_amd import frame
    n = {1: 700, 17: 5000, 300: 40000, 65536: 200000}[piece]
    d = data("text", n, 3)
    lens = [piece] * (n // piece) + ([n % piece] if n % piece else [])
    d_in = torch.frombuffer(bytearray(d), dtype=torch.uint8).cuda()
    out, flen = frame.compress_chunks_device(pair.second, d_in, lens)
    f = out[:flen].cpu().numpy().tobytes()
    assert O.frame_decompress(f) == d
    offs = chunk_offsets(f)
    exact = len(offs)
    assert exact == len(lens)
    assert pair.reference(f, n) == (n, OK, d)
    pair.same(f, n, exact, offs + [len(f)], front=INDEX)
    for spare in (0, 1, 5, 1000):
        pair.same(f, n, exact + spare, None, front=WALK)


def test_foreign_chunks_between_data_chunks(pair):
    """The data chunk offsets of frame.index_host do not tile such a stream:
    the sequential walk decides and the result is still exact."""
    from rust_snappy_amd import frame
    d, f = framed("text", 200000)
    g = with_foreign_chunks(f)
    assert O.frame_decompress(g) == d
    idx = [int(x) for x in frame.index_host(g)]
    assert idx[:-1] == chunk_offsets(g) and len(idx) == 5
    assert pair.reference(g, len(d)) == (len(d), OK, d)
    pair.same(g, len(d), 4, idx, front=WALK)
    for spare in (0, 1, 5, 1000):
        pair.same(g, len(d), 4 + spare, None, front=WALK)


HOSTILE = ["beyond", "wraps", "equal", "descending", "last_short", "payload"]


@pytest.mark.parametrize("how", HOSTILE)
def test_hostile_indexes(pair, how):
    d, f = framed("text", 200000)
    e = chunk_offsets(f) + [len(f)]
    idx = {"beyond": [e[0], len(f) + 1000] + e[2:],
           "wraps": [e[0], 2**64 - 8] + e[2:],
           "equal": [e[0]] * 5,
           "descending": e[::-1],
           "last_short": e[:-1] + [e[-1] - 1],
           "payload": [e[0]] + [x + 1 for x in e[1:-1]] + [e[-1]]}[how]
    got = pair.same(f, len(d), 4, idx, front=WALK)
    assert got[:3] == (len(d), OK, d)


# ----------------------------------------------------------- broken promise
def test_broken_promise(pair):
    d, f = framed("text", 200000)
    e = chunk_offsets(f) + [len(f)]
    d1, f1 = framed("text", 1)
    cases = [(f, len(d), 3, None, 4), (f, len(d), 3, e[:4], 4),
             (f1, 1, 0, None, 1), (f1, 1, 0, [10], 1),
             (f, len(d), 0, None, 4),
             # the promise counts data chunks in front of the first error
             (f[:-5], len(d), 2, None, 3)]
    for s, cap, bound, idx, found in cases:
        n, err, got, front = pair.flagged(s, cap, bound, idx)
        assert (n, err, front) == (0, (E_ARGUMENT, found, bound, 0),
                                   EXCEEDED), (bound, idx)
        n, err, got, front = pair.flagged(s, cap, bound, idx, has_out=False)
        assert (n, err, front) == (0, (E_ARGUMENT, found, bound, 0), EXCEEDED)
    # the bound itself: at most 2^31 - 1, and nothing is enqueued
    b = Bufs(f, len(d), 2)
    pair.S.synchronize()
    assert call(pair.ctx, b, 1 << 31, None, NO_WAIT) == E_ARGUMENT
    assert call(pair.ctx, b, 4, None, NO_WAIT | 2) == E_ARGUMENT
    pair.S.synchronize()
    b.slab.assert_guards("refused")
    assert b.slab.bytes(0, b.cap) == bytes([0xA5]) * b.cap
    assert int(b.out_len.item()) == -7
    assert b.err.cpu().tolist() == [0xEE] * 32


# ------------------------------------------------------ errors of the stream
def error_streams():
    d, f = framed("text", 200000)
    e = chunk_offsets(f) + [len(f)]
    out = {}
    for name, k in (("payload0", 0), ("payload_mid", 2), ("payload_last", 3)):
        b = bytearray(f)
        b[e[k] + 8 + 40] ^= 0x5A
        out[name] = bytes(b)
    b = bytearray(f)
    b[e[2] + 5] ^= 0x01
    out["crc"] = bytes(b)
    out["cut_header"] = f[:e[3] + 2]
    out["cut_payload"] = f[:-5]
    out["type02"] = f[:e[2]] + b"\x02\x01\x00\x00a" + f[e[2]:]
    out["identifier"] = f[:4] + b"sNaPpX" + f[10:]
    return d, f, e, out


def test_stream_errors_under_a_generous_bound(pair):
    d, f, e, streams = error_streams()
    kinds = set()
    for name, s in streams.items():
        want = pair.reference(s, len(d))
        assert want[1][0] != 0, name
        kinds.add(want[1][0])
        with pytest.raises(O.SnapError):
            O.frame_decompress(s)
        got = pair.same(s, len(d), 4 + 5, None, front=WALK)
        # the bytes in front of the failing chunk are delivered
        assert got[2] == d[:got[0]] and got[0] % 65536 == 0, name
        if name.startswith("payload") or name == "crc":
            pair.same(s, len(d), 4, e, front=INDEX)
    assert streams["payload_mid"] and pair.reference(
        streams["payload_mid"], len(d))[0] == 131072
    assert pair.reference(streams["payload0"], len(d))[0] == 0
    assert pair.reference(streams["payload_last"], len(d))[0] == 196608
    assert pair.reference(streams["cut_header"], len(d))[1][0] == \
        UNEXPECTED_EOF
    assert pair.reference(streams["cut_payload"], len(d))[1][0] == \
        UNEXPECTED_EOF
    assert len(kinds) >= 4


def test_capacity_null_output_and_continuation(pair):
    d, f = framed("text", 200000)
    e = chunk_offsets(f) + [len(f)]
    n = len(d)
    # one byte short: BufferTooSmall {cap, total}, nothing written
    want = pair.reference(f, n - 1)
    assert want == (0, (BUFFER_TOO_SMALL, n - 1, n, 0), b"")
    for bound, idx in ((4, e), (4, None), (9, None)):
        got = pair.flagged(f, n - 1, bound, idx)
        assert got[:3] == want
        b = Bufs(f, n - 1, 3)
        assert call(pair.ctx, b, bound, u64(idx) if idx else None,
                    NO_WAIT) == 0
        pair.S.synchronize()
        b.slab.assert_guards("too small")
        assert b.slab.bytes(0, n - 1) == bytes([0xA5]) * (n - 1)
    # d_out == NULL: lengths only
    assert pair.reference(f, 0, has_out=False)[:2] == (n, OK)
    for bound, idx, front in ((4, e, INDEX), (4, None, WALK), (9, None, WALK)):
        pair.same(f, 0, bound, idx, front=front, has_out=False)
    bad = bytearray(f)
    bad[e[2] + 8 + 40] ^= 0x5A   # (lengths only: the payload is not decoded)
    pair.same(bytes(bad), 0, 9, None, front=WALK, has_out=False)
    pair.same(f[:-5], 0, 9, None, front=WALK, has_out=False)
    # a later batch of a stream: no identifier in front
    body = f[10:]
    eb = [x - 10 for x in e]
    assert pair.reference(body, n, CONTINUATION) == (n, OK, d)
    pair.same(body, n, 4, eb, front=INDEX, flags=CONTINUATION)
    pair.same(body, n, 9, None, front=WALK, flags=CONTINUATION)
    # ... and without the flag it is a StreamHeader error, in both modes
    assert pair.reference(body, n)[1][0] != 0
    pair.same(body, n, 4, eb, front=WALK)
    pair.same(body, n, 9, None, front=WALK)


def test_short_varint_and_stale_bytes(pair):
    """The streams of test_frame_short_varint_reads_the_stale_scratch_buffer:
    a compressed payload without a varint terminator is judged together with
    the reference reader's scratch buffer, by the sequential walk - with an
    index or without, with the stale bytes of an earlier batch or without."""
    from rust_snappy_amd import frame
    html = (O.CORPUS / "html").read_bytes()
    good = O.frame_compress(html)[10:]
    crc = b"\x11\x22\x33\x44"
    skip = lambda body: chunk(0x80, body)  # noqa: E731
    streams = {
        "hdr": IDENT + chunk(0, b"\xff\xff", crc),
        "empty": IDENT + chunk(0, b"", crc),
        "toobig": IDENT + skip(b"\xaa" * 5 + b"\x7f" + b"\xaa" * 4)
                  + chunk(0, b"\xff" * 5, crc),
        "len": IDENT + skip(b"\xbb" * 4 + b"\x01" + b"\xbb" * 5)
               + chunk(0, b"\x80" * 4, crc),
        "after_data": IDENT + good + chunk(0, b"\x80" * 6, crc),
        "never": IDENT + skip(b"\xcc" * 10) + chunk(0, b"\x80" * 4, crc),
        "stored_between": IDENT + skip(b"\xdd" * 5 + b"\x03" + b"\xdd" * 4)
                          + chunk(1, b"x" * 20, struct.pack(
                              "<I", O.crc32c_masked(b"x" * 20)))
                          + chunk(0, b"\x80" * 5, crc),
    }
    cap = len(html) + 64
    seen = set()
    for name, s in streams.items():
        with pytest.raises(O.SnapError) as oe:
            O.frame_decompress(s)
        want = pair.reference(s, cap)
        assert oe.value.kind >= 0 and want[1] == (
            oe.value.kind, oe.value.a, oe.value.b, oe.value.c), name
        seen.add(oe.value.name)
        offs = chunk_offsets(s)   # every data chunk, the short one included
        pair.same(s, cap, len(offs) + 5, None, front=WALK)
        pair.same(s, cap, len(offs), offs + [len(s)], front=WALK)
        _, _, scan = frame.scan_host(s)
        scan = [int(x) for x in scan]
        pair.same(s, cap, len(scan) - 1, scan, front=WALK)
    assert seen == {"Header", "Empty", "TooBig", "UnsupportedChunkLength"}
    assert pair.reference(streams["after_data"], cap)[2] == html
    # the short chunk alone, as a later batch: the stale bytes decide
    s = chunk(0, b"\x80" * 4, crc)
    for stale in (bytes(10), b"\xbb" * 4 + b"\x01" + b"\xbb" * 5,
                  b"\xcc" * 10, b"\xaa" * 4 + b"\x7f" + b"\xaa" * 5):
        want = pair.reference(s, 64, CONTINUATION, stale)
        assert want[1][0] != 0
        pair.same(s, 64, 1, None, front=WALK, flags=CONTINUATION, stale=stale)
        pair.same(s, 64, 1, [0, len(s)], front=WALK, flags=CONTINUATION,
                  stale=stale)
    kinds = {pair.reference(s, 64, CONTINUATION, st)[1][0]
             for st in (bytes(10), b"\xbb" * 4 + b"\x01" + b"\xbb" * 5)}
    assert len(kinds) == 2


# ------------------------------------------------------- the parallel front
def test_parallel_front(built):
    """frame_parallel_walk_min 0 and segments of 128 KiB (test option): a
    text stream of four segments is decided by the parallel walk, exact bound
    or generous; a header the reader rejects in the second segment hands it
    to the sequential walk; a bound one short is a broken promise."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    p = Pair("test")
    try:
        with torch.cuda.stream(p.S):
            p.ctx.set_option("frame_parallel_walk_min", 0)
            p.ctx.set_test_option("frame_walk_segment", 128 << 10)
            d = data("text", 800000, 2)
            f = O.frame_compress(d)
            seg = 128 << 10
            assert len(f) > 3 * seg
            e = chunk_offsets(f) + [len(f)]
            exact = len(e) - 1
            assert p.reference(f, len(d)) == (len(d), OK, d)
            p.same(f, len(d), exact, None, front=PARALLEL)
            p.same(f, len(d), exact + 5, None, front=PARALLEL)
            p.same(f, len(d), exact, None, front=PARALLEL, has_out=False)
            # with an index the parallel walk is not enqueued
            p.same(f, len(d), exact, e, front=INDEX)
            k = next(i for i, x in enumerate(e) if seg <= x < 2 * seg)
            bad = bytearray(f)
            bad[e[k]] = 0x05
            bad = bytes(bad)
            want = p.reference(bad, len(d))
            assert want[1][0] != 0 and want[0] == 65536 * k
            got = p.same(bad, len(d), exact, None, front=WALK)
            assert got[2] == d[:65536 * k]
            p.same(f[:-3], len(d), exact + 5, None, front=WALK)
            g = with_foreign_chunks(f)
            assert p.reference(g, len(d)) == (len(d), OK, d)
            p.same(g, len(d), exact, None, front=PARALLEL)
            for bound in (exact - 1, 0):
                n, err, _, front = p.flagged(f, len(d), bound, None)
                assert (n, err, front) == (
                    0, (E_ARGUMENT, exact, bound, 0), EXCEEDED)
            # ... and behind it the same context decodes on
            p.same(f, len(d), exact, None, front=PARALLEL)
    finally:
        p.close()


# ------------------------------------------------------------------ no wait
@pytest.mark.parametrize("library", ["test", "product"])
def test_flagged_calls_return_while_the_stream_is_held(built, library):
    """Four flagged decodes - with the index, without, one whose index sends
    it to the walk, one whose bound is exceeded - are enqueued behind a hold
    of the stream: all four return, S.query() is still False behind the last,
    and the results are right after the single wait.  The scratch is warm
    (the same calls ran before).  The hold is 20x the slowest of three idle
    enqueues of the four, at least HOLD_FLOOR_MS."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    p = Pair(library)
    S = p.S
    d, f = framed("text", 200000)
    e = chunk_offsets(f) + [len(f)]
    plans = [(4, e), (9, None), (4, [e[0]] + [x + 1 for x in e[1:-1]]
                                 + [e[-1]]), (3, None)]
    try:
        with torch.cuda.stream(S):
            rate = sleep_rate(S)
            want = p.reference(f, len(d))
            assert want == (len(d), OK, d)
            idx = [u64(i) if i else None for _, i in plans]

            def four(seed):
                bufs = [Bufs(f, len(d), seed + k) for k in range(4)]
                S.synchronize()
                return bufs

            def enqueue(bufs):
                t0 = time.perf_counter()
                for b, (bound, _), i in zip(bufs, plans, idx):
                    assert call(p.ctx, b, bound, i, NO_WAIT) == 0
                return (time.perf_counter() - t0) * 1e3

            def check(bufs, what):
                S.synchronize()
                for k in range(3):
                    assert bufs[k].result(what) == want, (what, k)
                assert bufs[3].result(what)[:2] == (
                    0, (E_ARGUMENT, 4, 3, 0)), what
                assert p.ctx.info("frame_nowait_front") == EXCEEDED

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
            print(f"\n[{library}] four flagged enqueues idle {idle_ms:.3f} "
                  f"ms, held {held_ms:.3f} ms; hold asked {hold_ms:.0f} ms, "
                  f"lasted {lasted:.0f} ms")
            assert lasted >= 20 * idle_ms, (lasted, idle_ms)
            assert busy, (idle_ms, held_ms, hold_ms, lasted)
    finally:
        p.close()


# -------------------------------------------------------------------- graphs
def padded_to(f, length):
    """f with trailing padding chunks, `length` bytes in all."""
    gap = length - len(f)
    assert gap >= 4
    out = bytearray(f)
    while gap:
        take = min(gap, 60004)
        if 0 < gap - take < 4:
            take -= 4
        out += bytes([0xFE]) + (take - 4).to_bytes(3, "little") + bytes(
            take - 4)
        gap -= take
    assert len(out) == length
    return bytes(out)


@pytest.mark.parametrize("library", ["test", "product"])
def test_graph_capture_and_replay(built, library):
    """A flagged decode with its index, captured behind one eager run of the
    identical call and replayed over what is written into the same buffers:
    the captured noise stream; another noise stream of the same framed length
    with its own index values; a text stream brought to that length by
    trailing padding, whose index no longer tiles, so that the sequential walk
    decides inside the replay; the first stream with a flipped CRC.  Then
    twice with no wait in between.  Outputs and bands are reset before every
    replay."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    p = Pair(library)
    S = p.S
    n, cap = 131077, 196608
    A = O.frame_compress(data("noise", n, 1))
    B = O.frame_compress(data("noise", n, 2))
    assert len(A) == len(B) == 10 + n + 8 * 3
    text = data("text", cap, 4)
    Cc = padded_to(O.frame_compress(text), len(A))
    Dd = bytearray(A)
    Dd[chunk_offsets(A)[1] + 4] ^= 0x10
    Dd = bytes(Dd)
    runs = {"A": A, "B": B, "C": Cc, "D": Dd}
    idx = {k: (chunk_offsets(v) + [len(v)])[:4] for k, v in runs.items()}
    assert all(len(i) == 4 for i in idx.values()) and idx["A"] != idx["C"]
    try:
        with torch.cuda.stream(S):
            want = {k: p.reference(v, cap) for k, v in runs.items()}
            assert want["A"][:2] == (n, OK) and want["B"][:2] == (n, OK)
            assert want["C"] == (cap, OK, text)
            assert want["D"][1][0] != 0 and want["D"][0] == 65536
            fronts = {"A": INDEX, "B": INDEX, "C": WALK, "D": INDEX}
            b = Bufs(A, cap, 7)
            d_idx = u64(idx["A"])

            def load(k):
                b.load(runs[k])
                d_idx.copy_(u64(idx[k]))
                b.reset()

            S.synchronize()
            assert call(p.ctx, b, 3, d_idx, NO_WAIT) == 0   # eager: scratch
            S.synchronize()
            assert b.result("eager") == want["A"]
            b.reset()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=S):
                assert call(p.ctx, b, 3, d_idx, NO_WAIT) == 0
            for k in "ABCDA":
                load(k)
                g.replay()
                S.synchronize()
                assert b.result(f"replay over {k}") == want[k], k
                assert p.ctx.info("frame_nowait_front") == fronts[k], k
            load("C")
            g.replay()
            g.replay()
            S.synchronize()
            assert b.result("two replays, no wait between") == want["C"]
    finally:
        p.close()


@pytest.mark.parametrize("library", ["test", "product"])
def test_round_trip_in_one_graph(built, library):
    """snapmi_frame_compress writing its chunk offsets, then the flagged
    decode reading them on the device with n_chunks = ceil(n / 65536), in one
    graph: replayed over three incompressible inputs (the framed length is
    the same every time), the output is the input and the index never visits
    the host."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from rust_snappy_amd import frame
    p = Pair(library)
    S = p.S
    n = 200000
    chunks = math.ceil(n / 65536)
    flen = 10 + n + 8 * chunks
    L = p.ctx._L
    try:
        with torch.cuda.stream(S):
            src = torch.zeros(n, dtype=torch.uint8, device="cuda")
            mid = Slab([frame.frame_max_len(n)], 11)
            o = int(mid.offs[0])
            d_mid = mid.data[o:o + mid.caps[0]]
            mid_len = torch.full((1,), -7, dtype=torch.int64, device="cuda")
            d_idx = torch.full((chunks + 1,), -7, dtype=torch.int64,
                               device="cuda")
            out = Bufs(b"", n, 12)
            out.d_in, out.s = d_mid, b"\0" * flen   # decode what lies in mid

            def both():
                rc = L.snapmi_frame_compress(
                    p.ctx._h, C.c_void_p(src.data_ptr()), n,
                    C.c_void_p(d_mid.data_ptr()), mid.caps[0],
                    C.c_void_p(mid_len.data_ptr()),
                    C.c_void_p(d_idx.data_ptr()))
                assert rc == 0
                assert call(p.ctx, out, chunks, d_idx, NO_WAIT) == 0

            def load(salt):
                d = data("noise", n, salt)
                src.copy_(torch.frombuffer(bytearray(d), dtype=torch.uint8))
                mid.refill()
                mid_len.fill_(-7)
                d_idx.fill_(-7)
                out.reset()
                return d

            def check(d, what):
                S.synchronize()
                mid.assert_guards(what)
                assert int(mid_len.item()) == flen, what
                assert out.result(what) == (n, OK, d), what
                assert p.ctx.info("frame_nowait_front") == INDEX, what
                assert d_idx.cpu().tolist()[-1] == flen

            d = load(20)
            both()
            check(d, "eager")
            load(20)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=S):
                both()
            for salt in (21, 22, 23):
                d = load(salt)
                g.replay()
                check(d, f"replay {salt}")
    finally:
        p.close()
