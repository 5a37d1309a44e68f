"""GPU suite of the host-memory batch calls (snapmi_compress_batch_host /
snapmi_decompress_batch_host, raw.compress_many / decompress_many): stream i of
a batch is exactly what snapmi_raw_compress / snapmi_raw_decompress gives for
it alone - the oracle's bytes, its error variant and fields -, no stream
affects another, a failed stream's buffer is untouched, nothing is written
outside [0, out_len) of any buffer, and only what was written crosses the
link on the way home."""
import ctypes as C
import random

import numpy as np
import pytest

import foreign
import kats
import oracle_lib as O

pytestmark = pytest.mark.gpu

OK = (0, 0, 0, 0)
EMPTY, BUFFER_TOO_SMALL = 3, 2
E_ARGUMENT = 101
LENGTHS = [0, 1, 15, 16, 17, 255, 256, 1023, 1024, 8192, 65535, 65536, 65537,
           200000]
CORPUS = ["html", "urls.10K", "fireworks.jpeg", "paper-100k.pdf", "html_x_4",
          "alice29.txt", "asyoulik.txt", "lcet10.txt", "plrabn12.txt",
          "geo.protodata", "kppkn.gtb", "Mark.Twain-Tom.Sawyer.txt"]
GUARD = 96
_memo = {}


def memo(key, make):
    if key not in _memo:
        _memo[key] = make()
    return _memo[key]


def text():
    return memo("text", lambda: b"".join(
        (O.CORPUS / n).read_bytes()
        for n in ("alice29.txt", "lcet10.txt", "plrabn12.txt")))


def inputs():
    """The lengths at which the codec changes path, as text, and a slice of
    every corpus file; 1.9 MB."""
    def make():
        t = text()
        datas = [t[7:7 + n] for n in LENGTHS]
        for k, name in enumerate(CORPUS):
            d = (O.CORPUS / name).read_bytes()
            datas.append(d[100 * k:100 * k + 90_000 + 1111 * k])
        return datas
    return memo("inputs", make)


def oracle_compressed():
    return memo("compressed", lambda: [O.compress(d) for d in inputs()])


class Arena:
    """Caller buffers of the given sizes, each at an odd distance inside one
    array of sentinel bytes - pageable, or page-locked by snapmi_host_alloc."""

    def __init__(self, sizes, seed, pinned=False, fill=None):
        rng = random.Random(seed)
        self.sizes = [int(s) for s in sizes]
        self.offs, pos = [], 0
        for s in self.sizes:
            pos += GUARD + rng.randrange(16)
            self.offs.append(pos)
            pos += s
        pos += GUARD
        self._L = self._p = None
        if pinned:
            from rust_snappy_amd import _lib
            self._L = _lib.load()
            self._p = self._L.snapmi_host_alloc(pos)
            assert self._p
            self.buf = np.frombuffer((C.c_uint8 * pos).from_address(self._p),
                                     dtype=np.uint8)
        else:
            self.buf = np.empty(pos, dtype=np.uint8)
        self.buf[:] = np.frombuffer(rng.randbytes(pos), dtype=np.uint8)
        for i, d in enumerate(fill or []):
            self.buf[self.offs[i]:self.offs[i] + len(d)] = np.frombuffer(
                bytes(d), dtype=np.uint8)
        self.before = self.buf.copy()
        base = self.buf.ctypes.data
        self.ptrs = np.array([base + o for o in self.offs], dtype=np.uint64)

    def bytes(self, i, n):
        return self.buf[self.offs[i]:self.offs[i] + int(n)].tobytes()

    def assert_only(self, written):
        """written[i]: the bytes stream i must hold at its start, None for a
        stream that failed; every other byte of the arena is as it was."""
        want = self.before.copy()
        for i, w in enumerate(written):
            if w:
                want[self.offs[i]:self.offs[i] + len(w)] = np.frombuffer(
                    w, dtype=np.uint8)
        bad = np.flatnonzero(self.buf != want)
        assert bad.size == 0, f"first wrong byte at {bad[0]} of the arena"

    def close(self):
        if self._p:
            self.buf = self.before = None
            self._L.snapmi_host_free(self._p)
            self._p = None


def errs_of(errs):
    return [(int(e["kind"]), int(e["a"]), int(e["b"]), int(e["c"]))
            for e in errs]


def run(ctx, compress, streams, caps, pinned=False, seed=1):
    """One host batch call from guarded buffers: (lens, errs, outputs), after
    checking that exactly [0, len) of the successful streams changed."""
    from rust_snappy_amd import raw
    src = Arena([len(s) for s in streams], seed, pinned, fill=streams)
    dst = Arena(caps, seed + 100, pinned)
    try:
        lens, errs = raw.batch_host(ctx, compress, src.ptrs,
                                    [len(s) for s in streams], dst.ptrs, caps)
        errs = errs_of(errs)
        outs = [dst.bytes(i, lens[i]) if errs[i] == OK else None
                for i in range(len(streams))]
        for i, e in enumerate(errs):
            assert e == OK or lens[i] == 0, (i, e, lens[i])
        dst.assert_only(outs)
        src.assert_only([None] * len(streams))
        return [int(x) for x in lens], errs, outs
    finally:
        src.close()
        dst.close()


def scalar(ctx, compress, data, cap):
    """snapmi_raw_compress / snapmi_raw_decompress of one stream:
    (written, error, bytes or None)."""
    from rust_snappy_amd import _lib
    L = _lib.of(ctx)
    out = np.zeros(max(cap, 1), dtype=np.uint8)
    n = C.c_size_t(0)
    err = _lib.SnapmiError()
    f = L.snapmi_raw_compress if compress else L.snapmi_raw_decompress
    rc = f(ctx._h, bytes(data), len(data), out.ctypes.data_as(C.c_void_p),
           cap, C.byref(n), C.byref(err))
    assert rc < 100, rc
    e = (err.kind, err.a, err.b, err.c)
    assert rc == e[0]
    return n.value, e, out[:n.value].tobytes() if rc == 0 else None


def oracle_error(s, cap):
    with pytest.raises(O.SnapError) as ei:
        O.decompress(s, cap)
    oe = ei.value
    return (oe.kind, oe.a, oe.b, oe.c)


@pytest.fixture(scope="module")
def tctx(built):
    """A context of the test build, for the test options."""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import rust_snappy_amd as R
    c = R.raw.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("slice_bytes", [64 << 10, 1 << 20])
@pytest.mark.parametrize("cctx", ["product", "spans", "lanes", "small_tables",
                                  "product-lanes"], indirect=True)
def test_compress_equals_oracle_and_the_scalar_call(cctx, slice_bytes):
    from rust_snappy_amd import raw
    datas, want = inputs(), oracle_compressed()
    cctx.set_option("host_batch_slice", slice_bytes)
    caps = [raw.max_compress_len(len(d)) for d in datas]
    lens, errs, outs = run(cctx, True, datas, caps)
    assert cctx.info("host_batch_slices") >= (4 if slice_bytes == 64 << 10
                                              else 2)
    assert cctx.info("host_batch_h2d_bytes") >= sum(len(d) for d in datas)
    for i, d in enumerate(datas):
        assert errs[i] == OK, (i, errs[i])
        assert outs[i] == want[i], (i, len(d))
        assert lens[i] == len(want[i])
    if slice_bytes == 1 << 20:
        for i, d in enumerate(datas):
            assert scalar(cctx, True, d, caps[i]) == (lens[i], OK, outs[i]), i
        # n = 1
        for i in (0, 3, 13, len(datas) - 1):
            assert run(cctx, True, [datas[i]], [caps[i]]) == \
                ([lens[i]], [OK], [want[i]])


def decode_streams():
    """(compressed, original): the oracle's forms of inputs(), streams no
    encoder of this family writes (copy-4, far offsets) and the golden
    file."""
    def make():
        pairs = list(zip(oracle_compressed(), inputs())) + foreign.cases()
        name = "Mark.Twain-Tom.Sawyer.txt"
        pairs.append(((O.CORPUS / (name + ".rawsnappy")).read_bytes(),
                      (O.CORPUS / name).read_bytes()))
        return pairs
    return memo("decode", make)


@pytest.mark.parametrize("slice_bytes", [64 << 10, 1 << 20])
def test_decompress_good_streams(ctx, slice_bytes):
    pairs = decode_streams()
    ctx.set_option("host_batch_slice", slice_bytes)
    comp = [c for c, _ in pairs]
    caps = [len(d) for _, d in pairs]
    lens, errs, outs = run(ctx, False, comp, caps, seed=2)
    assert ctx.info("host_batch_slices") >= (4 if slice_bytes == 64 << 10
                                             else 2)
    for i, (c, d) in enumerate(pairs):
        assert (errs[i], outs[i]) == (OK, d), (i, errs[i])
    if slice_bytes == 1 << 20:
        for i, (c, d) in enumerate(pairs):
            assert scalar(ctx, False, c, caps[i]) == (len(d), OK, d), i
        assert run(ctx, False, [comp[5]], [caps[5]]) == \
            ([caps[5]], [OK], [pairs[5][1]])
        # room to spare changes nothing
        roomy = [c + 1000 for c in caps]
        assert run(ctx, False, comp, roomy, seed=3) == (lens, errs, outs)


def error_batch():
    """The reference's error KATs, the corpus' bad files, an empty input and
    capacities one short, each between two good streams:
    (streams, caps, expected error or None, original or None)."""
    def make():
        bad = [(s, 64) for _, s, _, _ in kats.ERROR_KATS]
        assert len(bad) == 21
        for k in (1, 2, 3):
            s = (O.CORPUS / f"baddata{k}.snappy").read_bytes()
            try:
                cap = O.decompress_len(s)
            except O.SnapError:
                cap = 64
            bad.append((s, min(cap, 1 << 20)))
        bad.append((b"", 16))
        goods = decode_streams()
        for k in (2, 8, 11, 20):               # a capacity one short
            bad.append((goods[k][0], len(goods[k][1]) - 1))
        streams, caps, want, origs = [], [], [], []
        for k, (s, cap) in enumerate(bad):
            c, d = goods[(5 * k) % len(goods)]
            streams += [c, s]
            caps += [len(d), cap]
            want += [None, oracle_error(s, cap)]
            origs += [d, None]
        c, d = goods[9]
        return streams + [c], caps + [len(d)], want + [None], origs + [d]
    return memo("errors", make)


@pytest.mark.parametrize("pinned", [False, True])
def test_decompress_errors_stay_in_their_stream(ctx, pinned):
    streams, caps, want, origs = error_batch()
    ctx.set_option("host_batch_slice", 64 << 10)
    lens, errs, outs = run(ctx, False, streams, caps, pinned=pinned, seed=4)
    kinds = set()
    for i, s in enumerate(streams):
        if origs[i] is not None:
            assert (errs[i], outs[i]) == (OK, origs[i]), i
            continue
        # the oracle's variant and fields; nothing delivered (run() has
        # checked that the buffer is untouched)
        assert errs[i] == want[i], (i, errs[i], want[i])
        assert lens[i] == 0 and outs[i] is None
        kinds.add(errs[i][0])
        if not pinned:
            assert scalar(ctx, False, s, caps[i]) == (0, errs[i], None), i
    assert {1, 2, 3, 4, 5, 6, 7, 8, 9} <= kinds, kinds
    for name, s, key, _ in kats.ERROR_KATS:
        i = streams.index(s)
        assert (O.KIND_NAMES[errs[i][0]],) + errs[i][1:len(key)] == key, name
    i = streams.index(b"")
    assert errs[i] == (EMPTY, 0, 0, 0)
    short = [i for i in range(len(streams))
             if errs[i][0] == BUFFER_TOO_SMALL]
    assert len(short) >= 4
    for i in short[-4:]:
        assert errs[i] == (BUFFER_TOO_SMALL, caps[i], caps[i] + 1, 0)


@pytest.mark.parametrize("pinned", [False, True])
def test_compress_cap_one_short_fails_that_stream_only(cctx_product, pinned):
    from rust_snappy_amd import raw
    ctx = cctx_product
    datas, want = inputs(), oracle_compressed()
    ctx.set_option("host_batch_slice", 64 << 10)
    need = [raw.max_compress_len(len(d)) for d in datas]
    caps = [w - 1 if i % 3 == 1 else w + (7 if i % 3 == 2 else 0)
            for i, w in enumerate(need)]
    lens, errs, outs = run(ctx, True, datas, caps, pinned=pinned, seed=5)
    refused = 0
    for i, d in enumerate(datas):
        if caps[i] < need[i]:
            refused += 1
            assert errs[i] == (BUFFER_TOO_SMALL, caps[i], need[i], 0), i
            assert lens[i] == 0 and outs[i] is None
            if not pinned:
                assert scalar(ctx, True, d, caps[i]) == (0, errs[i], None)
        else:
            assert (errs[i], outs[i]) == (OK, want[i]), i
    assert refused >= 8


@pytest.fixture(scope="module")
def cctx_product(built):
    """The shipped library with its default options."""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from conftest import product_context
    c = product_context()
    yield c
    c.close()


@pytest.mark.parametrize("direct_min,to_host", [(4096, 1), (1 << 20, 0),
                                                (0, 0), (70_000, 1)])
def test_direct_copies_and_both_ways_home(tctx, direct_min, to_host):
    """Streams above the threshold go to the device from where they lie - in
    runs between staged ones -, and the packed output comes home by k_hb_pack's
    own stores or by one copy: the same bytes every way."""
    from rust_snappy_amd import raw
    tctx.set_test_option("host_batch_direct_min", direct_min)
    tctx.set_test_option("host_batch_pack_to_host", to_host)
    try:
        tctx.set_option("host_batch_slice", 256 << 10)
        datas, want = inputs(), oracle_compressed()
        caps = [raw.max_compress_len(len(d)) for d in datas]
        lens, errs, outs = run(tctx, True, datas, caps, seed=6)
        assert errs == [OK] * len(datas) and outs == want
        d2h = tctx.info("host_batch_d2h_bytes")
        assert sum(lens) <= d2h <= sum(lens) + 56 * len(datas) + 16 * \
            tctx.info("host_batch_slices")
        pairs = decode_streams()
        lens, errs, outs = run(tctx, False, [c for c, _ in pairs],
                               [len(d) for _, d in pairs], seed=7)
        assert errs == [OK] * len(pairs)
        assert outs == [d for _, d in pairs]
    finally:
        tctx.set_test_option("host_batch_direct_min", 1 << 20)
        tctx.set_test_option("host_batch_pack_to_host", 1)


def test_a_stream_above_the_default_direct_threshold(cctx_product):
    """1.06 MB: copied from where it lies by the shipped library's default,
    between staged streams, in a slice of its own."""
    from rust_snappy_amd import raw
    ctx = cctx_product
    ctx.set_option("host_batch_slice", 1 << 20)
    t = text()
    assert len(t) > 1 << 20
    datas = [t[:5000], t, t[5000:9000], b"", t[:300]]
    want = memo("big", lambda: [O.compress(d) for d in datas])
    caps = [raw.max_compress_len(len(d)) for d in datas]
    lens, errs, outs = run(ctx, True, datas, caps, seed=8)
    assert errs == [OK] * 5 and outs == want
    assert ctx.info("host_batch_slices") == 3
    lens, errs, outs = run(ctx, False, want, [len(d) for d in datas], seed=9)
    assert errs == [OK] * 5 and outs == datas


def test_copy_volume_is_what_was_written(cctx_product):
    """4 096 streams of 4 KiB of text: what comes home is the packed outputs,
    their alignment padding, one length and one error record per stream and a
    constant - not max_compress_len per stream."""
    from rust_snappy_amd import _lib, raw
    ctx = cctx_product
    ctx.set_option("host_batch_slice", 4 << 20)
    t = text()
    n = 4096
    datas = [t[200 * i:200 * i + 4096] for i in range(n)]
    want = memo("4k", lambda: [O.compress(d) for d in datas])
    outs, errors = raw.compress_many(datas, ctx)
    assert errors == [None] * n and outs == want
    d2h = ctx.info("host_batch_d2h_bytes")
    clens = sum(len(w) for w in want)
    bound = clens + 16 * n + n * (8 + C.sizeof(_lib.SnapmiError)) + 4096
    print(f"d2h {d2h} bytes, compressed {clens}, bound {bound}, slot copies "
          f"would be {n * raw.max_compress_len(4096)}")
    assert clens <= d2h <= bound
    assert ctx.info("host_batch_slices") == 4
    assert ctx.info("host_batch_h2d_bytes") >= n * 4096


def test_options_and_info(cctx_product):
    import rust_snappy_amd as R
    ctx = cctx_product
    ctx.set_option("host_batch_slice", 64 << 10)
    ctx.set_option("host_batch_slice", 1 << 30)
    for name, value in (("host_batch_slice", (64 << 10) - 1),
                        ("host_batch_slice", 0), ("host_batch_slices", 1),
                        ("host_batch_nonsense", 1)):
        with pytest.raises(R.Error) as ei:
            ctx.set_option(name, value)
        assert ei.value.kind == E_ARGUMENT, name
    for name in ("host_batch_slices", "host_batch_h2d_bytes",
                 "host_batch_d2h_bytes"):
        assert ctx.info(name) >= 0
    with pytest.raises(R.Error) as ei:
        ctx.info("host_batch_slice")
    assert ei.value.kind == E_ARGUMENT


def test_edges_and_reuse_of_the_context(cctx_product):
    from rust_snappy_amd import _lib, batch, frame, raw
    ctx = cctx_product
    L = _lib.of(ctx)
    ctx.set_option("host_batch_slice", 64 << 10)
    datas, want = inputs(), oracle_compressed()
    # n == 0 does nothing, whatever the pointers
    for f in (L.snapmi_compress_batch_host, L.snapmi_decompress_batch_host):
        assert f(ctx._h, None, None, None, None, None, None, 0) == 0
    # a NULL h_out_caps is an argument error and nothing is written
    src = Arena([len(datas[4])], 11, fill=[datas[4]])
    dst = Arena([64], 12)
    in_lens = np.array([len(datas[4])], dtype=np.uint64)
    out_lens = np.array([99], dtype=np.uint64)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    for f in (L.snapmi_compress_batch_host, L.snapmi_decompress_batch_host):
        assert f(ctx._h, p(src.ptrs), p(in_lens), p(dst.ptrs), None,
                 p(out_lens), None, 1) == E_ARGUMENT
        assert f(ctx._h, p(src.ptrs), p(in_lens), p(dst.ptrs), p(in_lens),
                 None, None, 1) == E_ARGUMENT
    assert b"bad args" in L.snapmi_last_error(ctx._h)
    assert out_lens[0] == 99
    dst.assert_only([None])
    # the next call on the same context is as good as the first; h_errs
    # may be NULL
    caps = np.array([64], dtype=np.uint64)
    assert L.snapmi_compress_batch_host(ctx._h, p(src.ptrs), p(in_lens),
                                        p(dst.ptrs), p(caps), p(out_lens),
                                        None, 1) == 0
    assert dst.bytes(0, out_lens[0]) == want[4]
    # a batch of failures only, then a good one
    lens, errs, outs = run(ctx, False, [b"\xff", b"", b"\x05\x00a"],
                           [8, 8, 8], seed=13)
    assert [e[0] for e in errs] == [4, 3, 5] and lens == [0, 0, 0]
    caps = [raw.max_compress_len(len(d)) for d in datas]
    assert run(ctx, True, datas, caps, seed=14)[2] == want
    # the pipe's slots are shared with the frame host calls, the context's
    # scratch with the device batch calls: both still give the oracle's bytes
    sb = batch.StreamBatch.from_bytes(datas[:20])
    dst_b, lens_b, errs_b = batch.compress(ctx, sb)
    for i in range(20):
        assert errs_b[i] == OK and dst_b.stream_bytes(i, lens_b[i]) == want[i]
    html = (O.CORPUS / "html").read_bytes()
    chunks = [65536] + [len(html) - 65536]
    assert frame.encode_host(ctx, bytearray(html), chunks) == \
        O.frame_compress(html)
    assert run(ctx, True, datas, caps, seed=15)[2] == want


def test_python_round_trip_and_error_display(ctx):
    import rust_snappy_amd as R
    from rust_snappy_amd import raw
    datas = memo("corpus", lambda: [(O.CORPUS / n).read_bytes()
                                    for n in CORPUS]) + [b"", b"x"]
    ctx.set_option("host_batch_slice", 1 << 20)
    comp, errors = raw.compress_many(datas, ctx)
    assert errors == [None] * len(datas)
    want = memo("corpus_c", lambda: [O.compress(d) for d in datas])
    assert comp == want
    # bytes-like objects of any kind, addressed in place
    views = [memoryview(c) if i % 2 else bytearray(c)
             for i, c in enumerate(comp)]
    back, errors = raw.decompress_many(views, ctx)
    assert errors == [None] * len(datas) and back == datas
    # errors are snap::Error objects that read like the scalar path's
    bad = [s for _, s, _, _ in kats.ERROR_KATS]
    mixed = []
    for k, s in enumerate(bad):
        mixed += [comp[k % len(comp)], s]
    caps = []
    for k, s in enumerate(bad):
        caps += [len(datas[k % len(comp)]), 64]
    outs, errors = raw.decompress_many(mixed, ctx, caps=caps)
    dec = raw.Decoder(ctx)
    for k, (name, s, key, _) in enumerate(kats.ERROR_KATS):
        assert (outs[2 * k], errors[2 * k]) == (datas[k % len(comp)], None)
        e = errors[2 * k + 1]
        assert isinstance(e, R.Error) and outs[2 * k + 1] == b""
        assert e.key() == key, name
        with pytest.raises(R.Error) as ei:
            dec.decompress(s, bytearray(64))
        assert e == ei.value and e.display() == ei.value.display(), name
    # the default capacities: what the headers announce
    outs, errors = raw.decompress_many([comp[0], b"\xff", comp[1]], ctx)
    assert outs == [datas[0], b"", datas[1]]
    assert [e and e.key() for e in errors] == [None, ("Header",), None]
