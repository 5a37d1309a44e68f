"""GPU suite: the streams of tests/decoder_shapes.py - built at the edges of
the wave decoders' window loops, each proven by the lane-level model to reach
the edge it is named for (tests/test_decoder_shapes_cpu.py) - through every
decoder: the window loops of both generations and the shipped library (the
ctx fixture), the sequential decoder, the lane-per-stream kernels, the scalar
call, the long-stream route and the block index builder.  Bytes are the
builders' (which the oracle confirmed on the CPU); errors are the oracle's on
the very bytes sent, all four fields."""
import numpy as np
import pytest
import torch

import decoder_shapes as D
import indexbuild_ref as IB
import long_streams as LS
import oracle_lib as O
from conftest import set_scan_geometry

pytestmark = pytest.mark.gpu

FILL = 0xEE
SLACK = 4096      # bytes behind the last stream's capacity, checked too


def oracle_error(comp, cap):
    try:
        O.decompress(comp, cap)
    except O.SnapError as e:
        return (e.kind, e.a, e.b, e.c)
    raise AssertionError("the oracle accepts a stream of `beyond`")


def mixed(the_set, valid):
    """`valid` with the streams of `beyond` spread among them."""
    cases = list(valid)
    step = max(len(cases) // (len(the_set["beyond"]) + 1), 1)
    for i, b in enumerate(the_set["beyond"]):
        cases.insert(min((i + 1) * step + i, len(cases)), b)
    return cases


def decode_packed(ctx, cases):
    """ONE snapmi_decompress_batch call; the outputs back to back, every
    capacity exactly the announced length, so a byte written past a stream's
    end lands in its neighbour.  Checks every stream."""
    from rust_snappy_amd import batch, raw
    src = batch.StreamBatch.from_bytes([c.comp for c in cases])
    caps = [O.decompress_len(c.comp) for c in cases]
    offs = np.concatenate([[0], np.cumsum(caps)[:-1]]).astype(np.int64)
    total = int(sum(caps))
    dst = batch.StreamBatch(
        torch.full((total + SLACK,), FILL, dtype=torch.uint8, device="cuda"),
        offs, caps)
    out_lens = torch.full((len(cases),), -1, dtype=torch.int64, device="cuda")
    errs = torch.zeros(32 * len(cases), dtype=torch.uint8, device="cuda")
    raw.decompress_batch(ctx, src.d_ptrs, src.d_lens, dst.d_ptrs, dst.d_lens,
                         out_lens, errs)
    ctx.synchronize()
    e = batch.read_errors(errs)
    flat = dst.data.cpu().numpy().tobytes()
    lens = out_lens.cpu().numpy()
    assert flat[total:] == bytes([FILL]) * SLACK
    bad = 0
    for i, c in enumerate(cases):
        o = int(offs[i])
        if c.out is None:
            assert e[i] == oracle_error(c.comp, caps[i]), (c.name, e[i])
            assert lens[i] == 0, c.name
            bad += 1
        else:
            assert e[i] == (0, 0, 0, 0), (c.name, e[i])
            assert lens[i] == len(c.out) == caps[i], c.name
            assert flat[o:o + caps[i]] == c.out, c.name
    return bad


@pytest.fixture(scope="module")
def the_set():
    return D.the_set()


@pytest.fixture(scope="module")
def long_one():
    comp, out = D.long_stream(LS.long_stream_rule)
    assert LS.long_stream_rule(len(comp), len(out))
    return comp, out


def test_the_set_in_one_batch(ctx, the_set):
    cases = mixed(the_set, D.valid_cases())
    assert decode_packed(ctx, cases) == len(the_set["beyond"]) >= 20


def test_the_set_on_the_sequential_decoder(built, the_set):
    """decode_kernel 0: k_decompress_sequential, whose copy loop has a
    reciprocal of its own."""
    import rust_snappy_amd as R
    c = R.raw.Context(0)
    try:
        c.set_option("decode_kernel", 0)
        cases = mixed(the_set, D.valid_cases())
        assert decode_packed(c, cases) == len(the_set["beyond"])
    finally:
        c.close()


def test_short_streams_one_batch(ctx, the_set):
    """k_decompress_tiny, k_decompress_small and the wavefront decoder's
    short class on the overlapping copies, by themselves in a batch (so the
    plan sorts nothing else between them)."""
    short = the_set["overlap_short"]
    assert {c.name.split("-")[0] for c in short} == {"lds", "short_wide",
                                                     "small"}
    assert decode_packed(ctx, short) == 0


def test_scalar_call(ctx, the_set):
    """snapmi_raw_decompress on one stream of each family."""
    import rust_snappy_amd as R
    dec = R.raw.Decoder(ctx=ctx)
    for name, cases in the_set.items():
        c = cases[-1]
        if c.out is not None:
            assert dec.decompress_vec(c.comp) == c.out, c.name
        else:
            with pytest.raises(R.Error) as ei:
                dec.decompress(c.comp, bytearray(O.decompress_len(c.comp)))
            want = oracle_error(c.comp, O.decompress_len(c.comp))
            assert (ei.value.kind,) + ei.value.abc == want, c.name


def stream_decode(ctx, comp, cap):
    """snapmi_decompress_stream on one device-resident stream."""
    from rust_snappy_amd import raw
    d_in = torch.frombuffer(bytearray(comp), dtype=torch.uint8).cuda()
    d_out = torch.full((cap + SLACK,), FILL, dtype=torch.uint8, device="cuda")
    out_len = torch.zeros(1, dtype=torch.int64, device="cuda")
    err = torch.zeros(32, dtype=torch.uint8, device="cuda")
    raw.decompress_stream(ctx, d_in, len(comp), d_out[:cap], out_len, err)
    ctx.synchronize()
    from rust_snappy_amd import batch
    got = d_out.cpu().numpy().tobytes()
    assert got[cap:] == bytes([FILL]) * SLACK
    return got[:int(out_len.item())], batch.read_errors(err)[0]


def test_long_stream_by_itself(ctx, long_one):
    """The valid families as one long stream through
    snapmi_decompress_stream."""
    comp, out = long_one
    got, e = stream_decode(ctx, comp, len(out))
    assert e == (0, 0, 0, 0) and got == out


@pytest.mark.parametrize("geom", [pytest.param((10, 0), id="1k"),
                                  pytest.param(None, id="own")])
def test_long_stream_in_a_batch(ctx, the_set, long_one, geom):
    """... and in a batch, beside short streams, with the long-stream pieces
    on and off: at the scan's 1 KiB geometry (a knob of the test build: on
    the shipped library that case is skipped, as everywhere in this suite)
    and at the library's own, which every library runs."""
    class Long:
        name = "long"
    Long.comp, Long.out = long_one
    cases = the_set["handover"] + [Long] + the_set["behind_long_literal"]
    if geom is not None:
        set_scan_geometry(ctx, geom)
    try:
        for pieces in (1, 0):
            ctx.set_option("batch_long_streams", pieces)
            assert decode_packed(ctx, cases) == 0
    finally:
        ctx.set_option("batch_long_streams", 1)
        if geom is not None:
            set_scan_geometry(ctx, None)


def test_block_index(ctx, the_set, long_one):
    """snapmi_build_block_index on the long stream and on the block-aligned
    stream of the set: verdicts, entries and counters are
    indexbuild_ref.build's."""
    from rust_snappy_amd import batch
    aligned = next(c for c in the_set["foreign_whole"]
                   if c.name.endswith("aligned"))
    streams = [long_one[0], aligned.comp, the_set["ring"][0].comp]
    dlens = [len(long_one[1]), len(aligned.out), len(the_set["ring"][0].out)]
    want = [IB.build(s, d) for s, d in zip(streams, dlens)]
    assert want[1][0] == IB.BUILT and len(want[1][1]) >= 3
    src = batch.StreamBatch.from_bytes(streams)
    first, index, status = batch.build_index(ctx, src, dlens)
    first = [int(v) for v in first.cpu().tolist()]
    flat = [int(v) for v in index.cpu().tolist()]
    for i, (st, entries) in enumerate(want):
        assert status[i] == st, (i, status)
        assert flat[first[i]:first[i + 1]] == entries, i
    counts = [sum(1 for st, _ in want if st == k) for k in (1, 2, 3, 4)]
    got = [ctx.info("index_build_" + k)
           for k in ("built", "unaligned", "corrupt", "missized")]
    assert got == counts
    # ... and the index decodes: the aligned stream's copies reach across its
    # blocks, which the indexed decoder must notice
    out, lens, errs = batch.decompress(ctx, src, index=(
        torch.tensor(first, dtype=torch.int64, device="cuda"),
        torch.tensor(flat, dtype=torch.int64, device="cuda")))
    for i, s in enumerate(streams):
        assert errs[i] == (0, 0, 0, 0), i
        assert out.stream_bytes(i, lens[i]) == O.decompress(s), i
