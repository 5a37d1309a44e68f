"""GPU suite: the compressors and decoders on the inputs of
tests/token_shapes.py - blocks built, and shown by the oracle's parse
(tests/test_token_shapes_cpu.py), to hold a token at every edge of the
four-byte token format and of the encoder's size arithmetic, token pages at
full density (15 000 tokens and more a block, 128 blocks and a 128-block
stream), all four exception pages, an exception at token 63 / 64 / 511 / 512,
and the same in blocks at a position k > 0 of a stream (direct positions).

Every compressor route (`cctx`) must write the oracle's bytes; on routes
whose every block goes through the token path, with a pool that cannot run
out, the pages the launch asked for must be at least what the oracle's tokens
need - the proof that the pages under test were written; every decoder
(`ctx`) must give the inputs back from the oracle's streams, plainly and
through the block index the compressor wrote."""
import pytest
import torch

import token_shapes as T

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def S():
    return T.the_set()


_uploaded = {}


def _batch(S, name):
    """(cases, their inputs on the device), uploaded once per process."""
    if name not in _uploaded:
        from rust_snappy_amd import batch
        cases = {"grid": lambda: S.grid,
                 "dense_exceptions": S.dense_and_exceptions,
                 "streams": lambda: S.streams,
                 "everything": S.everything}[name]()
        _uploaded[name] = (cases, batch.StreamBatch.from_bytes(
            [c.data for c in cases]))
    return _uploaded[name]


def _slices(sb, lens):
    host = sb.data.cpu().numpy()
    return [host[int(o):int(o) + int(n)].tobytes()
            for o, n in zip(sb.offsets, lens)]


def check_compress(ctx, cases, src):
    from rust_snappy_amd import batch
    dst, lens, errs = batch.compress(ctx, src)
    assert all(e == (0, 0, 0, 0) for e in errs), \
        [(c.name, e) for c, e in zip(cases, errs) if e != (0, 0, 0, 0)][:5]
    assert lens.tolist() == [len(c.comp) for c in cases], \
        [(c.name, int(n), len(c.comp)) for c, n in zip(cases, lens)
         if n != len(c.comp)][:5]
    for c, got in zip(cases, _slices(dst, lens)):
        assert got == c.comp, c.name


@pytest.mark.parametrize("name", ["grid", "dense_exceptions", "streams"])
def test_compress_gives_the_oracle_bytes(cctx, S, name):
    check_compress(cctx, *_batch(S, name))


@pytest.mark.parametrize("route", ["lanes", "spans_match", "coresident"])
def test_token_path_asks_for_the_pages_the_tokens_need(built, S, route):
    """Every block of the dense-and-exceptions batch goes through the token
    path here (the lane kernel, the window kernel as match finder, both on
    every CU) and the pool holds the worst case of every block
    (token_pool_pct 100): no block spills, and the launch asked for at least
    ceil(tokens / 512) + ceil(exceptions / 256) pages per block, the oracle's
    tokens counted - 30 to 32 token pages for a dense block, four exception
    pages for a block of phrases."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import rust_snappy_amd as R
    cases, src = _batch(S, "dense_exceptions")
    need = sum(T.pages(b) for c in cases for b in c.blocks)
    blocks = sum(len(c.blocks) for c in cases)
    assert need > 30 * 256 and blocks == 2 * 128 + len(S.exceptions)
    with R.raw.Context(0) as c:
        c.set_option("compress_mode", 1)
        c.set_option("lane_min_blocks", 1)
        c.set_option("small_table_kernel", 0)
        c.set_option("match_kernel", 1 if route == "spans_match" else 0)
        c.set_option("lane_coresident", 1 if route == "coresident" else 0)
        c.set_option("lane_coresident_min_blocks", 1)
        c.set_option("token_pool_pct", 100)
        check_compress(c, cases, src)
        asked = c.info("token_pages_asked")
        spilled = c.info("token_blocks_spilled")
        print(f"\n{route}: {blocks} blocks need {need} pages, asked {asked}, "
              f"spilled {spilled}, {c.last_kernel()}")
        assert spilled == 0
        assert asked >= need, (asked, need)
        assert c.last_kernel() == {"lanes": "k_match_blocks",
                                   "spans_match": "k_match_spans",
                                   "coresident": "k_match_both"}[route]


def test_decoders_give_the_inputs_back(ctx, S):
    """The oracle's streams of the whole set - 16 000 two- and three-byte
    elements per 64 KiB in the dense blocks, copies in pieces of 64 and 60,
    offsets of 1 to 4 and to the block's first byte - by
    snapmi_decompress_batch, then through the block index the compressor
    writes for them (every multi-block stream decoded a block per
    wavefront)."""
    from rust_snappy_amd import batch
    cases, src = _batch(S, "everything")
    sizes = [len(c.data) for c in cases]
    enc = batch.StreamBatch.from_bytes([c.comp for c in cases])
    dec, lens, errs = batch.decompress(ctx, enc, caps=sizes)
    assert all(e == (0, 0, 0, 0) for e in errs)
    assert lens.tolist() == sizes
    for c, got in zip(cases, _slices(dec, lens)):
        assert got == c.data, c.name
    # the compressor's own streams are the oracle's; its index with them
    own, first, index = batch.compress(ctx, src, want_index=True)
    assert own.lens.tolist() == [len(c.comp) for c in cases]
    for c, got in zip(cases, _slices(own, own.lens)):
        assert got == c.comp, c.name
    dec, lens, errs = batch.decompress(ctx, own, caps=sizes,
                                       index=(first, index))
    long_ones = sum(1 for n in sizes if n > T.BLOCK)
    assert long_ones == 1 + len(S.streams)
    assert ctx.info("index_streams_pieced") == long_ones
    assert ctx.info("index_streams_fallback") == 0
    assert all(e == (0, 0, 0, 0) for e in errs)
    assert lens.tolist() == sizes
    for c, got in zip(cases, _slices(dec, lens)):
        assert got == c.data, c.name
