"""GPU suite: the block index of raw streams.

snapmi_compress_batch_indexed writes, beside exactly what
snapmi_compress_batch writes, where the elements of every 64 KiB block begin
in each compressed stream - checked entry for entry against the oracle
(blockindex_ref.expected_index) on every compressor configuration (`cctx`).
snapmi_decompress_batch_indexed must give what snapmi_decompress_batch gives
whatever the index holds: its own index, hostile ones, corrupt streams,
streams no 64 KiB-block encoder would write, the reference's error vectors -
length, error variant and fields, and the bytes [0, length) of every output,
between guard bands that must stay intact.  (Behind the length of a stream
that FAILED the buffer holds whatever the decoders got to before the error:
that differs between the decoders of the unindexed call already and is not
compared.)  Info "index_streams_pieced" / "index_streams_fallback" prove which
way a stream went."""
import random

import numpy as np
import pytest
import torch

import blockindex_ref as B
import foreign
import kats
import oracle_lib as O
import tiled_batch as TB
from gpu_buffers import Slab, hostile, read_errs, u64

pytestmark = pytest.mark.gpu

E_ARGUMENT = 101
LENGTHS = [0, 1, 255, 256, 1023, 1024, 65535, 65536, 65537, 131072,
           3 * 65536 + 5, 1 << 20]


def _kinds(n):
    text = (O.CORPUS / "alice29.txt").read_bytes()
    text = (text * ((1 << 20) // len(text) + 2))
    rng = random.Random(n)
    return {"text": text[7:7 + n], "zeros": bytes(n),
            "noise": rng.randbytes(n)}


def _inputs():
    """One batch mixing text, zeros and incompressible bytes of every length;
    ordered so that the 1 MiB stream of noise lies across block 64 of the
    batch (the segment boundary of the "lanes_segmented" configuration)
    whatever blocks the short streams behind it get."""
    by = {n: _kinds(n) for n in LENGTHS}
    order = []
    for n in (1 << 20, 3 * 65536 + 5, 131072, 65537, 65536, 65535):
        order += [by[n]["text"], by[n]["zeros"]]
    order += [by[3 * 65536 + 5]["noise"], by[131072]["noise"],
              by[1 << 20]["noise"]]
    for n in (65537, 65536, 65535, 1024, 1023, 256, 255, 1, 0):
        order.append(by[n]["noise"])
    for n in (1024, 1023, 256, 255, 1, 0):
        order += [by[n]["text"], by[n]["zeros"]]
    assert len(order) == 3 * len(LENGTHS)
    return order


class Case:
    """The batch, what the oracle says of it, and the one stream whose
    capacity is a byte short."""

    def __init__(self):
        self.inputs = _inputs()
        self.short = 6  # text, 65537 bytes
        assert len(self.inputs[self.short]) == 65537
        self.comps = [O.compress(d) for d in self.inputs]
        self.caps = [O.max_compress_len(len(d)) for d in self.inputs]
        self.caps[self.short] -= 1
        self.index = [B.expected_index(d) for d in self.inputs]
        self.index[self.short] = [0] * B.entries(65537)
        self.first = [0]
        for d in self.inputs:
            self.first.append(self.first[-1] + B.entries(len(d)))
        self.flat = [e for idx in self.index for e in idx]
        # block 64 of the batch lies inside a stream
        blocks = np.cumsum([0] + [-(-len(d) // 65536) for i, d in
                                  enumerate(self.inputs[:16])
                                  if i != self.short])
        assert any(a < 64 < b for a, b in zip(blocks, blocks[1:]))


@pytest.fixture(scope="module")
def case():
    return Case()


# ------------------------------------------------------------------ compress
def run_compress(ctx, case, indexed, index_cap=None, seed=0):
    from rust_snappy_amd import raw
    n = len(case.inputs)
    src = Slab([max(len(d), 1) for d in case.inputs], seed + 1, case.inputs)
    lens = torch.tensor([len(d) for d in case.inputs], dtype=torch.int64)
    dst = Slab(case.caps, seed)
    out_lens = torch.full((n,), -7, dtype=torch.int64, device="cuda")
    errs = torch.zeros(32 * n, dtype=torch.uint8, device="cuda")
    total = len(case.flat)
    first = torch.full((n + 1,), -7, dtype=torch.int64, device="cuda")
    index = torch.full((total + 8,), -7, dtype=torch.int64, device="cuda")
    kw = {}
    if indexed:
        kw = dict(index_first=first, index=index,
                  index_cap=total if index_cap is None else index_cap)
    raw.compress_batch(ctx, src.d_ptrs, lens.cuda(), dst.d_ptrs, dst.d_caps,
                       out_lens, errs, host_in_lens=lens, **kw)
    ctx.synchronize()
    dst.assert_guards("compress")
    return (dst, out_lens.cpu().numpy(), read_errs(errs),
            first.cpu().numpy(), index.cpu().numpy())


def check_compress(ctx, case):
    from rust_snappy_amd import raw
    assert raw.block_index_entries([len(d) for d in case.inputs]) \
        == len(case.flat) == case.first[-1]
    plain, plens, perrs, _, _ = run_compress(ctx, case, False)
    dst, lens, errs, first, index = run_compress(ctx, case, True)
    for i, c in enumerate(case.comps):
        if i == case.short:
            assert lens[i] == 0 and errs[i][0] != 0
            assert errs[i][1:3] == (case.caps[i], case.caps[i] + 1)
        else:
            assert errs[i] == (0, 0, 0, 0) and lens[i] == len(c), i
            assert dst.bytes(i, lens[i]) == c, i
        # exactly the unindexed call's
        assert lens[i] == plens[i] and errs[i] == perrs[i], i
        assert dst.bytes(i, lens[i]) == plain.bytes(i, plens[i]), i
    assert first.tolist() == case.first
    total = len(case.flat)
    got = index[:total].tolist()
    for i in range(len(case.inputs)):
        a, b = case.first[i], case.first[i + 1]
        assert got[a:b] == case.index[i], (i, len(case.inputs[i]))
    assert got[case.first[case.short]:case.first[case.short + 1]] == [0, 0, 0]
    assert (index[total:] == -7).all()  # nothing behind the index


def test_compress_index_every_route(cctx, case):
    check_compress(cctx, case)


def test_compress_index_spilled_and_segmented(built, case):
    """The lane kernel with a token pool of a page or two (blocks spill and
    are redone by k_redo_spilled) and launches cut every 64 blocks, inside
    the 1 MiB stream of noise."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import rust_snappy_amd as R
    with R.raw.Context(0) as c:
        c.set_option("compress_mode", 1)
        c.set_option("lane_min_blocks", 1)
        c.set_option("match_kernel", 0)
        c.set_option("lane_coresident", 0)
        c.set_option("lane_segment_blocks", 64)
        c.set_option("token_pool_pct", 1)
        c.set_option("token_pool_min_pages", 0)
        check_compress(c, case)
        assert c.info("token_blocks_spilled") > 0


def test_compress_index_cap_too_small(ctx, case):
    from rust_snappy_amd.error import DeviceError
    with pytest.raises(DeviceError) as e:
        run_compress(ctx, case, True, index_cap=len(case.flat) - 1)
    assert e.value.kind == E_ARGUMENT
    # nothing was enqueued: no tensor of the call changes
    from rust_snappy_amd import raw
    n = len(case.inputs)
    src = Slab([max(len(d), 1) for d in case.inputs], 1, case.inputs)
    lens = torch.tensor([len(d) for d in case.inputs], dtype=torch.int64)
    dst = Slab(case.caps, 0)
    before = dst.fetch().copy()
    out_lens = torch.full((n,), -7, dtype=torch.int64, device="cuda")
    first = torch.full((n + 1,), -7, dtype=torch.int64, device="cuda")
    index = torch.full((len(case.flat),), -7, dtype=torch.int64, device="cuda")
    with pytest.raises(DeviceError):
        raw.compress_batch(ctx, src.d_ptrs, lens.cuda(), dst.d_ptrs,
                           dst.d_caps, out_lens, None, host_in_lens=lens,
                           index_first=first, index=index,
                           index_cap=len(case.flat) - 1)
    ctx.synchronize()
    assert (dst.fetch() == before).all()
    for t in (out_lens, first, index):
        assert (t == -7).all()


# ---------------------------------------------------------------- decompress
def decode(ctx, comps, caps, index=None, seed=0, entries=None):
    """index: per stream its entries (a list; [] = none), or None for the
    unindexed call.  Returns (slab, lens, errs)."""
    from rust_snappy_amd import raw
    n = len(comps)
    src = Slab([max(len(c), 1) for c in comps], seed + 1, comps)
    in_lens = torch.tensor([len(c) for c in comps], dtype=torch.int64,
                           device="cuda")
    dst = Slab(caps, seed)
    out_lens = torch.full((n,), -7, dtype=torch.int64, device="cuda")
    errs = torch.full((32 * n,), 0xEE, dtype=torch.uint8, device="cuda")
    kw = {}
    if index is not None:
        first = [0]
        for idx in index:
            first.append(first[-1] + len(idx))
        flat = [e for idx in index for e in idx] + [0]
        kw = dict(index_first=u64(first), index=u64(flat),
                  index_entries=first[-1] if entries is None else entries)
    raw.decompress_batch(ctx, src.d_ptrs, in_lens, dst.d_ptrs, dst.d_caps,
                         out_lens, errs, **kw)
    ctx.synchronize()
    dst.assert_guards("decode")
    return dst, out_lens.cpu().numpy(), read_errs(errs)


def same_as_unindexed(ctx, comps, caps, index, entries=None, oracle=True):
    """The indexed call against the unindexed one (and the oracle): length,
    error variant and fields, bytes.  Returns (pieced, fallback)."""
    ref, rlens, rerrs = decode(ctx, comps, caps)
    got, lens, errs = decode(ctx, comps, caps, index, entries=entries)
    pieced = ctx.info("index_streams_pieced")
    fallback = ctx.info("index_streams_fallback")
    for i, (m, cap) in enumerate(zip(comps, caps)):
        assert lens[i] == rlens[i] and errs[i] == rerrs[i], \
            (i, lens[i], rlens[i], errs[i], rerrs[i])
        assert got.bytes(i, lens[i]) == ref.bytes(i, rlens[i]), i
        if not oracle:
            continue
        try:
            want = O.decompress(m, cap)
            assert errs[i] == (0, 0, 0, 0) and got.bytes(i, lens[i]) == want
        except O.SnapError as oe:
            assert (oe.kind, oe.a, oe.b, oe.c) == errs[i] and lens[i] == 0
    return pieced, fallback


def good(case):
    ok = [i for i in range(len(case.inputs)) if i != case.short]
    return ([case.comps[i] for i in ok], [len(case.inputs[i]) for i in ok],
            [case.index[i] for i in ok])


def test_decode_with_its_own_index(ctx, case):
    comps, caps, index = good(case)
    pieced, fallback = same_as_unindexed(ctx, comps, caps, index)
    assert pieced == sum(1 for c in caps if c > 65536) > 0
    assert fallback == 0
    # the index the compressor itself wrote, through batch.py
    from rust_snappy_amd import batch
    src = batch.StreamBatch.from_bytes([case.inputs[i] for i in
                                        range(len(case.inputs))])
    enc, first, idx = batch.compress(ctx, src, want_index=True)
    assert first.cpu().tolist() == case.first[:1] + [
        sum(B.entries(len(d)) for d in case.inputs[:k + 1])
        for k in range(len(case.inputs))]
    dec, lens, errs = batch.decompress(ctx, enc, index=(first, idx))
    for i, d in enumerate(case.inputs):
        assert errs[i][0] == 0 and dec.stream_bytes(i, lens[i]) == d, i
    assert ctx.info("index_streams_pieced") == sum(
        1 for d in case.inputs if len(d) > 65536)
    assert ctx.info("index_streams_fallback") == 0


@pytest.mark.parametrize("how", ["plus1", "minus1", "swapped", "equal",
                                 "beyond", "last_short", "random", "other",
                                 "none", "mid_element"])
def test_decode_with_a_hostile_index(ctx, case, how):
    comps, caps, index = good(case)
    rng = random.Random(how)
    bad = [hostile(idx, len(c), how, rng, index[(i + 1) % len(index)])
           for i, (idx, c) in enumerate(zip(index, comps))]
    pieced, fallback = same_as_unindexed(ctx, comps, caps, bad)
    long_ones = sum(1 for c in caps if c > 65536)
    assert pieced + fallback <= long_ones
    if how == "mid_element":
        # every long stream but those of one literal per block (noise) has an
        # entry inside an element now
        assert fallback > 0
    if how in ("equal", "random", "none", "last_short"):
        assert pieced == fallback == 0
    # ... and with index_entries short of what first[] says
    same_as_unindexed(ctx, comps, caps, index, entries=len(index[0]) + 1)
    # first[] itself hostile: every stream claims the same range
    from rust_snappy_amd import raw
    n = len(comps)
    flat = [e for idx in bad for e in idx] + [0, 0, 0]
    for first in ([0, 17] * n, [2**63] * (n + 1),
                  list(range(3 * n, -1, -3))):
        first = first[:n + 1]
        src = Slab([max(len(c), 1) for c in comps], 3, comps)
        in_lens = torch.tensor([len(c) for c in comps], dtype=torch.int64,
                               device="cuda")
        dst = Slab(caps, 2)
        out_lens = torch.zeros(n, dtype=torch.int64, device="cuda")
        errs = torch.zeros(32 * n, dtype=torch.uint8, device="cuda")
        raw.decompress_batch(ctx, src.d_ptrs, in_lens, dst.d_ptrs, dst.d_caps,
                             out_lens, errs, index_first=u64(first),
                             index=u64(flat), index_entries=len(flat) - 3)
        ctx.synchronize()
        dst.assert_guards("hostile first[]")
        lens = out_lens.cpu().numpy()
        for i, e in enumerate(read_errs(errs)):
            assert e == (0, 0, 0, 0) and lens[i] == caps[i]
            assert dst.bytes(i, lens[i]) == O.decompress(comps[i]), i


def test_decode_corrupt_streams_with_their_true_index(ctx, case):
    comps, caps, index = good(case)
    rng = random.Random(5)
    long_ones = [i for i, c in enumerate(caps) if c > 65536]
    streams, rooms, idxs, flipped = [], [], [], 0
    for i in long_ones:
        c = comps[i]
        # a flipped byte behind the header (the index still passes)
        p = rng.randrange(index[i][0] + 1, len(c))
        streams.append(c[:p] + bytes([c[p] ^ 0x5A]) + c[p + 1:])
        rooms.append(caps[i])
        idxs.append(index[i])
        flipped += 1
        # truncated: the last entry is not in_len any more
        cut = rng.randrange(index[i][0] + 1, len(c))
        streams.append(c[:cut])
        rooms.append(caps[i])
        idxs.append(index[i])
    # (a flipped byte may still decode - to other bytes - or break a piece:
    # both are the unindexed call's result; the oracle agrees either way)
    pieced, fallback = same_as_unindexed(ctx, streams, rooms, idxs)
    assert pieced + fallback == flipped
    # one flip that is certain to break its piece: a copy offset of zero
    i = long_ones[0]
    c, e = comps[i], index[i]
    broken = c[:e[1]] + foreign.copy(0, 8, 2) + c[e[1] + 3:]
    pieced, fallback = same_as_unindexed(ctx, [broken, c], [caps[i]] * 2,
                                         [e, e])
    assert (pieced, fallback) == (1, 1)


def test_decode_copy_across_a_boundary(ctx):
    """Two blocks whose second begins at an element boundary - the index is
    true - with a copy that reaches back into the first: the piece reports
    the offset, the stream is handed back and decodes."""
    rng = random.Random(9)
    a = rng.randbytes(65536)
    b = rng.randbytes(1000)
    out = bytearray(a)
    body1 = foreign.lit(a)
    body2 = foreign.copy(100, 64, 2)
    for _ in range(64):
        out.append(out[-100])
    body2 += foreign.lit(b)
    out += b
    stream = foreign.varint(len(out)) + body1 + body2
    hdr = len(foreign.varint(len(out)))
    idx = [hdr, hdr + len(body1), len(stream)]
    assert B.indexed(stream, len(out), idx, 0, 3, 3)
    assert O.decompress(stream) == bytes(out)
    # beside it: the same stream with the copy inside its block
    inner = foreign.varint(len(out)) + body1 + foreign.lit(b) \
        + foreign.copy(100, 64, 2)
    idx2 = [hdr, hdr + len(body1), len(inner)]
    pieced, fallback = same_as_unindexed(ctx, [stream, inner],
                                         [len(out)] * 2, [idx, idx2])
    assert (pieced, fallback) == (1, 1)


def test_decode_foreign_streams(ctx):
    """Streams no 64 KiB-block encoder writes (copy-4, offsets that cross
    64 KiB) with an index that passes the rule."""
    comps, caps, idxs = [], [], []
    for stream, out in foreign.cases():
        hdr = len(foreign.varint(len(out)))
        blocks = B.entries(len(out)) - 1
        step = (len(stream) - hdr) // blocks
        comps.append(stream)
        caps.append(len(out))
        idxs.append([hdr + k * step for k in range(blocks)] + [len(stream)])
    pieced, fallback = same_as_unindexed(ctx, comps, caps, idxs)
    assert pieced + fallback == sum(1 for c in caps if c > 65536)
    assert fallback > 0


def test_decode_error_kats_with_a_made_up_index(ctx):
    comps = [k[1] for k in kats.ERROR_KATS]
    caps = [64] * len(comps)
    idxs = [[1, max(len(c) // 2, 2), len(c)] for c in comps]
    pieced, fallback = same_as_unindexed(ctx, comps, caps, idxs)
    assert pieced == 0
    # (those never pass the rule: 64 bytes of room are one block.)  Through
    # the pieces and back: every KAT's elements behind a header that
    # announces two blocks, with room for them and an index that passes -
    # the first piece cannot fill its 64 KiB, the stream is handed back and
    # the batch launch names the error with whole-stream fields
    rng = random.Random(11)
    comps, caps, idxs = [], [], []
    for name, stream, _, bad_header in kats.ERROR_KATS:
        if bad_header or not stream:
            continue
        hdr0, _ = B.header(stream)
        body = stream[hdr0:]
        dlen = rng.randrange(65537, 131073)
        c = foreign.varint(dlen) + body
        assert len(body) >= 2, name
        idx = [3, 3 + rng.randrange(1, len(body)), len(c)]
        assert B.indexed(c, dlen, idx, 0, 3, 3), name
        comps.append(c)
        caps.append(dlen)
        idxs.append(idx)
    assert len(comps) >= 15
    pieced, fallback = same_as_unindexed(ctx, comps, caps, idxs)
    assert (pieced, fallback) == (0, len(comps))


def test_index_of_more_streams_than_one_workgroup_scans(ctx):
    """20 000 streams: first[] comes from the three-launch scan
    (k_index_first_a / _b / _c, beyond 16 384 streams), with multi-block
    streams in its first workgroup, behind stream 16 384 and last."""
    from rust_snappy_amd import batch
    rng = random.Random(21)
    text = (O.CORPUS / "alice29.txt").read_bytes()
    n = 20000
    lens = [rng.choice([0, 1, 17, 100, 255, 256, 300, 1023, 1500])
            for _ in range(n)]
    for pos, size in ((5, 65537), (1023, 131072), (1024, 3 * 65536 + 5),
                      (16384, 65537), (17000, 200000), (n - 1, 131073)):
        lens[pos] = size
    datas = []
    for size in lens:
        o = rng.randrange(len(text) - 1500) if size < 65536 else 0
        datas.append((text * 2)[o:o + size])
    want_first = [0]
    for size in lens:
        want_first.append(want_first[-1] + B.entries(size))
    cache = {}
    want = []
    for d in datas:
        if d not in cache:
            cache[d] = (B.expected_index(d), O.compress(d))
        want += cache[d][0]
    src = batch.StreamBatch.from_bytes(datas)
    enc, first, idx = batch.compress(ctx, src, want_index=True)
    assert first.cpu().tolist() == want_first
    assert idx.cpu().tolist() == want
    assert enc.lens.tolist() == [len(cache[d][1]) for d in datas]
    kinds = list(cache)
    at = {d: k for k, d in enumerate(kinds)}
    assert TB.assert_all(enc.data, enc.offsets, enc.lens,
                         [at[d] for d in datas],
                         [cache[d][1] for d in kinds],
                         what="20 000 streams compressed") == n
    dec, out_lens, errs = batch.decompress(ctx, enc, caps=lens,
                                           index=(first, idx))
    assert ctx.info("index_streams_pieced") == 6
    assert ctx.info("index_streams_fallback") == 0
    assert out_lens.tolist() == lens and all(e[0] == 0 for e in errs)
    host = dec.data.cpu().numpy()
    for i, d in enumerate(datas):
        o = int(dec.offsets[i])
        assert host[o:o + len(d)].tobytes() == d, i


@pytest.fixture(scope="module")
def seam_payloads():
    """length -> (payload, its index, its compressed stream): the six inputs
    the oracle sees for the seam batches below."""
    text = (O.CORPUS / "alice29.txt").read_bytes() * 2
    out = {}
    for k, size in enumerate((0, 1, 300, 2100, 65537, 131073)):
        d = text[1000 * k:1000 * k + size]
        out[size] = (d, B.expected_index(d), O.compress(d))
    return out


@pytest.mark.parametrize("n", [16384, 16385, 17408, 17409])
def test_planner_and_index_at_the_workgroup_seams(ctx, seam_payloads, n):
    """The planner's and the index's scans where one launch becomes three and
    where the last workgroup ends: 16 384 streams are the most the
    one-workgroup kernels take (k_plan_compress, k_index_first), one more goes
    to _a / _b / _c; 17 408 = 17 x 1 024 puts the last stream at the end of
    the last workgroup, 17 409 alone in an 18th.  Multi-block streams sit at
    the end of the first workgroup, at the start of the second and last."""
    from rust_snappy_amd import batch
    cycle = (0, 1, 300, 2100, 65537)
    lens = [cycle[i % 5] for i in range(n)]
    for pos in (1023, 1024, n - 1):
        lens[pos] = 131073
    datas = [seam_payloads[size][0] for size in lens]
    want_first, want = [0], []
    for size in lens:
        want_first.append(want_first[-1] + B.entries(size))
        want += seam_payloads[size][1]
    src = batch.StreamBatch.from_bytes(datas)
    enc, first, idx = batch.compress(ctx, src, want_index=True)
    assert first.cpu().tolist() == want_first
    assert idx.cpu().tolist() == want
    assert enc.lens.tolist() == [len(seam_payloads[size][2]) for size in lens]
    sizes = list(seam_payloads)
    assert TB.assert_all(enc.data, enc.offsets, enc.lens,
                         [sizes.index(size) for size in lens],
                         [seam_payloads[size][2] for size in sizes],
                         what=f"{n} streams compressed") == n
    dec, out_lens, errs = batch.decompress(ctx, enc, caps=lens,
                                           index=(first, idx))
    assert out_lens.tolist() == lens and all(e[0] == 0 for e in errs)
    host = dec.data.cpu().numpy()
    for i, d in enumerate(datas):
        o = int(dec.offsets[i])
        assert host[o:o + len(d)].tobytes() == d, i


def test_decode_more_long_streams_than_the_unindexed_path_takes(ctx):
    from rust_snappy_amd import batch
    n, size = 4100, 65537
    data = torch.zeros(n * (size + 15), dtype=torch.uint8, device="cuda")
    offs = np.arange(n, dtype=np.int64) * (size + 15)
    src = batch.StreamBatch(data, offs, [size] * n)
    enc, first, idx = batch.compress(ctx, src, want_index=True)
    assert idx.numel() == 3 * n
    one = O.compress(bytes(size))
    assert (enc.lens == len(one)).all()
    assert idx.view(n, 3)[0].tolist() == B.expected_index(bytes(size))
    assert (idx.view(n, 3) == idx.view(n, 3)[0]).all()
    dec, lens, errs = batch.decompress(ctx, enc, caps=[size] * n,
                                       index=(first, idx))
    assert ctx.info("index_streams_pieced") == n
    assert ctx.info("index_streams_fallback") == 0
    assert (lens == size).all() and all(e[0] == 0 for e in errs)
    # every output on the device against one expected tensor
    stride = int(dec.offsets[1] - dec.offsets[0])
    assert (np.diff(dec.offsets) == stride).all() and dec.offsets[0] == 0
    out = dec.data[:n * stride].view(n, stride)[:, :size]
    expected = torch.zeros(size, dtype=torch.uint8, device="cuda")
    assert bool((out == expected[None, :]).all())


def test_nothing_to_do(ctx):
    from rust_snappy_amd import raw
    empty = torch.zeros(0, dtype=torch.int64, device="cuda")
    raw.decompress_batch(ctx, empty, empty, empty, empty, empty, None,
                         index_first=empty, index=empty, index_entries=0)
    raw.compress_batch(ctx, empty, empty, empty, empty, empty, None,
                       host_in_lens=torch.zeros(0, dtype=torch.int64),
                       index_first=empty, index=empty, index_cap=0)
    ctx.synchronize()
    # streams, but no entries: the plain launch
    c = O.compress(b"hello" * 30000)
    pieced, fallback = same_as_unindexed(ctx, [c], [150000], [[]])
    assert pieced == fallback == 0
