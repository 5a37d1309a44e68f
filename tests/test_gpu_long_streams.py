"""GPU suite: the long-stream decoder (k_long_plan, k_bstream_*) at full scale
and at its batch limits.

The streams come from tests/long_streams.py: distinct, stamped 64 KiB blocks
of text, incompressible bytes, zeros and runs, and 2-4-symbol noise, so a
piece decoded into the wrong place, or into another stream, cannot match.
tests/test_long_streams_cpu.py pins the plan geometry every shape here
reaches.  Valid streams are compared byte for byte with the known input
(large ones on the device, against the pool), errors with the oracle's
(kind, a, b, c) at the same capacity, and every output lies between bands of
0xA5 that must stay intact.

  a. lone streams (snapmi_decompress_stream) from 6 MiB to 315 MiB: scan
     groups of 8 .. 64 segments by size, both sides of the 256 MiB switch
     to 4 KiB segments, and more than 64 level-3 blocks at 1 KiB segments;
  b. the format's limits: 2^32 - 65536 and 2^32 - 1 output bytes (65535 and
     65536 pieces, kmax 65537, 74 level-3 blocks), and a buffer one short;
  c. errors at scale, one of them past 2^31 output bytes;
  d. batches at kBatchLongMaxL (4096 long streams) and one over, at
     kBatchLongMaxN (16384 streams) and one over, and a batch of every kind
     of long stream at once, each with batch_long_streams on and off;
  e. batches whose long bytes are just under and just over 256 MiB.
"""
import resource
import time

import numpy as np
import pytest
import torch

import long_streams as LS
import oracle_lib as O
from conftest import set_scan_geometry
from test_gpu_bounds import GUARD, Guarded, read_errs

pytestmark = pytest.mark.gpu

BAND = 4096          # guard bytes in front of and behind a lone output
CHUNK = 4096         # blocks compared per step on the device (256 MiB)


@pytest.fixture(scope="module")
def lctx(built):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import rust_snappy_amd as R
    c = R.raw.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def dpool(lctx):
    return torch.from_numpy(LS.pool().raw).cuda()


@pytest.fixture(autouse=True)
def report(request):
    """Wall time and peak memory of each case (pytest -s shows them)."""
    if torch.cuda.is_available():
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    yield
    if torch.cuda.is_available():
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() / 2**30
        torch.cuda.empty_cache()
        host = resource.getrusage(resource.RUSAGE_SELF).ru_maxrss / 2**20
        print(f"\n[long-streams] {request.node.name}: "
              f"{time.perf_counter() - t0:.1f} s, torch peak {peak:.2f} GiB, "
              f"host peak {host:.2f} GiB")


def to_device(comp):
    """comp at the very end of an allocation of a 2 MiB multiple: a read
    behind the stream leaves the allocation."""
    n = len(comp)
    room = max((n + (2 << 20) - 1) // (2 << 20) * (2 << 20), 2 << 20)
    big = torch.empty(room, dtype=torch.uint8, device="cuda")
    d = big[room - n:]
    if n:
        d.copy_(torch.frombuffer(bytearray(comp), dtype=torch.uint8))
    return big, d


def decode_lone(ctx, comp, cap):
    """snapmi_decompress_stream into exactly cap bytes between guard bands:
    (slab, out, out_len, error, seconds of the call)."""
    from rust_snappy_amd import raw
    big, d_in = to_device(comp)
    slab = torch.full((BAND + cap + BAND,), GUARD, dtype=torch.uint8,
                      device="cuda")
    out = slab[BAND:BAND + cap]
    out_len = torch.zeros(1, dtype=torch.int64, device="cuda")
    err = torch.zeros(32, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    raw.decompress_stream(ctx, d_in, len(comp), out, out_len, err)
    ctx.synchronize()
    dt = time.perf_counter() - t0
    del big, d_in
    assert bool((slab[:BAND] == GUARD).all()), "guard in front overwritten"
    assert bool((slab[BAND + cap:] == GUARD).all()), \
        "guard behind the output overwritten"
    return slab, out, int(out_len.item()), read_errs(err)[0], dt


def assert_output(out, st, dpool):
    """out (device) holds stream st's blocks, compared in slices."""
    n, B = len(st.idx), LS.BLOCK
    didx = torch.from_numpy(st.idx).cuda()
    full = out[:n * B].view(n, B)
    for a in range(0, n, CHUNK):
        b = min(n, a + CHUNK)
        bad = (full[a:b] != dpool.index_select(0, didx[a:b])).any(dim=1)
        if bool(bad.any()):
            k = a + int(torch.nonzero(bad)[0])
            row = (full[k] != dpool[st.idx[k]]).nonzero()
            raise AssertionError(
                f"block {k} of {n} (pool {st.idx[k]}, "
                f"{st.pool.kinds[st.idx[k]]}) differs from byte "
                f"{int(row[0])} on")
    t = len(st.tail)
    if t:
        want = torch.from_numpy(st.tail.copy()).cuda()
        assert bool((out[n * B:n * B + t] == want).all()), "the tail differs"


def lone_valid(ctx, st, dpool, cap=None):
    from rust_snappy_amd import raw
    comp = st.bytes()
    assert len(comp) == st.in_len
    slab, out, n, e, dt = decode_lone(ctx, comp, st.dlen if cap is None
                                      else cap)
    del comp
    assert e[0] == 0, e
    assert n == st.dlen
    assert_output(out, st, dpool)
    # a stream of 64 KiB blocks never needs the sequential decoder
    assert raw.stream_decode_path(ctx) == 0
    print(f"\n[long-streams] in {st.in_len} out {st.dlen}: decode "
          f"{dt * 1e3:.1f} ms")
    del slab, out


# ---------------------------------------------------------------------
# a. lone streams
# ---------------------------------------------------------------------
@pytest.mark.parametrize("name", list(LS.LADDER))
def test_lone_stream_ladder(lctx, dpool, name):
    _, forced = LS.LADDER[name]
    set_scan_geometry(lctx, forced)
    try:
        lone_valid(lctx, LS.ladder(name), dpool)
    finally:
        set_scan_geometry(lctx, None)


@pytest.mark.parametrize("seed", [1, 2])
def test_lone_foreign_long_literals(lctx, seed):
    """Literals of 1 MiB and 16 MiB with copy-4 elements behind them that
    reach back across pieces: the cuts kernel hands such a stream to the
    sequential decoder."""
    comp, want = LS.foreign_long(seed)
    slab, out, n, e, _ = decode_lone(lctx, comp, len(want))
    assert e[0] == 0 and n == len(want), e
    assert out.cpu().numpy().tobytes() == want


# ---------------------------------------------------------------------
# b. the format's limits
# ---------------------------------------------------------------------
def oracle_header_error(stream, cap):
    """The oracle's error for a stream whose header announces more than cap:
    it is reported from the header, before any output, so the stream's
    first bytes and a one-byte buffer are enough."""
    out = (O.C.c_char * 1)()
    n = O.C.c_size_t(0)
    e = O.OracleError()
    k = O.lib().snapo_decompress(bytes(stream), len(stream), out, cap,
                                 O.C.byref(n), O.C.byref(e))
    assert k == O.KIND_NAMES.index("BufferTooSmall"), e.astuple()
    return e.astuple()


@pytest.mark.parametrize("tail", [False, True], ids=["2^32-65536", "2^32-1"])
def test_format_limits(lctx, dpool, tail):
    st = LS.limit(tail)
    lone_valid(lctx, st, dpool)
    # a buffer one byte short: BufferTooSmall, as the oracle gives it
    cap = st.dlen - 1
    comp = st.bytes()
    slab, _, _, e, _ = decode_lone(lctx, comp, cap)
    del slab
    assert e == oracle_header_error(comp[:4096], cap), e


# ---------------------------------------------------------------------
# c. errors at scale
# ---------------------------------------------------------------------
@pytest.mark.parametrize("name", LS.ERROR_CASES)
def test_errors_at_scale(lctx, name):
    from rust_snappy_amd import raw
    comp, cap, _ = LS.error_case(name)
    with pytest.raises(O.SnapError) as oe:
        O.decompress(comp, cap)
    want = (oe.value.kind, oe.value.a, oe.value.b, oe.value.c)
    if name == "beyond2g":
        assert oe.value.name == "Offset" and oe.value.b > (1 << 31), want
    slab, _, _, e, dt = decode_lone(lctx, comp, cap)
    del slab
    assert e == want, (e, oe.value)
    assert raw.stream_decode_path(lctx) == 1
    print(f"\n[long-streams] {name}: in {len(comp)} cap {cap} "
          f"{oe.value}: {dt:.2f} s")


# ---------------------------------------------------------------------
# d, e. batches
# ---------------------------------------------------------------------
def decode_batch(ctx, comps, caps, seed):
    """decode_guarded of test_gpu_bounds.py for slabs of a GiB: the bands
    are checked one by one, without a map of the slab."""
    from rust_snappy_amd import raw
    n = len(comps)
    src = Guarded([max(len(c), 1) for c in comps], seed + 1, False, comps)
    d_in_lens = torch.tensor([len(c) for c in comps], dtype=torch.int64,
                             device="cuda")
    dst = Guarded(caps, seed, False)
    out_lens = torch.zeros(n, dtype=torch.int64, device="cuda")
    errs = torch.zeros(32 * n, dtype=torch.uint8, device="cuda")
    raw.decompress_batch(ctx, src.d_ptrs, d_in_lens, dst.d_ptrs, dst.d_caps,
                         out_lens, errs)
    ctx.synchronize()
    del src
    host = dst.fetch()
    ends = dst.offs + np.array(caps, dtype=np.int64)
    starts = np.append(dst.offs[1:], dst.size)
    assert (host[:dst.offs[0]] == GUARD).all()
    for i in range(n):
        assert (host[ends[i]:starts[i]] == GUARD).all(), \
            f"guard behind buffer {i} (cap {caps[i]}) overwritten"
    return dst, out_lens.cpu().numpy(), read_errs(errs)


def check_batch(ctx, items, seed):
    """Decode the batch in guarded buffers; every stream against its known
    output or the oracle.  Returns (lens, errs) for the comparison of the
    two settings."""
    comps = [s.bytes() if isinstance(s, LS.Stream) else s for s, _ in items]
    caps = [c for _, c in items]
    dst, lens, errs = decode_batch(ctx, comps, caps, seed)
    for i, ((src, cap), comp) in enumerate(zip(items, comps)):
        if isinstance(src, LS.Stream) and cap >= src.dlen:
            assert errs[i][0] == 0 and lens[i] == src.dlen, (i, errs[i])
            assert dst.bytes(i, lens[i]) == src.expected(), i
            continue
        try:
            want = O.decompress(comp, cap)
            assert errs[i][0] == 0 and dst.bytes(i, lens[i]) == want, \
                (i, errs[i])
        except O.SnapError as oe:
            assert (oe.kind, oe.a, oe.b, oe.c) == errs[i], (i, errs[i], oe)
    ok = np.array([e[0] == 0 for e in errs])
    return np.where(ok, lens, -1), errs


def batch_on_off(ctx, name, geom):
    items = LS.batch_items(name)
    set_scan_geometry(ctx, geom)
    try:
        got = []
        for on in (1, 0):
            ctx.set_option("batch_long_streams", on)
            t0 = time.perf_counter()
            got.append(check_batch(ctx, items, 40 + on))
            print(f"\n[long-streams] {name} batch_long_streams={on}: "
                  f"{time.perf_counter() - t0:.1f} s")
    finally:
        ctx.set_option("batch_long_streams", 1)
        set_scan_geometry(ctx, None)
    (l1, e1), (l0, e0) = got
    assert np.array_equal(l1, l0)
    assert e1 == e0


@pytest.mark.parametrize("name", ["long4096", "long4097", "n16384",
                                  "n16385"])
def test_batch_limits(lctx, name):
    batch_on_off(lctx, name, None)


def test_batch_of_every_long_kind(lctx):
    """At forced 1 KiB segments: a stream of 75 level-3 blocks (two spread3
    workgroups), a thousand streams of the rule's minimum size, corrupt and
    truncated long streams, long streams whose buffer is a byte short."""
    batch_on_off(lctx, "mixed", (10, 0))


@pytest.mark.parametrize("side", ["under256", "over256"])
def test_batch_natural_geometry(lctx, side):
    set_scan_geometry(lctx, None)
    lctx.set_option("batch_long_streams", 1)
    check_batch(lctx, LS.batch_items(side), 50)
