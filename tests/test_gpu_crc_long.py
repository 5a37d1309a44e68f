"""GPU suite: masked CRC32C of buffers of any length
(snapmi_crc32c_masked_batch past its old limit of 64 KiB a buffer).

Every result is the CPU codec's; where that would take gigabytes of host
work (one buffer past 2^32 bytes) it is the model's of tests/crc_ref.py,
which tests/test_crc_long_cpu.py ties to the CPU codec.  The enqueue-only
form (frame.crc32c_masked_ptrs) is what runs; both libraries."""
import random

import numpy as np
import pytest
import torch

import crc_ref as M
import oracle_lib as O
from gpu_buffers import Slab

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A5A5A  # what d_out holds in front of a call


@pytest.fixture(scope="module", autouse=True)
def _gpu(built):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def make_context(library, stream=None):
    import rust_snappy_amd as R
    lib = R._lib.load_product() if library == "product" else None
    return R.raw.Context(0, stream=stream.cuda_stream if stream else None,
                         lib=lib)


@pytest.fixture(scope="module", params=["test", "product"])
def lctx(request):
    c = make_context(request.param)
    yield c
    c.close()


def seg():
    from rust_snappy_amd import frame
    return frame.CRC_SEGMENT


def i64(values):
    return torch.tensor([int(v) for v in values], dtype=torch.int64,
                        device="cuda")


def u32(t):
    return [int(v) & 0xFFFFFFFF for v in t.cpu().tolist()]


_want = {}


def want(key, make):
    """The CPU codec's answer, computed once for both libraries."""
    if key not in _want:
        _want[key] = O.crc32c_masked(make())
    return _want[key]


# --------------------------------------------------------------------
# 1. single buffers
# --------------------------------------------------------------------
def single_lengths():
    S = seg()
    return [65536, 65537, 65536 + 255, 65536 + 256, 131072, S - 1, S, S + 1,
            3 * S + 17, (1 << 20) + 1, (5 << 20) + 3]


@pytest.fixture(scope="module")
def single_host():
    n = max(single_lengths()) + 3
    rng = np.random.default_rng(0xC3C)
    return {"random": rng.integers(0, 256, n, dtype=np.uint8),
            "zero": np.zeros(n, dtype=np.uint8),
            "ff": np.full(n, 0xFF, dtype=np.uint8)}


@pytest.mark.parametrize("kind", ["random", "zero", "ff"])
def test_single_buffers(lctx, single_host, kind):
    """One call per buffer (n = 1): lengths on both sides of the old limit,
    of a step and of a segment, at every alignment of the first byte."""
    from rust_snappy_amd import frame
    host = single_host[kind]
    dev = torch.from_numpy(host).cuda()
    cases = [(n, off) for n in single_lengths() for off in range(4)]
    ptrs = i64([dev.data_ptr() + off for _, off in cases])
    lens = i64([n for n, _ in cases])
    out = torch.full((len(cases),), SENTINEL, dtype=torch.int32,
                     device="cuda")
    torch.cuda.synchronize()
    for k in range(len(cases)):
        frame.crc32c_masked_ptrs(lctx, ptrs[k:k + 1], lens[k:k + 1],
                                 out[k:k + 1])
    lctx.synchronize()
    for (n, off), got in zip(cases, u32(out)):
        o = off if kind == "random" else 0
        exp = want((kind, n, o), lambda: host[o:o + n].tobytes())
        assert got == exp, (kind, n, off, hex(got), hex(exp))


def test_python_forms(lctx, single_host):
    """frame.crc32c_masked of bytes and of a device tensor, and
    crc32c_masked_many of a mixed list, past 64 KiB."""
    from rust_snappy_amd import frame
    host = single_host["random"]
    n = 65536 + 255
    exp = want(("random", n, 1), lambda: host[1:1 + n].tobytes())
    assert frame.crc32c_masked(lctx, host[1:1 + n].tobytes()) == exp
    dev = torch.from_numpy(host[:200000]).cuda()
    assert frame.crc32c_masked(lctx, dev[1:1 + n]) == exp
    got = frame.crc32c_masked_many(lctx, [b"", dev[1:1 + n], b"123456789",
                                          host[:70000].tobytes()])
    assert got == [O.crc32c_masked(b""), exp, 0xC78AB0E5,
                   O.crc32c_masked(host[:70000].tobytes())]
    assert frame.crc32c_masked_many(lctx, []) == []


# --------------------------------------------------------------------
# 2. one mixed batch
# --------------------------------------------------------------------
@pytest.fixture(scope="module")
def mixed():
    S = seg()
    rng = random.Random(0xB47C)
    pick = [0, 1, 255, 256, 4096, 65536, 65537, 200000, 2 * S,
            (3 << 20) + 5]
    lens = pick * 4          # every length four times: 40 buffers
    rng.shuffle(lens)
    nrng = np.random.default_rng(5)
    datas = [nrng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in lens]
    return lens, datas, [O.crc32c_masked(d) for d in datas]


def test_mixed_batch_in_one_call(lctx, mixed):
    """Short, empty and long buffers shuffled into one call, at every
    alignment (gpu_buffers.Slab); d_out lies between guard words."""
    from rust_snappy_amd import frame
    lens, datas, exp = mixed
    n = len(lens)
    src = Slab(lens, seed=11, fill=datas)
    band = 64
    out = torch.full((n + 2 * band,), SENTINEL, dtype=torch.int32,
                     device="cuda")
    d_lens = i64(lens)
    torch.cuda.synchronize()
    frame.crc32c_masked_ptrs(lctx, src.d_ptrs, d_lens, out[band:band + n])
    lctx.synchronize()
    got = u32(out)
    assert got[band:band + n] == exp, [
        (i, lens[i]) for i in range(n) if got[band + i] != exp[i]]
    guard = SENTINEL & 0xFFFFFFFF
    assert set(got[:band]) == {guard} and set(got[band + n:]) == {guard}
    src.assert_guards("inputs")     # (they are only read)
    assert d_lens.cpu().tolist() == lens


# --------------------------------------------------------------------
# 3. past 32 bits
# --------------------------------------------------------------------
def test_one_buffer_past_4_gib(built):
    """2^32 + 5 zero bytes - a length whose low 32 bits say 5 -, then the
    same buffer with random bytes at its end.  4 GiB are allocated once, for
    both libraries, and freed."""
    from rust_snappy_amd import frame
    n, tail_n = (1 << 32) + 5, 70000
    tail = np.random.default_rng(77).integers(0, 256, tail_n, dtype=np.uint8)
    exp_zero = M.mask(M.crc32c_zeros(n))
    exp_tail = M.mask(M.combine(M.crc32c_zeros(n - tail_n),
                                O.crc32c(tail.tobytes()), tail_n))
    assert exp_zero != M.mask(M.crc32c_zeros(5))
    buf = torch.zeros(n, dtype=torch.uint8, device="cuda")
    try:
        ptrs, lens = i64([buf.data_ptr()]), i64([n])
        outs = {}
        for library in ("test", "product"):
            ctx = make_context(library)
            try:
                out = torch.full((2,), SENTINEL, dtype=torch.int32,
                                 device="cuda")
                buf[n - tail_n:].zero_()
                torch.cuda.synchronize()
                frame.crc32c_masked_ptrs(ctx, ptrs, lens, out[0:1])
                ctx.synchronize()
                buf[n - tail_n:].copy_(torch.from_numpy(tail))
                torch.cuda.synchronize()
                frame.crc32c_masked_ptrs(ctx, ptrs, lens, out[1:2])
                ctx.synchronize()
                outs[library] = u32(out)
            finally:
                ctx.close()
    finally:
        del buf
        torch.cuda.empty_cache()
    for library, got in outs.items():
        assert got == [exp_zero, exp_tail], (library, [hex(g) for g in got])


# --------------------------------------------------------------------
# 4. enqueue-only and capturable
# --------------------------------------------------------------------
@pytest.mark.parametrize("library", ["test", "product"])
def test_graph_capture_and_replay(built, library):
    """One eager call on a context over a torch stream, the identical call
    captured, then replays over lengths and bytes rewritten in place: all
    long, all short, mixed with an empty buffer; d_out reset to a sentinel in
    front of every replay; two replays with no wait between; the scratch does
    not grow."""
    from rust_snappy_amd import frame
    S = seg()
    cap = 3 * S + 64
    nbuf = 6
    rng = np.random.default_rng(0x6A)
    lens_of = {
        "eager": [S + 1, 65536, 2 * S + 17, 0, 65537, 300],
        "long": [65537, S, S + 1, 3 * S + 17, 2 * S - 1, 100000],
        "short": [0, 1, 255, 65536, 4096, 300],
        "mixed": [3 * S, 0, 65536, 65537, 7, 2 * S + 255],
    }
    images = {k: rng.integers(0, 256, nbuf * cap, dtype=np.uint8)
              for k in lens_of}

    def expected(k):
        return [want(("graph", k, i),
                     lambda: images[k][i * cap + 1:i * cap + 1 + n].tobytes())
                for i, n in enumerate(lens_of[k])]

    stream = torch.cuda.Stream()
    ctx = make_context(library, stream)
    try:
        with torch.cuda.stream(stream):
            pool = torch.zeros(nbuf * cap, dtype=torch.uint8, device="cuda")
            # (every buffer starts one byte into its room: odd addresses)
            ptrs = i64([pool.data_ptr() + i * cap + 1 for i in range(nbuf)])
            lens = i64([0] * nbuf)
            out = torch.zeros(nbuf, dtype=torch.int32, device="cuda")

            def load(k):
                pool.copy_(torch.from_numpy(images[k]))
                lens.copy_(torch.tensor(lens_of[k], dtype=torch.int64))
                out.fill_(SENTINEL)

            def check(what, k):
                stream.synchronize()
                assert u32(out) == expected(k), (what, k)

            load("eager")
            frame.crc32c_masked_ptrs(ctx, ptrs, lens, out)  # scratch, tables
            check("eager", "eager")
            scratch = ctx.info("scratch_bytes")
            assert scratch > 0
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=stream):
                frame.crc32c_masked_ptrs(ctx, ptrs, lens, out)
            for k in ("long", "short", "mixed"):
                load(k)
                g.replay()
                check("replay", k)
            load("long")
            g.replay()
            g.replay()
            check("two replays, no wait between", "long")
            assert ctx.info("scratch_bytes") == scratch
    finally:
        ctx.close()
