"""The host-memory batch calls (snapmi_compress_batch_host /
snapmi_decompress_batch_host) on the CPU: their plan
(csrc/snapmi_hostbatch.hpp, compiled for the host as test_route_cpu.py does
with the route header) - which streams form a slice, where they lie, and
which thread of k_hb_pack copies which byte of the packed output -, the
exports and bindings, the option and info names, and the loud failure without
a GPU."""
import ctypes as C
import random
import subprocess

import numpy as np
import pytest
import torch

from conftest import ROOT

LENGTHS = [0, 1, 15, 16, 17, 4095, 4096, 4097, 65536]
E_DEVICE, E_ARGUMENT = 100, 101


@pytest.fixture(scope="module")
def H(tmp_path_factory):
    so = tmp_path_factory.mktemp("hostbatch") / "hostbatch_host.so"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-shared",
                           "-fPIC", str(ROOT / "tests" / "hostbatch_host.cpp"),
                           "-o", str(so)])
    L = C.CDLL(str(so))
    u64, p = C.c_uint64, C.c_void_p
    L.t_tile_bytes.restype = u64
    L.t_max_slice_streams.restype = u64
    L.t_plan.restype = C.c_size_t
    L.t_plan.argtypes = [p, p, C.c_size_t, u64, u64, p, C.c_size_t, p, p]
    L.t_pack.restype = u64
    L.t_pack.argtypes = [p, p, C.c_uint32, C.c_uint32, p, p, p, p]
    return L


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def align(x):
    return (x + 15) // 16 * 16


def plan(H, in_lens, rooms, in_limit, out_limit=2**64 - 1):
    in_lens = np.asarray(in_lens, dtype=np.uint64)
    rooms = np.asarray(rooms, dtype=np.uint64)
    n = len(in_lens)
    slices = np.zeros(5 * (n + 1), dtype=np.uint64)
    in_offs = np.zeros(n + 1, dtype=np.uint64)
    out_offs = np.zeros(n + 1, dtype=np.uint64)
    k = H.t_plan(ptr(in_lens), ptr(rooms), n, in_limit, out_limit,
                 ptr(slices), n + 1, ptr(in_offs), ptr(out_offs))
    assert k <= n
    return ([tuple(int(v) for v in slices[5 * i:5 * i + 5])
             for i in range(k)], in_offs[:n], out_offs[:n])


def check_plan(in_lens, rooms, in_limit, out_limit, slices, in_offs,
               out_offs):
    n = len(in_lens)
    # the slices tile the batch in order
    assert slices[0][0] == 0 and slices[-1][1] == n
    for a, b in zip(slices, slices[1:]):
        assert a[1] == b[0]
    for s0, s1, in_raw, in_bytes, out_bytes in slices:
        assert s1 > s0
        assert in_raw == sum(in_lens[s0:s1])
        # no slice exceeds a limit, except a lone oversized stream
        if s1 - s0 > 1:
            assert in_raw <= in_limit
            assert sum(rooms[s0:s1]) <= out_limit
        # 16-aligned, disjoint, in order, inside the slabs; the slack the
        # kernels read behind an input is the stream's own
        pos_in = pos_out = 0
        for i in range(s0, s1):
            assert in_offs[i] % 16 == 0 and out_offs[i] % 16 == 0
            assert in_offs[i] >= pos_in and out_offs[i] >= pos_out
            pos_in = int(in_offs[i]) + in_lens[i] + 16
            pos_out = int(out_offs[i]) + rooms[i]
        assert pos_in <= in_bytes and pos_out <= out_bytes
        assert in_bytes == sum(align(x + 16) for x in in_lens[s0:s1])
        assert out_bytes == sum(align(x) for x in rooms[s0:s1])
    # greedy: a slice ends only where the next stream would not fit
    for (s0, s1, in_raw, _, _), nxt in zip(slices, slices[1:]):
        if s1 - s0 < 2**20:
            assert (in_raw + in_lens[s1] > in_limit
                    or sum(rooms[s0:s1]) + rooms[s1] > out_limit)


def test_slices_tile_the_batch_within_the_limit(H):
    rng = random.Random(1)
    for limit in (65536, 100_000, 1 << 20):
        lens = [rng.choice(LENGTHS + [200, 70_000, 300_000, 2_000_000])
                for _ in range(400)]
        rooms = [32 + x + x // 6 for x in lens]
        slices, io, oo = plan(H, lens, rooms, limit)
        check_plan(lens, rooms, limit, 2**64 - 1, slices, io, oo)
        assert len(slices) >= 4
        # a stream larger than the limit is a slice of its own
        for s0, s1, in_raw, _, _ in slices:
            if in_raw > limit:
                assert s1 - s0 == 1
    assert any(x > 1 << 20 for x in lens)


def test_output_limit_cuts_a_slice_too(H):
    # decompression: small inputs that announce large outputs
    lens = [100] * 50
    rooms = [60_000] * 50
    slices, io, oo = plan(H, lens, rooms, 65536, 4 * 65536)
    check_plan(lens, rooms, 65536, 4 * 65536, slices, io, oo)
    assert [s[1] - s[0] for s in slices[:-1]] == [4] * (len(slices) - 1)
    # rooms of 0 (streams that will be refused) take no room
    slices, io, oo = plan(H, [10, 20, 30], [0, 0, 5], 65536)
    assert slices == [(0, 3, 60, 32 + 48 + 48, 16)]
    assert list(oo) == [0, 0, 0] and list(io) == [0, 32, 80]


def test_one_stream_and_exact_fit(H):
    assert plan(H, [0], [32], 65536)[0] == [(0, 1, 0, 16, 32)]
    slices, _, _ = plan(H, [65536, 1, 65535, 1], [1, 1, 1, 1], 65536)
    assert [(s[0], s[1]) for s in slices] == [(0, 1), (1, 3), (3, 4)]


def test_many_empty_streams_are_cut_by_count(H):
    most = H.t_max_slice_streams()
    n = most + 5
    slices, _, _ = plan(H, np.zeros(n, dtype=np.uint64),
                        np.zeros(n, dtype=np.uint64), 65536)
    assert [(s[0], s[1]) for s in slices] == [(0, most), (most, n)]


def pack(H, lens, ok=None, grid=7):
    lens = np.asarray(lens, dtype=np.uint64)
    n = len(lens)
    ok = np.ones(n, dtype=np.uint8) if ok is None \
        else np.asarray(ok, dtype=np.uint8)
    room = int(sum(align(int(x)) for x in lens)) + 16
    offs = np.zeros(n + 1, dtype=np.uint64)
    count = np.zeros(room, dtype=np.uint32)
    stream = np.full(room, 0xFFFFFFFF, dtype=np.uint32)
    src = np.zeros(room, dtype=np.uint64)
    total = H.t_pack(ptr(lens), ptr(ok), n, grid, ptr(offs), ptr(count),
                     ptr(stream), ptr(src))
    return total, offs, count, stream, src


def check_pack(lens, ok, total, offs, count, stream, src):
    want = np.zeros(len(count), dtype=np.uint32)
    pos = 0
    for i, x in enumerate(lens):
        assert offs[i] == pos and pos % 16 == 0
        if not ok[i]:
            continue
        x = int(x)
        # every byte of the stream exactly once, from its own place
        assert (stream[pos:pos + x] == i).all(), i
        assert (src[pos:pos + x] == np.arange(x, dtype=np.uint64)).all(), i
        want[pos:pos + x] = 1
        pos += align(x)
    assert total == pos == offs[len(lens)]
    # ... and nothing else: not the padding, not a failed stream's bytes
    assert (count == want).all()


def test_pack_covers_every_packed_byte_exactly_once(H):
    assert H.t_tile_bytes() == 4096
    rng = random.Random(2)
    for trial in range(6):
        lens = LENGTHS * 3
        rng.shuffle(lens)
        ok = [1] * len(lens)
        check_pack(lens, ok, *pack(H, lens, ok, grid=rng.choice([1, 3, 64])))
    for x in LENGTHS:                      # every length alone, and in pairs
        check_pack([x], [1], *pack(H, [x]))
        for y in LENGTHS:
            check_pack([x, y], [1, 1], *pack(H, [x, y]))


def test_pack_skips_a_run_of_empty_streams(H):
    for a, b in ((17, 4097), (4096, 1), (1, 1), (65536, 65536)):
        lens = [a] + [0] * 1000 + [b]
        ok = [1] * len(lens)
        check_pack(lens, ok, *pack(H, lens, ok))
    # empty streams first and last
    lens = [0] * 1000 + [5000] + [0] * 1000
    check_pack(lens, [1] * len(lens), *pack(H, lens))
    # nothing at all
    total, offs, count, _, _ = pack(H, [0, 0, 0])
    assert total == 0 and not count.any()


def test_pack_leaves_failed_streams_out(H):
    rng = random.Random(3)
    lens = [rng.choice(LENGTHS[1:]) for _ in range(200)]
    ok = [rng.random() < 0.7 for _ in lens]
    ok[0] = ok[-1] = False
    check_pack(lens, ok, *pack(H, lens, ok))
    check_pack(lens, [0] * len(lens), *pack(H, lens, [0] * len(lens)))


def test_pack_many_small_streams_and_one_large(H):
    rng = random.Random(4)
    lens = [rng.randrange(1, 300) for _ in range(20_000)]
    check_pack(lens, [1] * len(lens), *pack(H, lens, grid=256))
    check_pack([3_000_001], [1], *pack(H, [3_000_001], grid=256))


def test_symbols_are_exported_and_bound(built):
    from rust_snappy_amd import _lib
    bound = dict((s[0], s) for s in _lib.SYMBOLS)
    for L in (_lib.load(), _lib.load_product()):
        for name in ("snapmi_compress_batch_host",
                     "snapmi_decompress_batch_host"):
            f = getattr(L, name)
            assert name in bound and len(bound[name][2]) == 8
            assert f.argtypes == bound[name][2] and f.restype is C.c_int
    for m in ("snapmi.map", "snapmi_test.map"):
        text = (ROOT / "rust-snappy_amd" / "csrc" / m).read_text()
        assert "snapmi_compress_batch_host;" in text
        assert "snapmi_decompress_batch_host;" in text
    from rust_snappy_amd import raw
    assert callable(raw.compress_many) and callable(raw.decompress_many)


def test_library_carries_the_pack_kernel(built):
    for lib in ("libsnapmi.so", "libsnapmi_test.so"):
        blob = (ROOT / "rust-snappy_amd" / lib).read_bytes()
        assert b"k_hb_pack" in blob and b"k_hb_sizes" in blob, lib


def test_option_and_info_names_in_the_sources():
    """A context cannot be made without a GPU (the GPU suite sets and reads
    them); what is checked here: the names the header documents are names of
    the library's tables (csrc/snapmi_options.hpp)."""
    from test_options_cpu import options_table
    T = options_table()
    header = (ROOT / "include" / "snapmi.h").read_text()
    for name in ("host_batch_slice", "host_batch_slices",
                 "host_batch_h2d_bytes", "host_batch_d2h_bytes"):
        assert f'"{name}"' in header, name
    assert T.has_option("host_batch_slice", test_only=False)
    for name in ("host_batch_slices", "host_batch_h2d_bytes",
                 "host_batch_d2h_bytes"):
        assert T.has_info(name), name


def test_null_context_names_are_refused(built):
    """Without a context the option and info calls are E_ARGUMENT whatever
    the name - the accepted names need a device (GPU suite)."""
    from rust_snappy_amd import _lib
    L = _lib.load()
    v = C.c_int64(7)
    assert L.snapmi_ctx_set_option(None, b"host_batch_slice", 65536) == \
        E_ARGUMENT
    assert L.snapmi_ctx_get_info(None, b"host_batch_slices", C.byref(v)) == \
        E_ARGUMENT
    assert v.value == 7


@pytest.mark.skipif(torch.cuda.is_available(), reason="GPU present")
def test_no_gpu_fails_loudly(built):
    """No context can be made, so the calls get none: SNAPMI_E_DEVICE, and
    not one byte of the outputs, the lengths or the errors is written -
    never a silent CPU result."""
    import rust_snappy_amd as R
    from rust_snappy_amd import _lib, raw
    with pytest.raises(R.DeviceError):
        raw.compress_many([b"hello"])
    with pytest.raises(R.DeviceError):
        raw.decompress_many([b"\x05\x10hello"])
    L = _lib.load()
    data = np.frombuffer(b"hello world, hello world", dtype=np.uint8).copy()
    out = np.full(128, 0xA5, dtype=np.uint8)
    in_ptrs = np.array([data.ctypes.data], dtype=np.uint64)
    in_lens = np.array([data.size], dtype=np.uint64)
    out_ptrs = np.array([out.ctypes.data], dtype=np.uint64)
    out_caps = np.array([out.size], dtype=np.uint64)
    out_lens = np.array([77], dtype=np.uint64)
    errs = np.full(32, 0x5A, dtype=np.uint8)
    for f in (L.snapmi_compress_batch_host, L.snapmi_decompress_batch_host):
        rc = f(None, ptr(in_ptrs), ptr(in_lens), ptr(out_ptrs),
               ptr(out_caps), ptr(out_lens), ptr(errs), 1)
        assert rc == E_DEVICE
        assert (out == 0xA5).all() and out_lens[0] == 77
        assert (errs == 0x5A).all()
