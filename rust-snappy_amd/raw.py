"""snap::raw -- host-side mirror of the reference's raw block API
(src/raw.rs:13-14) on top of the C ABI of libsnapmi.so.

  max_compress_len(n)            reference src/compress.rs:42-53
  decompress_len(buf)            reference src/decompress.rs:30-35
  Encoder().compress / compress_vec   reference src/compress.rs:99-169
  Decoder().decompress / decompress_vec  reference src/decompress.rs:75-110

plus the batched, device-resident form (`compress_batch`, `decompress_batch`)
that takes torch CUDA tensors -- torch is only the owner of device memory --
and the batched host-memory form (`compress_many`, `decompress_many`) over
sequences of bytes-like objects.
All compute happens in the HIP kernels; without a GPU these raise
`DeviceError`.
"""
import ctypes as C

import numpy as np

from . import _lib
from .error import DeviceError, Error

MAX_INPUT_SIZE = 0xFFFFFFFF  # reference src/lib.rs:93
MAX_BLOCK_SIZE = 1 << 16     # reference src/lib.rs:97


def _raise(ctx, rc, err=None):
    if rc >= 100:
        msg = None
        if ctx is not None and ctx._h:
            msg = _lib.of(ctx).snapmi_last_error(ctx._h).decode()
        raise DeviceError(rc, message=msg or "no usable HIP device")
    if err is not None and err.kind == rc:
        raise Error(rc, err.a, err.b, err.c)
    raise Error(rc)


class TestOnlyOption(RuntimeError):
    """set_test_option on a context of the product library (the knobs of
    include/snapmi_test.h exist in libsnapmi_test.so only)."""
    __test__ = False


class Context:
    """snapmi_ctx: one HIP device + stream + device scratch.  `lib`: the
    loaded library that makes it (default: the process's, _lib.load())."""

    def __init__(self, device=0, stream=None, lib=None):
        self._h = None
        L = self._L = lib or _lib.load()
        h = C.c_void_p()
        rc = L.snapmi_ctx_create(int(device), stream, C.byref(h))
        if rc != 0:
            raise DeviceError(rc, message=f"snapmi_ctx_create({device}) failed"
                              ": no usable HIP device (no CPU fallback)")
        self._h = h
        self.device = device

    def close(self):
        if self._h:
            self._L.snapmi_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def set_option(self, name, value):
        """snapmi_ctx_set_option: tuning knobs (never change results)."""
        rc = self._L.snapmi_ctx_set_option(self._h, name.encode(),
                                               int(value))
        if rc:
            _raise(self, rc)

    def set_test_option(self, name, value):
        """snapmi_ctx_set_test_option (include/snapmi_test.h): knobs of the
        test suite and the experiment drivers."""
        L = self._L
        if not hasattr(L, "snapmi_ctx_set_test_option"):
            raise TestOnlyOption(
                "set_test_option: this is the product library; the test "
                "knobs live in libsnapmi_test.so (SNAPMI_TESTING=1)")
        rc = L.snapmi_ctx_set_test_option(self._h, name.encode(),
                                          int(value))
        if rc:
            _raise(self, rc)

    def prepare(self, blocks, top_of_memory=False):
        """snapmi_ctx_prepare: the lane tables of a batch of `blocks` 64 KiB
        blocks now; top_of_memory: SNAPMI_PREPARE_TOP_OF_MEMORY (holds the
        whole device for a moment - see include/snapmi.h)."""
        rc = self._L.snapmi_ctx_prepare(self._h, int(blocks),
                                        1 if top_of_memory else 0)
        if rc:
            _raise(self, rc)

    def info(self, name):
        """snapmi_ctx_get_info: "scratch_bytes", "token_scratch_bytes",
        "token_pool_pages", "token_pool_pct_now", "token_pages_asked",
        "token_blocks_spilled", "host_batch_slices", "host_batch_h2d_bytes",
        "host_batch_d2h_bytes", "host_batch_listed_slices",
        "index_streams_pieced", "index_streams_fallback", "range_pieces",
        "range_ranges_ok", "range_ranges_failed", "index_build_built",
        "index_build_unaligned", "index_build_corrupt",
        "index_build_missized", "index_build_walked", "write_blocks",
        "write_blocks_decoded", "write_streams_ok", "write_streams_failed",
        "append_blocks", "append_blocks_decoded", "append_streams_ok",
        "append_streams_failed", "frame_nowait_front" (include/snapmi.h);
        the test build also "lane_multi_rounds", "scratch_fill_buffers",
        "scratch_fill_bytes", "scratch_fill_seen" (include/snapmi_test.h)."""
        v = C.c_int64(0)
        rc = self._L.snapmi_ctx_get_info(self._h, name.encode(), C.byref(v))
        if rc:
            _raise(self, rc)
        return v.value

    def table_probe_log(self):
        """snapmi_table_probe_log: what the last placement of the lane tables
        probed, held, kept and took."""
        return self._L.snapmi_table_probe_log(self._h).decode()

    @property
    def stream(self):
        return self._L.snapmi_ctx_stream(self._h)

    def synchronize(self):
        rc = self._L.snapmi_ctx_synchronize(self._h)
        if rc:
            _raise(self, rc)

    def last_kernel(self):
        """snapmi_last_kernel: the dominant kernel of the last batch call."""
        return self._L.snapmi_last_kernel(self._h).decode()

    def last_timing(self):
        t = _lib.SnapmiTiming()
        rc = self._L.snapmi_last_timing(self._h, C.byref(t))
        if rc:
            _raise(self, rc)
        return {"plan_ms": t.plan_ms, "codec_ms": t.codec_ms,
                "compact_ms": t.compact_ms, "total_ms": t.total_ms,
                "codec_launches": t.codec_launches,
                "dominant_ms": t.dominant_ms}


_default_ctx = None


def default_context():
    global _default_ctx
    if _default_ctx is None:
        _default_ctx = Context(0)
    return _default_ctx


def max_compress_len(input_len):
    return _lib.load().snapmi_max_compress_len(int(input_len))


def decompress_len(data):
    data = bytes(data)
    n = C.c_size_t(0)
    err = _lib.SnapmiError()
    rc = _lib.load().snapmi_decompress_len(data, len(data), C.byref(n),
                                           C.byref(err))
    if rc:
        _raise(None, rc, err)
    return n.value


class Encoder:
    """snap::raw::Encoder.  Owns a context (device scratch + stream), like the
    reference's encoder owns its hash tables; reuse it."""

    def __init__(self, ctx=None):
        self.ctx = ctx or default_context()

    def compress(self, data, output):
        """Compress into the writable buffer `output`; returns bytes written.
        `output` must hold max_compress_len(len(data)) bytes."""
        data = bytes(data)
        out = (C.c_char * len(output)).from_buffer(output)
        n = C.c_size_t(0)
        err = _lib.SnapmiError()
        rc = _lib.of(self.ctx).snapmi_raw_compress(self.ctx._h, data, len(data),
                                             out, len(output), C.byref(n),
                                             C.byref(err))
        if rc:
            _raise(self.ctx, rc, err)
        return n.value

    def compress_vec(self, data):
        cap = max_compress_len(len(data))
        if cap == 0:
            raise Error(1, len(data), MAX_INPUT_SIZE)
        buf = bytearray(cap)
        n = self.compress(data, buf)
        return bytes(buf[:n])


class Decoder:
    """snap::raw::Decoder (stateless in the reference)."""

    def __init__(self, ctx=None):
        self.ctx = ctx or default_context()

    def decompress(self, data, output):
        data = bytes(data)
        out = (C.c_char * max(len(output), 1)).from_buffer(
            output if len(output) else bytearray(1))
        n = C.c_size_t(0)
        err = _lib.SnapmiError()
        rc = _lib.of(self.ctx).snapmi_raw_decompress(self.ctx._h, data, len(data),
                                               out, len(output), C.byref(n),
                                               C.byref(err))
        if rc:
            _raise(self.ctx, rc, err)
        return n.value

    def decompress_vec(self, data):
        buf = bytearray(decompress_len(data))
        n = self.decompress(data, buf)
        return bytes(buf[:n])


# ---------------------------------------------------------------------
# batched, host memory (section 2b of include/snapmi.h)
# ---------------------------------------------------------------------
ERROR_DTYPE = np.dtype([("kind", "<i4"), ("reserved", "<u4"), ("a", "<u8"),
                        ("b", "<u8"), ("c", "<u8")])


def _np_ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def batch_host(ctx, compress, in_ptrs, in_lens, out_ptrs, out_caps):
    """snapmi_compress_batch_host / snapmi_decompress_batch_host over arrays of
    host addresses and lengths (anything np.asarray takes); the buffers behind
    them are the caller's to keep alive.  Returns (out_lens as uint64 array,
    errors as an ERROR_DTYPE array)."""
    in_ptrs = np.ascontiguousarray(in_ptrs, dtype=np.uint64)
    in_lens = np.ascontiguousarray(in_lens, dtype=np.uint64)
    out_ptrs = np.ascontiguousarray(out_ptrs, dtype=np.uint64)
    out_caps = np.ascontiguousarray(out_caps, dtype=np.uint64)
    n = int(in_ptrs.size)
    assert in_lens.size == out_ptrs.size == out_caps.size == n
    out_lens = np.zeros(n, dtype=np.uint64)
    errs = np.zeros(n, dtype=ERROR_DTYPE)
    L = _lib.of(ctx)
    f = L.snapmi_compress_batch_host if compress \
        else L.snapmi_decompress_batch_host
    rc = f(ctx._h, _np_ptr(in_ptrs), _np_ptr(in_lens), _np_ptr(out_ptrs),
           _np_ptr(out_caps), _np_ptr(out_lens), _np_ptr(errs), n)
    if rc:
        _raise(ctx, rc)
    return out_lens, errs


def _many(ctx, compress, streams, caps):
    ctx = ctx or default_context()
    # the inputs where they lie (no join, no copy)
    views = [np.frombuffer(s, dtype=np.uint8) if len(s) else None
             for s in streams]
    in_ptrs = [v.ctypes.data if v is not None else 0 for v in views]
    in_lens = [v.size if v is not None else 0 for v in views]
    caps = np.asarray([int(c) for c in caps], dtype=np.uint64)
    offs = np.zeros(len(caps) + 1, dtype=np.uint64)
    np.cumsum(caps, out=offs[1:])
    slab = np.empty(max(int(offs[-1]), 1), dtype=np.uint8)
    out_ptrs = offs[:-1] + np.uint64(slab.ctypes.data)
    out_lens, errs = batch_host(ctx, compress, in_ptrs, in_lens, out_ptrs,
                                caps)
    del views
    outputs, errors = [], []
    for i in range(len(caps)):
        e = errs[i]
        if e["kind"] == 0:
            o = int(offs[i])
            outputs.append(slab[o:o + int(out_lens[i])].tobytes())
            errors.append(None)
        else:
            outputs.append(b"")
            errors.append(Error(int(e["kind"]), int(e["a"]), int(e["b"]),
                                int(e["c"])))
    return outputs, errors


def compress_many(streams, ctx=None):
    """Encoder::compress_vec of every stream (bytes-like objects) in one
    snapmi_compress_batch_host call.  Returns (outputs, errors): the
    compressed bytes (b"" for a stream that failed) and None or the Error of
    every stream."""
    return _many(ctx, True, streams,
                 [max_compress_len(len(s)) for s in streams])


def decompress_many(streams, ctx=None, caps=None):
    """Decoder::decompress_vec of every stream in one
    snapmi_decompress_batch_host call; caps: output capacities (default: what
    every stream's header announces; a header that does not parse gets none
    and the device reports the error).  Returns (outputs, errors) as
    compress_many."""
    if caps is None:
        L, n = _lib.load(), C.c_size_t(0)
        caps = []
        for s in streams:
            s = bytes(s[:16])
            ok = L.snapmi_decompress_len(s, len(s), C.byref(n), None) == 0
            caps.append(n.value if ok else 0)
    return _many(ctx, False, streams, caps)


# ---------------------------------------------------------------------
# batched, device-resident (torch tensors own the HBM)
# ---------------------------------------------------------------------
def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def block_index_entries(lens):
    """snapmi_block_index_entries: entries the block index of streams of
    these input lengths takes, sum(ceil(len / 65536) + 1)."""
    a = (C.c_uint64 * len(lens))(*[int(x) for x in lens])
    return int(_lib.load().snapmi_block_index_entries(a, len(lens)))


def compress_batch(ctx, in_ptrs, in_lens, out_ptrs, out_caps, out_lens,
                   errs=None, host_in_lens=None, index_first=None, index=None,
                   index_cap=None):
    """snapmi_compress_batch.  in_ptrs/out_ptrs: int64 CUDA tensors of device
    addresses; in_lens/out_caps/out_lens: uint64-as-int64 CUDA tensors;
    errs: optional uint8 CUDA tensor of 32*n bytes; host_in_lens: optional
    CPU int64 tensor (or None -> fetched from the device).
    With index_first (int64 CUDA tensor [n + 1]) and index (int64 CUDA tensor
    of index_cap entries, default its size): snapmi_compress_batch_indexed,
    which also writes the streams' block index."""
    n = in_ptrs.numel()
    h = None
    if host_in_lens is not None:
        h = C.c_void_p(host_in_lens.data_ptr())
    if index_first is not None or index is not None:
        if index_cap is None:
            index_cap = index.numel() if index is not None else 0
        rc = _lib.of(ctx).snapmi_compress_batch_indexed(
            ctx._h, _ptr(in_ptrs), _ptr(in_lens), h, _ptr(out_ptrs),
            _ptr(out_caps), _ptr(out_lens), _ptr(errs), n, _ptr(index_first),
            _ptr(index), int(index_cap))
    else:
        rc = _lib.of(ctx).snapmi_compress_batch(
            ctx._h, _ptr(in_ptrs), _ptr(in_lens), h, _ptr(out_ptrs),
            _ptr(out_caps), _ptr(out_lens), _ptr(errs), n)
    if rc:
        _raise(ctx, rc)


def decompress_batch(ctx, in_ptrs, in_lens, out_ptrs, out_caps, out_lens,
                     errs=None, index_first=None, index=None,
                     index_entries=None):
    """snapmi_decompress_batch; with index_first / index (int64 CUDA tensors
    as compress_batch wrote them; index_entries: the host's copy of
    index_first[n], default the size of index):
    snapmi_decompress_batch_indexed - the same results, the long streams on
    a wavefront per 64 KiB block, enqueue-only."""
    n = in_ptrs.numel()
    if index_first is not None or index is not None:
        if index_entries is None:
            index_entries = index.numel() if index is not None else 0
        rc = _lib.of(ctx).snapmi_decompress_batch_indexed(
            ctx._h, _ptr(in_ptrs), _ptr(in_lens), _ptr(out_ptrs),
            _ptr(out_caps), _ptr(out_lens), _ptr(errs), n, _ptr(index_first),
            _ptr(index), int(index_entries))
    else:
        rc = _lib.of(ctx).snapmi_decompress_batch(
            ctx._h, _ptr(in_ptrs), _ptr(in_lens), _ptr(out_ptrs),
            _ptr(out_caps), _ptr(out_lens), _ptr(errs), n)
    if rc:
        _raise(ctx, rc)


def _u64_array(values):
    return (C.c_uint64 * len(values))(*[int(x) & (2**64 - 1) for x in values])


def range_pieces(offs, lens):
    """snapmi_range_pieces: pieces the ranges [off, off + len) take, the sum
    of the 64 KiB blocks each touches."""
    assert len(offs) == len(lens)
    return int(_lib.load().snapmi_range_pieces(
        _u64_array(offs), _u64_array(lens), len(offs)))


def decompress_ranges_indexed(ctx, in_ptrs, in_lens, index_first, index,
                              range_stream, range_off, range_len,
                              host_range_off, host_range_len, range_out,
                              range_got, range_errs=None, index_entries=None):
    """snapmi_decompress_ranges_indexed: output bytes [off, off + len) of
    stream range_stream[r] into the buffer at range_out[r], decoding only the
    blocks the range touches.  in_ptrs / in_lens / index_first / index: the
    streams and their block index as compress_batch wrote them (int64 CUDA
    tensors); range_stream: int32 CUDA tensor; range_off / range_len /
    range_out / range_got: uint64-as-int64 CUDA tensors [m]; host_range_off /
    host_range_len: the host's copies, sequences of ints; range_errs: optional
    uint8 CUDA tensor of 32*m bytes.  Enqueue-only."""
    m = range_stream.numel()
    assert len(host_range_off) == m and len(host_range_len) == m
    if index_entries is None:
        index_entries = index.numel() if index is not None else 0
    rc = _lib.of(ctx).snapmi_decompress_ranges_indexed(
        ctx._h, _ptr(in_ptrs), _ptr(in_lens),
        in_ptrs.numel() if in_ptrs is not None else 0, _ptr(index_first),
        _ptr(index), int(index_entries), _ptr(range_stream), _ptr(range_off),
        _ptr(range_len), _u64_array(host_range_off),
        _u64_array(host_range_len), _ptr(range_out), _ptr(range_got),
        _ptr(range_errs), m)
    if rc:
        _raise(ctx, rc)


def write_blocks(streams, offs, lens):
    """snapmi_write_blocks: blocks the writes [off, off + len) of streams[w]
    touch - a block that two neighbouring writes share counts once."""
    assert len(streams) == len(offs) == len(lens)
    return int(_lib.load().snapmi_write_blocks(
        (C.c_uint32 * len(streams))(*[int(x) & 0xFFFFFFFF for x in streams]),
        _u64_array(offs), _u64_array(lens), len(streams)))


def write_ranges_indexed(ctx, in_ptrs, in_lens, index_first, index,
                         write_stream, write_off, write_len, write_src,
                         out_ptrs, out_caps, out_lens, errs, new_index,
                         index_entries=None):
    """snapmi_write_ranges_indexed: write_src[w][0, len) replaces output bytes
    [off, off + len) of stream write_stream[w]; only the touched blocks are
    decoded and compressed, the others are copied.  in_ptrs / in_lens /
    index_first / index: the streams and their block index (int64 CUDA
    tensors); write_stream / write_off / write_len: sequences of ints sorted
    by (stream, off); write_src: sequence of device addresses (ints);
    out_ptrs / out_caps / out_lens / new_index: uint64-as-int64 CUDA tensors
    ([n], [n], [n], [index_entries]); errs: optional uint8 CUDA tensor of 32*n
    bytes.  Enqueues on the context's stream."""
    m = len(write_stream)
    assert len(write_off) == m and len(write_len) == m and len(write_src) == m
    if index_entries is None:
        index_entries = index.numel() if index is not None else 0
    rc = _lib.of(ctx).snapmi_write_ranges_indexed(
        ctx._h, _ptr(in_ptrs), _ptr(in_lens),
        in_ptrs.numel() if in_ptrs is not None else 0, _ptr(index_first),
        _ptr(index), int(index_entries),
        (C.c_uint32 * m)(*[int(x) & 0xFFFFFFFF for x in write_stream]),
        _u64_array(write_off), _u64_array(write_len), _u64_array(write_src),
        m, _ptr(out_ptrs), _ptr(out_caps), _ptr(out_lens), _ptr(errs),
        _ptr(new_index))
    if rc:
        _raise(ctx, rc)


def append_indexed(ctx, in_ptrs, in_lens, host_out_lens, index_first, index,
                   app_src, app_len, out_ptrs, out_caps, out_lens, errs,
                   new_index_first, new_index, index_entries=None,
                   new_index_cap=None):
    """snapmi_append_indexed: app_src[i][0, app_len[i]) is appended to the
    output of stream i (app_len[i] == 0: not named); only the stream's short
    last block and the new bytes are decoded and compressed, the full old
    blocks are copied.  in_ptrs / in_lens / index_first / index: the streams
    and their block index (int64 CUDA tensors); host_out_lens: the lengths
    the headers announce, app_len: sequences of ints; app_src: sequence of
    device addresses (ints); out_ptrs / out_caps / out_lens: uint64-as-int64
    CUDA tensors [n]; errs: optional uint8 CUDA tensor of 32*n bytes;
    new_index_first [n + 1] and new_index (new_index_cap entries, default its
    size; block_index_entries of the summed lengths are needed): int64 CUDA
    tensors.  Enqueues on the context's stream."""
    n = in_ptrs.numel() if in_ptrs is not None else 0
    assert len(host_out_lens) == n and len(app_src) == n and len(app_len) == n
    if index_entries is None:
        index_entries = index.numel() if index is not None else 0
    if new_index_cap is None:
        new_index_cap = new_index.numel() if new_index is not None else 0
    rc = _lib.of(ctx).snapmi_append_indexed(
        ctx._h, _ptr(in_ptrs), _ptr(in_lens), _u64_array(host_out_lens), n,
        _ptr(index_first), _ptr(index), int(index_entries),
        _u64_array(app_src), _u64_array(app_len), _ptr(out_ptrs),
        _ptr(out_caps), _ptr(out_lens), _ptr(errs), _ptr(new_index_first),
        _ptr(new_index), int(new_index_cap))
    if rc:
        _raise(ctx, rc)


INDEX_BUILT, INDEX_UNALIGNED, INDEX_CORRUPT, INDEX_MISSIZED = 1, 2, 3, 4


def build_block_index(ctx, in_ptrs, in_lens, host_in_lens, host_out_lens,
                      index_first, index, status=None, index_cap=None):
    """snapmi_build_block_index: the block index of streams that came without
    one, into index_first (int64 CUDA tensor [n + 1]) and index (int64 CUDA
    tensor of index_cap entries, default its size; block_index_entries(
    host_out_lens) are needed).  in_ptrs / in_lens: the streams (int64 CUDA
    tensors); host_in_lens / host_out_lens: the host's copies of in_lens and
    of the lengths the headers announce, sequences of ints; status: optional
    uint8 CUDA tensor [n] of INDEX_* verdicts.  Enqueues on the context's
    stream."""
    n = in_ptrs.numel() if in_ptrs is not None else 0
    assert len(host_in_lens) == n and len(host_out_lens) == n
    if index_cap is None:
        index_cap = index.numel() if index is not None else 0
    rc = _lib.of(ctx).snapmi_build_block_index(
        ctx._h, _ptr(in_ptrs), _ptr(in_lens), _u64_array(host_in_lens),
        _u64_array(host_out_lens), n, _ptr(index_first), _ptr(index),
        int(index_cap), _ptr(status))
    if rc:
        _raise(ctx, rc)


def decompress_stream(ctx, d_in, n_in, d_out, out_len, err):
    """ONE long raw stream (uint8 CUDA tensor d_in[:n_in]) decoded by many
    wavefronts into d_out; out_len: int64[1], err: uint8[32] CUDA tensors.
    Same results and errors as decompress_batch with one stream."""
    rc = _lib.of(ctx).snapmi_decompress_stream(
        ctx._h, _ptr(d_in), int(n_in), _ptr(d_out), d_out.numel(),
        _ptr(out_len), _ptr(err))
    if rc:
        _raise(ctx, rc)


def stream_decode_path(ctx):
    """0 = the last decompress_stream ran as pieces on many wavefronts, 1 =
    sequential path, -1 = none yet."""
    return _lib.of(ctx).snapmi_stream_decode_path(ctx._h)


def decompress_len_batch(ctx, in_ptrs, in_lens, out_lens, errs=None):
    n = in_ptrs.numel()
    rc = _lib.of(ctx).snapmi_decompress_len_batch(
        ctx._h, _ptr(in_ptrs), _ptr(in_lens), _ptr(out_lens), _ptr(errs), n)
    if rc:
        _raise(ctx, rc)
