"""Device-resident batches of raw streams (torch tensors own the HBM).

Plumbing only: lays streams out back to back in one uint8 tensor, builds the
pointer / length arrays the C ABI wants, and calls the batched entry points.
"""
import numpy as np
import torch

from . import raw

ALIGN = 16


def _align(x, a=ALIGN):
    return (x + a - 1) // a * a


class StreamBatch:
    """n byte streams in one device slab: data[offsets[i] : +lens[i]]."""

    def __init__(self, data, offsets, lens):
        self.data = data                      # uint8 CUDA tensor
        self.offsets = np.asarray(offsets, dtype=np.int64)
        self.lens = np.asarray(lens, dtype=np.int64)
        dev = data.device
        self.h_lens = torch.from_numpy(self.lens.copy())
        self.d_lens = self.h_lens.to(dev)
        self.d_ptrs = (torch.from_numpy(self.offsets).to(dev)
                       + data.data_ptr())

    @property
    def n(self):
        return len(self.lens)

    @classmethod
    def from_bytes(cls, streams, device="cuda:0"):
        lens = [len(s) for s in streams]
        offs, pos = [], 0
        for n in lens:
            offs.append(pos)
            pos += _align(max(n, 1))
        host = np.zeros(max(pos, ALIGN), dtype=np.uint8)
        for s, o in zip(streams, offs):
            host[o:o + len(s)] = np.frombuffer(bytes(s), dtype=np.uint8)
        return cls(torch.from_numpy(host).to(device), offs, lens)

    @classmethod
    def empty(cls, caps, device="cuda:0"):
        """Output slab with capacity caps[i] for stream i."""
        offs, pos = [], 0
        for c in caps:
            offs.append(pos)
            pos += _align(max(int(c), 1))
        data = torch.empty(max(pos, ALIGN), dtype=torch.uint8, device=device)
        return cls(data, offs, [int(c) for c in caps])

    def stream_bytes(self, i, n=None):
        n = int(self.lens[i]) if n is None else int(n)
        o = int(self.offsets[i])
        return self.data[o:o + n].cpu().numpy().tobytes()


def read_errors(errs):
    """uint8 tensor [32*n] of snapmi_error -> list of (kind, a, b, c)."""
    raw_ = errs.cpu().numpy().tobytes()
    rec = np.frombuffer(raw_, dtype=np.dtype(
        [("kind", "<i4"), ("r", "<u4"), ("a", "<u8"), ("b", "<u8"),
         ("c", "<u8")]))
    return [(int(r["kind"]), int(r["a"]), int(r["b"]), int(r["c"]))
            for r in rec]


def compress(ctx, src: StreamBatch, check_caps=True, want_index=False):
    """Compress every stream of `src`; returns (dst batch, out_lens, errs) -
    or, with want_index, (dst batch, index_first, index): the streams' block
    index as int64 device tensors (snapmi_compress_batch_indexed; dst.lens
    are then the compressed lengths).  The per-stream errors are not
    returned in that form: a stream that failed (BufferTooSmall) has
    dst.lens[i] == 0 and all its index entries 0; call without want_index to
    see why."""
    caps = [raw.max_compress_len(int(n)) or 32 for n in src.lens]
    dst = StreamBatch.empty(caps, src.data.device)
    dev = src.data.device
    out_lens = torch.zeros(src.n, dtype=torch.int64, device=dev)
    errs = torch.zeros(32 * src.n, dtype=torch.uint8, device=dev)
    if want_index:
        entries = raw.block_index_entries(src.lens)
        index_first = torch.zeros(src.n + 1, dtype=torch.int64, device=dev)
        index = torch.zeros(entries, dtype=torch.int64, device=dev)
        raw.compress_batch(ctx, src.d_ptrs, src.d_lens, dst.d_ptrs,
                           dst.d_lens if check_caps else None, out_lens, errs,
                           host_in_lens=src.h_lens, index_first=index_first,
                           index=index, index_cap=entries)
        ctx.synchronize()
        done = StreamBatch(dst.data, dst.offsets, out_lens.cpu().numpy())
        return done, index_first, index
    raw.compress_batch(ctx, src.d_ptrs, src.d_lens, dst.d_ptrs,
                       dst.d_lens if check_caps else None, out_lens, errs,
                       host_in_lens=src.h_lens)
    ctx.synchronize()
    return dst, out_lens.cpu().numpy(), read_errors(errs)


def decompress(ctx, src: StreamBatch, caps=None, index=None):
    """Decompress every stream; caps default to the header lengths.  index:
    the (index_first, index) pair compress(want_index=True) returned - the
    same results through snapmi_decompress_batch_indexed."""
    dev = src.data.device
    if caps is None:
        lens = torch.zeros(src.n, dtype=torch.int64, device=dev)
        raw.decompress_len_batch(ctx, src.d_ptrs, src.d_lens, lens)
        ctx.synchronize()
        caps = lens.cpu().numpy()
    dst = StreamBatch.empty(caps, dev)
    out_lens = torch.zeros(src.n, dtype=torch.int64, device=dev)
    errs = torch.zeros(32 * src.n, dtype=torch.uint8, device=dev)
    if index is not None:
        index_first, index_tensor = index
        raw.decompress_batch(ctx, src.d_ptrs, src.d_lens, dst.d_ptrs,
                             dst.d_lens, out_lens, errs,
                             index_first=index_first, index=index_tensor,
                             index_entries=index_tensor.numel())
    else:
        raw.decompress_batch(ctx, src.d_ptrs, src.d_lens, dst.d_ptrs,
                             dst.d_lens, out_lens, errs)
    ctx.synchronize()
    return dst, out_lens.cpu().numpy(), read_errors(errs)


def build_index(ctx, src: StreamBatch, out_lens=None):
    """The block index of streams that came without one - the reference's,
    libsnappy's, an earlier compress() - built on the device
    (snapmi_build_block_index).  out_lens: the lengths the streams' headers
    announce, when the caller has them (default: asked of the device with
    snapmi_decompress_len_batch; a header that does not parse counts as 0).
    Returns (index_first, index, status): the pair decompress(index=...) and
    read_ranges take, and the per-stream verdicts (raw.INDEX_*) as a list.  A
    stream that is not INDEX_BUILT has all its entries 0: it is decoded whole,
    and a range on it has no usable index."""
    dev = src.data.device
    if out_lens is None:
        lens = torch.zeros(src.n, dtype=torch.int64, device=dev)
        raw.decompress_len_batch(ctx, src.d_ptrs, src.d_lens, lens)
        ctx.synchronize()
        out_lens = lens.cpu().tolist()
    out_lens = [int(d) & (2**64 - 1) for d in out_lens]
    entries = raw.block_index_entries(out_lens)
    index_first = torch.zeros(src.n + 1, dtype=torch.int64, device=dev)
    index = torch.zeros(max(entries, 1), dtype=torch.int64, device=dev)
    status = torch.zeros(max(src.n, 1), dtype=torch.uint8, device=dev)
    raw.build_block_index(ctx, src.d_ptrs, src.d_lens,
                          [int(x) for x in src.lens], out_lens, index_first,
                          index, status, index_cap=entries)
    ctx.synchronize()
    return index_first, index[:entries], status[:src.n].cpu().tolist()


def _i64(values):
    """Python ints below 2^64 as the int64 tensor of the same bits."""
    return torch.from_numpy(
        np.asarray([int(v) & (2**64 - 1) for v in values],
                   dtype=np.uint64).view(np.int64).copy())


def read_ranges(ctx, src: StreamBatch, index, ranges):
    """Range reads of compressed streams: ranges is a list of (stream, off,
    len) into the streams' OUTPUT; index the (index_first, index) pair
    compress(want_index=True) returned.  Only the 64 KiB blocks a range
    touches are decoded (snapmi_decompress_ranges_indexed).  Returns (bytes
    per range - b"" for one that failed -, per-range errors as (kind, a, b,
    c)).  The call's limits hold: the blocks of all ranges together, as
    asked, stay below 2^31 (raw.range_pieces)."""
    dev = src.data.device
    index_first, index_tensor = index
    m = len(ranges)
    if m == 0:
        return [], []
    # (as the call sees them: a stream number of 32 bits, offsets and
    # lengths of 64)
    streams = [int(r[0]) & 0xFFFFFFFF for r in ranges]
    offs = [int(r[1]) & (2**64 - 1) for r in ranges]
    lens = [int(r[2]) & (2**64 - 1) for r in ranges]
    # a buffer for every range that fits the length its stream announces:
    # the call fails every other range (no such stream, a header that does
    # not parse, off + len beyond the stream) without writing a byte for it,
    # so a wrong length costs its own range an error and no memory
    dlens = torch.zeros(src.n, dtype=torch.int64, device=dev)
    raw.decompress_len_batch(ctx, src.d_ptrs, src.d_lens, dlens)
    ctx.synchronize()
    dlens = [int(d) & (2**64 - 1) for d in dlens.cpu().tolist()]
    dst = StreamBatch.empty(
        [n if s < src.n and o + n <= dlens[s] else 0
         for s, o, n in zip(streams, offs, lens)], dev)
    d_stream = torch.tensor(streams,
                            dtype=torch.int64).to(torch.int32).to(dev)
    got = torch.zeros(m, dtype=torch.int64, device=dev)
    errs = torch.zeros(32 * m, dtype=torch.uint8, device=dev)
    raw.decompress_ranges_indexed(
        ctx, src.d_ptrs, src.d_lens, index_first, index_tensor, d_stream,
        _i64(offs).to(dev), _i64(lens).to(dev), offs, lens, dst.d_ptrs, got,
        errs, index_entries=index_tensor.numel())
    ctx.synchronize()
    got = got.cpu().numpy()
    return ([dst.stream_bytes(r, got[r]) for r in range(m)],
            read_errors(errs))


def write_ranges(ctx, src: StreamBatch, index, writes):
    """Range writes of compressed streams: writes is a list of (stream, off,
    bytes) into the streams' OUTPUT, sorted by (stream, off) and not
    overlapping; index the (index_first, index) pair of the streams.  Only the
    64 KiB blocks a write touches are decoded and compressed again, every
    other block's compressed bytes are copied (snapmi_write_ranges_indexed).
    Returns (the new StreamBatch - a stream no write names, or whose writes
    failed, is the old one -, the new (index_first, index) pair, per-stream
    errors as (kind, a, b, c))."""
    dev = src.data.device
    index_first, index_tensor = index
    writes = [(int(s), int(o), bytes(b)) for s, o, b in writes]
    if not any(len(b) for _, _, b in writes):
        return src, index, [(0, 0, 0, 0)] * src.n
    data = StreamBatch.from_bytes([b for _, _, b in writes], dev)
    # a touched stream grows by at most what its touched blocks can: room for
    # the worst case of each
    touched = {}
    for s, o, b in writes:
        if b:
            touched.setdefault(s, set()).update(
                range(o // 65536, (o + len(b) - 1) // 65536 + 1))
    caps = [int(src.lens[i]) + 5 + len(touched[i]) *
            raw.max_compress_len(65536) if i in touched else 0
            for i in range(src.n)]
    dst = StreamBatch.empty(caps, dev)
    out_lens = torch.zeros(src.n, dtype=torch.int64, device=dev)
    errs = torch.zeros(32 * src.n, dtype=torch.uint8, device=dev)
    new_index = torch.zeros_like(index_tensor)
    raw.write_ranges_indexed(
        ctx, src.d_ptrs, src.d_lens, index_first, index_tensor,
        [w[0] for w in writes], [w[1] for w in writes],
        [len(w[2]) for w in writes],
        [int(p) for p in data.d_ptrs.cpu().tolist()], dst.d_ptrs, dst.d_lens,
        out_lens, errs, new_index, index_entries=index_tensor.numel())
    ctx.synchronize()
    out_lens = out_lens.cpu().numpy()
    # one slab of the streams to keep and the new ones
    offs, lens, parts, pos = [], [], [], 0
    for i in range(src.n):
        from_, n = (dst, int(out_lens[i])) if out_lens[i] else \
            (src, int(src.lens[i]))
        o = int(from_.offsets[i])
        parts.append(from_.data[o:o + n])
        offs.append(pos)
        lens.append(n)
        pos += _align(max(n, 1))
        pad = pos - offs[-1] - n
        if pad:
            parts.append(torch.zeros(pad, dtype=torch.uint8, device=dev))
    merged = StreamBatch(torch.cat(parts), offs, lens)
    return merged, (index_first, new_index), read_errors(errs)


def append(ctx, src: StreamBatch, index, appends):
    """Appends to compressed streams: appends is a list of (stream, bytes),
    a stream at most once; the bytes go behind the stream's OUTPUT.  index:
    the (index_first, index) pair of the streams.  Only a stream's short last
    block and the new bytes go through the codec, the full old blocks'
    compressed bytes are copied (snapmi_append_indexed).  Returns (the new
    StreamBatch - a stream nobody names, or whose append failed, is the old
    one -, the new (index_first, index) pair, per-stream errors as (kind, a,
    b, c)).  A stream that failed has all its new entries 0: its old index
    is the caller's to keep."""
    dev = src.data.device
    index_first, index_tensor = index
    add = [b""] * src.n
    for s, b in appends:
        assert not add[int(s)], f"stream {s} is named twice"
        add[int(s)] = bytes(b)
    dlens = torch.zeros(src.n, dtype=torch.int64, device=dev)
    raw.decompress_len_batch(ctx, src.d_ptrs, src.d_lens, dlens)
    ctx.synchronize()
    dlens = [int(d) & (2**64 - 1) for d in dlens.cpu().tolist()]
    data = StreamBatch.from_bytes(add, dev)
    # a named stream takes its old bytes, a header that may grow, and at most
    # the worst case of every block the codec sees: the tail's and the new ones
    caps = [int(src.lens[i]) + 5 + (len(b) // 65536 + 2) *
            raw.max_compress_len(65536) if b else 0
            for i, b in enumerate(add)]
    dst = StreamBatch.empty(caps, dev)
    out_lens = torch.zeros(src.n, dtype=torch.int64, device=dev)
    errs = torch.zeros(32 * src.n, dtype=torch.uint8, device=dev)
    entries = raw.block_index_entries([d + len(b)
                                       for d, b in zip(dlens, add)])
    new_first = torch.zeros(src.n + 1, dtype=torch.int64, device=dev)
    new_index = torch.zeros(max(entries, 1), dtype=torch.int64, device=dev)
    raw.append_indexed(
        ctx, src.d_ptrs, src.d_lens, dlens, index_first, index_tensor,
        [int(p) if b else 0
         for p, b in zip(data.d_ptrs.cpu().tolist(), add)],
        [len(b) for b in add], dst.d_ptrs, dst.d_lens, out_lens, errs,
        new_first, new_index, index_entries=index_tensor.numel(),
        new_index_cap=entries)
    ctx.synchronize()
    out_lens = out_lens.cpu().numpy()
    # one slab of the streams to keep and the new ones
    offs, lens, parts, pos = [], [], [], 0
    for i in range(src.n):
        from_, n = (dst, int(out_lens[i])) if out_lens[i] else \
            (src, int(src.lens[i]))
        o = int(from_.offsets[i])
        parts.append(from_.data[o:o + n])
        offs.append(pos)
        lens.append(n)
        pos += _align(max(n, 1))
        pad = pos - offs[-1] - n
        if pad:
            parts.append(torch.zeros(pad, dtype=torch.uint8, device=dev))
    merged = StreamBatch(torch.cat(parts), offs, lens)
    return merged, (new_first, new_index[:entries]), read_errors(errs)
