// snapmi_frame.hip -- Snappy frame format on the device (gfx950): the
// compress side.
//
// Reference: src/frame.rs (chunk layout, compress_frame), src/crc32.rs
// (masked CRC32C), src/write.rs (chunking of write::FrameEncoder),
// src/read.rs (read::FrameDecoder state machine).  A framed stream is a
// 10-byte stream identifier followed by chunks
//     type(1) | len24 LE (= 4 + payload) | masked crc32c(uncompressed) LE | payload
// and every data chunk (<= 64 KiB of input) is an independent raw stream, so
// the chunk is the parallel unit: the raw codec kernels run unchanged on a
// batch whose "streams" are the chunks.  The chunks of all the streams of a
// call form one list (stream i owns chunks [first[i], first[i+1])); a call
// for one stream is a list of one stream.
//
// The checksums are snapmi_crc.hip's, the decode side is snapmi_framedec.hip,
// the host-buffer calls over both are snapmi_hostpipe.hip; what the four
// share is declared in snapmi_frame.hpp.
//
// Kernels here:
//   k_scan_u64        exclusive scan (one workgroup; snapmi_scan.hpp), for the
//                     whole frame layer and the host-memory batch calls
//                     (launch_scan_u64)
//   k_fb_lone         a lone stream's scalars in the places of the arrays
//   k_fb_counts       chunks per stream
//   k_fb_chunks       chunk descriptors for the raw compressor
//   k_fb_sizes        compressed-vs-stored decision (src/frame.rs:85) + sizes
//   k_fb_base         list offset of every stream that starts in a segment
//   k_fb_emit         headers + payloads into the framed streams
//   k_fb_advance      list bytes of the segments in front
#include <hip/hip_runtime.h>

#include <vector>

#include "snapmi.h"
#include "snapmi_ctx.hpp"
#include "snapmi_launch.hpp"
#include "snapmi_device.hpp"
#include "snapmi_kernels.hpp"
#include "snapmi_scan.hpp"
#include "snapmi_frame.hpp"

using namespace snapmi;

namespace snapmi {

static_assert(kFwMaxBlock == kMaxBlock && kFwMaxInput == kMaxInput,
              "snapmi_framewalk.hpp restates the codec's limits");

// exclusive scan of n u64 values, out[n] = total; one workgroup
__global__ __launch_bounds__(1024) void k_scan_u64(const uint64_t *in,
                                                   uint64_t *out, uint32_t n)
{
    uint64_t carry[1] = {0};
    wg_scan_strided(
        n, carry, [&](uint32_t i, uint64_t (&x)[1]) { x[0] = in[i]; },
        [&](uint32_t i, const uint64_t (&)[1], const uint64_t (&ex)[1]) {
            out[i] = ex[0];
        });
    if (threadIdx.x == 0)
        out[n] = carry[0];
}

int launch_scan_u64(snapmi_ctx *ctx, hipStream_t st, const uint64_t *in,
                    uint64_t *out, uint32_t n)
{
    hipLaunchKernelGGL(k_scan_u64, dim3(1), dim3(1024), 0, st, in, out, n);
    HIP_TRY(ctx, hipGetLastError());
    return SNAPMI_OK;
}

__device__ inline uint64_t frame_max_len_dev(uint64_t n)
{
    return 10 + n + 8 * ((n + kMaxBlock - 1) / kMaxBlock);
}

// stream i has no room: cap_i < snapmi_frame_max_len(len_i) (an empty input
// writes nothing and needs none, as snapmi_frame_compress)
__device__ inline bool fb_refused(const FrameBatchCompressArgs &a, uint32_t i)
{
    const uint64_t len = a.in_lens[i];
    return a.out_caps && len && a.out_caps[i] < frame_max_len_dev(len);
}

// A lone stream as a list of one stream: the call's scalars in the places of
// the per-stream arrays (chunks: as the caller cut them, or one per 65536
// bytes); its first chunk is the list's first.
__global__ void k_fb_lone(const void **in_ptrs, uint64_t *in_lens,
                          void **out_ptrs, uint64_t *first, uint64_t *sbase,
                          const void *in, uint64_t in_len, void *out,
                          uint64_t chunks)
{
    in_ptrs[0] = in;
    in_lens[0] = in_len;
    out_ptrs[0] = out;
    first[0] = 0;
    first[1] = chunks;
    sbase[0] = 0;
}

__global__ void k_fb_counts(FrameBatchCompressArgs a)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < a.n)
        a.counts[i] = (a.in_lens[i] + kMaxBlock - 1) / kMaxBlock;
}

// the stream owning list entry t: the last i with first[i] <= t
__device__ inline uint32_t fb_stream_of(const uint64_t *first, uint32_t n,
                                        uint32_t t)
{
    uint32_t lo = 0, hi = n - 1;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo + 1) / 2;
        if (first[mid] <= t)
            lo = mid;
        else
            hi = mid - 1;
    }
    return lo;
}

// thread t: stream t's capacity check and result slots, list entry t's
// chunk descriptor, segment slot t's pointer; thread 0 clears the carry (here,
// not by a memset: a memset a call costs a one-stream call 4 us)
__global__ void k_fb_chunks(FrameBatchCompressArgs a)
{
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t == 0)
        a.carry[0] = 0;
    if (t < a.n) {
        const bool r = fb_refused(a, t);
        a.refused[t] = r;
        a.out_lens[t] = 0;
        if (a.errs)
            a.errs[t] = r ? frame_err(SNAPMI_BUFFER_TOO_SMALL, a.out_caps[t],
                                      frame_max_len_dev(a.in_lens[t]))
                          : frame_err(SNAPMI_OK, 0, 0);
    }
    if (t < a.total) {
        const uint32_t i = fb_stream_of(a.first, a.n, t);
        uint64_t off, len;
        if (a.chunk_in_off) {
            off = a.chunk_in_off[t];
            len = a.chunk_in_off[t + 1] - off;
        } else {
            off = (t - a.first[i]) * (uint64_t)kMaxBlock;
            len = a.in_lens[i] - off < kMaxBlock ? a.in_lens[i] - off
                                                 : kMaxBlock;
        }
        a.c_in[t] = (const uint8_t *)a.in_ptrs[i] + off;
        a.c_len[t] = len;
        a.c_stream[t] = i;
    }
    if (t < a.seg)
        a.slot_ptrs[t] = a.slots + (uint64_t)t * kFrameSlot;
}

// reference compress_frame, src/frame.rs:83-89; nothing for a refused stream
__global__ void k_fb_sizes(FrameBatchCompressArgs a)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.cnt)
        return;
    const uint32_t gi = a.lo + i;
    const uint64_t len = a.c_len[gi];
    const uint64_t clen = a.clens[i];
    const bool stored = clen >= len - len / 8;
    a.sizes[i] = a.refused[a.c_stream[gi]] ? 0 : 8 + (stored ? len : clen);
}

// The list offset of every stream whose first chunk lies in this segment,
// fixed before the segment's emit (which reads it in other workgroups; a
// stream that started in an earlier segment has it already).
__global__ void k_fb_base(FrameBatchCompressArgs a)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.cnt)
        return;
    const uint32_t gi = a.lo + i;
    const uint32_t s = a.c_stream[gi];
    if (a.first[s] == gi)
        a.sbase[s] = a.carry[0] + a.offs[i];
}

// one chunk at o: header (src/frame.rs:91-93) by thread 0, then the payload
// from `from` by the whole workgroup
__device__ inline void frame_put_chunk(gptr o, bool stored, uint64_t payload,
                                       uint32_t crc, gcptr from)
{
    if (threadIdx.x == 0) {
        const uint32_t cl = 4 + (uint32_t)payload;
        o[0] = stored ? 0x01 : 0x00;
        o[1] = (uint8_t)cl;
        o[2] = (uint8_t)(cl >> 8);
        o[3] = (uint8_t)(cl >> 16);
        o[4] = (uint8_t)crc;
        o[5] = (uint8_t)(crc >> 8);
        o[6] = (uint8_t)(crc >> 16);
        o[7] = (uint8_t)(crc >> 24);
    }
    gptr to = o + 8;
    for (uint64_t k = 4 * threadIdx.x; k + 4 <= payload; k += 4 * blockDim.x)
        st32u(to + k, ld32u(from + k));
    const uint64_t t = payload & ~3ull;
    if (threadIdx.x < (payload & 3))
        to[t + threadIdx.x] = from[t + threadIdx.x];
}

// one workgroup per chunk of the segment: the stream identifier (first
// chunk), header (src/frame.rs:91-93) and payload at the chunk's offset in
// its stream; the stream's last chunk writes its length
__global__ __launch_bounds__(256) void k_fb_emit(FrameBatchCompressArgs a)
{
    const uint32_t i = blockIdx.x;
    const uint32_t gi = a.lo + i;
    const uint32_t s = a.c_stream[gi];
    if (a.refused[s])
        return;
    const uint64_t len = a.c_len[gi];
    const uint64_t clen = a.clens[i];
    const bool stored = clen >= len - len / 8;
    const uint64_t payload = stored ? len : clen;
    const uint64_t at = a.ident + a.carry[0] + a.offs[i] - a.sbase[s];
    gptr base = (gptr)a.out_ptrs[s];
    gptr o = base + at;
    if (gi == a.first[s] && threadIdx.x < a.ident) {
        const uint8_t ident[10] = {0xFF, 0x06, 0x00, 0x00, 's',
                                   'N',  'a',  'P',  'p',  'Y'};
        base[threadIdx.x] = ident[threadIdx.x];
    }
    frame_put_chunk(o, stored, payload, a.crcs[i],
                    stored ? (gcptr)a.c_in[gi]
                           : (gcptr)(a.slots + (uint64_t)i * kFrameSlot));
    if (threadIdx.x == 0) {
        if (a.chunk_offsets) {
            a.chunk_offsets[gi] = at;
            if (gi + 1 == a.total)
                a.chunk_offsets[a.total] = at + 8 + payload;
        }
        if (gi + 1 == a.first[s + 1])
            a.out_lens[s] = at + 8 + payload;
    }
}

__global__ void k_fb_advance(FrameBatchCompressArgs a)
{
    a.carry[0] += a.offs[a.cnt];
}

// ---------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------
} // namespace snapmi

extern "C" {

size_t snapmi_frame_max_len(size_t n)
{
    const size_t chunks = (n + kMaxBlock - 1) / kMaxBlock;
    return 10 + n + 8 * chunks;
}

} // extern "C"

namespace snapmi {
// The one place that frames chunks: descriptors of the list, then per segment
// the checksums, the raw compressor, sizes, their scan and the emit.
int frame_compress_list(snapmi_ctx *ctx, const FrameList &l)
{
    hipStream_t s = ctx->stream;
    const size_t n = l.n;
    const uint64_t total = l.total;
    const bool lone = l.lone;
    // segments of at most lane_segment_blocks chunks (16 GiB of input by
    // default): 76 KiB of slot + 72 KiB of tokens per chunk of a segment;
    // per segment the chunks of at most 8 KiB for the compressor's routing
    // (chunks cut short by the caller - flushes, short reads -, else only a
    // stream's last chunk can be one)
    const uint32_t seg = total < ctx->lane_segment_blocks
                             ? (uint32_t)total
                             : ctx->lane_segment_blocks;
    std::vector<uint64_t> c8(seg ? (total + seg - 1) / seg : 0, 0);
    if (l.h_chunk_lens) {
        for (uint64_t t = 0; t < total; t++)
            c8[t / seg] += l.h_chunk_lens[t] <= 8192;
    } else {
        for (uint64_t i = 0, at = 0; i < n; i++) {
            const uint64_t len = l.h_in_lens[i];
            const uint64_t k = (len + kMaxBlock - 1) / kMaxBlock;
            if (k && len - (k - 1) * kMaxBlock <= 8192)
                c8[(at + k - 1) / seg]++;
            at += k;
        }
    }
    int rc = ensure_tables(ctx);
    if (rc)
        return rc;
    FrameBatchCompressArgs a;
    a.in_ptrs = l.in_ptrs; // (a lone stream: the layout's places, k_fb_lone)
    a.in_lens = l.in_lens;
    a.out_ptrs = l.out_ptrs;
    a.out_caps = l.out_caps;
    a.out_lens = l.out_lens;
    a.errs = l.errs;
    a.n = (uint32_t)n;
    a.total = (uint32_t)total;
    a.seg = seg;
    a.chunk_in_off = l.chunk_in_off;
    a.chunk_offsets = l.chunk_offsets;
    a.ident = l.ident ? 10 : 0;
    Carver measure;
    fb_desc_layout(measure, a, lone);
    if ((rc = reserve(ctx, ctx->fr_desc, measure.bytes())) ||
        (seg && (rc = reserve(ctx, ctx->fr_slots, (size_t)seg * kFrameSlot))))
        return rc;
    Carver place(ctx->fr_desc.p);
    const FrameLonePlaces lp = fb_desc_layout(place, a, lone);
    a.slots = (uint8_t *)ctx->fr_slots.p;
    a.lo = a.cnt = 0;

    const uint32_t tb = 256;
    uint64_t most = total > n ? total : n;
    if (lone) {
        hipLaunchKernelGGL(k_fb_lone, dim3(1), dim3(1), 0, s, lp.in, lp.len,
                           lp.out, a.first, a.sbase, l.in, l.in_len, l.out,
                           total);
    } else {
        hipLaunchKernelGGL(k_fb_counts, dim3((uint32_t)((n + tb - 1) / tb)),
                           dim3(tb), 0, s, a);
        if ((rc = launch_scan_u64(ctx, s, a.counts, a.first, (uint32_t)n)))
            return rc;
    }
    hipLaunchKernelGGL(k_fb_chunks, dim3((uint32_t)((most + tb - 1) / tb)),
                       dim3(tb), 0, s, a);
    for (uint32_t lo = 0; lo < total; lo += seg) {
        const uint32_t cnt = total - lo < seg ? (uint32_t)total - lo : seg;
        a.lo = lo;
        a.cnt = cnt;
        const uint32_t gb = (cnt + tb - 1) / tb;
        // The checksums only need the input: they run on the side stream,
        // under the match finder (which waits on HBM round trips and leaves
        // 16 KiB of LDS per CU free - room for three CRC workgroups).  Fusing
        // the CRC into the match finder's own block loads would add ~380
        // vector instructions per 128-byte line to a loop of ~150 per round
        // to save a kernel of 1 % of the pass: not done.
        const bool side = ctx->frame_crc_side_stream;
        if (side) {
            HIP_TRY(ctx, hipEventRecord(ctx->ev_crc[0], s));
            HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream2, ctx->ev_crc[0], 0));
        }
        if ((rc = launch_crc32c(ctx, side ? ctx->stream2 : s, a.c_in + lo,
                                a.c_len + lo, a.crcs, cnt)))
            return rc;
        if (side)
            HIP_TRY(ctx, hipEventRecord(ctx->ev_crc[1], ctx->stream2));
        // every chunk is a one-block raw stream: cnt blocks, no scratch slots
        rc = launch_compress(ctx, a.c_in + lo, a.c_len + lo, a.slot_ptrs,
                             nullptr, a.clens, nullptr, cnt, cnt, 0, 0xF,
                             c8[lo / seg]);
        if (rc)
            return rc;
        if (side)
            HIP_TRY(ctx, hipStreamWaitEvent(s, ctx->ev_crc[1], 0));
        hipLaunchKernelGGL(k_fb_sizes, dim3(gb), dim3(tb), 0, s, a);
        if ((rc = launch_scan_u64(ctx, s, a.sizes, a.offs, cnt)))
            return rc;
        if (!lone) // (a lone stream's first chunk is the list's: k_fb_lone)
            hipLaunchKernelGGL(k_fb_base, dim3(gb), dim3(tb), 0, s, a);
        hipLaunchKernelGGL(k_fb_emit, dim3(cnt), dim3(256), 0, s, a);
        hipLaunchKernelGGL(k_fb_advance, dim3(1), dim3(1), 0, s, a);
    }
    HIP_TRY(ctx, hipGetLastError());
    return SNAPMI_OK;
}
} // namespace snapmi

extern "C" {

int snapmi_frame_compress(snapmi_ctx *ctx, const void *d_in, uint64_t in_len,
                          void *d_out, uint64_t out_cap, uint64_t *d_out_len,
                          uint64_t *d_chunk_offsets)
{
    if (!ctx || !d_out_len || (in_len && (!d_in || !d_out)))
        return SNAPMI_E_ARGUMENT;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    if (in_len == 0) { // the identifier is written lazily: src/write.rs:154-170
        HIP_TRY(ctx, hipMemsetAsync(d_out_len, 0, sizeof(uint64_t), s));
        return SNAPMI_OK;
    }
    if (out_cap < snapmi_frame_max_len(in_len))
        return fail_ctx(ctx, SNAPMI_E_ARGUMENT,
                        "frame_compress: out_cap %llu < frame_max_len %zu",
                        (unsigned long long)out_cap,
                        snapmi_frame_max_len(in_len));
    const uint64_t n64 = (in_len + kMaxBlock - 1) / kMaxBlock;
    if (n64 > 0x7FFFFFFFu)
        return fail_ctx(ctx, SNAPMI_E_ARGUMENT, "frame_compress: too long");
    FrameList l;
    l.lone = true;
    l.in = d_in;
    l.in_len = in_len;
    l.out = d_out;
    l.out_lens = d_out_len;
    l.h_in_lens = &in_len;
    l.total = n64;
    l.chunk_offsets = d_chunk_offsets;
    return frame_compress_list(ctx, l);
}

int snapmi_frame_compress_chunks(snapmi_ctx *ctx, const void *d_in,
                                 const uint32_t *h_chunk_lens, size_t n,
                                 uint32_t flags, void *d_out, uint64_t out_cap,
                                 uint64_t *d_out_len,
                                 uint64_t *d_chunk_offsets)
{
    if (!ctx || !d_out_len || (n && (!d_in || !d_out || !h_chunk_lens)) ||
        n > 0x7FFFFFFFu || (flags & ~(uint32_t)SNAPMI_FRAME_NO_IDENT))
        return SNAPMI_E_ARGUMENT;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    if (n == 0) {
        HIP_TRY(ctx, hipMemsetAsync(d_out_len, 0, sizeof(uint64_t), s));
        return SNAPMI_OK;
    }
    // input offsets of the chunks: chunk i = d_in[off[i], off[i+1])
    std::vector<uint64_t> off(n + 1);
    off[0] = 0;
    for (size_t i = 0; i < n; i++) {
        if (h_chunk_lens[i] == 0 || h_chunk_lens[i] > kMaxBlock)
            return fail_ctx(ctx, SNAPMI_E_ARGUMENT,
                            "frame_compress_chunks: chunk %zu has %u bytes "
                            "(1..65536)", i, h_chunk_lens[i]);
        off[i + 1] = off[i] + h_chunk_lens[i];
    }
    const bool ident = !(flags & SNAPMI_FRAME_NO_IDENT);
    const uint64_t need = (ident ? 10 : 0) + off[n] + 8 * (uint64_t)n;
    if (out_cap < need)
        return fail_ctx(ctx, SNAPMI_E_ARGUMENT,
                        "frame_compress_chunks: out_cap %llu < %llu",
                        (unsigned long long)out_cap, (unsigned long long)need);
    int rc = reserve(ctx, ctx->fr_chunk_off, (n + 1) * sizeof(uint64_t));
    if (rc)
        return rc;
    HIP_TRY(ctx, hipMemcpyAsync(ctx->fr_chunk_off.p, off.data(),
                                (n + 1) * sizeof(uint64_t),
                                hipMemcpyHostToDevice, s));
    HIP_TRY(ctx, hipStreamSynchronize(s)); // `off` is pageable host memory
    FrameList l;
    l.lone = true;
    l.in = d_in;
    l.in_len = off[n];
    l.out = d_out;
    l.out_lens = d_out_len;
    l.total = n;
    l.chunk_in_off = (const uint64_t *)ctx->fr_chunk_off.p;
    l.h_chunk_lens = h_chunk_lens;
    l.ident = ident;
    l.chunk_offsets = d_chunk_offsets;
    return frame_compress_list(ctx, l);
}

int snapmi_frame_compress_batch(snapmi_ctx *ctx, const void *const *d_in_ptrs,
                                const uint64_t *d_in_lens,
                                const uint64_t *h_in_lens,
                                void *const *d_out_ptrs,
                                const uint64_t *d_out_caps,
                                uint64_t *d_out_lens, snapmi_error *d_errs,
                                size_t n)
{
    if (!ctx)
        return SNAPMI_E_ARGUMENT;
    if (n == 0)
        return SNAPMI_OK;
    if (!d_in_ptrs || !d_in_lens || !d_out_ptrs || !d_out_lens)
        return fail_ctx(ctx, SNAPMI_E_ARGUMENT,
                        "frame_compress_batch: bad args");
    if (n > 0x7FFFFFFFu)
        return fail_ctx(ctx, SNAPMI_E_ARGUMENT,
                        "frame_compress_batch: %zu streams (at most 2^31 - 1)",
                        n);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    std::vector<uint64_t> fetched;
    if (!h_in_lens) {
        fetched.resize(n);
        HIP_TRY(ctx, hipMemcpyAsync(fetched.data(), d_in_lens,
                                    n * sizeof(uint64_t),
                                    hipMemcpyDeviceToHost, s));
        HIP_TRY(ctx, hipStreamSynchronize(s));
        h_in_lens = fetched.data();
    }
    uint64_t total = 0;
    for (size_t i = 0; i < n; i++)
        total += (h_in_lens[i] + kMaxBlock - 1) / kMaxBlock;
    if (total > 0x7FFFFFFFu)
        return fail_ctx(ctx, SNAPMI_E_ARGUMENT,
                        "frame_compress_batch: %llu chunks (at most 2^31 - 1)",
                        (unsigned long long)total);
    FrameList l;
    l.in_ptrs = d_in_ptrs;
    l.in_lens = d_in_lens;
    l.out_ptrs = d_out_ptrs;
    l.out_caps = d_out_caps;
    l.out_lens = d_out_lens;
    l.errs = d_errs;
    l.n = n;
    l.h_in_lens = h_in_lens;
    l.total = total;
    return frame_compress_list(ctx, l);
}

// room for n_chunks chunks of total_bytes in all, framed
// (snapmi_frame_encode_host, snapmi_hostpipe.hip)
size_t snapmi_frame_encode_bound(size_t total_bytes, size_t n_chunks)
{
    return 10 + total_bytes + 8 * n_chunks;
}

} // extern "C"
