// snapmi_longstream.hip -- long raw streams decoded in pieces (the
// k_bstream_* kernels, planned by snapmi_streamplan.hpp): the long streams of
// a small batch, snapmi_decompress_batch, and a lone stream as a batch of one.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "snapmi.h"
#include "snapmi_test.h"
#include "snapmi_ctx.hpp"
#include "snapmi_launch.hpp"
#include "snapmi_device.hpp"
#include "snapmi_kernels.hpp"

using namespace snapmi;

namespace snapmi {

// ---------------------------------------------------------------------
// A batch of few streams waits for its longest one: a stream is decoded by
// one wavefront, 0.14 GiB/s, so the 702 KB of urls.10K are 4.9 ms whatever
// else the batch holds (extras.sweep: 64 MiB of the corpus round decoded at
// 12.8 GiB/s; now 34).  For batches of at most kBatchLongMaxN streams the long ones
// (long_stream_rule, k_long_plan; at
// most kBatchLongMaxL of them) go the way of snapmi_decompress_stream instead - scan, cuts, pieces,
// all long streams of the batch in the same launches (k_bstream_*) - and the
// batch's own launch skips them (mode 3).  The price is one look at the
// lengths on the host (k_long_plan, a copy of what it found, a stream
// synchronisation: ~30 us), which is why large batches, whose long streams
// hide behind each other, do not take it.
// ---------------------------------------------------------------------
// compressed bytes from which a stream can be worth its pieces
// (long_stream_rule; the test build reads SNAPMI_LONG_STREAM: the scalar
// entry points and snapmi_decompress_batch both use it).  Measured per bench
// input at 16 / 64 / 256 KiB (profiles/r4_scalar_latency.txt): the ten small
// launches of the scan cost ~0.5 ms, a wavefront decodes 100-250 MB/s of
// text: html (23 KB) 0.62 -> 0.73 ms through pieces, kppkn.gtb's 69 KB
// 2.12 -> 1.43, urls.10K 4.7 -> 1.3, fireworks.jpeg (literals) 0.17 -> 0.40
size_t long_stream_min()
{
    static const size_t v = [] {
#ifdef SNAPMI_TESTING
        if (const char *e = getenv("SNAPMI_LONG_STREAM"))
            return (size_t)atoll(e);
#endif
        return (size_t)(32 << 10);
    }();
    return v;
}

constexpr size_t kBatchLongMaxN = 16384;
constexpr uint32_t kBatchLongMaxL = 4096;

// The geometry of stream `g` of plan `p` and where its tables and piece
// descriptors lie in sd_tables / sd_desc (reserved for the plan); the caller
// sets the stream's own fields (in, out, out_len, err, fb_mode).
// (snapmi_build_block_index plans without pieces and may find sd_desc never
// reserved: it gets no piece pointers here and sets its own to nullptr.)
void stream_pointers(snapmi_ctx *ctx, const StreamPlan &p, const StreamSlot &g,
                     StreamArgs &a)
{
    uint8_t *const t = (uint8_t *)ctx->sd_tables.p;
    a.nseg = g.nseg;
    a.nsuper = g.nsuper;
    a.nsuper3 = g.nsuper3;
    a.kmax = g.kmax;
    a.seg_log2 = p.seg_log2;
    a.scan_segs = p.scan_segs;
    a.meta = (unsigned long long *)(t + g.meta);
    a.s1 = (unsigned long long *)(t + g.s1);
    a.s2 = (unsigned long long *)(t + g.s2);
    a.s3 = (unsigned long long *)(t + g.s3);
    a.e1 = (unsigned long long *)(t + g.e1);
    a.e2 = (unsigned long long *)(t + g.e2);
    a.e3 = (unsigned long long *)(t + g.e3);
    a.cuts = (unsigned long long *)(t + g.cuts);
    if (!ctx->sd_desc.p)
        return;
    a.c = piece_list_from(piece_list(ctx->sd_desc.p, p.pieces), g.entry);
}

// The streams of plan `p`, whose descriptor block (descriptors, then the
// workgroup prefixes) the device holds at `dev`, from their headers to the
// element boundaries at every 64 KiB of output: head, scan, the levels,
// chain, cuts.  (snapmi_build_block_index stops here: it keeps cuts[] and
// decodes nothing.)
int launch_stream_cuts(snapmi_ctx *ctx, const StreamPlan &p, const void *dev)
{
    hipStream_t s = ctx->stream;
    const uint32_t L = p.n;
    const uint32_t *pre = (const uint32_t *)((const uint8_t *)dev + p.pre_off);
    auto B = [&](int k) {
        BatchStreams b;
        b.descs = (const StreamArgs *)dev;
        b.pre = k < 0 ? nullptr : pre + (size_t)k * (L + 1);
        b.n = L;
        return b;
    };
    hipLaunchKernelGGL(k_bstream_head, dim3(L), dim3(1), 0, s, B(-1));
    LAUNCH_CHECK(k_bstream_head);
    hipLaunchKernelGGL(k_bstream_scan, dim3(p.grid[kPScan]), dim3(64), 0, s,
                       B(kPScan));
    LAUNCH_CHECK(k_bstream_scan);
    hipLaunchKernelGGL(k_bstream_super, dim3(p.grid[kPSuper]), dim3(kEntry), 0,
                       s, B(kPSuper));
    LAUNCH_CHECK(k_bstream_super);
    hipLaunchKernelGGL(k_bstream_super3, dim3(p.grid[kPSuper3]), dim3(kEntry),
                       0, s, B(kPSuper3));
    LAUNCH_CHECK(k_bstream_super3);
    hipLaunchKernelGGL(k_bstream_chain, dim3(L), dim3(1), 0, s, B(-1));
    LAUNCH_CHECK(k_bstream_chain);
    hipLaunchKernelGGL(k_bstream_spread3, dim3(p.grid[kPSpread3]), dim3(64), 0,
                       s, B(kPSpread3));
    LAUNCH_CHECK(k_bstream_spread3);
    hipLaunchKernelGGL(k_bstream_spread2, dim3(p.grid[kPSpread2]), dim3(64), 0,
                       s, B(kPSpread2));
    LAUNCH_CHECK(k_bstream_spread2);
    hipLaunchKernelGGL(k_bstream_cuts, dim3(p.grid[kPCuts]), dim3(64), 0, s,
                       B(kPCuts));
    LAUNCH_CHECK(k_bstream_cuts);
    return SNAPMI_OK;
}

// ... and on to their piece descriptors: the same, then pieces.
static int launch_stream_chain(snapmi_ctx *ctx, const StreamPlan &p,
                               const void *dev)
{
    if (int rc = launch_stream_cuts(ctx, p, dev))
        return rc;
    BatchStreams b;
    b.descs = (const StreamArgs *)dev;
    b.pre = (const uint32_t *)((const uint8_t *)dev + p.pre_off) +
            (size_t)kPPieces * (p.n + 1);
    b.n = p.n;
    hipLaunchKernelGGL(k_bstream_pieces, dim3(p.grid[kPPieces]), dim3(256), 0,
                       ctx->stream, b);
    LAUNCH_CHECK(k_bstream_pieces);
    return SNAPMI_OK;
}

static int decompress_batch_long(snapmi_ctx *ctx,
                                 const void *const *d_in_ptrs,
                                 const uint64_t *d_in_lens,
                                 void *const *d_out_ptrs,
                                 const uint64_t *d_out_caps,
                                 uint64_t *d_out_lens, snapmi_error *d_errs,
                                 size_t n, bool *done)
{
    *done = false;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    int rc;
    const size_t list_bytes = 16 + (size_t)kBatchLongMaxL * sizeof(LongItem);
    if ((rc = reserve(ctx, ctx->bl_modes, 2 * n + 64)) ||
        (rc = reserve(ctx, ctx->bl_list, list_bytes)) ||
        (rc = pin_reserve(ctx, ctx->pin_bl, list_bytes)))
        return rc;
    uint8_t *modes = (uint8_t *)ctx->bl_modes.p, *modes2 = modes + n;
    uint32_t *d_count = (uint32_t *)ctx->bl_list.p;
    LongItem *d_list = (LongItem *)((uint8_t *)ctx->bl_list.p + 16);
    HIP_TRY(ctx, hipMemsetAsync(d_count, 0, 16, s));
    hipLaunchKernelGGL(k_long_plan, dim3(1), dim3(1024), 0, s, d_in_ptrs,
                       d_in_lens, d_out_ptrs, d_out_caps, (uint32_t)n,
                       (uint64_t)long_stream_min(), modes, d_list,
                       kBatchLongMaxL,
                       d_count);
    LAUNCH_CHECK(k_long_plan);
    HIP_TRY(ctx, hipMemcpyAsync(ctx->pin_bl.p, ctx->bl_list.p, list_bytes,
                                hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipStreamSynchronize(s));
    const uint32_t found = *(const uint32_t *)ctx->pin_bl.p;
    // (none - or so many that they fill the chip a wavefront each: 3 670
    // long streams in 1 GiB of the corpus round decode in 4.0 ms through
    // pieces and in 5.9 a wavefront each, 3 058 streams of urls.10K at 314
    // and 288 GiB/s, and the gain goes on shrinking: the caller goes on
    // without modes)
    if (found == 0 || found > kBatchLongMaxL)
        return SNAPMI_OK;
    const uint32_t L = found;
    const LongItem *items =
        (const LongItem *)((const uint8_t *)ctx->pin_bl.p + 16);

    // ---- plan, scratch, descriptors --------------------------------------
    // (descriptors and prefixes are written into pinned memory of the
    // context: their copy to the device needs no wait - the next call's
    // synchronisation behind k_long_plan comes before they are written again)
    if ((rc = pin_reserve(ctx, ctx->pin_bl2,
                          (size_t)L * sizeof(StreamArgs) +
                              (size_t)kPre * (L + 1) * sizeof(uint32_t) + 64)))
        return rc;
    StreamArgs *const descs = (StreamArgs *)ctx->pin_bl2.p;
    std::vector<StreamSlot> slot(L);
    for (uint32_t j = 0; j < L; j++) {
        slot[j].in_len = items[j].in_len;
        slot[j].bound = items[j].dlen;
    }
    const StreamPlan p = plan_streams(
        slot.data(), L, false, ctx->stream_seg_log2, ctx->stream_scan_segs,
        sizeof(StreamArgs), (uint32_t *)(descs + L));
    if ((rc = reserve(ctx, ctx->sd_tables, p.t_bytes)) ||
        (rc = reserve(ctx, ctx->sd_desc, p.d_bytes)) ||
        (rc = reserve(ctx, ctx->bl_descs, p.desc_bytes + 64)))
        return rc;
    for (uint32_t j = 0; j < L; j++) {
        StreamArgs &a = descs[j];
        a.in = (const uint8_t *)items[j].in;
        a.in_len = items[j].in_len;
        a.out = (uint8_t *)items[j].out;
        a.out_cap = items[j].out_cap;
        a.out_len = (unsigned long long *)(d_out_lens + items[j].idx);
        a.err = d_errs ? d_errs + items[j].idx : nullptr;
        a.fb_mode = modes2 + items[j].idx;
        stream_pointers(ctx, p, slot[j], a);
    }
    HIP_TRY(ctx, hipMemcpyAsync(ctx->bl_descs.p, descs, p.desc_bytes,
                                hipMemcpyHostToDevice, s));
    HIP_TRY(ctx, hipMemsetAsync((uint8_t *)ctx->sd_tables.p + p.e_off, 0xFF,
                                p.e_bytes, s));
    HIP_TRY(ctx, hipMemsetAsync(modes2, 3, n, s));
    // the batch's other streams beside all this, on the second stream
    // (their longest is 0.6-0.8 ms of one wavefront on the corpus)
    HIP_TRY(ctx, hipEventRecord(ctx->ev_fork, s));
    HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream2, ctx->ev_fork, 0));
    // from here on every way out joins the side stream again: whatever
    // it was given still writes the caller's arrays and reads bl_modes /
    // bl_order, which the next call reuses
    struct SideJoin {
        snapmi_ctx *c;
        hipStream_t s;
        bool joined = false;
        void join()
        {
            if (joined)
                return;
            joined = true;
            if (hipEventRecord(c->ev_join, c->stream2) != hipSuccess ||
                hipStreamWaitEvent(s, c->ev_join, 0) != hipSuccess) {
                (void)hipGetLastError();
                (void)hipStreamSynchronize(c->stream2);
            }
        }
        ~SideJoin() { join(); }
    } side{ctx, s};
    if ((rc = launch_decompress(ctx, d_in_ptrs, d_in_lens, d_out_ptrs,
                                d_out_caps, d_out_lens, d_errs, modes, n,
                                nullptr, 0, ctx->stream2, &ctx->bl_order)) ||
        (rc = launch_stream_chain(ctx, p, ctx->bl_descs.p)))
        return rc;
    // the pieces of the long streams; which of the long ones were
    // irregular; those, by the wavefront decoder
    if ((rc = launch_pieces(ctx, piece_list(ctx->sd_desc.p, p.pieces),
                            p.pieces)))
        return rc;
    hipLaunchKernelGGL(k_bstream_finish, dim3(L), dim3(1024), 0, s,
                       BatchStreams{(const StreamArgs *)ctx->bl_descs.p,
                                    nullptr, L});
    LAUNCH_CHECK(k_bstream_finish);
    side.join();
    // (without timing events: snapmi_last_timing reports the pieces)
    if ((rc = launch_decompress(ctx, d_in_ptrs, d_in_lens, d_out_ptrs,
                                d_out_caps, d_out_lens, d_errs, modes2, n,
                                nullptr, 0, s, nullptr)))
        return rc;
    *done = true;
    return SNAPMI_OK;
}

} // namespace snapmi

extern "C" {

int snapmi_decompress_batch(snapmi_ctx *ctx, const void *const *d_in_ptrs,
                            const uint64_t *d_in_lens,
                            void *const *d_out_ptrs,
                            const uint64_t *d_out_caps, uint64_t *d_out_lens,
                            snapmi_error *d_errs, size_t n)
{
    if (!ctx)
        return SNAPMI_E_ARGUMENT;
    if (n == 0)
        return SNAPMI_OK;
    if (!d_in_ptrs || !d_in_lens || !d_out_ptrs || !d_out_caps ||
        !d_out_lens || n > 0x7FFFFFFFu)
        return fail_ctx(ctx, SNAPMI_E_ARGUMENT, "decompress_batch: bad args");
    // (the look at the batch waits for the device once: never while the
    // caller's stream is being captured into a graph - such a caller gets the
    // enqueue-only path, a wavefront per stream)
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(ctx->stream, &cap) != hipSuccess) {
        (void)hipGetLastError();
        cap = hipStreamCaptureStatusNone;
    }
    if (ctx->batch_long_streams && n <= kBatchLongMaxN &&
        cap == hipStreamCaptureStatusNone) {
        bool done = false;
        const int rc = decompress_batch_long(ctx, d_in_ptrs, d_in_lens,
                                             d_out_ptrs, d_out_caps,
                                             d_out_lens, d_errs, n, &done);
        if (rc || done)
            return rc;
    }
    return launch_decompress(ctx, d_in_ptrs, d_in_lens, d_out_ptrs, d_out_caps,
                             d_out_lens, d_errs, nullptr, n);
}

// One stream as a batch of one, enqueue-only (the scalar entry points wait
// for nothing else).  Its descriptor, the prefixes of its launches and the
// whole stream for the sequential decoder reach the device in one copy from
// this frame: the runtime stages a pageable copy before the call returns.
int snapmi_decompress_stream(snapmi_ctx *ctx, const void *d_in,
                             uint64_t in_len, void *d_out, uint64_t out_cap,
                             uint64_t *d_out_len, snapmi_error *d_err)
{
    if (!ctx || !d_out_len || !d_err || (in_len && !d_in) ||
        (out_cap && !d_out))
        return fail_ctx(ctx, SNAPMI_E_ARGUMENT, "decompress_stream: bad args");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    struct Lone {
        StreamArgs a;
        uint32_t pre[kPre * 2];
        // the whole stream, mode 0 (decode it), for the sequential decoder
        const void *in;
        uint64_t in_len;
        void *out;
        uint64_t cap;
        uint8_t mode;
    } h = {};
    static_assert(offsetof(Lone, pre) == sizeof(StreamArgs),
                  "the descriptor block of plan_streams");
    StreamSlot slot;
    slot.in_len = in_len;
    slot.bound = lone_stream_bound(in_len, out_cap);
    const StreamPlan p =
        plan_streams(&slot, 1, true, ctx->stream_seg_log2,
                     ctx->stream_scan_segs, sizeof(StreamArgs), h.pre);
    if (!p.fits)
        return fail_ctx(ctx, SNAPMI_E_ARGUMENT, "decompress_stream: too long");
    int rc;
    if ((rc = reserve(ctx, ctx->sd_tables, p.t_bytes)) ||
        (rc = reserve(ctx, ctx->sd_desc, p.d_bytes)) ||
        (rc = reserve(ctx, ctx->bl_descs, sizeof h)))
        return rc;
    StreamArgs &a = h.a;
    a.in = (const uint8_t *)d_in;
    a.in_len = in_len;
    a.out = (uint8_t *)d_out;
    a.out_cap = out_cap;
    a.out_len = (unsigned long long *)d_out_len;
    a.err = d_err;
    a.fb_mode = nullptr;
    stream_pointers(ctx, p, slot, a);
    h.in = d_in;
    h.in_len = in_len;
    h.out = d_out;
    h.cap = out_cap;
    const Lone *dh = (const Lone *)ctx->bl_descs.p;
    HIP_TRY(ctx, hipMemcpyAsync(ctx->bl_descs.p, &h, sizeof h,
                                hipMemcpyHostToDevice, s));
    HIP_TRY(ctx, hipMemsetAsync((uint8_t *)ctx->sd_tables.p + p.e_off, 0xFF,
                                p.e_bytes, s));
    if ((rc = launch_stream_chain(ctx, p, dh)))
        return rc;
    // the pieces, unless the scan gave up (meta[2] == 1) ...
    if ((rc = launch_pieces(ctx, piece_list(ctx->sd_desc.p, p.pieces),
                            a.kmax, a.meta + 2, 0)))
        return rc;
    hipLaunchKernelGGL(k_bstream_finish, dim3(1), dim3(1024), 0, s,
                       BatchStreams{&dh->a, nullptr, 1});
    LAUNCH_CHECK(k_bstream_finish);
    // ... and the sequential decoder over the whole stream if anything was
    // irregular: it owns the error report
    return launch_decompress(ctx, &dh->in, &dh->in_len, &dh->out, &dh->cap,
                             d_out_len, d_err, &dh->mode, 1, a.meta + 2, 1);
}

int snapmi_stream_decode_path(snapmi_ctx *ctx)
{
    if (!ctx || !ctx->sd_tables.p)
        return -1;
    unsigned long long meta[4];
    if (hipSetDevice(ctx->device) != hipSuccess ||
        hipStreamSynchronize(ctx->stream) != hipSuccess ||
        hipMemcpy(meta, ctx->sd_tables.p, sizeof meta,
                  hipMemcpyDeviceToHost) != hipSuccess)
        return -1;
    return meta[2] ? 1 : 0;
}

} // extern "C"
