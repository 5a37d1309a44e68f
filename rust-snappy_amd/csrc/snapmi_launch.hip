// snapmi_launch.hip -- the launchers of the raw codec: the batch compress
// entry points and launch_compress (route, scratch, the kernels of the route),
// launch_decompress.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>
#include <vector>

#include "snapmi.h"
#include "snapmi_test.h"
#include "snapmi_ctx.hpp"
#include "snapmi_launch.hpp"
#include "snapmi_pool.hpp"
#include "snapmi_route.hpp"
#include "snapmi_device.hpp"
#include "snapmi_kernels.hpp"

using namespace snapmi;

namespace snapmi {
static_assert(kRouteCompressWaves == kCompressWaves &&
                  kRouteSmallTableWaves == kSmallTableWaves &&
                  kRouteBothWaves == kBothWaves &&
                  kRouteBothLaneWaves == kBothLaneWaves &&
                  kRouteTinyCompress == kTinyCompress &&
                  kRouteSmallCompress == kSmallCompress,
              "snapmi_route.hpp and snapmi_kernels.hpp disagree");

static_assert(snapmi::kPoolTokPage == kTokPage &&
                  snapmi::kPoolExcPage == kExcPage &&
                  snapmi::kPoolPagesPerBlock ==
                      kTokPagesPerBlock + kExcPagesPerBlock,
              "snapmi_pool.hpp and snapmi_kernels.hpp disagree");

} // namespace snapmi

extern "C" {

// ----------------------------------------------------------------------
// batched device-resident API
// ----------------------------------------------------------------------
// snapmi_compress_batch, and with `indexed` snapmi_compress_batch_indexed:
// the same launches, and behind them the kernels that write the block index
static int compress_batch(snapmi_ctx *ctx, const void *const *d_in_ptrs,
                          const uint64_t *d_in_lens,
                          const uint64_t *h_in_lens, void *const *d_out_ptrs,
                          const uint64_t *d_out_caps, uint64_t *d_out_lens,
                          snapmi_error *d_errs, size_t n, bool indexed,
                          uint64_t *d_index_first, uint64_t *d_index,
                          uint64_t index_cap)
{
    if (!ctx)
        return SNAPMI_E_ARGUMENT;
    if (n == 0)
        return SNAPMI_OK;
    if (!d_in_ptrs || !d_in_lens || !d_out_ptrs || !d_out_lens ||
        n > 0x7FFFFFFFu || (indexed && (!d_index_first || !d_index)))
        return fail_ctx(ctx, SNAPMI_E_ARGUMENT, "compress_batch: bad args");
    HIP_TRY(ctx, hipSetDevice(ctx->device));

    std::vector<uint64_t> fetched;
    if (!h_in_lens) {
        fetched.resize(n);
        HIP_TRY(ctx, hipMemcpyAsync(fetched.data(), d_in_lens,
                                    n * sizeof(uint64_t),
                                    hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        h_in_lens = fetched.data();
    }
    uint64_t blocks = 0, slots = 0, cnt8 = 0, block_bytes = 0;
    // streams under this length are the lane-per-stream kernels': no block
    const uint64_t small = small_stream_limit(*ctx);
    uint32_t classes = 0; // which of those kernels have anything to do
    for (size_t i = 0; i < n; i++) {
        const uint64_t len = h_in_lens[i];
        // (first the cheap test: a batch of ten million tiny streams is
        // walked here once per call)
        if (len < small) {
            classes |= len < kTinyCompress ? (len ? 1u : 0u)
                                           : (len < 512 ? 2u
                                                        : (len < 1024 ? 4u : 8u));
            continue;
        }
        if (len == 0 || max_compress_len_u64(len) == 0)
            continue;
        const uint64_t nb = (len + kMaxBlock - 1) / kMaxBlock;
        blocks += nb;
        block_bytes += len;
        slots += nb - 1;
        // the stream's last block: a page, a short chunk, a tail?
        const uint64_t last = len - (nb - 1) * kMaxBlock;
        cnt8 += last <= 8192;
    }
    uint64_t entries = 0;
    if (indexed) {
        entries = snapmi_block_index_entries(h_in_lens, n);
        if (entries > index_cap)
            return fail_ctx(ctx, SNAPMI_E_ARGUMENT,
                            "compress_batch_indexed: the index takes %llu "
                            "entries, index_cap is %llu",
                            (unsigned long long)entries,
                            (unsigned long long)index_cap);
    }
    return launch_compress(ctx, d_in_ptrs, d_in_lens, d_out_ptrs, d_out_caps,
                           d_out_lens, d_errs, n, blocks, slots, classes,
                           cnt8, block_bytes, indexed ? d_index_first : nullptr,
                           d_index, entries);
}

uint64_t snapmi_block_index_entries(const uint64_t *h_in_lens, size_t n)
{
    uint64_t entries = 0;
    for (size_t i = 0; h_in_lens && i < n; i++)
        entries += snapmi::bi_entries(h_in_lens[i]);
    return entries;
}

int snapmi_compress_batch(snapmi_ctx *ctx, const void *const *d_in_ptrs,
                          const uint64_t *d_in_lens,
                          const uint64_t *h_in_lens, void *const *d_out_ptrs,
                          const uint64_t *d_out_caps, uint64_t *d_out_lens,
                          snapmi_error *d_errs, size_t n)
{
    return compress_batch(ctx, d_in_ptrs, d_in_lens, h_in_lens, d_out_ptrs,
                          d_out_caps, d_out_lens, d_errs, n, false, nullptr,
                          nullptr, 0);
}

int snapmi_compress_batch_indexed(snapmi_ctx *ctx,
                                  const void *const *d_in_ptrs,
                                  const uint64_t *d_in_lens,
                                  const uint64_t *h_in_lens,
                                  void *const *d_out_ptrs,
                                  const uint64_t *d_out_caps,
                                  uint64_t *d_out_lens, snapmi_error *d_errs,
                                  size_t n, uint64_t *d_index_first,
                                  uint64_t *d_index, uint64_t index_cap)
{
    return compress_batch(ctx, d_in_ptrs, d_in_lens, h_in_lens, d_out_ptrs,
                          d_out_caps, d_out_lens, d_errs, n, true,
                          d_index_first, d_index, index_cap);
}

} // extern "C"

namespace snapmi {

// k_scan_sizes over the blocks [a.blk_lo, min(a.blk_hi, host_blocks))
static void launch_scan_sizes(const CompressArgs &a, hipStream_t s)
{
    const uint32_t hi = a.blk_hi < a.host_blocks ? a.blk_hi : a.host_blocks;
    launch_scan(
        hi > a.blk_lo ? hi - a.blk_lo : 0,
        [&] { hipLaunchKernelGGL(k_scan_sizes, dim3(1), dim3(1024), 0, s, a); },
        [&](uint32_t parts) {
            hipLaunchKernelGGL(k_scan_sizes_a, dim3(parts), dim3(1024), 0, s,
                               a, parts);
            hipLaunchKernelGGL(k_scan_sizes_b, dim3(1), dim3(1024), 0, s, a,
                               parts);
            hipLaunchKernelGGL(k_scan_sizes_c, dim3(parts), dim3(1024), 0, s,
                               a);
        });
}

// match_kernel 2's hint: the latest batch that has finished (a slot reads 0
// in word 4 while a kernel is writing it) compressed to no less than
// match_spans_ratio_pct of its input
static bool spans_hint(const snapmi_ctx *ctx)
{
    if (ctx->match_kernel != 2 || !ctx->h_ratio)
        return false;
    const volatile uint32_t *r = ctx->h_ratio;
    const uint32_t s0 = r[4], s1 = r[12];
    const volatile uint32_t *slot = s1 > s0 ? r + 8 : r;
    const uint32_t seq = slot[4];
    const uint64_t c = ((uint64_t)slot[1] << 32) | slot[0];
    const uint64_t u = ((uint64_t)slot[3] << 32) | slot[2];
    return seq && slot[4] == seq && u &&
           c * 100 >= u * ctx->match_spans_ratio_pct;
}

// the route's window kernel over the whole batch, on stream ws
static void launch_window(const CompressRoute &route, const CompressArgs &a,
                          hipStream_t ws)
{
    const dim3 grid(route.window_grid);
    switch (route.window) {
    case WindowKernel::spans:
        hipLaunchKernelGGL(k_compress_spans, grid, dim3(kCompressWaves * 64),
                           0, ws, a);
        break;
    case WindowKernel::span_lds:
        hipLaunchKernelGGL(k_compress_span_lds, grid, dim3(64), 0, ws, a);
        break;
#ifdef SNAPMI_TESTING // (span_kernel 0: the product refuses it)
    case WindowKernel::blocks:
        hipLaunchKernelGGL(k_compress_blocks, grid, dim3(kCompressWaves * 64),
                           0, ws, a);
        break;
    case WindowKernel::block_lds:
        hipLaunchKernelGGL(k_compress_block_lds, grid, dim3(64), 0, ws, a);
        break;
#endif
    default:
        break;
    }
}

// the route's match finder over the blocks [a.blk_lo, a.blk_hi) of segment g
static void launch_match(const RouteDevice &d, const CompressRoute &route,
                         const Segment &g, CompressArgs a, hipStream_t s)
{
    const dim3 grid(match_grid(d, route, a.blk_hi - a.blk_lo));
    switch (route.match) {
    case MatchKernel::spans:
        hipLaunchKernelGGL(k_match_spans, grid, dim3(kCompressWaves * 64), 0,
                           s, a);
        break;
    case MatchKernel::both:
        a.tok_stage_wave0 = kBothLaneWaves;
        hipLaunchKernelGGL(a.lane_tail_depth > 1 ? k_match_both
                                                 : k_match_both_plain,
                           grid, dim3(kBothWaves * 64), 0, s, a);
        break;
    case MatchKernel::blocks:
        a.lane_depth = g.spec ? 2 : 1;
        // (the tail form only where it would ever run more probes)
        hipLaunchKernelGGL(a.lane_tail_depth > a.lane_depth
                               ? k_match_blocks
                               : (g.spec ? k_match_blocks_spec
                                         : k_match_blocks_plain),
                           grid, dim3(64), 0, s, a);
        break;
    case MatchKernel::none:
        break;
    }
}

int launch_compress(snapmi_ctx *ctx, const void *const *d_in_ptrs,
                    const uint64_t *d_in_lens, void *const *d_out_ptrs,
                    const uint64_t *d_out_caps, uint64_t *d_out_lens,
                    snapmi_error *d_errs, size_t n, uint64_t blocks,
                    uint64_t slots, uint32_t small_classes, uint64_t cnt8,
                    uint64_t block_bytes, uint64_t *d_index_first,
                    uint64_t *d_index, uint64_t index_entries)
{
    if (blocks > 0x7FFFFFFFu)
        return fail_ctx(ctx, SNAPMI_E_ARGUMENT,
                        "compress_batch: %llu blocks in one batch",
                        (unsigned long long)blocks);
    HIP_TRY(ctx, hipSetDevice(ctx->device));

    int rc;
    if ((rc = reserve(ctx, ctx->blk_first, (n + 1) * sizeof(uint32_t))) ||
        (rc = reserve(ctx, ctx->slot_first, (n + 1) * sizeof(uint32_t))) ||
        (rc = reserve(ctx, ctx->blk_size, (blocks + 1) * sizeof(uint32_t))) ||
        (rc = reserve(ctx, ctx->blk_off, (blocks + 2) * sizeof(uint64_t))) ||
        (rc = reserve(ctx, ctx->plan_part,
                      ((n > blocks ? n : blocks) / 1024 + 4) * 16)) ||
        (rc = reserve(ctx, ctx->ticket, 64)))
        return rc;

    // which kernels the batch runs (snapmi_route.hpp)
    const RouteDevice d = {ctx->lds_order_ok, (uint32_t)ctx->num_cus};
    const CompressRoute route =
        compress_route(*ctx, d, blocks, cnt8, spans_hint(ctx));

    CompressArgs a;
    a.in_ptrs = d_in_ptrs;
    a.in_lens = d_in_lens;
    a.out_ptrs = d_out_ptrs;
    a.out_caps = d_out_caps;
    a.out_lens = d_out_lens;
    a.errs = d_errs;
    a.blk_first = (uint32_t *)ctx->blk_first.p;
    a.slot_first = (uint32_t *)ctx->slot_first.p;
    a.blk_size = (uint32_t *)ctx->blk_size.p;
    a.blk_off = (uint64_t *)ctx->blk_off.p;
    // (the two scans never run at the same time: one buffer for both)
    a.plan_part = (uint32_t *)ctx->plan_part.p;
    a.scan_part = (unsigned long long *)ctx->plan_part.p;
    a.n_streams = (uint32_t)n;
    a.host_blocks = (uint32_t)blocks;
    a.host_slots = (uint32_t)slots;
    a.ticket = (uint32_t *)ctx->ticket.p;
    a.tok_pool = nullptr;
    a.tok_pages = nullptr;
    a.tok_ctl = nullptr;
    a.tok_pool_pages = 0;
    a.tok_stage = nullptr;
    a.tok_stage_waves = 0;
    a.tok_stage_wave0 = 0;
    a.sched = nullptr;
    a.ntok = nullptr;
    a.lane_tables = nullptr;
    a.lane_epochs = nullptr;
    a.lane_stride = kMaxTable;
    a.lane_chunks = 0;
    a.lane_per_chunk = 0;
    a.n_lanes = 0;
    a.lane_depth = 1;
    a.lane_tail_depth = 0;
    a.lane_tail_idle = 0;
    a.tok_base = 0;
    a.small_limit = (uint32_t)small_stream_limit(*ctx);
    a.cls_lo = 0;
    a.cls_hi = kMaxBlock;
    a.direct = route.direct ? 1 : 0;
    if (!route.direct &&
        (rc = reserve(ctx, ctx->slots, (slots + 1) * (size_t)kSlotBytes)))
        return rc;
    a.scratch = (uint8_t *)ctx->slots.p;
    a.blk_lo = 0;
    a.blk_hi = (uint32_t)blocks;
    // The token pool (CompressArgs::tok_pool): pages of 2 KiB for the tokens
    // of a launch's blocks - token_pool_pct per cent of what the worst case
    // of every block would take, and what the launch keeps in hand on top;
    // never fewer than 32 768 pages (64 MiB: a small batch does not spill);
    // grown for the batch behind one of which more than a hundredth spilled
    // - by half, or by a sixth when it was less than a tenth (k_redo_spilled
    // posts the counts; read without waiting, like the ratio hint).
    if (ctx->h_tokstat) {
        const volatile uint32_t *t = ctx->h_tokstat;
        const uint32_t seq = t[3];
        if (seq != ctx->tokstat_seen) {
            ctx->tokstat_seen = seq;
            const uint32_t asked = t[0], spilled = t[1], of = t[2];
            if (t[3] == seq && of) {
                ctx->tok_pages_asked = asked;
                ctx->tok_blocks_spilled = spilled;
                ctx->token_pool_now =
                    snapmi::pool_grow(ctx->token_pool_now, spilled, of);
            }
        }
    }
    if (ctx->token_pool_now < ctx->token_pool_pct)
        ctx->token_pool_now = ctx->token_pool_pct;
    // (snapmi_pool.hpp: the share of the worst case, what the launch keeps in
    // hand, the floor, and "100 means never")
    const uint64_t pool_pages =
        snapmi::pool_pages(block_bytes, blocks, route.seg_blocks, route.lanes,
                           ctx->token_pool_now, ctx->token_pool_min_pages);
    // (+ the dump page of the lanes)
    const size_t pool_bytes = (size_t)(pool_pages + 1) * kTokPage * 4;
    const size_t stage_bytes =
        (size_t)ctx->num_cus * route.stage_waves * kTokStageWords * 4;
    a.tok_stage_waves = route.stage_waves;
    a.tok_stage_wave0 = 0;
    // ... and behind its control words and the list of the spilled blocks,
    // the blocks' page tables
    const size_t tab_off =
        ((size_t)(kTokCtlList + route.seg_blocks) * 4 + 255) & ~(size_t)255;
    const size_t tab_bytes =
        tab_off + (size_t)route.seg_blocks * kPageTabStride * 4;
    if (route.tokens) {
        if (route.lanes > ctx->n_lanes) {
            if ((rc = place_lane_tables(ctx, route.lanes,
                                        /*top_of_memory=*/false)))
                return rc;
            ctx->lane_tables_top = false;
        }
        if ((rc = reserve(ctx, ctx->tokens, pool_bytes, /*slack=*/false)) ||
            (rc = reserve(ctx, ctx->tok_pages, tab_bytes)) ||
            (rc = reserve(ctx, ctx->tok_stage, stage_bytes + 256)) ||
            (rc = reserve(ctx, ctx->ntok, (size_t)blocks * sizeof(uint32_t))))
            return rc;
        // test knob, see snapmi_ctx.hpp
        if (route.lanes && ctx->lane_epoch_preset >= 0) {
            HIP_TRY(ctx, hipMemsetD32Async((hipDeviceptr_t)ctx->lane_epochs.p,
                                           (int)ctx->lane_epoch_preset,
                                           ctx->n_lanes, ctx->stream));
            ctx->lane_epoch_preset = -1;
        }
        a.tok_pool = (uint32_t *)ctx->tokens.p;
        a.tok_ctl = (uint32_t *)ctx->tok_pages.p;
        a.tok_pages = (uint32_t *)((uint8_t *)ctx->tok_pages.p + tab_off);
        a.tok_pool_pages = (uint32_t)pool_pages;
        a.tok_stage = (uint32_t *)ctx->tok_stage.p;
        ctx->tok_pool_pages_last = (uint32_t)pool_pages;
        a.ntok = (uint32_t *)ctx->ntok.p;
        if (route.lanes) {
            a.lane_tables = (unsigned long long *)ctx->lane_tables.p;
            a.lane_epochs = (uint32_t *)ctx->lane_epochs.p;
            a.lane_stride = ctx->lane_stride;
            a.lane_chunks = ctx->lane_chunk_count;
            a.lane_per_chunk = ctx->lane_per_chunk;
            a.n_lanes = route.lanes;
            // options lane_tail_probes, lane_tail_idle_pct: lanes out of
            // work from which a wavefront resolves more probes a round (one
            // lane at least: 0 means from the first round)
            if (ctx->lane_tail_probes > 1) {
                const uint64_t idle =
                    ((uint64_t)route.lanes * ctx->lane_tail_idle_pct + 99) /
                    100;
                a.lane_tail_depth = ctx->lane_tail_probes;
                a.lane_tail_idle = ctx->lane_tail_idle_pct == 0 ? 0
                                   : idle                       ? (uint32_t)idle
                                                                : 1;
            }
        }
    }
    a.prof = nullptr;
    PROF(
    if ((rc = reserve(ctx, ctx->st_prof, 16 * sizeof(uint64_t))))
        return rc;
    HIP_TRY(ctx, hipMemsetAsync(ctx->st_prof.p, 0, 16 * sizeof(uint64_t),
                                ctx->stream));
    a.prof = (unsigned long long *)ctx->st_prof.p;
    )
    PROF_TAIL(
    {
        const size_t bytes =
            (size_t)(kProfTailLanes + route.lanes) * sizeof(uint64_t);
        if ((rc = reserve(ctx, ctx->st_prof, bytes)))
            return rc;
        HIP_TRY(ctx, hipMemsetAsync(ctx->st_prof.p, 0, bytes, ctx->stream));
        a.prof = (unsigned long long *)ctx->st_prof.p;
        ctx->prof_tail_lanes = route.lanes;
    }
    )

    hipStream_t s = ctx->stream;
    ctx->timing_valid = false;
    HIP_TRY(ctx, hipEventRecord(ctx->ev[0], s));
    launch_scan(
        n,
        [&] {
            hipLaunchKernelGGL(k_plan_compress, dim3(1), dim3(1024), 0, s, a);
        },
        [&](uint32_t parts) {
            hipLaunchKernelGGL(k_plan_compress_a, dim3(parts), dim3(1024), 0,
                               s, a);
            hipLaunchKernelGGL(k_plan_compress_b, dim3(1), dim3(1024), 0, s, a,
                               parts);
            hipLaunchKernelGGL(k_plan_compress_c, dim3(parts), dim3(1024), 0,
                               s, a);
        });
    HIP_TRY(ctx, hipEventRecord(ctx->ev[1], s));
    // the lane-per-stream kernels: streams under 256 bytes one per lane,
    // streams under 1 KiB a few per wavefront (a wavefront of streams that
    // are all larger returns at once: 16 384 idle wavefronts for a million
    // 64 KiB chunks).  small_classes: what the caller knows of the lengths -
    // a class without a stream is not launched.
    {
        const dim3 grid((uint32_t)((n + 63) / 64));
        if (a.small_limit && (small_classes & 1))
            hipLaunchKernelGGL(k_compress_tiny, grid, dim3(64), 0, s, a);
        if (a.small_limit > kTinyCompress) {
            if (small_classes & 2)
                hipLaunchKernelGGL(k_compress_small512, grid, dim3(64), 0, s,
                                   a);
            if (small_classes & 4)
                hipLaunchKernelGGL(k_compress_small1k, grid, dim3(64), 0, s,
                                   a);
            if (small_classes & 8)
                hipLaunchKernelGGL(k_compress_small2k, grid, dim3(64), 0, s,
                                   a);
        }
    }
    if (route.window != WindowKernel::none) {
        HIP_TRY(ctx, hipMemsetAsync(ctx->ticket.p, 0, 64, s));
        hipStream_t ws = s; // stream of the window kernel
        if (route.window_beside) {
            HIP_TRY(ctx, hipEventRecord(ctx->ev_fork, s));
            HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream2, ctx->ev_fork, 0));
            ws = ctx->stream2;
        }
        if (route.sched) {
            const size_t head = (size_t)(16 + n) * 4;
            const size_t lists = (size_t)2 * (slots + 1) * 4;
            if ((rc = reserve(ctx, ctx->sched, head + lists)))
                return rc;
            HIP_TRY(ctx, hipMemsetAsync(ctx->sched.p, 0, head, ws));
            HIP_TRY(ctx, hipMemsetAsync((uint8_t *)ctx->sched.p + head, 0xFF,
                                        lists, ws));
            a.sched = (uint32_t *)ctx->sched.p;
        }
        launch_window(route, a, ws);
        a.sched = nullptr;
    }
    if (route.tokens) {
        HIP_TRY(ctx, hipEventRecord(ctx->ev[4], s));
        for (uint64_t lo = 0; lo < blocks; lo += route.seg_blocks) {
            const uint64_t hi = lo + route.seg_blocks < blocks
                                    ? lo + route.seg_blocks
                                    : blocks;
            const Segment g = segment(*ctx, d, route, lo, hi);
            a.tok_base = (uint32_t)lo;
            a.blk_lo = (uint32_t)lo;
            a.blk_hi = (uint32_t)g.mid;
            // the pool is the segment's: no page handed out, no block
            // spilled, k_redo_spilled's ticket at 0
            HIP_TRY(ctx, hipMemsetAsync(ctx->tok_pages.p, 0,
                                        kTokCtlList * 4, s));
            if (route.window == WindowKernel::none) // (else shared with it)
                HIP_TRY(ctx, hipMemsetAsync(ctx->ticket.p, 0, 64, s));
            // (with the small-block kernels on, this launch's class is the
            // blocks of more than 8 KiB - if the batch has any)
            a.cls_lo = route.small_grid ? 8192 : 0;
            launch_match(d, route, g, a, s);
            if (route.small_grid) {
                HIP_TRY(ctx, hipMemsetAsync(ctx->ticket.p, 0, 64, s));
                a.cls_lo = 0;
                a.cls_hi = 8192;
                hipLaunchKernelGGL(k_match_spans_8k, dim3(route.small_grid),
                                   dim3(kSmallTableWaves * 64), 0, s, a);
            }
            a.cls_lo = 0;
            a.cls_hi = kMaxBlock;
            if (g.mid < hi) {
                HIP_TRY(ctx, hipEventRecord(ctx->ev_fork, s));
                HIP_TRY(ctx,
                        hipStreamWaitEvent(ctx->stream2, ctx->ev_fork, 0));
                hipLaunchKernelGGL(k_encode_tokens,
                                   dim3((uint32_t)(g.mid - lo)), dim3(64), 0,
                                   ctx->stream2, a);
                HIP_TRY(ctx, hipEventRecord(ctx->ev_join, ctx->stream2));
                a.blk_lo = (uint32_t)g.mid;
                a.blk_hi = (uint32_t)hi;
                HIP_TRY(ctx, hipMemsetAsync(ctx->ticket.p, 0, 64, s));
                launch_match(d, route, g, a, s);
            }
            if (hi == blocks) // dominant_ms: first match start .. last end
                HIP_TRY(ctx, hipEventRecord(ctx->ev[5], s));
            if (route.window_beside) {
                HIP_TRY(ctx, hipEventRecord(ctx->ev_join, ctx->stream2));
                HIP_TRY(ctx, hipStreamWaitEvent(s, ctx->ev_join, 0));
            }
            if (route.direct)
                launch_scan_sizes(a, s);
            hipLaunchKernelGGL(k_encode_tokens,
                               dim3((uint32_t)(hi - a.blk_lo)), dim3(64), 0, s,
                               a);
            if (g.mid < hi) // the side stream's half is done as well
                HIP_TRY(ctx, hipStreamWaitEvent(s, ctx->ev_join, 0));
            // the blocks whose tokens found no page: once more, by the window
            // kernel, to where the encoder would have put them
            // (CompressArgs::tok_pool)
            if (!ctx->h_tokstat) {
                HIP_TRY(ctx, hipHostMalloc((void **)&ctx->h_tokstat, 64,
                                           hipHostMallocDefault));
                memset((void *)ctx->h_tokstat, 0, 64);
            }
            CompressArgs r = a;
            r.blk_lo = (uint32_t)lo;
            r.blk_hi = (uint32_t)hi;
            r.cls_lo = 0;
            r.cls_hi = kMaxBlock;
            hipLaunchKernelGGL(k_redo_spilled, dim3(g.redo_grid),
                               dim3(kCompressWaves * 64), 0, s, r,
                               (uint32_t *)ctx->h_tokstat, ++ctx->tokstat_seq);
        }
        a.blk_lo = 0;
        a.tok_base = 0;
        a.blk_hi = (uint32_t)blocks;
    }
    HIP_TRY(ctx, hipEventRecord(ctx->ev[2], s));
    if (route.direct) {
        hipLaunchKernelGGL(k_stream_lens, dim3((uint32_t)((n + 255) / 256)),
                           dim3(256), 0, s, a);
        // what this batch compressed to, for the next batch's choice of
        // match finder (read without waiting: a hint)
        if (route.post_ratio) {
            if (!ctx->h_ratio) {
                HIP_TRY(ctx, hipHostMalloc((void **)&ctx->h_ratio, 64,
                                           hipHostMallocDefault));
                memset((void *)ctx->h_ratio, 0, 64);
            }
            hipLaunchKernelGGL(k_post_ratio, dim3(1), dim3(1024), 0, s,
                               (uint32_t *)ctx->h_ratio, a.blk_off,
                               (uint32_t)blocks, a.in_lens, a.n_streams,
                               ++ctx->ratio_seq);
        }
    } else if (blocks) {
        launch_scan_sizes(a, s);
        hipLaunchKernelGGL(k_compact, dim3((uint32_t)blocks), dim3(256), 0,
                           s, a);
    }
    // the block index, behind every scan of the batch
    if (d_index_first)
        launch_block_index(ctx, a, d_index_first, d_index, index_entries);
    HIP_TRY(ctx, hipEventRecord(ctx->ev[3], s));
    HIP_TRY(ctx, hipGetLastError());
    ctx->timing_valid = true;
    ctx->timing_is_compress = true;
    ctx->last_kernel = route.last_kernel;
    ctx->dominant_split = route.tokens;
    ctx->codec_launches = blocks ? 1 : 0;
    return SNAPMI_OK;
}

int launch_decompress(snapmi_ctx *ctx, const void *const *d_in_ptrs,
                      const uint64_t *d_in_lens, void *const *d_out_ptrs,
                      const uint64_t *d_out_caps, uint64_t *d_out_lens,
                      snapmi_error *d_errs, const uint8_t *d_modes, size_t n,
                      const unsigned long long *d_gate,
                      unsigned long long gate_value, hipStream_t side,
                      DevBuf *side_order, bool wide_only)
{
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    DevBuf &order = side_order ? *side_order : ctx->order;
    DecompressArgs a;
    a.gate = d_gate;
    a.gate_value = gate_value;
    a.in_ptrs = d_in_ptrs;
    a.in_lens = d_in_lens;
    a.out_ptrs = d_out_ptrs;
    a.out_caps = d_out_caps;
    a.out_lens = d_out_lens;
    a.errs = d_errs;
    a.modes = d_modes;
    a.n_streams = (uint32_t)n;
    {
        // (+ 64 bucket counters of the many-workgroup sort behind the order,
        // + the number of streams that are not tiny)
        int rc = reserve(ctx, order, (n + 72) * sizeof(uint32_t));
        if (rc)
            return rc;
    }
    a.order = (uint32_t *)order.p;
    a.bucket_pos = a.order + n;
    a.prof = nullptr;
    PROF(
    {
        int rc = reserve(ctx, ctx->st_prof, 16 * sizeof(uint64_t));
        if (rc)
            return rc;
        HIP_TRY(ctx, hipMemsetAsync(ctx->st_prof.p, 0, 16 * sizeof(uint64_t),
                                    ctx->stream));
        a.prof = (unsigned long long *)ctx->st_prof.p;
    }
    )
    hipStream_t s = side ? side : ctx->stream;
    if (!side) {
        ctx->timing_valid = false;
        HIP_TRY(ctx, hipEventRecord(ctx->ev[0], s));
    }
    if (n > kPlanOneWg) {
        const uint32_t parts = (uint32_t)((n + 1023) / 1024);
        HIP_TRY(ctx, hipMemsetAsync(a.bucket_pos, 0, 64 * sizeof(uint32_t), s));
        hipLaunchKernelGGL(k_plan_decompress_a, dim3(parts), dim3(1024), 0, s,
                           a);
        hipLaunchKernelGGL(k_plan_decompress_b, dim3(1), dim3(64), 0, s, a);
        hipLaunchKernelGGL(k_plan_decompress_c, dim3(parts), dim3(1024), 0, s,
                           a);
    } else {
        hipLaunchKernelGGL(k_plan_decompress, dim3(1), dim3(1024), 0, s, a);
    }
    if (!side)
        HIP_TRY(ctx, hipEventRecord(ctx->ev[1], s));
    if (ctx->decode_kernel == 0)
        hipLaunchKernelGGL(k_decompress_sequential, dim3((uint32_t)n),
                           dim3(64), 0, s, a);
#ifdef SNAPMI_TESTING
    else if (ctx->decode_kernel == 2)
        hipLaunchKernelGGL(k_decompress_streams2, dim3((uint32_t)n), dim3(64),
                           0, s, a);
#endif
    else {
        if (n > ctx->decode_many_min)
            hipLaunchKernelGGL(
                k_decompress_streams3_many,
                dim3((uint32_t)((n + kManyStreams - 1) / kManyStreams)),
                dim3(64), 0, s, a);
        else
            hipLaunchKernelGGL(k_decompress_streams3, dim3((uint32_t)n),
                               dim3(64), 0, s, a);
        // the streams of fewer than 256 compressed bytes, one per lane (how
        // many there are only the device knows: workgroups without any leave
        // at once, in both launches)
        if (!wide_only)
            hipLaunchKernelGGL(k_decompress_tiny,
                               dim3((uint32_t)((n + 63) / 64)), dim3(64), 0, s,
                               a);
        // ... and those of under 512 bytes in and out, 32 per wavefront
        if (!wide_only)
            hipLaunchKernelGGL(k_decompress_small,
                               dim3((uint32_t)((n + 31) / 32)), dim3(64), 0, s,
                               a);
    }
    HIP_TRY(ctx, hipGetLastError());
    if (side)
        return SNAPMI_OK;
    HIP_TRY(ctx, hipEventRecord(ctx->ev[2], s));
    HIP_TRY(ctx, hipEventRecord(ctx->ev[3], s));
    ctx->timing_valid = true;
    ctx->timing_is_compress = false;
    ctx->last_kernel = ctx->decode_kernel == 0   ? "k_decompress_sequential"
                       : ctx->decode_kernel == 2 ? "k_decompress_streams2"
                                                 : "k_decompress_streams3";
    ctx->dominant_split = false;
    ctx->codec_launches = 1;
    return SNAPMI_OK;
}

} // namespace snapmi
