// snapmi - which kernels a compress batch runs (DESIGN 4.1's routing table):
// plain functions of the context's options and the batch (no HIP), so that
// tests/test_route_cpu.py can pin every row of it on the CPU.
// launch_compress (snapmi_launch.hip) computes a CompressRoute, reserves what
// it names and launches it; the functions read the context's own Options.
#pragma once
#include <cstdint>

#include "snapmi_options.hpp"
#include "snapmi_pool.hpp"

namespace snapmi {

// wavefronts per workgroup of the window kernel, of k_match_spans_8k and of
// k_match_both (all of it, and its lane wavefronts); streams under these
// lengths are k_compress_tiny's / k_compress_small's (snapmi_kernels.hpp and
// snapmi_tiny.hpp have the same numbers; a static_assert in snapmi_launch.hip
// ties them)
constexpr uint32_t kRouteCompressWaves = 5, kRouteSmallTableWaves = 10;
constexpr uint32_t kRouteBothWaves = 6, kRouteBothLaneWaves = 4;
constexpr uint32_t kRouteTinyCompress = 256, kRouteSmallCompress = 2048;

// what the route reads beside the context's options (snapmi_options.hpp says
// what each of those means): the two facts of the device
struct RouteDevice {
    bool lds_order_ok; // the LDS order self-check passed (snapmi_ctx.hpp)
    uint32_t num_cus;
};

// the wavefront-per-block kernels that match and encode in one pass
enum class WindowKernel : uint8_t {
    none,
    spans,     // k_compress_spans
    span_lds,  // k_compress_span_lds: one block per CU, input in LDS too
    blocks,    // k_compress_blocks (test build, span_kernel 0)
    block_lds, // k_compress_block_lds (test build, span_kernel 0)
};

// the token path's match finder over the blocks of more than 8 KiB (or all
// of them when k_match_spans_8k does not run)
enum class MatchKernel : uint8_t {
    none,   // k_match_spans_8k has every block
    spans,  // k_match_spans: a wavefront per block, table in LDS
    both,   // k_match_both: lane and window wavefronts on every CU
    blocks, // k_match_blocks (k_match_blocks_spec: see Segment)
};

struct CompressRoute {
    // the window kernel: its grid, whether it runs on the side stream beside
    // the token path (compress_mode 2) and whether SpanSched orders its
    // blocks
    WindowKernel window = WindowKernel::none;
    uint32_t window_grid = 0;
    bool window_beside = false;
    bool sched = false;
    // the token path: a match finder, k_encode_tokens, k_redo_spilled
    bool tokens = false;
    MatchKernel match = MatchKernel::none;
    // k_match_spans_8k's workgroups (0: not launched) and the blocks of
    // more than 8 KiB
    uint32_t small_grid = 0;
    uint64_t nb_big = 0;
    // the encoder writes every block at its final position; otherwise
    // scratch slots and k_compact
    bool direct = false;
    // k_post_ratio posts this batch's ratio for the next one's match finder
    bool post_ratio = false;
    uint64_t seg_blocks = 0; // blocks per token-path launch
    uint32_t lanes = 0;      // lane tables (0: no lane kernel)
    uint32_t stage_waves = 0; // staging arrays of window wavefronts, per CU
    // snapmi_last_kernel: k_compress_span_lds and k_compress_blocks* are
    // reported as k_compress_spans, k_match_blocks_spec as k_match_blocks
    const char *last_kernel = "k_compress_tiny";
};

// streams shorter than this are compressed by the lane-per-stream kernels
// (k_compress_tiny under 256 bytes, k_compress_small under 1 KiB - under
// 2 KiB with small_stream_kernel = 2) and get no blocks; 0: every stream goes
// through the block kernels
inline uint64_t small_stream_limit(const Options &o)
{
    if (!o.tiny_stream_kernel)
        return 0;
    return o.small_stream_kernel == 2
               ? kRouteSmallCompress
               : (o.small_stream_kernel ? kRouteSmallCompress / 2
                                        : kRouteTinyCompress);
}

inline uint64_t min_u64(uint64_t a, uint64_t b) { return a < b ? a : b; }

// workgroups of a window-kernel launch over `count` blocks on `cus` CUs
inline uint32_t window_grid(uint64_t count, uint64_t cus)
{
    return (uint32_t)min_u64(
        (count + kRouteCompressWaves - 1) / kRouteCompressWaves, cus);
}

inline uint32_t lane_count(const Options &o, const RouteDevice &d,
                           uint64_t seg_blocks, bool both_cores)
{
    // waves of the lane-per-block match finder: a few per CU saturate the
    // random-access rate of HBM; never more lanes than blocks
    uint64_t waves = (uint64_t)d.num_cus * o.lane_waves_per_cu;
    const uint64_t need = (seg_blocks + 63) / 64;
    if (waves > need)
        waves = need ? need : 1;
    if (o.lane_max_waves && waves > o.lane_max_waves)
        waves = o.lane_max_waves;
    // k_match_both: its lane wavefronts on every CU, beside two of the
    // window kernel
    if (both_cores)
        waves = (uint64_t)d.num_cus * kRouteBothLaneWaves;
    return (uint32_t)waves * 64;
}

// spans_hint: the context's last batch compressed to no less than
// match_spans_ratio_pct of its input (read by the caller; only
// match_kernel 2 follows it)
inline CompressRoute compress_route(const Options &o, const RouteDevice &d,
                                    uint64_t blocks, uint64_t cnt8,
                                    bool spans_hint)
{
    CompressRoute r;
    r.seg_blocks = segment_blocks(blocks, o.lane_segment_blocks);
    if (!blocks)
        return r;
    // Small batches are latency-bound: the wavefront kernel finishes a block
    // in ~2 ms, a lane needs tens of ms.  Large batches are throughput-bound
    // and go to the lane-per-block kernel.
    // Blocks of at most 8 KiB (cnt8 of them: the caller counted one-block
    // streams and tails): a window kernel with the table the reference gives
    // such blocks, ten per CU instead of five (k_match_spans_8k), whatever
    // the size of the batch - every probe of the lane kernel into a block's
    // fresh table is an HBM transaction, and the 64 KiB window kernel keeps a
    // CU's issue slots four fifths idle.  (Twenty tables of 8 KiB per CU for
    // blocks of at most 4 KiB were built too and measured the same: at ten
    // wavefronts the CU's one scalar unit is 70 % busy.)
    const uint64_t nb_small = min_u64(cnt8, blocks);
    const bool small = d.lds_order_ok && o.compress_mode == 1 &&
                       o.small_table_kernel &&
                       nb_small >= o.small_table_min_blocks;
    r.nb_big = small ? blocks - nb_small : blocks;
    const bool big = r.nb_big >= o.lane_min_blocks;
    // The token path: a device that failed the LDS order self-check only has
    // the lane kernel; the small-block kernel runs on it too, with the
    // window kernel as the match finder of a batch that is not big.
    r.tokens = !d.lds_order_ok || (o.compress_mode != 0 && big) || small;
    // (segment_blocks: equal launches that bound the token scratch; "both at
    // once" needs the whole list in one segment)
    const bool window =
        d.lds_order_ok &&
        (!r.tokens || o.compress_mode == 0 ||
         (o.compress_mode == 2 && r.seg_blocks == blocks));
    if (window) {
        r.window_beside = r.tokens;
        // persistent: one 5-wave workgroup per CU (all of its LDS), each
        // wavefront pulls blocks from the back of the ticket
        // the smallest batches (no more than two blocks per CU: scalar
        // calls, short frames) run one block per CU with the input block
        // in LDS too - half the time per block, a fifth of the blocks in
        // flight; five tables per CU from there
        const bool lds_input =
            o.small_batch_kernel == 2 ||
            (o.small_batch_kernel == 1 && blocks <= 2 * (uint64_t)d.num_cus);
        if (lds_input) {
            r.window = o.span_kernel ? WindowKernel::span_lds
                                     : WindowKernel::block_lds;
            r.window_grid = (uint32_t)min_u64(blocks, d.num_cus);
        } else {
            r.window = o.span_kernel ? WindowKernel::spans
                                     : WindowKernel::blocks;
            // (beside the lane kernel it takes a share of the CUs only: a
            // persistent workgroup owns its CU's whole LDS)
            r.window_grid = window_grid(
                blocks, r.window_beside ? (o.both_wave_cus ? o.both_wave_cus
                                                           : d.num_cus / 2)
                                        : d.num_cus);
            // several blocks per wavefront, the window kernel alone: the
            // order of the blocks is chosen as the launch goes (SpanSched,
            // snapmi_window.hip: heavy streams first, light ones last - a
            // launch ends with its small jobs)
            r.sched = !r.window_beside && o.span_kernel &&
                      (o.span_schedule == 2 ||
                       (o.span_schedule == 1 &&
                        blocks > (uint64_t)r.window_grid * kRouteCompressWaves));
        }
    }
    if (!r.tokens) {
        r.last_kernel = "k_compress_spans";
        return r;
    }
    // The lane kernel knows every block's encoded size before a byte of it
    // is written, so its encoder puts the blocks where they belong; only the
    // wavefront kernel (which encodes while it matches) and the overlap
    // split need a scratch slot per block and the k_compact pass.
    r.direct = !window && o.lane_overlap_encode == 0;
    r.post_ratio =
        r.direct && o.match_kernel == 2 && blocks >= 2 * o.lane_min_blocks;
    // The token path's match finder: the lane kernel, or - option
    // match_kernel - the window kernel (k_match_spans: table in LDS, no
    // tables in HBM).  By default the context's last batch decides: data that
    // does not compress costs a lane three HBM transactions per probe for
    // nothing (cfg5: 12 ms of lane kernel for 32 GiB against ~4 of windows).
    const bool span_match =
        !window && d.lds_order_ok &&
        (o.match_kernel == 1 || (small && !big) ||
         (o.match_kernel == 2 && spans_hint));
    // both match finders on every CU (k_match_both): launches that fill the
    // chip with lanes anyway
    const bool both_cores = !window && !span_match && d.lds_order_ok &&
                            o.lane_coresident &&
                            r.nb_big >= o.lane_coresident_min_blocks;
    if (span_match)
        r.match = small && r.nb_big == 0 ? MatchKernel::none
                                         : MatchKernel::spans;
    else
        r.match = both_cores ? MatchKernel::both : MatchKernel::blocks;
    if (!span_match)
        r.lanes = lane_count(o, d, r.seg_blocks, both_cores);
    if (small) // one 640-thread workgroup per CU: ten 16 KiB tables
        r.small_grid = (uint32_t)min_u64(
            (nb_small + kRouteSmallTableWaves - 1) / kRouteSmallTableWaves,
            d.num_cus);
    // the window wavefronts' staging arrays (TokenWriter): one per wavefront
    // of the largest workgroup this call launches
    r.stage_waves = small ? kRouteSmallTableWaves
                    : both_cores ? kRouteBothWaves - kRouteBothLaneWaves
                    : span_match ? kRouteCompressWaves
                                 : 0;
    r.last_kernel = !span_match ? (both_cores ? "k_match_both"
                                              : "k_match_blocks")
                    : r.match == MatchKernel::none ? "k_match_spans_8k"
                                                   : "k_match_spans";
    return r;
}

// workgroups of a match launch over `count` blocks of a segment (with the
// small-block kernel on, the window kernel's share is the blocks of more
// than 8 KiB: the whole batch's, whatever the segment)
inline uint32_t match_grid(const RouteDevice &d, const CompressRoute &r,
                           uint64_t count)
{
    switch (r.match) {
    case MatchKernel::spans:
        return window_grid(r.small_grid ? min_u64(r.nb_big, count) : count,
                           d.num_cus);
    case MatchKernel::both:
        return d.num_cus;
    case MatchKernel::blocks:
        return r.lanes / 64;
    default:
        return 0;
    }
}

// a token-path launch over the blocks [lo, hi)
struct Segment {
    // Option lane_overlap_encode (off by default): the segment is matched in
    // two halves, [lo, mid) and [mid, hi), and the first half's tokens are
    // encoded on the side stream while the second half is matched.  Two
    // halves alone cost the match finder nothing (114.2 vs 115 ms), but the
    // encoder's streaming traffic under it does: 121.6 -> 135 ms at cfg2.
    // Kept as a measured dead end that the encoder tests still run through.
    // mid == hi: one match launch.
    uint64_t mid;
    // A launch of few blocks waits for the latency of its rounds with the
    // memory system idle: the kernel that also fetches the next probe's
    // entry (k_match_blocks_spec) takes 10-15 % off 2 048 .. 16 384 blocks
    // of text.  From 32 768 blocks on the launch is at the random-access
    // rate of HBM even with one block per lane (1.6e10 rounds a second, as
    // at 146 700 blocks) and the extra reads buy nothing
    // (profiles/r3_lane_speculation.txt).
    bool spec;
    uint32_t redo_grid; // k_redo_spilled's workgroups
};

inline Segment segment(const Options &o, const RouteDevice &d,
                       const CompressRoute &r, uint64_t lo, uint64_t hi)
{
    Segment g;
    const uint64_t n = hi - lo;
    const bool split =
        r.window == WindowKernel::none && !r.small_grid &&
        (o.lane_overlap_encode == 2
             ? n >= 2
             : (o.lane_overlap_encode == 1 &&
                n * 10 >= (uint64_t)r.lanes * 14));
    g.mid = split ? lo + n / 2 : hi;
    g.spec = o.lane_speculate && n <= r.lanes &&
             n <= o.lane_speculate_max_blocks;
    g.redo_grid = window_grid(n, d.num_cus);
    return g;
}

// snapmi_ctx_prepare: the lane tables a batch of `blocks` blocks is given
// ahead of its first compress call (0: none).  This is its own rule, not the
// launch's: it knows neither the hint nor cnt8, and it answers with lanes
// where the launch runs none (match_kernel 1; a hint that picks
// k_match_spans) or the reverse (compress_mode 0 on a device that failed the
// LDS order self-check).
inline uint32_t prepare_lanes(const Options &o, const RouteDevice &d,
                              uint64_t blocks)
{
    if (o.compress_mode == 0 || blocks < o.lane_min_blocks)
        return 0;
    const bool both = o.compress_mode == 1 && d.lds_order_ok &&
                      o.lane_coresident &&
                      blocks >= o.lane_coresident_min_blocks;
    return lane_count(o, d, segment_blocks(blocks, o.lane_segment_blocks),
                      both);
}

} // namespace snapmi
