// snapmi_window.hip -- the kernels of the window match finder
// (snapmi_window.hpp): k_compress_spans and k_compress_span_lds match and
// encode (blocks in ticket order or in SpanSched's), k_match_spans and
// k_match_spans_8k are match finders of the token path, k_redo_spilled takes
// the blocks whose tokens found no page once more; and k_probe_lds_order, the
// self-check of every context for what these kernels rest on.
#include "snapmi_window.hpp"

namespace snapmi {

// ---------------------------------------------------------------------
// Self-check run once per context (snapmi_ctx_create): the window kernels
// need one wave64 ds_mskor_rtn_b32 to apply lanes that hit the same address
// in ascending lane order - every lane must get back the value left by the
// nearest lower lane with the same slot, and the highest lane's value must
// be the one that stays.  256 patterns (all lanes one slot, heavy, some and
// rare duplicates), slots from a counter-based hash.  *bad != 0 afterwards
// means the property does not hold on this device: the context then never
// uses a window kernel (the lane kernel does not depend on it).
// ---------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_probe_lds_order(uint32_t *bad)
{
    __shared__ uint16_t tab[2048];
    const uint32_t lane = threadIdx.x;
    const uint32_t tbase = (uint32_t)(uintptr_t)(lptr16)&tab[0];
    uint32_t fails = 0;
    for (uint32_t t = 0; t < 256; t++) {
        for (uint32_t i = lane; i < 2048; i += 64)
            tab[i] = (uint16_t)(0x8000u + i);
        __builtin_amdgcn_wave_barrier(); // one wave: its LDS ops are in order
        uint32_t r = (t * 64 + lane + 131u * blockIdx.x) * 2654435761u +
                     0x9E3779B9u;
        r ^= r >> 15;
        r *= 0x2C1B3C6Du;
        r ^= r >> 12;
        const uint32_t mode = t & 3;
        const uint32_t slot =
            mode == 0 ? 5u : (mode == 1 ? r % 8 : (mode == 2 ? r % 64 : r % 2048));
        const uint32_t sh = (slot & 1) * 16;
        const uint32_t old = lds_mskor_rtn(tbase + (slot >> 1) * 4,
                                           0xFFFFu << sh, (lane + 1) << sh);
        __builtin_amdgcn_wave_barrier();
        const uint32_t fin = tab[slot];
        uint32_t want = 0x8000u + slot, want_fin = 0;
#pragma unroll
        for (uint32_t j = 0; j < 64; j++) {
            const uint32_t sj = rdlane(slot, j);
            if (sj == slot) {
                if (j < lane)
                    want = j + 1;
                want_fin = j + 1;
            }
        }
        fails += ((old >> sh) & 0xFFFFu) != want;
        fails += fin != want_fin;
        __builtin_amdgcn_wave_barrier();
    }
    if (__ballot(fails != 0) != 0 && lane == 0)
        atomicOr(bad, 1u);
    // Second property (k_decompress_streams2): overlapping lanes of ONE plain
    // DS store are applied in ascending lane order too, so a lane may store a
    // whole 16 bytes for a shorter element and the lanes above it repair the
    // excess.  64 layouts: lane strides 1..23 and pseudo-random gaps, every
    // alignment.  bit 1 of *bad.
    {
        typedef __attribute__((address_space(3))) uint8_t l_u8;
        l_u8 *m = (l_u8 *)tab; // 4 KiB
        uint32_t sfail = 0;
        for (uint32_t t = 0; t < 64; t++) {
            const uint32_t gap =
                t < 23 ? t + 1
                       : 1 + ((lane * 2654435761u + t * 40503u) >> 7) % 20;
            uint32_t pos = wave_inclusive_scan(gap) + 3 * t;
            const uint32_t nextpos = (uint32_t)__builtin_amdgcn_ds_bpermute(
                (int)(((lane + 1) & 63) << 2), (int)pos);
            u32x4 x;
            x.x = x.y = x.z = x.w = 0x01010101u * (lane + 1);
            __builtin_amdgcn_wave_barrier();
            __builtin_memcpy(m + pos, &x, 16);
            __builtin_amdgcn_wave_barrier();
            for (uint32_t k = 0; k < 16; k++) {
                const uint32_t b = pos + k;
                if ((lane == 63 || b < nextpos) &&
                    m[b] != (uint8_t)(lane + 1))
                    sfail++;
            }
            __builtin_amdgcn_wave_barrier();
        }
        // ... and the decoders' multi-piece form: elements of 1..64 bytes,
        // whole 16-byte pieces, last piece first (four store instructions);
        // every byte must end up with the element that owns it.  The launch
        // fills the chip (32 waves per CU, each with LDS of its own), so the
        // property is checked under the LDS contention of the real kernels,
        // not by one idle wave.
        for (uint32_t t = 0; t < 48; t++) {
            uint32_t r = (t * 64 + lane + 977u * blockIdx.x) * 2654435761u;
            r ^= r >> 13;
            // mostly short elements, some of every length up to 64; the last
            // lanes short enough that 64 elements fit in the 4 KiB
            uint32_t len = (t & 1) ? 1 + (r >> 8) % 64 : 1 + (r >> 8) % 20;
            if (t >= 40)
                len = 17 + (r >> 8) % 48;
            const uint32_t end = wave_inclusive_scan(len) + t;
            const uint32_t pos = end - len;
            __builtin_amdgcn_wave_barrier();
            for (uint32_t c = 48;; c -= 16) {
                if (c < len && pos + c + 16 <= 4096) {
                    u32x4 x;
                    x.x = x.y = x.z = x.w = 0x01010101u * (lane + 1);
                    __builtin_memcpy(m + pos + c, &x, 16);
                }
                if (c == 0)
                    break;
            }
            __builtin_amdgcn_wave_barrier();
            for (uint32_t k = 0; k < len; k++)
                if (pos + k < 4096 - 16 && m[pos + k] != (uint8_t)(lane + 1))
                    sfail++;
            __builtin_amdgcn_wave_barrier();
        }
        if (__ballot(sfail != 0) != 0 && lane == 0)
            atomicOr(bad, 2u);
    }
}

// The window kernel as the match finder of the token path (k_scan_sizes +
// k_encode_tokens behind it, every block at its final position): what
// launch_compress runs instead of k_match_blocks where the lane kernel's
// tables buy nothing - batches that do not compress (every probe of a lane is
// an HBM transaction, here it is an LDS access: cfg5), and whenever the
// option says so.  Blocks [blk_lo, blk_hi) from the front of the ticket.
__global__ __launch_bounds__(kCompressWaves * 64) void k_match_spans(
    CompressArgs a)
{
    __shared__ __attribute__((aligned(16)))
    uint16_t tables[kCompressWaves][kMaxTable];
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t wave = uni(threadIdx.x >> 6);
    const lptr16 table = (lptr16)&tables[wave][0];
    const uint32_t tbase = (uint32_t)(uintptr_t)table;
    const uint32_t nblocks = segment_blocks(a);
    // (the ticket through a helper that is not inlined: DESIGN section 5)
    uint32_t b = a.blk_lo + uni(next_front_ticket(a.ticket, lane));
    while (b < nblocks) {
        compress_one_block_span<false, true>(a, b, lane, table, tbase);
        b = a.blk_lo + uni(next_front_ticket(a.ticket, lane));
    }
}

// k_match_spans for blocks of at most 8 KiB: a table of 8 192 u16 is all the
// reference gives such a block (src/compress.rs:491-518), so ten wavefronts
// fit a CU where the 64 KiB kernel has room for five, and the window kernel
// is bound by the instructions and latencies of ONE wavefront per SIMD.  Only
// blocks of the launch's class (CompressArgs::cls_lo / cls_hi) are taken.
// 4 KiB of alice29.txt per stream, 1 GiB: 38 -> 70 GiB/s.  (Twenty wavefronts
// with 8 KiB tables for blocks of at most 4 KiB measured no better: from ten
// on the CU's one scalar unit is the limit, profiles/r5_small_blocks.txt.)
__global__ __launch_bounds__(kSmallTableWaves * 64) void k_match_spans_8k(
    CompressArgs a)
{
    constexpr uint32_t kEntries = 8192;
    __shared__ __attribute__((aligned(16)))
    uint16_t tables[kSmallTableWaves][kEntries];
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t wave = uni(threadIdx.x >> 6);
    const lptr16 table = (lptr16)&tables[wave][0];
    const uint32_t tbase = (uint32_t)(uintptr_t)table;
    const uint32_t nblocks = segment_blocks(a);
    uint32_t b = a.blk_lo + uni(next_front_ticket(a.ticket, lane));
    while (b < nblocks) {
        compress_one_block_span<false, true>(a, b, lane, table, tbase,
                                             nullptr, kEntries);
        b = a.blk_lo + uni(next_front_ticket(a.ticket, lane));
    }
}

// ---------------------------------------------------------------------
// The order of a window-kernel launch (round 6).  A block is one wavefront's
// from start to end, blocks differ in cost by what they hold (kppkn.gtb:
// 1 884 window steps a block, HTML 740, a PDF 100), and a launch of a few
// blocks per wavefront in ticket order ends when its last-started heavy block
// does: 256 MiB of the corpus round took 7.9 ms where the work divided by the
// wavefronts is 5 (list scheduling: makespan <= mean + the heaviest job).
// Longest-first needs the costs, and the only cheap predictor of a block's
// cost is a block of the same stream.  So: pass 1 = the FIRST block of every
// stream; whoever finishes a block posts its cycles per KiB for its stream.
// Pass 2 = the other blocks in stream order - but a wavefront that draws a
// block of a stream known to be light or middling (under 0.7 / 1.3 of the
// launch's running mean) puts it on a list instead and draws again: the heavy
// and the unknown run first, the middle list next, the light list last, and
// the launch ends with small jobs.  Every block is run exactly once; results
// do not depend on the order (blocks are independent:
// src/compress.rs:148,514-516).
//   sched[0] ticket  [1] blocks classified in pass 2  [2] blocks costed
//   [3] (unused)  [4..5] u64 sum of costs  [6] pushed M  [7] popped M
//   [8] pushed L  [9] popped L            then: cost[n_streams],
//   listM[slots], listL[slots] (kSchedEmpty = not written yet)
// ---------------------------------------------------------------------
namespace {
constexpr uint32_t kSchedEmpty = 0xFFFFFFFFu, kSchedHead = 16;
struct SpanSched {
    uint32_t *w;
    uint32_t n_streams, slots, nblocks;
    __device__ __forceinline__ uint32_t *cost() const { return w + kSchedHead; }
    __device__ __forceinline__ uint32_t *list(int which) const
    {
        return w + kSchedHead + n_streams + (which ? slots : 0);
    }
    // the stream of pass-2 entry j: slot_first[st] <= j < slot_first[st + 1]
    __device__ __forceinline__ uint32_t stream_of_slot(
        const uint32_t *slot_first, uint32_t j) const
    {
        uint32_t lo = 0, hi = n_streams;
        while (hi - lo > 1) {
            const uint32_t mid = (lo + hi) >> 1;
            if (slot_first[mid] <= j)
                lo = mid;
            else
                hi = mid;
        }
        return lo;
    }
    // lane 0: the next block to run, or kSchedEmpty when the launch is over
    // (out of line, like next_ticket: an inlined ticket loop under `if (lane
    // == 0)` inside a persistent loop once compiled into a hang)
    __device__ __forceinline__ uint32_t next(const uint32_t *blk_first,
                                             const uint32_t *slot_first)
    {
        for (;;) {
            const uint32_t t = atomicAdd(&w[0], 1u);
            if (t >= n_streams + slots)
                break;
            if (t < n_streams) { // pass 1: the stream's first block
                const uint32_t b = blk_first[t];
                if (blk_first[t + 1] > b && b < nblocks)
                    return b;
                continue; // a stream without blocks
            }
            const uint32_t j = t - n_streams;
            const uint32_t st = stream_of_slot(slot_first, j);
            const uint32_t b = blk_first[st] + (j - slot_first[st]) + 1;
            uint32_t cls = 0; // 0 run now, 1 middle list, 2 light list
            if (b < nblocks) {
                const uint32_t c = __hip_atomic_load(
                    &cost()[st], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                const uint32_t done = __hip_atomic_load(
                    &w[2], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (c && done >= 64) {
                    const unsigned long long sum = __hip_atomic_load(
                        (unsigned long long *)&w[4], __ATOMIC_RELAXED,
                        __HIP_MEMORY_SCOPE_AGENT);
                    const unsigned long long mean = sum / done;
                    cls = 10ull * c < 7ull * mean    ? 2
                          : 10ull * c < 13ull * mean ? 1
                                                     : 0;
                }
                if (cls) {
                    const uint32_t i = atomicAdd(&w[cls == 1 ? 6 : 8], 1u);
                    __hip_atomic_store(&list(cls - 1)[i], b, __ATOMIC_RELEASE,
                                       __HIP_MEMORY_SCOPE_AGENT);
                }
            }
            __threadfence();
            atomicAdd(&w[1], 1u); // this entry is classified
            if (b < nblocks && cls == 0)
                return b;
        }
        // the lists: middle first, then light; an entry may still be on its
        // way while pass 2 is being classified by others
        for (int which = 0; which < 2; which++) {
            for (;;) {
                const uint32_t i = atomicAdd(&w[which ? 9 : 7], 1u);
                if (i >= slots)
                    break;
                uint32_t b;
                for (;;) {
                    b = __hip_atomic_load(&list(which)[i], __ATOMIC_ACQUIRE,
                                          __HIP_MEMORY_SCOPE_AGENT);
                    if (b != kSchedEmpty)
                        break;
                    const uint32_t cl = __hip_atomic_load(
                        &w[1], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT);
                    if (cl >= slots &&
                        i >= __hip_atomic_load(&w[which ? 8 : 6],
                                               __ATOMIC_ACQUIRE,
                                               __HIP_MEMORY_SCOPE_AGENT))
                        break; // all of pass 2 is classified: none will come
                    __builtin_amdgcn_s_sleep(8);
                }
                if (b == kSchedEmpty)
                    break;
                return b;
            }
        }
        return kSchedEmpty;
    }
    // lane 0, behind a block of n bytes of stream st that took `cycles`
    __device__ __forceinline__ void post(uint32_t st, uint32_t n,
                                         unsigned long long cycles)
    {
        unsigned long long c = (cycles << 10) / (n ? n : 1);
        if (c > 0x7FFFFFFFull)
            c = 0x7FFFFFFFull;
        if (c == 0)
            c = 1;
        __hip_atomic_store(&cost()[st], (uint32_t)c, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
        atomicAdd((unsigned long long *)&w[4], c);
        atomicAdd(&w[2], 1u);
    }
};
} // namespace

// (the whole wavefront calls, lane 0 draws - the shape of next_ticket, which
// is known to compile into what it says inside a persistent loop; the two
// arrays it reads, not the kernel's argument block: a reference to that makes
// the kernel keep a copy of it in scratch memory)
__device__ __noinline__ uint32_t span_sched_next(SpanSched sc,
                                                 const uint32_t *blk_first,
                                                 const uint32_t *slot_first,
                                                 uint32_t lane)
{
    uint32_t b = 0;
    if (lane == 0)
        b = sc.next(blk_first, slot_first);
    return uni(b);
}

__global__ __launch_bounds__(kCompressWaves * 64) void k_compress_spans(
    CompressArgs a)
{
    __shared__ __attribute__((aligned(16)))
    uint16_t tables[kCompressWaves][kMaxTable];
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t wave = uni(threadIdx.x >> 6);
    const lptr16 table = (lptr16)&tables[wave][0];
    const uint32_t tbase = (uint32_t)(uintptr_t)table;
    const uint32_t nblocks = launch_blocks(a);
    if (a.sched) { // the order chosen as the launch goes (SpanSched)
        SpanSched sc;
        sc.w = a.sched;
        sc.n_streams = a.n_streams;
        sc.slots = a.slot_first[a.n_streams] < a.host_slots
                       ? a.slot_first[a.n_streams]
                       : a.host_slots;
        sc.nblocks = nblocks;
        for (;;) {
            const uint32_t b = uni(
                span_sched_next(sc, a.blk_first, a.slot_first, lane));
            if (b == kSchedEmpty)
                break;
            const unsigned long long t0 = __builtin_readcyclecounter();
            compress_one_block_span<false>(a, b, lane, table, tbase);
            if (lane == 0) {
                // (the block's stream and length once more: a few loads and
                // a short search per block of ~4 M cycles)
                const BlockAt at = locate_block(a, b);
                sc.post(at.st, at.n, __builtin_readcyclecounter() - t0);
            }
        }
        return;
    }
    uint32_t b = uni(next_ticket(a.ticket, lane, nblocks));
    while (b != 0xFFFFFFFFu) {
        if (lane == 0 && a.ntok)
            a.ntok[b] = 0xFFFFFFFFu; // encoded here, not by k_encode_tokens
        compress_one_block_span<false>(a, b, lane, table, tbase);
        b = uni(next_ticket(a.ticket, lane, nblocks));
    }
}

// The blocks of a token-path launch whose tokens found no page in the pool
// (CompressArgs::tok_pool), once more: the window kernel compresses them to
// where k_encode_tokens would have put them (its destination rules, with
// a.direct the final position - k_scan_sizes has run).  Launched behind every
// k_encode_tokens; a launch without spilled blocks costs its wavefronts one
// load.  h_stat (pinned host memory, may be null): what the next batch sizes
// its pool by - pages asked for, blocks spilled, blocks of the launch, seq.
__global__ __launch_bounds__(kCompressWaves * 64) void k_redo_spilled(
    CompressArgs a, uint32_t *h_stat, uint32_t seq)
{
    __shared__ __attribute__((aligned(16)))
    uint16_t tables[kCompressWaves][kMaxTable];
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t wave = uni(threadIdx.x >> 6);
    const lptr16 table = (lptr16)&tables[wave][0];
    const uint32_t tbase = (uint32_t)(uintptr_t)table;
    uint32_t count = a.tok_ctl[1];
    if (count > a.blk_hi - a.blk_lo)
        count = a.blk_hi - a.blk_lo;
    if (h_stat && blockIdx.x == 0 && threadIdx.x == 0) {
        h_stat[0] = a.tok_ctl[0];
        h_stat[1] = count;
        h_stat[2] = a.blk_hi - a.blk_lo;
        __threadfence_system();
        h_stat[3] = seq;
    }
    if (count == 0)
        return;
    uint32_t i = uni(next_ticket(a.tok_ctl + 2, lane, count));
    while (i != 0xFFFFFFFFu) {
        const uint32_t b = uni(a.tok_ctl[kTokCtlList + i]);
        compress_one_block_span<false>(a, b, lane, table, tbase);
        i = uni(next_ticket(a.tok_ctl + 2, lane, count));
    }
}

// one block per CU, table and input block in LDS (the smallest batches)
__global__ __launch_bounds__(64) void k_compress_span_lds(CompressArgs a)
{
    __shared__ __attribute__((aligned(16))) uint16_t table_mem[kMaxTable];
    __shared__ __attribute__((aligned(16))) uint8_t block_mem[kMaxBlock + 32];
    const uint32_t lane = threadIdx.x;
    const lptr16 table = (lptr16)&table_mem[0];
    const uint32_t tbase = (uint32_t)(uintptr_t)table;
    const uint32_t nblocks = launch_blocks(a);
    uint32_t b = uni(next_ticket(a.ticket, lane, nblocks));
    while (b != 0xFFFFFFFFu) {
        if (lane == 0 && a.ntok)
            a.ntok[b] = 0xFFFFFFFFu;
        compress_one_block_span<true>(
            a, b, lane, table, tbase,
            (__attribute__((address_space(3))) uint8_t *)block_mem);
        b = uni(next_ticket(a.ticket, lane, nblocks));
    }
}

} // namespace snapmi
