// snapmi_longstream.hip -- long raw streams decoded in pieces, kernels and
// host side: k_long_plan and the k_bstream_* kernels (planned by
// snapmi_streamplan.hpp, which also holds what they are handed), then what
// launches them: the long streams of a small batch, snapmi_decompress_batch,
// and a lone stream as a batch of one.
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

using namespace snapmi;

namespace snapmi {

// ---------------------------------------------------------------------
// One long raw stream on many wavefronts (snapmi_decompress_stream, and the
// long streams of a small batch).
//
// A raw stream has no index and its elements form a chain, but where the
// chain goes is cheap to tabulate: a lane that starts at byte o of a 4 KiB
// segment and hops from element to element leaves the segment at some
// position, having produced some number of bytes.  Chains from neighbouring
// offsets merge within a few elements, so the 64 lanes of a wave mostly read
// the same bytes.  Segments -> super-segments (64 segments) -> one short
// sequential pass over the super-segments -> the exact (src, dst) positions
// of the element boundaries at every 64 KiB of output -> those pieces are
// decoded by k_decompress_streams3 like independent streams.  Anything
// irregular (an element the scan cannot follow, a piece that fails one of
// the reference's checks - which includes a copy reaching back into another
// piece) sets meta[2] and the whole stream is decoded by the sequential
// path instead, which also produces the reference's exact error.
// ---------------------------------------------------------------------
namespace {
constexpr unsigned long long kNone = ~0ull;
// k_bstream_scan follows a chain at most this many elements behind its
// segment's end.  Compressible data lands on a tabulated offset (within
// kEntry = 8 bytes of a 4 KiB boundary) at the next boundary unless an
// element of 9+ encoded bytes jumps over it, which costs a segment of small
// elements (~1 300 hops of 3 bytes) until the next chance; incompressible
// data (64 KiB literals) lands with probability 1/512 per element.  8 192
// hops cover several misses in a row and all but (511/512)^8192 = 1e-7 of
// the literal walks, and bound what a crafted stream can cost to 16 hops
// per input byte (it was quadratic in the input length without a bound).
constexpr uint32_t kScanOverrun = 8192;

typedef unsigned long long su64x2 __attribute__((ext_vector_type(2)));

// level 1 = segments (4 KiB; 1 KiB for short streams: StreamArgs::seg_log2),
// 2 = 64 of them, 3 = 64 of those
static_assert(kSegPerSuper == 64, "level_bytes shifts by 6 per level");
template <int L>
__device__ __forceinline__ uint64_t level_bytes(const StreamArgs &a)
{
    return 1ull << (a.seg_log2 + 6 * (L - 1));
}
template <int L>
__device__ __forceinline__ su64x2 *level_table(const StreamArgs &a)
{
    return (su64x2 *)(L == 1 ? a.s1 : (L == 2 ? a.s2 : a.s3));
}
template <int L>
__device__ __forceinline__ su64x2 *level_entry(const StreamArgs &a)
{
    return (su64x2 *)(L == 1 ? a.e1 : (L == 2 ? a.e2 : a.e3));
}

// Follow the chain from p to the end of the level-L block that contains p
// (or of the stream).  Tables: level 1 [segment][o]: enter the segment at
// offset o < kEntry; levels 2, 3 [block][child][o]: enter the block at offset
// o < kEntry of its child (a block of the level below).  A position deeper than
// kEntry bytes inside a child - the chain landed there after a long element - is
// first taken to that child's end one level down.
template <int L>
__device__ __forceinline__ bool reach_end(const StreamArgs &a, uint64_t &p,
                                          uint64_t &out);
template <>
__device__ __forceinline__ bool reach_end<1>(const StreamArgs &a, uint64_t &p,
                                             uint64_t &out)
{
    const uint64_t seg = p >> a.seg_log2;
    const uint64_t o = p - (seg << a.seg_log2);
    if (o < kEntry) {
        const su64x2 e = level_table<1>(a)[seg * kEntry + o];
        if (e.x == kNone)
            return false;
        p = e.x;
        out += e.y;
        return true;
    }
    uint64_t end = (seg + 1) << a.seg_log2;
    if (end > a.in_len)
        end = a.in_len;
    while (p < end)
        if (!elem_step(bytes_at((gcptr)a.in), a.in_len, p, out))
            return false;
    return true;
}
template <int L>
__device__ __forceinline__ bool reach_end(const StreamArgs &a, uint64_t &p,
                                          uint64_t &out)
{
    const uint64_t B = level_bytes<L>(a), Bc = level_bytes<L - 1>(a);
    const uint64_t blk = p / B;
    uint64_t end = (blk + 1) * B;
    if (end > a.in_len)
        end = a.in_len;
    while (p < end) {
        const uint64_t rel = p - blk * B;
        const uint64_t c = rel / Bc, o = rel - c * Bc;
        if (o < kEntry) {
            const su64x2 e =
                level_table<L>(a)[(blk * kSegPerSuper + c) * kEntry + o];
            if (e.x == kNone)
                return false;
            p = e.x;
            out += e.y;
            return true;
        }
        if (!reach_end<L - 1>(a, p, out))
            return false;
    }
    return true;
}

// table of one level-L block (L = 2, 3), children right to left: entering at
// child c continues, after that child, with an entry already tabulated
template <int L>
__device__ __forceinline__ void build_level(const StreamArgs &a, uint32_t wg)
{
    __shared__ su64x2 tab[kSegPerSuper * kEntry]; // 16 KiB
    if (a.meta[2])
        return;
    const uint64_t B = level_bytes<L>(a), Bc = level_bytes<L - 1>(a);
    const uint64_t blk = wg;
    uint64_t end = (blk + 1) * B;
    if (end > a.in_len)
        end = a.in_len;
    for (int c = kSegPerSuper - 1; c >= 0; c--) {
        uint64_t p = blk * B + (uint64_t)c * Bc + threadIdx.x, out = 0;
        bool ok = p < a.in_len && reach_end<L - 1>(a, p, out);
        while (ok && p < end) {
            const uint64_t rel = p - blk * B;
            const uint64_t c2 = rel / Bc, o2 = rel - c2 * Bc;
            if (o2 < kEntry) {
                const su64x2 e = tab[c2 * kEntry + o2]; // c2 > c: done before
                ok = e.x != kNone;
                p = e.x;
                out += e.y;
                break;
            }
            ok = reach_end<L - 1>(a, p, out);
        }
        tab[c * kEntry + threadIdx.x] = (su64x2){ok ? p : kNone, out};
        __syncthreads();
    }
    su64x2 *dst = level_table<L>(a) + blk * kSegPerSuper * kEntry;
    for (uint32_t i = threadIdx.x; i < kSegPerSuper * kEntry; i += kEntry)
        dst[i] = tab[i];
}

// entries of level L-1 from the entries of level L: one lane per block of
// level L walks its children
template <int L>
__device__ __forceinline__ void spread_level(const StreamArgs &a, uint32_t wg)
{
    if (a.meta[2])
        return;
    const uint64_t blk = (uint64_t)wg * blockDim.x + threadIdx.x;
    const uint64_t B = level_bytes<L>(a), Bc = level_bytes<L - 1>(a);
    if (blk * B >= a.in_len)
        return;
    const su64x2 e = level_entry<L>(a)[blk];
    if (e.x == kNone)
        return; // a long element spans this block
    uint64_t p = e.x, out = e.y;
    uint64_t end = (blk + 1) * B;
    if (end > a.in_len)
        end = a.in_len;
    while (p < end) {
        level_entry<L - 1>(a)[p / Bc] = (su64x2){p, out};
        if (!reach_end<L - 1>(a, p, out)) {
            a.meta[2] = 1;
            return;
        }
    }
}
} // namespace

__device__ __forceinline__ void stream_head(const StreamArgs &a, const uint32_t wg)
{
    // header checks of Decoder::decompress (src/decompress.rs:75-95); any
    // failure is left to the sequential decoder, which reports it
    uint32_t hdr = 0;
    uint64_t dlen = 0;
    a.meta[0] = 0;
    a.meta[1] = 0;
    a.meta[2] = 1;
    a.meta[3] = 0;
    if (a.in_len == 0)
        return;
    if (read_header((gcptr)a.in, a.in_len, &hdr, &dlen, nullptr, 0) !=
        SNAPMI_OK)
        return;
    if (dlen > a.out_cap || (dlen + kStreamChunk - 1) / kStreamChunk > a.kmax)
        return;
    a.meta[0] = hdr;
    a.meta[1] = dlen;
    a.meta[2] = 0;
    a.meta[3] = (dlen + kStreamChunk - 1) / kStreamChunk;
}

// ---------------------------------------------------------------------
// k_bstream_scan: the level-1 table, (exit, produced) for the kEntry entry
// offsets of every 4 KiB segment.
//
// Rounds 1-3 gave every (segment, entry) its own lane and let it hop through
// HBM: ~45 instructions and one dependent load per element, and the eight
// chains of a segment are ONE chain after a few elements - seven eighths of
// the hops were duplicates (8.1 ms of the 14.2 ms of a 2 GiB stream).  Now:
//   * the hop is two LDS reads and ~42 straight-line instructions: the tag
//     from the lane's window of the input (a ring of kHopLines lines; up to
//     kHopFetch lines are fetched WHILE the lanes hop through the ones that
//     are there - the round structure of k_match_blocks), then (encoded
//     bytes, produced bytes) from a 256-entry table of tags.  Literals with
//     length bytes - one per 64 KiB of incompressible data - are done between
//     the rounds;
//   * a wavefront owns 64 segments.  Phase A walks all 8 x 64 entries for
//     kHopMid bytes only; phase B walks ONE trunk per segment from where
//     entry 0 stood after phase A - entries that stood at the same place are
//     the trunk plus what they had produced - and the chains that had not
//     joined (chains through the bytes of a long literal never meet);
//   * a walk that leaves its segment off the landing zone goes on through
//     the next one - but kHopMid bytes into it, it stands as a rule where
//     that segment's own trunk started, and is that trunk from there on;
//   * walks are handed out lane by lane from a pool, so a lane that is done
//     takes the next walk instead of waiting for the longest.
// Positions are 32-bit offsets from the wavefront's first segment; a chain
// that a literal of a GiB takes out of that range finishes in the 64-bit
// loop of the old kernel (elem_step of snapmi_element.hpp, through HBM).
// Measured (one 2 GiB stream, profiles/r4_stream_scan_steps.txt): 8.07 ms ->
// 2.0 ms; a wavefront is bound by the latency of its own dependent chain
// (alone on the chip or not), the lanes of a round are busy to ~55 %.
// ---------------------------------------------------------------------
#define SNAPMI_HOP_LINE 32
#define SNAPMI_HOP_ITERS 12
constexpr uint32_t kHopLine = SNAPMI_HOP_LINE; // bytes of a line
constexpr uint32_t kHopLines = 4;              // lines of a lane's ring
constexpr uint32_t kHopFetch = 2;              // lines fetched per round
// hops per round: a lane whose elements are larger than kHopFetch * kHopLine
// / kHopIters bytes on average runs out of window before the round is over
constexpr uint32_t kHopIters = SNAPMI_HOP_ITERS;
constexpr uint32_t kHopMid = 128;               // phase A walks this far
constexpr uint32_t kHopFar = 1u << 30;
constexpr uint32_t kHopNone = 0xFFFFFFFFu;

struct HopShared {
    l_u32 *win;  // [kHopLines * kHopLine / 4][64]: dword r of lane l at win[r * 64 + l]
    l_u16x *lut; // [256] encoded bytes | produced << 8; 0 = length bytes follow
    gcptr in;    // the stream
    uint64_t in_len;
    uint64_t wbase;  // stream offset of the wavefront's first segment
    uint32_t seg;    // segment size of this call (a power of two)
    uint32_t mis;    // (in + wbase) mod kHopLine: the window's lines are aligned
    uint32_t lastR;  // end of the stream from wbase, at most 2^31
    uint64_t lastP;  // the same + mis, exact
};

// one lane's walk
struct Hopper {
    uint32_t L0, nl;   // lines L0 .. L0 + nl - 1 of the aligned view are in the window
    uint32_t R;        // position from wbase
    uint32_t out;      // produced
    uint32_t over;     // elements hopped behind the segment's end
    uint32_t endR;     // the segment's end (or the stream's)
    uint32_t stopR;    // phase A pauses at the first element start here
    uint32_t stopOut;  // k_bstream_cuts: ... at the first one that has produced this
    bool run;          // hopping
    bool slow;         // stands in front of a literal with length bytes
    bool fail;         // the chain cannot be followed
    bool punt;         // left the 32-bit range: p64 / out64 are its end
    uint64_t p64, out64;

    // (the loop condition of rounds 1-3: the exit is the first element start
    // at or behind the segment's end that lies within kEntry bytes of a
    // segment boundary, or the end of the stream)
    __device__ __forceinline__ bool more(const HopShared &h) const
    {
        return R < h.lastR && (R < endR || (R & (h.seg - 1)) >= kEntry);
    }
    __device__ __forceinline__ void start(const HopShared &h, uint32_t r,
                                          uint32_t o, uint32_t e, uint32_t st,
                                          bool valid)
    {
        L0 = 0; nl = 0; R = r; out = o; over = 0; endR = e; stopR = st;
        stopOut = kHopNone;
        slow = false; punt = false; p64 = 0; out64 = 0;
        fail = !valid;
        run = valid && more(h) && R < stopR;
    }
    // between rounds: the literal with length bytes the lane stands at
    // (src/decompress.rs:213-232), its bytes through HBM
    __device__ __forceinline__ void long_literal(const HopShared &h)
    {
        slow = false;
        const uint64_t p = h.wbase + R;
        uint64_t q = p, qo = out;
        if (!elem_step(bytes_at(h.in), h.in_len, q, qo)) {
            fail = true;
            return;
        }
        const uint64_t len = qo - out;
        if (len + R >= kHopFar) {
            // out of the 32-bit range: the rest of the walk right here
            const uint64_t end = h.wbase + endR;
            bool ok = true;
            while (ok && q < h.in_len &&
                   (q < end || (q & (h.seg - 1)) >= kEntry)) {
                if (q >= end && ++over > kScanOverrun) {
                    ok = false;
                    break;
                }
                ok = elem_step(bytes_at(h.in), h.in_len, q, qo);
            }
            punt = true;
            fail = !ok;
            p64 = q;
            out64 = qo;
            return;
        }
        R += (uint32_t)(q - p);
        out += (uint32_t)len;
        run = more(h) && R < stopR && out < stopOut;
    }
    __device__ __forceinline__ void result(const HopShared &h, uint64_t &p,
                                           uint64_t &o) const
    {
        p = punt ? p64 : h.wbase + R;
        o = punt ? out64 : (uint64_t)out;
    }
};

// Rounds over a pool of `npool` walks: a lane without a walk takes the next
// one (init(item, w)), hops while its window reaches, and hands the walk to
// done(item, w) when it stands; done returns false to send it on (with a new
// stopR).
template <class INIT, class DONE>
__device__ __forceinline__ void hop_pool(const HopShared &h, uint32_t npool,
                                         INIT init, DONE done)
{
    typedef __attribute__((address_space(1))) u32x4 g_u32x4;
    const uint32_t lane = threadIdx.x;
    const l_u8 *const winb = (const l_u8 *)(h.win + lane);
    uint32_t next = 0; // uniform: first walk not handed out
    bool busy = false;
    uint32_t item = 0;
    Hopper w;
    w.run = false;
    w.slow = false;
    w.nl = 0;
    w.L0 = 0;
    for (;;) {
        if (busy && !w.run && !w.slow) { // this lane's walk stands
            if (done(item, w)) // ... and is over
                busy = false;
        }
        {
            const uint64_t M = __ballot(!busy);
            const uint32_t mine =
                next + __builtin_amdgcn_mbcnt_hi(
                           (uint32_t)(M >> 32),
                           __builtin_amdgcn_mbcnt_lo((uint32_t)M, 0));
            if (!busy && mine < npool) {
                item = mine;
                init(item, w);
                busy = true;
            }
            next += (uint32_t)__builtin_popcountll(M);
            if (next > npool)
                next = npool;
        }
        if (__ballot(w.slow)) {
            if (w.slow)
                w.long_literal(h);
        }
        if (!__ballot(busy))
            break;
        // ---- one round: fetch up to kHopFetch lines behind the window ------
        uint32_t want = 0, cnt = 0;
        if (w.run) {
            const uint32_t lp = (w.R + h.mis) / kHopLine;
            if (w.nl != 0 && lp >= w.L0 && lp < w.L0 + w.nl) {
                w.nl -= lp - w.L0; // the lines below are used up
                w.L0 = lp;
            } else {
                w.L0 = lp; // nothing of use: the lane sits this round out
                w.nl = 0;
            }
            want = w.L0 + w.nl;
            cnt = kHopLines - w.nl < kHopFetch ? kHopLines - w.nl : kHopFetch;
            // (a line that starts behind the stream's end is never fetched:
            // the stream's last line may be the last of the allocation)
            while (cnt && (uint64_t)(want + cnt - 1) * kHopLine >= h.lastP)
                cnt--;
        }
        u32x4 f[kHopFetch * kHopLine / 16];
#pragma unroll
        for (uint32_t i = 0; i < kHopFetch * kHopLine / 16; i++)
            f[i] = (u32x4){0, 0, 0, 0};
        {
            const g_u32x4 *g = (const g_u32x4 *)(h.in + h.wbase - h.mis +
                                                 (uint64_t)want * kHopLine);
#pragma unroll
            for (uint32_t c = 0; c < kHopFetch; c++)
                if (c < cnt) {
#pragma unroll
                    for (uint32_t i = 0; i < kHopLine / 16; i++)
                        f[c * (kHopLine / 16) + i] = g[c * (kHopLine / 16) + i];
                }
        }
        // ---- at most kHopIters hops through the lines that are there (LDS
        // only: the fetch is in flight).  Straight-line code: a divergent
        // region in this loop costs the scalar unit three instructions per
        // flag it carries.
        {
            uint32_t R = w.R, out = w.out, over = w.over;
            bool run = w.run, slow = false, fail = w.fail;
            const uint32_t lo = w.L0 * kHopLine - h.mis, span = w.nl * kHopLine;
            const uint32_t endR = w.endR, stopOut = w.stopOut;
            const uint32_t capR = w.stopR < h.lastR ? w.stopR : h.lastR;
            const uint32_t segm = h.seg - kEntry; // landing zone: none set
#define SNAPMI_HOP_UNROLL SNAPMI_HOP_ITERS
            for (uint32_t it = 0; it < kHopIters; it += SNAPMI_HOP_UNROLL) {
                // (one look at "can anyone hop" per SNAPMI_HOP_UNROLL hops - by
                // default per round: a lane that cannot, idles through them.
                // With a test and a branch per hop the compiler keeps the
                // loop's flags in step with three scalar instructions each,
                // 65 instructions per hop; unrolled it is 42, and the next
                // tag is on its way while the flags of this one are computed:
                // 3.39 -> 2.03 ms)
                if (!__builtin_amdgcn_ballot_w64(run && R - lo < span))
                    break;
#pragma unroll
                for (uint32_t u = 0; u < SNAPMI_HOP_UNROLL; u++) {
                    const bool can = run && R - lo < span;
                    const uint32_t x =
                        (R + h.mis) & (kHopLines * kHopLine - 1);
                    const uint32_t tag = winb[((x & ~3u) << 6) + (x & 3)];
                    const uint32_t lv = h.lut[tag];
                    const uint32_t e = can ? lv : 0; // waiting: no step
                    over += (can && R >= endR) ? 1u : 0u;
                    R += e & 0xFF;
                    out += e >> 8;
                    slow = slow || (can && lv == 0);
                    // (the element behind the limit is hopped, then the walk
                    // fails)
                    fail = fail || over > kScanOverrun || R > h.lastR;
                    run = run && !slow && !fail && R < capR &&
                          out < stopOut &&
                          (R < endR || (R & segm) != 0);
                }
            }
            w.R = R;
            w.out = out;
            w.over = over;
            w.run = run;
            w.slow = slow;
            w.fail = fail;
        }
        // ---- the fetched lines into the ring ------------------------------
#pragma unroll
        for (uint32_t c = 0; c < kHopFetch; c++)
            if (c < cnt) {
                l_u32 *dst = h.win +
                             ((want + c) & (kHopLines - 1)) * (kHopLine / 4) * 64 +
                             lane;
#pragma unroll
                for (uint32_t i = 0; i < kHopLine / 16; i++) {
                    const u32x4 v = f[c * (kHopLine / 16) + i];
                    dst[(4 * i + 0) * 64] = v.x;
                    dst[(4 * i + 1) * 64] = v.y;
                    dst[(4 * i + 2) * 64] = v.z;
                    dst[(4 * i + 3) * 64] = v.w;
                }
            }
        w.nl += cnt;
    }
}

// the table of tags: encoded bytes | produced bytes << 8, 0 for a literal
// with length bytes (snapmi_element.hpp)
__device__ __forceinline__ void hop_lut(uint16_t *lutbuf)
{
    for (uint32_t t = threadIdx.x; t < 256; t += 64) {
        const uint32_t enc = tag_encoded(t), prod = tag_produced(t);
        lutbuf[t] = (uint16_t)(enc | (prod << 8));
    }
    __syncthreads();
}

__device__ __forceinline__ void stream_scan(const StreamArgs &a, const uint32_t wg)
{
    __shared__ uint32_t winbuf[kHopLines * (kHopLine / 4) * 64];
    __shared__ uint16_t lutbuf[256];
    __shared__ uint32_t midR[64 * kEntry], midO[64 * kEntry];
    __shared__ uint16_t todo[64 * kEntry];
    __shared__ unsigned long long trunkP[64], trunkO[64];
    __shared__ uint32_t todoO[64 * (kEntry - 1)];
    __shared__ uint8_t trunkL[64], todoL[64 * (kEntry - 1)];
    if (a.meta[2])
        return;
    const uint32_t lane = threadIdx.x;
    HopShared h;
    h.win = (l_u32 *)winbuf;
    h.lut = (l_u16x *)lutbuf;
    h.in = (gcptr)a.in;
    h.in_len = a.in_len;
    const uint32_t S = a.scan_segs; // segments of this wavefront: 8 .. 64
    const uint64_t seg0 = (uint64_t)wg * S;
    const uint32_t sl2 = a.seg_log2; // (the wavefront's S segments: < 2^31)
    h.seg = 1u << sl2;
    h.wbase = seg0 << sl2;
    h.mis = (uint32_t)((uintptr_t)a.in + h.wbase) & (kHopLine - 1);
    // the grid covers nseg + 1 sentinel: its last workgroup can begin behind
    // the input (lastR = 0 then: every walk is invalid and reads nothing)
    const uint64_t left = a.in_len > h.wbase ? a.in_len - h.wbase : 0;
    h.lastR = left < (1ull << 31) ? (uint32_t)left : 1u << 31;
    h.lastP = left + h.mis;
    const uint32_t nloc =
        a.nseg - seg0 < S ? (uint32_t)(a.nseg - seg0) : S; // segments here
    hop_lut(lutbuf);
    su64x2 *const table = level_table<1>(a) + seg0 * kEntry;
    const uint32_t lastR = h.lastR;
    auto seg_end = [lastR, sl2](uint32_t sl) {
        return ((sl + 1) << sl2) < lastR ? ((sl + 1) << sl2) : lastR;
    };

    // ---- phase A: every entry, kHopMid bytes far --------------------------
    hop_pool(
        h, nloc * kEntry,
        [&](uint32_t it, Hopper &w) {
            const uint32_t sl = it / kEntry,
                           r0 = (sl << sl2) + it % kEntry;
            w.start(h, r0, 0, seg_end(sl), (sl << sl2) + kHopMid, r0 < lastR);
        },
        [&](uint32_t it, Hopper &w) {
            const bool paused = !w.fail && !w.punt && w.more(h);
            midR[it] = paused ? w.R : kHopNone;
            midO[it] = w.out;
            if (!paused) { // the chain is over, or cannot be followed
                uint64_t p, o;
                w.result(h, p, o);
                table[it] = (su64x2){w.fail ? kNone : p, o};
            }
            return true;
        });
    __syncthreads();

    // ---- the chains that stand elsewhere than their segment's entry 0 -----
    uint32_t ntodo = 0;
    for (uint32_t o = 1; o < kEntry; o++) {
        const uint32_t it = lane * kEntry + o;
        const uint32_t r = lane < nloc ? midR[it] : kHopNone;
        const bool own = r != kHopNone && r != midR[lane * kEntry];
        const uint64_t M = __ballot(own);
        if (own)
            todo[ntodo + __builtin_amdgcn_mbcnt_hi(
                             (uint32_t)(M >> 32),
                             __builtin_amdgcn_mbcnt_lo((uint32_t)M, 0))] =
                (uint16_t)it;
        ntodo += (uint32_t)__builtin_popcountll(M);
    }
    __syncthreads();

    // ---- phase B: one trunk per segment, and those ------------------------
    // A walk that leaves its segment off the landing zone goes on through the
    // next one (30 % of the trunks on text, and again with the same odds: the
    // longest of 64 walks was 4 600 hops where the average is 1 190) - but
    // kHopMid bytes into that segment it stands, as a rule, where that
    // segment's own trunk started: then it IS that trunk from there on, and
    // its result is a sum.  Links go to higher segments only; they are
    // resolved from the last segment down.
    for (uint32_t i = lane; i < 64; i += 64)
        trunkL[i] = 0xFF;
    auto next_stop = [nloc, sl2](uint32_t sl) {
        return sl + 1 < nloc ? ((sl + 1) << sl2) + kHopMid : kHopNone;
    };
    hop_pool(
        h, nloc + ntodo,
        [&](uint32_t it, Hopper &w) {
            // (the last segment's trunk first: it has nobody to join)
            const uint32_t e =
                it < nloc ? (nloc - 1 - it) * kEntry : todo[it - nloc];
            const uint32_t r = midR[e];
            // (a trunk counts from 0: its entries add what they had)
            w.start(h, r, it < nloc ? 0 : midO[e], seg_end(e / kEntry),
                    next_stop(e / kEntry), r != kHopNone);
        },
        [&](uint32_t it, Hopper &w) {
            uint32_t link = 0xFF;
            if (!w.fail && !w.punt && w.more(h)) { // stands at a stop
                const uint32_t t = w.R >> sl2;
                if (t < nloc && midR[t * kEntry] == w.R) {
                    link = t;
                } else {
                    w.stopR = next_stop(t);
                    w.run = true;
                    return false;
                }
            }
            uint64_t p, o;
            w.result(h, p, o);
            if (it < nloc) {
                const uint32_t sl = nloc - 1 - it;
                trunkP[sl] = w.fail ? kNone : p;
                trunkO[sl] = o;
                trunkL[sl] = (uint8_t)link;
            } else if (link == 0xFF) {
                table[todo[it - nloc]] = (su64x2){w.fail ? kNone : p, o};
            } else {
                todoO[it - nloc] = w.out;
            }
            if (it >= nloc)
                todoL[it - nloc] = (uint8_t)link;
            return true;
        });
    __syncthreads();
    if (lane == 0) {
        for (uint32_t sl = nloc; sl-- > 0;) {
            const uint32_t t = trunkL[sl];
            if (t != 0xFF) {
                trunkP[sl] = trunkP[t];
                trunkO[sl] += trunkO[t];
            }
        }
    }
    __syncthreads();
    for (uint32_t i = lane; i < ntodo; i += 64) {
        const uint32_t t = todoL[i];
        if (t != 0xFF)
            table[todo[i]] = (su64x2){trunkP[t], todoO[i] + trunkO[t]};
    }
    if (lane < nloc) {
        const uint32_t t0 = midR[lane * kEntry];
        for (uint32_t o = 0; o < kEntry; o++) {
            const uint32_t it = lane * kEntry + o;
            if (t0 != kHopNone && midR[it] == t0)
                table[it] = (su64x2){trunkP[lane], trunkO[lane] + midO[it]};
        }
    }
}

// the one sequential pass: a table lookup per 16 MiB of input
__device__ __forceinline__ void stream_chain(const StreamArgs &a, const uint32_t wg)
{
    if (a.meta[2])
        return;
    uint64_t p = a.meta[0], out = 0;
    bool ok = true;
    while (ok && p < a.in_len) {
        level_entry<3>(a)[p / level_bytes<3>(a)] = (su64x2){p, out};
        ok = reach_end<3>(a, p, out);
    }
    // the elements must end with the stream and produce the announced
    // length (src/decompress.rs:141-147)
    if (!ok || p != a.in_len || out != a.meta[1])
        a.meta[2] = 1;
}

// The element boundary at (or first behind) every 64 KiB of output: the
// segments whose stretch of the chain holds such a boundary are collected -
// kCutSegs segments per wavefront, one in eight on text - and walked from
// where the chain enters them by the pool of k_bstream_scan (windows in LDS),
// a lane per segment, standing at every boundary on the way.  (Rounds 1-3:
// one lane per segment hopping through HBM, the wavefront as slow as its
// slowest lane: 1.7 ms of a 2 GiB stream.)
__device__ __forceinline__ void stream_cuts(const StreamArgs &a, const uint32_t wg)
{
    __shared__ uint32_t winbuf[kHopLines * (kHopLine / 4) * 64];
    __shared__ uint16_t lutbuf[256];
    __shared__ uint16_t todo[kCutSegs];
    if (a.meta[2])
        return;
    const uint32_t lane = threadIdx.x;
    const uint64_t seg0 = (uint64_t)wg * kCutSegs;
    if (seg0 == 0 && lane == 0) {
        const uint64_t K = a.meta[3];
        a.cuts[0] = a.meta[0];
        a.cuts[1] = 0;
        a.cuts[K * 2] = a.in_len;
        a.cuts[K * 2 + 1] = a.meta[1];
    }
    HopShared h;
    h.win = (l_u32 *)winbuf;
    h.lut = (l_u16x *)lutbuf;
    h.in = (gcptr)a.in;
    h.in_len = a.in_len;
    const uint32_t sl2 = a.seg_log2;
    h.seg = 1u << sl2;
    h.wbase = seg0 << sl2;
    h.mis = (uint32_t)((uintptr_t)a.in + h.wbase) & (kHopLine - 1);
    const uint64_t left = a.in_len > h.wbase ? a.in_len - h.wbase : 0;
    h.lastR = left < (1ull << 31) ? (uint32_t)left : 1u << 31;
    h.lastP = left + h.mis;
    hop_lut(lutbuf);
    const uint64_t dlen = a.meta[1];
    // ---- the segments with a boundary in their stretch --------------------
    uint32_t ntodo = 0;
    for (uint32_t j = 0; j < kCutSegs; j += 64) {
        const uint64_t seg = seg0 + j + lane;
        bool has = false;
        if ((seg << sl2) < a.in_len) {
            const su64x2 e = level_entry<1>(a)[seg];
            if (e.x != kNone) {
                uint64_t np = e.x, nout = e.y;
                if (!reach_end<1>(a, np, nout)) {
                    a.meta[2] = 1;
                } else {
                    const uint64_t t = (e.y / kStreamChunk + 1) * kStreamChunk;
                    has = t <= nout && t < dlen;
                }
            }
        }
        const uint64_t M = __ballot(has);
        if (has)
            todo[ntodo + __builtin_amdgcn_mbcnt_hi(
                             (uint32_t)(M >> 32),
                             __builtin_amdgcn_mbcnt_lo((uint32_t)M, 0))] =
                (uint16_t)(j + lane);
        ntodo += (uint32_t)__builtin_popcountll(M);
    }
    __syncthreads();
    // ---- walk them: a stop at every boundary ------------------------------
    uint64_t out0 = 0, nout = 0, k = 0; // of this lane's walk
    const uint32_t lastR = h.lastR;
    hop_pool(
        h, ntodo,
        [&](uint32_t it, Hopper &w) {
            const uint32_t sl = todo[it];
            const su64x2 e = level_entry<1>(a)[seg0 + sl];
            uint64_t np = e.x;
            out0 = e.y;
            nout = e.y;
            reach_end<1>(a, np, nout); // (true: it was, above)
            k = out0 / kStreamChunk + 1;
            const uint32_t endR =
                ((sl + 1) << sl2) < lastR ? ((sl + 1) << sl2) : lastR;
            w.start(h, (uint32_t)(e.x - h.wbase), 0, endR, kHopNone, true);
            w.stopOut = (uint32_t)(k * kStreamChunk - out0);
            w.run = w.run && w.out < w.stopOut;
        },
        [&](uint32_t it, Hopper &w) {
            const uint64_t qo = out0 + w.out;
            if (w.fail || w.punt || qo < k * kStreamChunk) {
                // cannot be followed here (or a literal of a GiB): the
                // sequential decoder owns the stream
                a.meta[2] = 1;
                return true;
            }
            // (a long element can cover several boundaries)
            while (k * kStreamChunk <= qo && k * kStreamChunk < dlen) {
                a.cuts[k * 2] = h.wbase + w.R;
                a.cuts[k * 2 + 1] = qo;
                k++;
            }
            if (k * kStreamChunk <= nout && k * kStreamChunk < dlen) {
                w.stopOut = (uint32_t)(k * kStreamChunk - out0);
                w.run = w.more(h);
                if (w.run)
                    return false;
                a.meta[2] = 1; // (the stretch ends before its last boundary)
            }
            return true;
        });
}

__device__ __forceinline__ void stream_pieces(const StreamArgs &a, const uint32_t wg)
{
    const uint64_t k = (uint64_t)wg * blockDim.x + threadIdx.x;
    if (k >= a.kmax)
        return;
    const bool live = a.meta[2] == 0 && k < a.meta[3];
    const uint64_t s0 = live ? a.cuts[k * 2] : 0,
                   d0 = live ? a.cuts[k * 2 + 1] : 0;
    const uint64_t s1 = live ? a.cuts[k * 2 + 2] : 0,
                   d1 = live ? a.cuts[k * 2 + 3] : 0;
    piece_put(a.c, k, a.in + s0, s1 - s0, a.out + d0, d1 - d0, 2);
}

__device__ __forceinline__ void stream_finish(const StreamArgs &a, const uint32_t wg)
{
    __shared__ uint32_t bad;
    if (threadIdx.x == 0)
        bad = a.meta[2] != 0;
    __syncthreads();
    const uint64_t K = a.meta[3];
    if (!bad)
        for (uint64_t k = threadIdx.x; k < K; k += blockDim.x)
            if (!piece_whole(a.c, k))
                atomicOr(&bad, 1u);
    __syncthreads();
    if (threadIdx.x == 0) {
        a.meta[2] = bad; // 1: the sequential decoder runs next
        if (a.fb_mode) // in a batch: 0 = decode it in the launch behind, 3 = not
            *a.fb_mode = bad ? 0 : 3;
        if (!bad) {
            a.out_len[0] = a.meta[1];
            set_error(a.err, 0, SNAPMI_OK, 0, 0, 0);
        }
    }
}

// ---------------------------------------------------------------------
// The kernels, for the long streams of a batch (snapmi_decompress_batch, few
// streams: every long stream gets its pieces instead of one wavefront) and
// for ONE stream as a batch of one (snapmi_decompress_stream): a workgroup
// first finds its stream and its place in that stream's workgroups.
// ---------------------------------------------------------------------
// b.pre[s] = first workgroup of stream s in this launch, pre[L] = all of them;
// pre == nullptr: one workgroup per stream
__device__ __forceinline__ bool batch_find(const BatchStreams &b, uint32_t &s,
                                           uint32_t &wg)
{
    const uint32_t g = blockIdx.x;
    if (!b.pre) {
        s = g;
        wg = 0;
        return g < b.n;
    }
    if (g >= b.pre[b.n])
        return false;
    uint32_t lo = 0, hi = b.n; // pre[lo] <= g < pre[hi]
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (b.pre[mid] <= g)
            lo = mid;
        else
            hi = mid;
    }
    s = lo;
    wg = g - b.pre[lo];
    return true;
}
#define SNAPMI_STREAM_KERNEL(name, bounds, call)                              \
    __global__ __launch_bounds__(bounds) void k_bstream_##name(BatchStreams b) \
    {                                                                         \
        uint32_t s_, wg;                                                      \
        if (!batch_find(b, s_, wg))                                           \
            return;                                                           \
        const StreamArgs a = b.descs[s_];                                     \
        call;                                                                 \
    }
SNAPMI_STREAM_KERNEL(head, 64, stream_head(a, wg))
SNAPMI_STREAM_KERNEL(scan, 64, stream_scan(a, wg))
SNAPMI_STREAM_KERNEL(super, kEntry, build_level<2>(a, wg))
SNAPMI_STREAM_KERNEL(super3, kEntry, build_level<3>(a, wg))
SNAPMI_STREAM_KERNEL(chain, 64, stream_chain(a, wg))
SNAPMI_STREAM_KERNEL(spread3, 64, spread_level<3>(a, wg))
SNAPMI_STREAM_KERNEL(spread2, 64, spread_level<2>(a, wg))
SNAPMI_STREAM_KERNEL(cuts, 64, stream_cuts(a, wg))
SNAPMI_STREAM_KERNEL(pieces, 256, stream_pieces(a, wg))
SNAPMI_STREAM_KERNEL(finish, 1024, stream_finish(a, wg))

// The long streams of a batch (long_stream_rule) whose header announces no
// more than the caller's buffer holds (anything else is left to the wavefront
// decoder, which names the error).  modes[i] = 3 for them (the
// batch's own launch skips them), 0 for the others.
__global__ __launch_bounds__(1024) void k_long_plan(
    const void *const *in_ptrs, const uint64_t *in_lens, void *const *out_ptrs,
    const uint64_t *out_caps, uint32_t n, uint64_t min_len, uint8_t *modes,
    LongItem *list, uint32_t cap, uint32_t *count)
{
    for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) {
        const uint64_t len = in_lens[i];
        uint8_t mode = 0;
        if (len >= min_len) {
            uint64_t dl = 0;
            const uint32_t hdr = read_varint((gcptr)in_ptrs[i], len, &dl);
            if (hdr && dl <= out_caps[i] && long_stream_rule(len, dl, min_len)) {
                const uint32_t slot = atomicAdd(count, 1u);
                if (slot < cap) {
                    LongItem it;
                    it.idx = i;
                    it.pad = 0;
                    it.in_len = len;
                    it.dlen = dl;
                    it.in = in_ptrs[i];
                    it.out = out_ptrs[i];
                    it.out_cap = out_caps[i];
                    list[slot] = it;
                    mode = 3;
                }
            }
        }
        modes[i] = mode;
    }
}

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

// The descriptor of stream `g` of plan `p`: its own ends `io`, its geometry,
// and where its tables and piece descriptors lie in sd_tables / sd_desc
// (reserved for the plan).
// io == nullptr: a stream of snapmi_build_block_index, which stops at the
// cuts.  No input pointer yet (k_index_build_adopt), no output - stream_head
// only asks that the length fits: out_cap is the slot's bound -, and no piece
// descriptors: nothing is decoded, and sd_desc may never have been reserved.
StreamArgs stream_desc(snapmi_ctx *ctx, const StreamPlan &p,
                       const StreamSlot &g, const StreamEnds *io)
{
    StreamArgs a = {};
    a.in_len = g.in_len;
    if (io) {
        a.in = (const uint8_t *)io->in;
        a.out = (uint8_t *)io->out;
        a.out_cap = io->out_cap;
        a.out_len = (unsigned long long *)io->out_len;
        a.err = io->err;
        a.fb_mode = io->fb_mode;
        a.c = piece_list_from(piece_list(ctx->sd_desc.p, p.pieces), g.entry);
    } else {
        a.out_cap = g.bound;
    }
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
    return a;
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
        const LongItem &it = items[j];
        const StreamEnds io = {it.in, it.out, it.out_cap,
                               d_out_lens + it.idx,
                               d_errs ? d_errs + it.idx : nullptr,
                               modes2 + it.idx};
        descs[j] = stream_desc(ctx, p, slot[j], &io);
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
    const StreamEnds io = {d_in, d_out, out_cap, d_out_len, d_err, nullptr};
    h.a = stream_desc(ctx, p, slot, &io);
    const StreamArgs &a = h.a;
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
