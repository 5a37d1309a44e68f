// snapmi_compress.hip -- the batch compressor's pipeline around its match
// finders, Snappy raw format for gfx950 (CDNA4); with it the small-stream
// kernels.
//
// What is computed is fixed by the reference (src/compress.rs: one greedy
// LZ77 parse per <= 64 KiB block with a 16-bit hash table, the skip heuristic
// and the literal / copy-1 / copy-2 encoders) and must be bit-exact; blocks
// are independent (src/compress.rs:148,514-516), so the work list is "all
// blocks of all streams of the batch".  A batch runs (launch_compress,
// snapmi_launch.hip; which kernels: snapmi_route.hpp):
//   1. plan   k_plan_compress*: validates every stream, gives it its global
//             blocks and scratch slots (what snapmi_block.hpp's rules read);
//   2. small  streams under CompressArgs::small_limit have no blocks: a lane
//             each compresses them (k_compress_tiny, k_compress_small*);
//   3. match  EITHER a window kernel over the whole batch, which encodes as
//             it matches, block 0 of a stream in place, later blocks into
//             scratch slots (snapmi_window.hip; the test build's
//             snapmi_steps.hip) - OR the token path, a segment of the block
//             list at a time: a match finder writes tokens and adds up what
//             they encode to (snapmi_lane.hip; k_match_spans*), k_scan_sizes*
//             turns sizes into positions, and
//   4. encode k_encode_tokens writes every block at its final position
//             (k_redo_spilled: the blocks whose tokens found no page);
//   5. lens   k_stream_lens, or k_scan_sizes* + k_compact (scratch slots into
//             place), leave every stream's compressed length; k_post_ratio
//             tells the next batch how this one compressed.
#include "snapmi_compress_dev.hpp"
#include "snapmi_scan.hpp"

namespace snapmi {

// What the batch compressed to, posted into pinned host memory for the NEXT
// batch's choice of match finder (launch_compress: a context whose data does
// not compress is better off with LDS tables).  Per slot: words 0..1 =
// compressed bytes of the blocks, 2..3 = input bytes of the batch, 4 = the
// batch's number (0 while the slot is being written).
__global__ __launch_bounds__(1024) void k_post_ratio(
    uint32_t *host_mapped, const uint64_t *blk_off, uint32_t blocks,
    const uint64_t *in_lens, uint32_t n_streams, uint32_t seq)
{
    __shared__ unsigned long long part[1024];
    unsigned long long sum = 0;
    for (uint32_t i = threadIdx.x; i < n_streams; i += 1024)
        sum += in_lens[i];
    part[threadIdx.x] = sum;
    __syncthreads();
    for (uint32_t w = 512; w; w >>= 1) {
        if (threadIdx.x < w)
            part[threadIdx.x] += part[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        // (two slots, taken in turn: the host reads the one whose number is
        // higher while the other is being written)
        uint32_t *slot = host_mapped + 8 * (seq & 1);
        const uint64_t total = blk_off[blocks];
        slot[4] = 0;
        __threadfence_system();
        slot[0] = (uint32_t)total;
        slot[1] = (uint32_t)(total >> 32);
        slot[2] = (uint32_t)part[0];
        slot[3] = (uint32_t)(part[0] >> 32);
        __threadfence_system();
        slot[4] = seq;
    }
}

// ---------------------------------------------------------------------
// K1t: streams of fewer than 256 bytes, ONE PER LANE, input and table in LDS.
//
// A block of a couple of hundred bytes costs the lane kernel ~190 rounds of
// an HBM (or L2) round trip, and the wavefront kernels a whole wavefront for
// ~100 probes.  Its whole state is tiny, though: the input and the
// reference's smallest table (256 entries, src/compress.rs:491-518 - and a
// position fits a byte) are two columns of 64 dwords per lane, 32 KiB per
// wavefront, four wavefronts per CU.  Every read of the parse is then an LDS
// access of ~100 cycles and the lane runs the reference's loop as it is
// written (snapmi_tiny.hpp: the test suite runs the same text over byte
// arrays on the CPU, tests/test_tiny_lane_cpu.py).  The columns are dword-
// interleaved (byte k of lane l at ((k >> 2) * 64 + l) * 4 + (k & 3)), so
// lanes at the same position hit 64 different banks.  The output goes
// straight to the caller's buffer, element by element: it is never read
// back, and a third column (65 dwords per lane) meant three wavefronts per
// CU instead of four - 202 against 276 GiB/s on 200-byte streams
// (profiles/r3_tiny_output_direct.txt; SNAPMI_TINY_STAGE_OUT=1 builds that
// variant).
// k_plan_compress gives these streams no blocks (CompressArgs::small_limit),
// so the block kernels never see them.
// ---------------------------------------------------------------------
namespace {
#define SNAPMI_TINY_STAGE_OUT 0 // 1: an output column in LDS (experiment)
template <bool kStage> struct TinyColumns {
    typedef __attribute__((address_space(3))) uint32_t l_u32;
    typedef __attribute__((address_space(3))) uint8_t l_u8;
    l_u32 *in, *tb, *out; // this lane's columns: dword w at [w * 64]
    gptr gout;            // !kStage: the stream's place in the caller's buffer
    __device__ __forceinline__ static uint32_t at(uint32_t k)
    {
        return (k >> 2) * 256 + (k & 3); // byte offset inside the column
    }
    __device__ __forceinline__ uint32_t in8(uint32_t k) const
    {
        return ((const l_u8 *)in)[at(k)];
    }
    __device__ __forceinline__ uint32_t in32(uint32_t k) const
    {
        const l_u32 *w = in + (k >> 2) * 64; // k + 4 <= n <= 255: w[64] exists
        return __builtin_amdgcn_alignbyte(w[64], w[0], k & 3);
    }
    __device__ __forceinline__ uint32_t tab(uint32_t h) const
    {
        return ((const l_u8 *)tb)[at(h)];
    }
    __device__ __forceinline__ void tab_set(uint32_t h, uint32_t v)
    {
        ((l_u8 *)tb)[at(h)] = (uint8_t)v;
    }
    __device__ __forceinline__ void out8(uint32_t k, uint32_t v)
    {
        if (kStage)
            ((l_u8 *)out)[at(k)] = (uint8_t)v;
        else
            gout[k] = (uint8_t)v;
    }
    __device__ __forceinline__ void out32(uint32_t k, uint32_t v)
    {
        if (kStage)
            out[(k >> 2) * 64] = v;
        else
            st32u(gout + k, v);
    }
};
} // namespace

// stream i of the batch by this lane (k_compress_tiny: 64 consecutive streams
// per wavefront; k_seam_compress_tiny: one)
__device__ __forceinline__ void compress_tiny_stream(const CompressArgs &a,
                                                     const uint64_t i)
{
    constexpr bool kStage = SNAPMI_TINY_STAGE_OUT != 0;
    constexpr uint32_t kW = kTinyCompress / 4;         // dwords per column
    constexpr uint32_t kWo = kStage ? (kTinyOutMax + 3) / 4 : 1; // 65
    __shared__ uint32_t tin[kW * 64];
    __shared__ uint32_t ttab[kW * 64];
    __shared__ uint32_t tout[kWo * 64];
    const uint32_t lane = threadIdx.x;
    if (i >= a.n_streams)
        return;
    const uint64_t len = a.in_lens[i];
    if (len == 0 || len >= kTinyCompress || len >= a.small_limit)
        return; // not this kernel's
    if (a.out_caps && a.out_caps[i] < max_compress_len_u64(len))
        return; // BufferTooSmall, reported by k_plan_compress
    const uint32_t n = (uint32_t)len;
    typedef TinyColumns<kStage> Columns;
    Columns m;
    m.in = (typename Columns::l_u32 *)tin + lane;
    m.tb = (typename Columns::l_u32 *)ttab + lane;
    m.out = (typename Columns::l_u32 *)tout + lane;
    m.gout = (gptr)a.out_ptrs[i];
    gcptr src = (gcptr)a.in_ptrs[i];
    {
        // whole dwords; the last partial one bytewise (reads stay inside
        // the stream)
        uint32_t k = 0;
        for (; k + 4 <= n; k += 4)
            m.in[(k >> 2) * 64] = ld32u(src + k);
        uint32_t last = 0;
        for (uint32_t j = 0; k + j < n; j++)
            last |= (uint32_t)src[k + j] << (8 * j);
        m.in[(k >> 2) * 64] = last; // (k >> 2 <= 63)
    }
    if (n >= kMinNonLiteral)
        for (uint32_t w = 0; w < kW; w++) // fresh table: src/compress.rs:506
            m.tb[w * 64] = 0;
    const uint32_t d = tiny_compress(m, n);
    gptr dst = (gptr)a.out_ptrs[i];
    if (kStage) {
        uint32_t k = 0;
        for (; k + 4 <= d; k += 4)
            st32u(dst + k, m.out[(k >> 2) * 64]);
        const uint32_t last = m.out[(k >> 2) * 64];
        for (uint32_t j = 0; k + j < d; j++)
            dst[k + j] = (uint8_t)(last >> (8 * j));
    }
    a.out_lens[i] = d;
}

__global__ __launch_bounds__(64) void k_compress_tiny(CompressArgs a)
{
    compress_tiny_stream(a, (uint64_t)blockIdx.x * 64 + threadIdx.x);
}

// The libsnappy seam's single-launch path (snapmi_api.hip, seam_tiny): ONE
// stream of 1..255 bytes whose input and output lie in pinned host memory the
// device reaches over the link - no copy commands, no plan kernel, the
// stream's description in the kernel's arguments (a descriptor in host
// memory is a round trip over the link per dependent load), and the host
// learns of the end from *done (it polls it; a system-scope fence puts the
// output and the length in front of it).  All 64 lanes bring the input in -
// one load instruction, one round trip - and clear the table; lane 0 runs
// the reference's loop (snapmi_tiny.hpp) and stores the elements as they come.
__global__ __launch_bounds__(64) void k_seam_compress_tiny(
    const uint8_t *in, uint32_t n, uint8_t *out, unsigned long long *out_len,
    uint32_t *done, uint32_t seq)
{
    constexpr bool kStage = SNAPMI_TINY_STAGE_OUT != 0;
    constexpr uint32_t kW = kTinyCompress / 4; // dwords per column (64)
    constexpr uint32_t kWo = kStage ? (kTinyOutMax + 3) / 4 : 1;
    __shared__ uint32_t tin[kW * 64];
    __shared__ uint32_t ttab[kW * 64];
    __shared__ uint32_t tout[kWo * 64];
    const uint32_t lane = threadIdx.x;
    gcptr src = (gcptr)in;
    {
        // dword `lane` of the input into lane 0's column (reads stay inside
        // the stream: the last partial dword bytewise)
        const uint32_t k = 4 * lane;
        uint32_t v = 0;
        if (k + 4 <= n) {
            v = ld32u(src + k);
        } else {
            for (uint32_t j = 0; k + j < n; j++)
                v |= (uint32_t)src[k + j] << (8 * j);
        }
        tin[lane * 64] = v;
        ttab[lane * 64] = 0; // fresh table: src/compress.rs:506
    }
    __syncthreads();
    if (lane != 0)
        return;
    typedef TinyColumns<kStage> Columns;
    Columns m;
    m.in = (typename Columns::l_u32 *)tin;
    m.tb = (typename Columns::l_u32 *)ttab;
    m.out = (typename Columns::l_u32 *)tout;
    m.gout = (gptr)out;
    const uint32_t d = tiny_compress(m, n);
    *out_len = d;
    __threadfence_system();
    __hip_atomic_store(done, seq, __ATOMIC_RELEASE,
                       __HIP_MEMORY_SCOPE_SYSTEM);
}

// ---------------------------------------------------------------------
// K1s: streams of 256 .. 1023 (2047) bytes, a FEW per wavefront, input and
// table in LDS.
//
// The same idea one size class up.  A block of 1 KiB costs the lane kernel
// as many HBM table accesses per byte as a 64 KiB block (more: every block
// starts with an empty table), 24-28 ms per GiB whatever the size; its state,
// though, is 1 KiB of input + the reference's table for that length (1 024
// entries of u16) = 3 KiB, so 48 such streams fit a CU's LDS.  They are kept
// as contiguous per-lane regions, kL lanes of a wavefront each running the
// reference's loop on its own stream (snapmi_tiny.hpp) after all 64 lanes
// have brought the inputs in (16 bytes per lane and access).  The output goes
// straight to the caller's buffer, lane by lane: an output column in LDS
// costs a quarter of the streams per CU, and those are what the rate is made
// of (measured, profiles/r3_small_stream_variants.txt: 93.6 -> 116 GiB/s at
// 400 bytes, 43.5 -> 56.0 at 1 000; half the lanes per wavefront and twice
// the wavefronts, with or without the column: slower - the rounds are bound
// by instruction issue as much as by latency, and a wavefront issues for all
// of its lanes at once).  Classes by the stream's length: [256, 512) eight
// lanes per wavefront, [512, 1024) four, twelve wavefronts (12 KiB each) per
// CU.  [1024, 2048) with two lanes exists but is off by default: 26 GiB/s
// against the lane kernel's 35 (option small_stream_kernel = 2).
// A wavefront looks at 64 consecutive streams of the batch and works through
// the ones of its class kL at a time (no list, no ticket).
// ---------------------------------------------------------------------
namespace {
struct SmallRegion {
    typedef __attribute__((address_space(3))) uint8_t l_u8;
    typedef __attribute__((address_space(3), may_alias)) uint16_t l_u16s;
    l_u8 *in;
    l_u16s *tb;
    gptr out; // the stream's place in the caller's buffer
    __device__ __forceinline__ uint32_t in8(uint32_t k) const { return in[k]; }
    __device__ __forceinline__ uint32_t in32(uint32_t k) const
    {
        // (LDS takes unaligned dwords: tests/hw/lds_unaligned.hip)
        return ld32u((lcptr)(in + k));
    }
    __device__ __forceinline__ uint32_t tab(uint32_t h) const { return tb[h]; }
    __device__ __forceinline__ void tab_set(uint32_t h, uint32_t v)
    {
        tb[h] = (uint16_t)v;
    }
    __device__ __forceinline__ void out8(uint32_t k, uint32_t v)
    {
        out[k] = (uint8_t)v;
    }
    __device__ __forceinline__ void out32(uint32_t k, uint32_t v)
    {
        st32u(out + k, v);
    }
};

template <uint32_t kCap, uint32_t kL>
__device__ __forceinline__ void compress_small(const CompressArgs &a)
{
    // per-lane region: input, table (kCap entries)
    constexpr uint32_t kRegion = kCap + 2 * kCap;
    constexpr uint32_t kLo = kCap == 2 * kTinyCompress ? kTinyCompress
                                                       : kCap / 2;
    __shared__ __attribute__((aligned(16))) uint8_t mem[kL * kRegion];
    typedef SmallRegion::l_u8 l_u8;
    typedef __attribute__((address_space(3), may_alias)) u32x4 l_u32x4;
    l_u8 *const base = (l_u8 *)mem;
    const uint32_t lane = threadIdx.x;
    const uint64_t i = (uint64_t)blockIdx.x * 64 + lane;
    uint64_t len = i < a.n_streams ? a.in_lens[i] : 0;
    if (len >= a.small_limit ||
        (a.out_caps && len && a.out_caps[i] < max_compress_len_u64(len)))
        len = 0; // the block kernels' / reported by k_plan_compress
    uint64_t M = __ballot(len >= kLo && len < kCap);
    while (M) {
        // lane j < kL takes the j-th stream of the class that is left
        uint32_t mine = 64; // position of this lane's stream in the wavefront
        {
            uint64_t m = M;
            for (uint32_t j = 0; j < kL && m; j++) {
                const uint32_t b = (uint32_t)__builtin_ctzll(m);
                m &= m - 1;
                if (lane == j)
                    mine = b;
            }
            M = m;
        }
        // bring the inputs in and clear the tables, all lanes at it
        uint32_t n = 0;
        for (uint32_t j = 0; j < kL; j++) {
            const uint32_t b = rdlane(mine, j);
            if (b == 64)
                break;
            const uint64_t st = (uint64_t)blockIdx.x * 64 + b;
            const uint32_t nj = uni((uint32_t)a.in_lens[st]);
            if (lane == j)
                n = nj;
            gcptr src = (gcptr)uni64((uint64_t)a.in_ptrs[st]);
            l_u8 *const r = base + j * kRegion;
            for (uint32_t k = lane * 16; k + 16 <= nj; k += 1024)
                *(l_u32x4 *)(r + k) = ld128g(src + k);
            if (lane < (nj & 15))
                r[(nj & ~15u) + lane] = src[(nj & ~15u) + lane];
            // (the table this length needs: 512 .. kCap entries of 2 bytes)
            uint32_t tbytes = 1024;
            while (tbytes < 2 * nj)
                tbytes *= 2;
            for (uint32_t k = lane * 16; k < tbytes; k += 1024)
                *(l_u32x4 *)(r + kCap + k) = (u32x4){0, 0, 0, 0};
        }
        // (one wavefront: its LDS accesses complete in order; the barriers
        // keep the compiler from moving them across)
        __syncthreads();
        if (mine != 64) {
            const uint64_t st = (uint64_t)blockIdx.x * 64 + mine;
            SmallRegion m;
            m.in = base + lane * kRegion;
            m.tb = (SmallRegion::l_u16s *)(m.in + kCap);
            m.out = (gptr)a.out_ptrs[st];
            a.out_lens[st] = tiny_compress(m, n);
        }
        __syncthreads(); // (the next round's inputs overwrite the regions)
    }
}
} // namespace
__global__ __launch_bounds__(64) void k_compress_small512(CompressArgs a)
{
    compress_small<512, 8>(a);
}
__global__ __launch_bounds__(64) void k_compress_small1k(CompressArgs a)
{
    compress_small<1024, 4>(a);
}
__global__ __launch_bounds__(64) void k_compress_small2k(CompressArgs a)
{
    compress_small<2048, 2>(a);
}

// ---------------------------------------------------------------------
// K1c: tokens -> Snappy elements, one wavefront per block, 64 tokens per
// pass (TokenSink::flush: reference emit_literal / emit_copy).
// ---------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_encode_tokens(CompressArgs a)
{
    const uint32_t lane = threadIdx.x;
    const uint32_t b = a.blk_lo + blockIdx.x;
    if (b >= segment_blocks(a))
        return;
    if (a.ntok[b] >= kTokSpilled)
        return; // encoded by k_compress_blocks / left to k_redo_spilled
    const BlockAt at = locate_block(a, b);
    gcptr src = (gcptr)at.in + at.off();
    // (a.direct: the sizes of the blocks in front are known - the match
    // finder added them up, k_scan_sizes ran over this segment)
    gptr dst;
    if (!block_dest(a, at, b, lane == 0, dst))
        return; // stream rejected by k_plan_compress (E_ARGUMENT)
    TokenSink out;
    out.init(src, at.n, dst, lane);
    typedef __attribute__((address_space(1))) uint32_t g_tok;
    typedef __attribute__((address_space(1))) unsigned long long g_u64;
    // the block's page table (CompressArgs::tok_pool): a pass of 64 tokens
    // lies in one page
    // (lane i holds entry i: no load stands between a pass and its tokens)
    const uint32_t ptab =
        lane < kPageTabStride
            ? a.tok_pages[(uint64_t)(b - a.tok_base) * kPageTabStride + lane]
            : 0;
    const g_tok *const pool = (const g_tok *)a.tok_pool;
    const uint32_t count = a.ntok[b];
    uint32_t pos_base = 0, exc_base = 0;
    // (the next pass's tokens are loaded before this pass is encoded: one
    // memory latency less on the chain of every pass)
    uint32_t tnext =
        lane < count ? pool[(uint64_t)rdlane(ptab, 0) * kTokPage + lane] : 0;
    for (uint32_t t0 = 0; t0 < count; t0 += kWave) {
        const uint32_t m = count - t0 < kWave ? count - t0 : kWave;
        uint32_t L = 0, C = 0, O = 0;
        const uint32_t t = tnext;
        if (t0 + kWave < count) {
            const uint32_t pg = rdlane(ptab, (t0 + kWave) / kTokPage);
            if (t0 + kWave + lane < count)
                tnext = pool[(uint64_t)pg * kTokPage +
                             (t0 + kWave) % kTokPage + lane];
        }
        const uint32_t field = (t >> 10) & 63u;
        if (lane < m) {
            L = t & 1023u;
            C = field == kTokLiteral ? 0u : field + 4u;
            O = t >> 16;
        }
        // a token that did not fit four bytes: its numbers are in the
        // block's exception list, in the order of such tokens (rare: a pass
        // without one pays a ballot)
        const bool ex = lane < m && field == kTokException;
        const uint64_t E = __builtin_amdgcn_ballot_w64(ex);
        if (E) {
            // (every lane takes part in the exchange: its page table entry
            // may be the one an exception's lane needs)
            const uint32_t ei =
                exc_base + __builtin_amdgcn_mbcnt_hi(
                               (uint32_t)(E >> 32),
                               __builtin_amdgcn_mbcnt_lo((uint32_t)E, 0));
            const uint32_t eslot = ei / kExcPage < kExcPagesPerBlock
                                       ? ei / kExcPage
                                       : kExcPagesPerBlock - 1;
            const uint32_t epg = (uint32_t)__builtin_amdgcn_ds_bpermute(
                (int)((kTokPagesPerBlock + eslot) << 2), (int)ptab);
            if (ex) {
                const unsigned long long f =
                    ((const g_u64 *)(pool + (uint64_t)epg * kTokPage))
                        [ei % kExcPage];
                L = (uint32_t)f & 0x1FFFFu;
                C = (uint32_t)(f >> 17) & 0xFFFFu;
                O = (uint32_t)(f >> 33) & 0xFFFFu;
            }
            exc_base += (uint32_t)__builtin_popcountll(E);
        }
        const uint32_t span = L + C;
        const uint32_t incl = wave_inclusive_scan(span);
        const uint32_t P = pos_base + incl - span; // literal start
        pos_base += rdlane(incl, kWave - 1);
        out.a = (L & 0xFFFFu) | (O << 16);
        out.b = C | (P << 16);
        out.t = m;
        out.flush();
    }
    if (lane == 0 && !a.direct)
        a.blk_size[b] = out.d;
}

// ---------------------------------------------------------------------
// Plan: per-stream validation + block table.  One workgroup of 1024 threads
// walks the streams 1024 at a time with the workgroup scan of
// snapmi_scan.hpp (as every scan below: what a kernel names is what it loads
// and stores).
// Reference checks: src/compress.rs:104-125.
// ---------------------------------------------------------------------
namespace {
// blocks of stream i, or 0 for a stream that is rejected, empty or tiny
// (reference src/compress.rs:104-125)
__device__ __forceinline__ uint32_t plan_blocks(const CompressArgs &a,
                                                uint32_t i, bool report)
{
    const uint64_t len = a.in_lens[i];
    const uint64_t need = max_compress_len_u64(len);
    if (report)
        a.out_lens[i] = 0;
    if (need == 0) {
        if (report)
            set_error(a.errs, i, SNAPMI_TOO_BIG, len, kMaxInput, 0);
        return 0;
    }
    if (a.out_caps && a.out_caps[i] < need) {
        if (report)
            set_error(a.errs, i, SNAPMI_BUFFER_TOO_SMALL, a.out_caps[i], need,
                      0);
        return 0;
    }
    if (len == 0) { // src/compress.rs:120-125
        if (report) {
            ((gptr)a.out_ptrs[i])[0] = 0;
            a.out_lens[i] = 1;
            set_error(a.errs, i, SNAPMI_OK, 0, 0, 0);
        }
        return 0;
    }
    if (report)
        set_error(a.errs, i, SNAPMI_OK, 0, 0, 0);
    if (len < a.small_limit)
        return 0; // k_compress_tiny's / _small's: no blocks, they write out_lens
    return (uint32_t)((len + kMaxBlock - 1) / kMaxBlock);
}
// item i of the planner's scan: its blocks and its scratch slots
__device__ __forceinline__ void plan_load(const CompressArgs &a, uint32_t i,
                                          uint32_t (&x)[2])
{
    x[0] = plan_blocks(a, i, true);
    x[1] = x[0] ? x[0] - 1 : 0;
}
// ... and where they start.  The launch was sized from the host's copy of
// the lengths; a stream that does not fit in it is rejected, never overrun.
__device__ __forceinline__ void plan_store(const CompressArgs &a, uint32_t i,
                                           uint32_t nb, uint32_t fb,
                                           uint32_t fs)
{
    if (nb && !(blocks_fit(a, fb, nb) && slots_fit(a, fs, nb)))
        set_error(a.errs, i, SNAPMI_E_ARGUMENT, a.in_lens[i], 0, 0);
    a.blk_first[i] = fb;
    a.slot_first[i] = fs;
}
} // namespace

__global__ __launch_bounds__(1024) void k_plan_compress(CompressArgs a)
{
    uint32_t carry[2] = {0, 0};
    wg_scan_strided(
        a.n_streams, carry,
        [&](uint32_t i, uint32_t (&x)[2]) { plan_load(a, i, x); },
        [&](uint32_t i, const uint32_t (&x)[2], const uint32_t (&ex)[2]) {
            plan_store(a, i, x[0], ex[0], ex[1]);
        });
    if (threadIdx.x == 0) {
        a.blk_first[a.n_streams] = carry[0];
        a.slot_first[a.n_streams] = carry[1];
    }
}

// Exclusive scan of blk_size (u32) into blk_off (u64) over the blocks
// [blk_lo, blk_hi), one workgroup; blk_off[blk_lo] carries over from the
// segment in front.
__global__ __launch_bounds__(1024) void k_scan_sizes(CompressArgs a)
{
    const uint32_t nblocks = segment_blocks(a);
    uint64_t carry[1] = {a.blk_lo ? a.blk_off[a.blk_lo] : 0};
    __syncthreads(); // (blk_off[blk_lo] is rewritten below)
    wg_scan_strided(
        nblocks > a.blk_lo ? nblocks - a.blk_lo : 0, carry,
        [&](uint32_t i, uint64_t (&x)[1]) { x[0] = a.blk_size[a.blk_lo + i]; },
        [&](uint32_t i, const uint64_t (&)[1], const uint64_t (&ex)[1]) {
            a.blk_off[a.blk_lo + i] = ex[0];
        });
    if (threadIdx.x == 0 && nblocks >= a.blk_lo)
        a.blk_off[nblocks] = carry[0];
}

// ---------------------------------------------------------------------
// The same two scans on many workgroups, for batches of many streams /
// blocks (10.7 M streams of 200 bytes: the one-workgroup kernels above took
// 27.8 ms and 41 x 0.46 ms of a 104 ms pass).  Three launches each, the
// halves of snapmi_scan.hpp: (a) wg_scan_a, (b) wg_scan_b, (c) wg_scan_c.
// ---------------------------------------------------------------------
__global__ __launch_bounds__(1024) void k_plan_compress_a(CompressArgs a)
{
    wg_scan_a<uint32_t, 2>(
        a.n_streams, a.plan_part,
        [&](uint32_t i, uint32_t (&x)[2]) { plan_load(a, i, x); },
        [&](uint32_t i, const uint32_t (&)[2], const uint32_t (&ex)[2]) {
            a.blk_first[i] = ex[0]; // within this workgroup, for now
            a.slot_first[i] = ex[1];
        });
}

__global__ __launch_bounds__(1024) void k_plan_compress_b(CompressArgs a,
                                                          uint32_t nparts)
{
    uint32_t carry[2] = {0, 0};
    wg_scan_b(a.plan_part, nparts, carry);
    if (threadIdx.x == 0) {
        a.blk_first[a.n_streams] = carry[0];
        a.slot_first[a.n_streams] = carry[1];
    }
}

__global__ __launch_bounds__(1024) void k_plan_compress_c(CompressArgs a)
{
    wg_scan_c<uint32_t, 2>(
        a.n_streams, a.plan_part,
        [&](uint32_t i, const uint32_t (&off)[2]) {
            // (its own loads first: they are in flight beside plan_blocks')
            const uint32_t fb = a.blk_first[i] + off[0];
            const uint32_t fs = a.slot_first[i] + off[1];
            plan_store(a, i, plan_blocks(a, i, false), fb, fs);
        });
}

// scan_part[0, nparts): workgroup totals, then offsets; scan_part[nparts]: the
// carry from the segment in front (blk_off[blk_lo] before it is rewritten)
__global__ __launch_bounds__(1024) void k_scan_sizes_a(CompressArgs a,
                                                       uint32_t nparts)
{
    const uint32_t nblocks = segment_blocks(a);
    if (blockIdx.x == 0 && threadIdx.x == 0)
        a.scan_part[nparts] = a.blk_lo ? a.blk_off[a.blk_lo] : 0;
    __syncthreads();
    wg_scan_a<uint64_t, 1>(
        nblocks > a.blk_lo ? nblocks - a.blk_lo : 0, (uint64_t *)a.scan_part,
        [&](uint32_t i, uint64_t (&x)[1]) { x[0] = a.blk_size[a.blk_lo + i]; },
        [&](uint32_t i, const uint64_t (&)[1], const uint64_t (&ex)[1]) {
            a.blk_off[a.blk_lo + i] = ex[0];
        });
}

__global__ __launch_bounds__(1024) void k_scan_sizes_b(CompressArgs a,
                                                       uint32_t nparts)
{
    const uint32_t nblocks = segment_blocks(a);
    uint64_t carry[1] = {a.scan_part[nparts]};
    wg_scan_b((uint64_t *)a.scan_part, nparts, carry);
    if (threadIdx.x == 0 && nblocks >= a.blk_lo)
        a.blk_off[nblocks] = carry[0];
}

__global__ __launch_bounds__(1024) void k_scan_sizes_c(CompressArgs a)
{
    const uint32_t nblocks = segment_blocks(a);
    wg_scan_c<uint64_t, 1>(
        nblocks > a.blk_lo ? nblocks - a.blk_lo : 0,
        (const uint64_t *)a.scan_part,
        [&](uint32_t i, const uint64_t (&off)[1]) {
            a.blk_off[a.blk_lo + i] += off[0];
        });
}

// Direct encoding (k_encode_tokens wrote every block at its final position):
// what is left of k_compact is the compressed length of every stream.
__global__ __launch_bounds__(256) void k_stream_lens(CompressArgs a)
{
    const uint32_t st = blockIdx.x * 256 + threadIdx.x;
    if (st >= a.n_streams)
        return;
    const uint32_t first = a.blk_first[st];
    const uint32_t nb = a.blk_first[st + 1] - first;
    if (nb == 0 || !blocks_fit(a, first, nb))
        return; // empty, in error or rejected: k_plan_compress wrote out_lens
    a.out_lens[st] = varint_len(a.in_lens[st]) +
                     (a.blk_off[first + nb] - a.blk_off[first]);
}

// ---------------------------------------------------------------------
// K3: move blocks 1.. of every stream from their scratch slot to
// out_ptrs[st] + varint + sum(size of earlier blocks); block 0's workgroup
// publishes the stream's compressed length.
// ---------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_compact(CompressArgs a)
{
    const uint32_t b = blockIdx.x;
    if (b >= launch_blocks(a))
        return;
    const BlockAt at = locate_block(a, b);
    const uint32_t st = at.st, k = at.k;
    const uint32_t first = a.blk_first[st];
    const uint64_t total = at.total;
    const uint32_t vl = varint_len(total);
    const uint32_t nb = (uint32_t)stream_blocks(total);
    // (the plan's own test, blocks AND slots of the whole stream, not
    // block_dest's of this block's slot: its out_lens stays 0, nothing moves)
    if (!(blocks_fit(a, first, nb) && slots_fit(a, a.slot_first[st], nb)))
        return; // rejected by k_plan_compress (E_ARGUMENT)
    if (k == 0) {
        if (threadIdx.x == 0)
            a.out_lens[st] = vl + (a.blk_off[first + nb] - a.blk_off[first]);
        return;
    }
    gcptr from = (gcptr)a.scratch +
                 (uint64_t)(a.slot_first[st] + k - 1) * kSlotBytes;
    gptr to = (gptr)a.out_ptrs[st] + vl + (a.blk_off[b] - a.blk_off[first]);
    const uint32_t size = a.blk_size[b];
    // align the destination to 16 bytes, then 16-byte stores fed by
    // unaligned 16-byte loads (the slot is 16-aligned, `to` is arbitrary).
    uint32_t head = (uint32_t)((16 - ((uintptr_t)to & 15)) & 15);
    if (head > size)
        head = size;
    if (threadIdx.x < head)
        to[threadIdx.x] = from[threadIdx.x];
    const uint32_t body = (size - head) & ~15u;
    for (uint32_t i = 16 * threadIdx.x; i < body; i += 16 * blockDim.x) {
        u32x4 v;
        __builtin_memcpy(&v, from + head + i, 16);
        *(__attribute__((address_space(1))) u32x4 *)(to + head + i) = v;
    }
    const uint32_t tail = size - head - body;
    if (threadIdx.x < tail)
        to[head + body + threadIdx.x] = from[head + body + threadIdx.x];
}

} // namespace snapmi
