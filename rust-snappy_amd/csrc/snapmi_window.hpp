// snapmi_window.hpp -- the window match finder: one wavefront compresses one
// block, a WINDOW of 63 consecutive positions per step
// (compress_one_block_span, with TokenWriter and the token pool's pages, and
// WaveDev, the wave of snapmi_span.hpp's walk on the hardware).  A header: the
// window kernels (snapmi_window.hip) and k_match_both's window wavefronts
// (snapmi_lane.hip) run the same body.
// The one-copy-per-step kernel of rounds 1-3 (k_compress_blocks,
// snapmi_steps.hip: the test build's cross-check) pays one LDS atomic, one
// candidate gather and one ballot per emitted copy (~2 100 cycles, ~10 000
// copies per 64 KiB of text).  Here
// a step fetches what the table holds and how many bytes match for EVERY
// position of a 63-byte window - whether the parse will look them up or not -
// and the sequential part of the reference (which positions are looked up,
// which are inserted: src/compress.rs:195-317) becomes a walk over results
// that are already in registers: span_walk (snapmi_span.hpp, the text
// tests/test_span_wave_cpu.py runs on the host, byte for byte).  Nine
// copies per step on text, ~1 100 steps per block instead of ~10 000.
//   * lane L holds position s - 1 + L; ONE lane-ordered ds_mskor_rtn_b32
//     writes every position of the window into the table and returns what was
//     there - the reference's candidate, or the position of a lower lane with
//     the same hash ("C bit");
//   * one gather of the 16 bytes at every candidate, one compare: hit mask
//     and match lengths of the whole window;
//   * the walk (scalar unit: ~15 instructions per copy) marks the positions
//     the reference really inserts; one lane-ordered ds_mskor_b32 then puts
//     every slot right (touched lanes write their position, untouched lanes
//     without a C bit give back what they displaced);
//   * a run of more than 32 misses continues with k_compress_blocks' schedule
//     step (64 probes of the growing stride per step, first hit wins); a match
//     of 16 bytes or more is finished by extend_match.
// Persistent five-wave workgroups, one 32 KiB table a wavefront, TokenSink as
// the token encoder; kLds: the input block in LDS too (k_compress_span_lds).
#pragma once

#include <type_traits>

#include "snapmi_compress_dev.hpp"
#include "snapmi_span.hpp"

namespace snapmi {

namespace {
// The window kernel as a MATCH FINDER for k_encode_tokens (k_match_spans):
// tokens leave in that kernel's format (four bytes each and an exception
// list, snapmi_kernels.hpp) and what they will encode to is added up
// (token_bytes) - so that,
// as behind k_match_blocks, every block's size is known before a byte
// of it is written and the encoder can put it at its final position (no
// scratch slots, no k_compact).  Round 5: a step's tokens are stored by the
// lanes that found them, at their rank among the step's copies - no push into
// a token register (two ds_permute and their round trip per step), no flush:
// one predicated 8-byte store and a per-lane sum of sizes.
// How the match finders come by the pages of the token pool
// (CompressArgs::tok_pool).  Both are bound by the latency of their own
// dependent chains, and an atomic on the pool's one counter whose result is
// waited for where a page starts is one more link - for a whole wavefront,
// every 512 tokens of any of its lanes (the first form of this: + 6 % on
// k_match_both at cfg2).
//  - a window wavefront stages a block's tokens and moves them into pages at
//    the block's end (tok_commit_wave);
//  - a LANE has a page in hand; the lanes of a wavefront that have used
//    theirs get new ones where the round loop is convergent (its top), from a
//    run of kTokRun pages that the wavefront takes with one atomic, waited
//    for, every 32 pages (match_blocks).
// A lane's page in hand passes from block to block; a launch leaves a page or
// two per lane unused.
constexpr uint32_t kTokRun = 32, kNoPage = 0xFFFFFFFFu;
__device__ __forceinline__ uint32_t tok_page_ask(const CompressArgs &a)
{
    return atomicAdd(&a.tok_ctl[0], 1u);
}
// a lane's page in hand `spare` becomes slot `slot` of block b's page table
// - or, the pool having run out, the block is put on the spill list and gets
// the dump page.  `spilled`: it is on the list already.
__device__ __forceinline__ uint32_t tok_page_take(const CompressArgs &a,
                                                  uint32_t b, uint32_t slot,
                                                  uint32_t &spare,
                                                  bool &spilled)
{
    if (!spilled) {
        uint32_t p = spare;
        spare = kNoPage;
        // (the second page of one round - a token page and an exception
        // page, rare: asked for and waited for here)
        if (p == kNoPage)
            p = tok_page_ask(a);
        if (p < a.tok_pool_pages) {
            a.tok_pages[(uint64_t)(b - a.tok_base) * kPageTabStride + slot] =
                p;
            return p;
        }
        spilled = true;
        a.tok_ctl[kTokCtlList + atomicAdd(&a.tok_ctl[1], 1u)] = b;
    }
    return a.tok_pool_pages;
}

// ... for a window wavefront, whose step is bound by the instructions it
// issues and has no scalar register to spare (a comparison per step and a
// rarely taken branch for "this step opens a page" cost k_match_spans 11 %,
// in seven forms): the wavefront writes a block's tokens into a STAGING array
// of its own, as it did when every block had one, and at the block's end
// tok_commit_wave moves them into pages - as many as they need, consecutive,
// taken with one atomic.  Out of line, its arguments the fields it needs (a
// reference to the kernel's argument block would make the kernel keep a copy
// of it in scratch memory).  Returns what goes into CompressArgs::ntok.
__device__ __noinline__ uint32_t tok_commit_wave(
    const uint32_t *stage, uint32_t ntok, uint32_t nexc, uint32_t *ctl,
    uint32_t *tab, uint32_t *pool, uint32_t pool_pages, uint32_t b,
    uint32_t lane)
{
    typedef __attribute__((address_space(1))) unsigned long long g_u64;
    const uint32_t tp = (ntok + kTokPage - 1) / kTokPage,
                   ep = (nexc + kExcPage - 1) / kExcPage;
    uint32_t base = 0;
    if (lane == 0) {
        base = atomicAdd(&ctl[0], tp + ep);
        if (base + tp + ep > pool_pages) {
            ctl[kTokCtlList + atomicAdd(&ctl[1], 1u)] = b;
            base = kNoPage;
        }
    }
    base = uni(base);
    if (base == kNoPage)
        return kTokSpilled;
    if (lane < tp)
        tab[lane] = base + lane;
    if (lane < ep)
        tab[kTokPagesPerBlock + lane] = base + tp + lane;
    // (the wavefront's own stores of this block, read back: loads that see
    // the L2, where the atomic above has waited for them to arrive)
    const g_u64 *from = (const g_u64 *)stage;
    g_u64 *to = (g_u64 *)(pool + (uint64_t)base * kTokPage);
    const uint32_t words = (ntok + 1) / 2;
    for (uint32_t i = lane; i < words; i += 4 * kWave) {
        unsigned long long v0 = 0, v1 = 0, v2 = 0, v3 = 0;
        v0 = __hip_atomic_load(from + i, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
        if (i + kWave < words)
            v1 = __hip_atomic_load(from + i + kWave, __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
        if (i + 2 * kWave < words)
            v2 = __hip_atomic_load(from + i + 2 * kWave, __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
        if (i + 3 * kWave < words)
            v3 = __hip_atomic_load(from + i + 3 * kWave, __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
        to[i] = v0;
        if (i + kWave < words)
            to[i + kWave] = v1;
        if (i + 2 * kWave < words)
            to[i + 2 * kWave] = v2;
        if (i + 3 * kWave < words)
            to[i + 3 * kWave] = v3;
    }
    const g_u64 *efrom = (const g_u64 *)(stage + kMaxTokens);
    g_u64 *eto = (g_u64 *)(pool + (uint64_t)(base + tp) * kTokPage);
    for (uint32_t i = lane; i < nexc; i += kWave)
        eto[i] = __hip_atomic_load(efrom + i, __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
    return ntok;
}

struct TokenWriter {
    typedef __attribute__((address_space(1))) uint32_t g_u32;
    typedef __attribute__((address_space(1))) unsigned long long g_u64;
    g_u32 *tok;    // the wavefront's staging array: this block's tokens
    g_u64 *exc;    // ... and its exception list (tok_commit_wave)
    uint32_t ntok; // tokens stored so far (uniform)
    uint32_t nexc; // exceptions stored so far (uniform)
    uint32_t dsum; // encoded bytes of the tokens THIS LANE stored
    uint32_t d;    // finish(): encoded bytes of the block (uniform)
    uint32_t t;    // always 0 (TokenSink's interface: nothing is pending)
    uint32_t lane;

    __device__ __forceinline__ void init(const CompressArgs &a, uint32_t l)
    {
        tok = (g_u32 *)a.tok_stage +
              (uint64_t)uni(blockIdx.x * a.tok_stage_waves +
                            (threadIdx.x >> 6) - a.tok_stage_wave0) *
                  kTokStageWords;
        exc = (g_u64 *)(tok + kMaxTokens);
        ntok = 0;
        nexc = 0;
        dsum = 0;
        d = 0;
        t = 0;
        lane = l;
    }
    // the block's end: its tokens into pages; what goes into
    // CompressArgs::ntok
    __device__ __forceinline__ uint32_t commit(const CompressArgs &a,
                                               uint32_t b) const
    {
        return tok_commit_wave(
            (const uint32_t *)tok, ntok, nexc, a.tok_ctl,
            a.tok_pages + (uint64_t)(b - a.tok_base) * kPageTabStride,
            a.tok_pool, a.tok_pool_pages, b, lane);
    }
    // one token, the same in every lane
    __device__ __forceinline__ void record_nf(uint32_t lit_start,
                                              uint32_t lit_len,
                                              uint32_t offset,
                                              uint32_t copy_len)
    {
        (void)lit_start; // (k_encode_tokens adds the lengths up)
        const bool fits = tok_fits(lit_len, copy_len);
        if (lane == 0) {
            tok[ntok] = tok_pack(lit_len, copy_len, offset);
            if (!fits)
                exc[nexc] = tok_pack64(lit_len, copy_len, offset);
            dsum += token_bytes(lit_len, copy_len, offset);
        }
        ntok++;
        nexc += fits ? 0u : 1u;
    }
    // the copies of a window step: lane `mine` holds the rank-th of cnt
    // tokens, a copy of 4..15 bytes (one element: src/compress.rs:339-356).
    // Only the step's FIRST copy can come behind a literal of 1 024 bytes or
    // more (the literals between a window's copies are shorter than the
    // window): at most one exception per step, `first_long` (uniform) says so.
    __device__ __forceinline__ void put_step(bool mine, uint32_t rank,
                                             uint32_t cnt, uint32_t lit_len,
                                             uint32_t copy_len,
                                             uint32_t offset)
    {
        const bool big = mine && lit_len > 1023u;
        if (mine)
            tok[ntok + rank] = tok_pack(lit_len, copy_len, offset);
        if (big)
            exc[nexc] = tok_pack64(lit_len, copy_len, offset);
        const uint32_t lt =
            lit_len == 0 ? 0 : (lit_len <= 60 ? 1 : (lit_len <= 256 ? 2 : 3));
        const uint32_t fin = copy_len <= 11 && offset <= 2047 ? 2 : 3;
        dsum += mine ? lt + lit_len + fin : 0;
        ntok += cnt;
        nexc += __builtin_amdgcn_ballot_w64(big) ? 1u : 0u;
    }
    __device__ __forceinline__ void flush() {}
    __device__ __forceinline__ void finish()
    {
        d = rdlane(wave_inclusive_scan(dsum), kWave - 1);
    }
};
struct SpanLanes {
    uint32_t mv, ov; // this lane's match length and exchanged table entry
    __device__ __forceinline__ uint32_t m(uint32_t l) const
    {
        return rdlane(mv, l);
    }
    __device__ __forceinline__ uint32_t old(uint32_t l) const
    {
        return rdlane(ov, l);
    }
};
template <class OUT> struct SpanSink {
    OUT *out;
    uint32_t emit; // where the pending literal starts
    __device__ __forceinline__ void token(uint32_t lit, uint32_t len,
                                          uint32_t off)
    {
        out->record_nf(emit, lit, off, len);
        emit += lit + len;
    }
};

// the wave of span_par_walk (snapmi_span.hpp) on the hardware
struct WaveDev {
    typedef uint32_t u32;
    typedef bool b1;
    uint32_t l;
    __device__ __forceinline__ u32 lane() const { return l; }
    __device__ __forceinline__ void count_cut() const {}
    __device__ __forceinline__ u32 sel(b1 c, u32 a, u32 b) const
    {
        return c ? a : b;
    }
    __device__ __forceinline__ b1 lt(u32 a, u32 b) const { return a < b; }
    __device__ __forceinline__ b1 ge(u32 a, u32 b) const { return a >= b; }
    __device__ __forceinline__ b1 eq(u32 a, u32 b) const { return a == b; }
    __device__ __forceinline__ b1 band(b1 a, b1 b) const { return a & b; }
    __device__ __forceinline__ b1 bor(b1 a, b1 b) const { return a | b; }
    __device__ __forceinline__ b1 bnot(b1 a) const { return !a; }
    __device__ __forceinline__ uint64_t ballot(b1 a) const
    {
        return __builtin_amdgcn_ballot_w64(a);
    }
    __device__ __forceinline__ u32 bperm(u32 idx, u32 v) const
    {
        return (u32)__builtin_amdgcn_ds_bpermute((int)(idx << 2), (int)v);
    }
    __device__ __forceinline__ uint32_t readlane(u32 v, uint32_t i) const
    {
        return rdlane(v, i);
    }
    __device__ __forceinline__ b1 bit(uint64_t mask, u32 i) const
    {
        return ((uint32_t)(mask >> i) & 1u) != 0;
    }
    __device__ __forceinline__ u32 next_bit(uint64_t mask, u32 t) const
    {
        const uint64_t x = mask >> t;
        return x ? t + (u32)__builtin_ctzll(x) : 64u;
    }
    __device__ __forceinline__ u32 prev_bit(uint64_t mask, u32 t) const
    {
        const uint64_t x = mask & ((1ull << t) - 1);
        return x ? 63u - (u32)__builtin_clzll(x) : 64u;
    }
    __device__ __forceinline__ u32 shr_lo(uint64_t mask, u32 i) const
    {
        return (u32)(mask >> i);
    }
};

template <bool kLds, bool kTok = false>
__device__ __forceinline__ void compress_one_block_span(
    const CompressArgs &a, const uint32_t b, const uint32_t lane,
    const lptr16 table, const uint32_t tbase,
    __attribute__((address_space(3))) uint8_t *lblock = nullptr,
    const uint32_t tcap = kMaxTable)
{
    // locate_block(a, b) of snapmi_block.hpp, written out: the call moves
    // three kernels' VGPR counts (profiles/compress_split_resources.md)
    uint32_t lo_s = 0, hi_s = a.n_streams;
    if (b < a.n_streams && a.blk_first[b] == b && a.blk_first[b + 1] > b) {
        lo_s = b;
        hi_s = b + 1;
    }
    while (hi_s - lo_s > 1) {
        const uint32_t mid = (lo_s + hi_s) >> 1;
        if (a.blk_first[mid] <= b)
            lo_s = mid;
        else
            hi_s = mid;
    }
    const uint32_t st_i = lo_s;
    const uint32_t k = b - a.blk_first[st_i];
    const uint64_t total = a.in_lens[st_i];
    const uint64_t boff = (uint64_t)k * kMaxBlock;
    const void *const in = a.in_ptrs[st_i];
    gcptr src = (gcptr)in + boff;
    const uint64_t avail = total - boff;
    const uint32_t n = avail < kMaxBlock ? (uint32_t)avail : kMaxBlock;
    const BlockAt at{st_i, k, total, in, n};
    if (n <= a.cls_lo || n > a.cls_hi)
        return; // another launch's block (CompressArgs::cls_lo)

    typename std::conditional<kTok, TokenWriter, TokenSink>::type out;
    if constexpr (kTok) {
        // match finder only: tokens for k_encode_tokens (which also writes
        // the varint of block 0)
        out.init(a, lane);
    } else {
        // (a.direct: k_redo_spilled behind a lane-kernel batch - the sizes of
        // the blocks in front are known, as in k_encode_tokens)
        gptr dst;
        if (!block_dest(a, at, b, lane == 0, dst))
            return; // stream rejected by k_plan_compress (E_ARGUMENT)
        out.init(src, n, dst, lane);
    }
    if (n < kMinNonLiteral) { // src/compress.rs:140-146
        out.record_nf(0, n, 0, 0);
        if constexpr (kTok)
            out.finish();
        else
            out.flush();
        uint32_t count = 0;
        if constexpr (kTok)
            count = out.commit(a, b);
        if (lane == 0) {
            a.blk_size[b] = out.d;
            if constexpr (kTok)
                a.ntok[b] = count;
        }
        return;
    }
    typename std::conditional<kLds, lcptr, gcptr>::type msrc;
    if constexpr (kLds) {
        typedef __attribute__((address_space(3))) u32x4 l_u32x4;
        typedef __attribute__((address_space(1))) u32x4 g_u32x4c;
        const uint32_t mis = (uint32_t)(uintptr_t)src & 15u;
        l_u32x4 *to = (l_u32x4 *)lblock;
        const g_u32x4c *from = (const g_u32x4c *)(src - mis);
        const uint32_t lines = (n + mis + 15) / 16;
        for (uint32_t i = lane; i < lines; i += kWave)
            to[i] = from[i];
        __builtin_amdgcn_wave_barrier();
        msrc = (lcptr)lblock + mis;
    } else {
        msrc = src;
    }
    // table sizing + zero fill: src/compress.rs:491-518
    // (tcap: the entries this kernel's table has room for - kMaxTable, or the
    // 8 192 of the small-block kernel, whose class never needs more)
    // table_shift(n, tcap) of snapmi_block.hpp, written out for the same reason
    uint32_t shift = 32 - 8, tsize = 256;
    while (tsize < tcap && tsize < n) {
        shift--;
        tsize *= 2;
    }
    for (uint32_t i = 8 * lane; i < tsize; i += 8 * kWave)
        *(__attribute__((address_space(3))) u32x4 *)&table[i] =
            (u32x4){0, 0, 0, 0};
    __builtin_amdgcn_wave_barrier();

    const uint32_t s_limit = n - kInputMargin;
    const uint32_t n16 = n - 16, n4 = n - 4;
    SpanState st;
    st.s = 1;
    st.q = 0;
    st.chain = 0;
    st.next_emit = 0;
    uint32_t run0 = 1; // schedule steps: where the run began
    uint32_t dq = ~0u, d0 = 0, d1 = 0; // kDelta.d[dq + lane], [dq + lane + 1]
    // Register window of the input for the hashes (global input only): lane l
    // of wv[j] holds the dword at block offset wbase + 64 j + l; five
    // registers, so that a step may move s by up to 128 positions and the
    // next step's hash inputs are still a lane rotation (ds_bpermute) of
    // registers that arrived long ago.
    uint32_t wbase = 0, wv0 = 0, wv1 = 0, wv2 = 0, wv3 = 0, wv4 = 0;
    if constexpr (!kLds) {
        wv0 = ld32u(msrc + (lane < n4 ? lane : n4));
        wv1 = ld32u(msrc + (lane + 64 < n4 ? lane + 64 : n4));
        wv2 = ld32u(msrc + (lane + 128 < n4 ? lane + 128 : n4));
        wv3 = ld32u(msrc + (lane + 192 < n4 ? lane + 192 : n4));
        wv4 = ld32u(msrc + (lane + 256 < n4 ? lane + 256 : n4));
    }
    SpanSink<decltype(out)> sink;
    sink.out = &out;
    sink.emit = 0;
    PROF(
    uint64_t pt[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    uint64_t t_last = __builtin_readcyclecounter();
    uint64_t n_batches = 0, n_copies = 0;
    )
    for (;;) {
        PROF(
        n_batches++;
        )
        TICK(0);
        // room for a step's tokens (at most 16 copies of a window + a long
        // match): the one place where tokens are encoded
        if constexpr (!kTok) {
            if (out.t + 17 > kWave)
                out.flush();
        }
        if (!st.chain && st.q >= kSpanRun) {
            // ---- schedule step (k_compress_blocks' batch for q > 0): lane l
            // is probe q + l of the run that began at run0
            // (this lane's two schedule entries were requested one step
            // ahead: a run of misses goes on with q + 64, and a load from the
            // table costs a step of incompressible data a fifth of its time)
            if (dq != st.q) {
                d0 = kDelta.d[st.q + lane];
                d1 = kDelta.d[st.q + lane + 1];
            }
            const uint32_t p = run0 + d0;
            const uint32_t nextp = run0 + d1;
            {
                const uint32_t qn = st.q + kWave + lane;
                d0 = kDelta.d[qn < 446 ? qn : 446];
                d1 = kDelta.d[qn < 446 ? qn + 1 : 447];
                dq = st.q + kWave;
            }
            const bool valid = nextp <= s_limit; // src/compress.rs:212-214
            const B16 x = ld128u(msrc + (p < n16 ? p : n16));
            const uint32_t h = hash32(x.w[0], shift);
            uint32_t cand = 0;
            if (valid) {
                const uint32_t sh = (h & 1) * 16;
                const uint32_t old = lds_mskor_rtn(tbase + (h >> 1) * 4,
                                                   0xFFFFu << sh, p << sh);
                cand = (old >> sh) & 0xFFFFu;
            }
            const B16 y = ld128u(msrc + cand);
            const uint32_t m = common16(x, y);
            const uint64_t hits = __ballot(valid && m >= 4 && cand < p);
            if (hits == 0) {
                if (__ballot(!valid) != 0)
                    break;
                st.q += kWave;
                continue;
            }
            const uint32_t kh = (uint32_t)__builtin_ctzll(hits);
            const uint32_t pk = rdlane(p, kh);
            const uint32_t ck = rdlane(cand, kh);
            uint32_t len = rdlane(m, kh);
            if (valid && lane > kh && cand <= pk)
                table[h] = (uint16_t)cand;
            if (len == 16)
                len += extend_match(msrc, n, ck + 16, pk + 16, lane);
            sink.token(pk - sink.emit, len, pk - ck);
            PROF(
            n_copies++;
            )
            st.s = pk + len;
            st.next_emit = st.s;
            st.chain = 1;
            st.q = 0;
            if (st.s >= s_limit) // src/compress.rs:275-277
                break;
        } else {
            // ---- window step: lane L = position s - 1 + L
            const uint32_t base = st.s;
            const uint32_t lo = base - st.chain; // first position exchanged
            const uint32_t P = base - 1 + lane;
            const bool active = lane ? P <= n16 : st.chain != 0;
            uint32_t hx;
            if constexpr (kLds) {
                hx = ld32u(msrc + (P < n4 ? P : n4));
            } else {
                const uint32_t idx = base - 1 - wbase + lane; // < 128
                const int sel = (int)((idx & 63) << 2);
                const uint32_t g0 =
                    (uint32_t)__builtin_amdgcn_ds_bpermute(sel, (int)wv0);
                const uint32_t g1 =
                    (uint32_t)__builtin_amdgcn_ds_bpermute(sel, (int)wv1);
                hx = idx < 64 ? g0 : g1;
            }
            const B16 x = ld128u(msrc + (P < n16 ? P : n16));
            TICK(1);
            const uint32_t h = hash32(hx, shift);
            const uint32_t sh = (h & 1) * 16;
            const uint32_t taddr = tbase + (h >> 1) * 4;
            uint32_t old = 0;
            if (active)
                old = (lds_mskor_rtn(taddr, 0xFFFFu << sh, P << sh) >> sh) &
                      0xFFFFu;
            TICK(2);
            const B16 y = ld128u(msrc + old);
            TICK(3);
            SpanLanes ln;
            ln.mv = common16(x, y);
            ln.ov = old;
            const bool cbit = active && old >= lo;
            const uint64_t hits = __builtin_amdgcn_ballot_w64(
                active && lane && ln.mv >= 4);
            const uint64_t cbits = __builtin_amdgcn_ballot_w64(cbit);
            uint64_t touched = 0;
            uint32_t at = 0, rc = kSpanCont;
            st.next_emit = sink.emit;
            // the fast walk (snapmi_span.hpp): the scalar unit follows the
            // chain of copies, the lanes derive everything else at once
            const WaveDev w{lane};
            bool fast = span_fast_ok_w(w, st, hits, n);
            TICK(13);
            if (fast) {
                // the lane-parallel walk (span_par_walk): the copies of the
                // step by pointer jumping, everything else per lane
                uint64_t vh;
                uint32_t lit;
                rc = span_par_walk(w, st, hits, ln.mv, old, cbit, sink.emit,
                                   vh, lit, touched, at);
                TICK(14);
                const uint32_t cnt = (uint32_t)__builtin_popcountll(vh);
                if (cnt) {
                    const uint32_t rank = __builtin_amdgcn_mbcnt_hi(
                        (uint32_t)(vh >> 32),
                        __builtin_amdgcn_mbcnt_lo((uint32_t)vh, 0));
                    const bool is_vh = (vh >> lane) & 1;
                    if constexpr (kTok) {
                        out.put_step(is_vh, rank, cnt, lit, ln.mv, P - old);
                    } else {
                        // token of lane X goes to sink lane t + rank: a push
                        // (ds_permute); the other lanes push to a lane
                        // outside [t, t + cnt) whose value is not taken
                        const uint32_t to =
                            is_vh ? out.t + rank : (out.t + cnt) & 63u;
                        const uint32_t ta =
                            (lit & 0xFFFFu) | ((P - old) << 16);
                        const uint32_t tb = ln.mv | ((P - lit) << 16);
                        const uint32_t ra =
                            (uint32_t)__builtin_amdgcn_ds_permute(
                                (int)(to << 2), (int)ta);
                        const uint32_t rb =
                            (uint32_t)__builtin_amdgcn_ds_permute(
                                (int)(to << 2), (int)tb);
                        const bool got = lane - out.t < cnt;
                        out.a = got ? ra : out.a;
                        out.b = got ? rb : out.b;
                        out.t += cnt;
                    }
                }
            }
            if (!fast)
                rc = span_walk(st, hits, cbits, s_limit, ln, sink, touched,
                               at);
            TICK(4);
            // the table as the reference leaves it: one lane-ordered store
            {
                const bool t = (touched >> lane) & 1;
                if (active && (t || !cbit))
                    lds_mskor(taddr, 0xFFFFu << sh, (t ? P : old) << sh);
            }
            TICK(5);
            if (rc == kSpanLong) {
                const uint32_t pk = st.s, ck = rdlane(old, at);
                // (requesting the next 16 bytes of every 16-byte match under
                // the walk, so that a long match is measured to 32 bytes
                // without this round trip, was built and measured: 8 % SLOWER
                // on text and HTML alike - profiles/r5_span_ablations.txt)
                const uint32_t len =
                    16 + extend_match(msrc, n, ck + 16, pk + 16, lane);
                sink.token(pk - sink.emit, len, pk - ck);
                st.s = pk + len;
                st.chain = 1;
                st.q = 0;
                if (st.s >= s_limit)
                    break;
            } else if (rc == kSpanDone) {
                break;
            } else if (!st.chain && st.q >= kSpanRun) {
                run0 = st.s - st.q;
            }
            TICK(6);
        }
        // keep the register window covering s - 1 .. s + 126
        if constexpr (!kLds) {
            // (ONE slide per step and its load straight into wv4: a loop
            // here is unrolled by the compiler into register rotations that
            // wait for the load they have just issued - a memory round trip
            // per step, 770 of a step's 4 800 cycles in round 4's kernel.  A
            // step that went further - behind a long match - reloads)
            const uint32_t D = st.s - 1 - wbase;
            if (D >= 128) {
                wbase = st.s - 1;
                const uint32_t w0 = wbase + lane;
                wv0 = ld32u(msrc + (w0 < n4 ? w0 : n4));
                wv1 = ld32u(msrc + (w0 + 64 < n4 ? w0 + 64 : n4));
                wv2 = ld32u(msrc + (w0 + 128 < n4 ? w0 + 128 : n4));
                wv3 = ld32u(msrc + (w0 + 192 < n4 ? w0 + 192 : n4));
                wv4 = ld32u(msrc + (w0 + 256 < n4 ? w0 + 256 : n4));
            } else if (D >= 64) {
                wv0 = wv1;
                wv1 = wv2;
                wv2 = wv3;
                wv3 = wv4;
                wbase += 64;
                const uint32_t wp = wbase + 256 + lane;
                wv4 = ld32u(msrc + (wp < n4 ? wp : n4));
            }
        }
        TICK(7);
    }
    if (sink.emit < n) // done(): src/compress.rs:417-426
        out.record_nf(sink.emit, n - sink.emit, 0, 0);
    if constexpr (kTok) {
        out.finish();
    } else {
        if (out.t)
            out.flush();
    }
    uint32_t count = 0;
    if constexpr (kTok)
        count = out.commit(a, b);
    if (lane == 0) {
        a.blk_size[b] = out.d;
        if constexpr (kTok)
            a.ntok[b] = count;
    }
    PROF(
    TICK(8);
    if (lane == 0 && a.prof) {
        for (int i = 0; i < 9; i++)
            atomicAdd(&a.prof[i], (unsigned long long)pt[i]);
        for (int i = 13; i < 16; i++)
            atomicAdd(&a.prof[i], (unsigned long long)pt[i]);
        atomicAdd(&a.prof[10], (unsigned long long)n_batches);
        atomicAdd(&a.prof[11], (unsigned long long)n_copies);
        atomicAdd(&a.prof[12], 1ull);
    }
    )
}
} // namespace

} // namespace snapmi
