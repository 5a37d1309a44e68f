// snapmi_lane.hip -- the lane match finder: match_blocks and its kernels
// k_match_blocks, k_match_blocks_plain, k_match_blocks_spec; and k_match_both /
// k_match_both_plain, which run it and the window match finder
// (snapmi_window.hpp) side by side on every CU.  All of them write tokens for
// k_encode_tokens (snapmi_compress.hip).
//
// The wavefront-per-block kernels are bound by a dependent chain per step
// and by "five tables per CU".  This kernel turns the problem around: every
// LANE runs the reference's sequential parse (src/compress.rs:195-317) on its
// own block, with its own hash table in HBM, and a wave advances 64
// independent chains per instruction.
//   * table entries are 16 bytes: the 12 input bytes at the position, the
//     position and an epoch.  The epoch means a table is never zeroed (an
//     entry of another epoch reads as position 0, the reference's fresh
//     table; epochs persist in the context across launches).  The stored
//     bytes decide hit or miss and measure matches shorter than 12 bytes
//     without touching the candidate's cache line;
//   * the loop is organised in ROUNDS of one memory round trip: every lane
//     issues the same three loads (16 B, 16 B, 4 B) whatever it is doing -
//     probing the table, inserting after a copy, or extending a long match
//     16 bytes further - then all lanes wait once and update their state
//     with ALU work only.  A lane never waits for another lane's match
//     extension, so the time of a wave is (rounds of its slowest lane) x
//     (one round trip), not the sum of every lane's serial loops;
//   * a lane that finishes its block takes the next one from the ticket
//     counter, so lanes stay busy whatever the mix of block costs;
//   * the lane only records tokens (literal length, copy length, offset);
//     k_encode_tokens turns them into Snappy elements, one wavefront per
//     block, 64 tokens at a time.
#include "snapmi_window.hpp"

namespace snapmi {

__device__ __forceinline__ uint64_t ld64p(gcptr p)
{
    uint64_t v;
    __builtin_memcpy(&v, p, 8);
    return v;
}
namespace {
// kSpec: for launches of few blocks (snapmi_api.hip: at most 24 576), where
// what is waited for is the latency of a block's dependent rounds and the
// memory system is idle.  A probe's round also fetches the table entry of
// the probe that FOLLOWS IF IT MISSES - its position is known at the start
// of the round (src/compress.rs:207-216: the skip schedule; after a copy,
// s + 1) and its bytes are in the registers the window was read into - and a
// miss goes on to that probe in the same round.  Same table states in the
// same order (what this round wrote is forwarded), same tokens
// (tests/model_match_lane.py: the round order as a model, checked on the
// CPU); 27-39 % fewer rounds on text, each a fifth more expensive: 10-15 %
// off 2 048 .. 16 384 blocks.  A launch of 32 768 blocks and more is at the
// random-access rate of HBM even with one block per lane, and the extra
// table reads buy nothing there: the plain kernel.
// one wavefront's LDS: the lanes' input windows (two 128-byte lines of a
// lane's block) and token buffers (16 tokens = one 128-byte line: every store
// of a lane is its own DRAM transaction, and those are what bounds the kernel)
constexpr uint32_t kLaneRingWords = 64 * 64;
constexpr uint32_t kLaneTokWords = 64 * 16; // (in 8-byte words: 32 tokens a lane)
// lane: 0..63 of this wavefront; g: its lane id among all lanes of the launch
// (its table, its epoch)
// kTail: the form with a run-time depth (options lane_tail_probes,
// lane_tail_idle_pct); without it the round is the plain one or kSpec's, as
// compiled, and nothing of the tail's bookkeeping exists.
template <bool kSpec, bool kTail>
__device__ __forceinline__ void match_blocks(
    const CompressArgs &a, const uint32_t lane, const uint32_t g,
    __attribute__((address_space(3))) uint32_t *const ring,
    __attribute__((address_space(3))) unsigned long long *const tokbuf)
{
    typedef __attribute__((address_space(3))) uint32_t l_tok;
    l_tok *const tbuf = (l_tok *)(tokbuf + lane * 16); // 32 tokens = 128 B
    typedef __attribute__((address_space(3))) uint32_t l_u32;
    typedef __attribute__((address_space(3))) u32x4 l_u32x4;
    typedef __attribute__((address_space(1))) u32x4 g_u32x4;
    l_u32 *const win = ring + lane * 64;

    typedef __attribute__((address_space(1))) unsigned long long g_u64;
    typedef unsigned long long u64x2 __attribute__((ext_vector_type(2)));
    typedef __attribute__((address_space(1))) u64x2 g_entry;
    // 16-byte entries: x = bytes 0..7 at the position, y = bytes 8..11 |
    // position << 32 | epoch << 48
    const uint32_t slot =
        a.lane_chunks ? (g % a.lane_chunks) * a.lane_per_chunk + g / a.lane_chunks
                      : g;
    g_entry *const tab =
        (g_entry *)a.lane_tables + (uint64_t)slot * a.lane_stride;
    unsigned long long epoch = a.lane_epochs[g]; // 16 bits used
    unsigned long long first8 = 0; // bytes 0..11 of the block (empty entry)
    uint32_t first4b = 0;
    // (this launch covers blocks [blk_lo, blk_hi))
    const uint32_t nblocks = segment_blocks(a);

    // what the lane does in the next round
    enum : uint32_t {
        kProbe = 0,  // look up position s (the skip loop, compress.rs:207-245)
        kChain = 1,  // after a copy: insert s-1, look up s (compress.rs:290-312)
        kExtend = 2, // compare 16 more bytes of an open match (compress.rs:378-412)
    };
    // per-lane block state
    bool have = false, out_of_work = false;
    uint32_t b = 0, n = 0, s_limit = 0, shift = 0;
    uint32_t mode = kProbe;
    uint32_t s = 0, s_next = 0, skip = 0, next_emit = 0;
    uint32_t mpos = 0, mcand = 0, p = 0, c = 0; // the open match
    uint32_t ntok = 0;
    uint32_t csize = 0; // encoded bytes of the block's tokens so far
    // input window: the bytes [hi - 256, hi) of the 128-byte aligned view of
    // the block (src_al = src - mis) are in `win`, at their offset mod 256
    uint32_t mis = 0, hi = 0;
    gcptr src = nullptr, src_al = nullptr;
    typedef __attribute__((address_space(1))) uint32_t g_tok;
    // the pages the block's tokens and exceptions are going to (the dump
    // page once the pool has run out: CompressArgs::tok_pool)
    uint32_t tpage = a.tok_pool_pages, epage = a.tok_pool_pages;
    bool spilled = false;
    uint32_t nexc = 0;
    // the lane's page in hand, and what is left of the wavefront's run
    // (uniform): see tok_page_ask
    uint32_t spare = kNoPage, run_next = 0, run_end = 0;
    // probes a round resolves (uniform): CompressArgs::lane_depth; raised to
    // lane_tail_depth, and never lowered again, once this wavefront has seen
    // the ticket run out (seen_idle) and then reads, every 64 passes of the
    // loop, that lane_tail_idle lanes of the launch are out of work.  Nothing
    // waits for anything: a wavefront that reads no fresh count stays as it is.
    uint32_t depth = a.lane_depth;
    if (kTail && a.lane_tail_idle == 0 && depth < a.lane_tail_depth)
        depth = a.lane_tail_depth;
    auto D = [&]() -> uint32_t { return kTail ? depth : (kSpec ? 2u : 1u); };
    bool seen_idle = false;
    uint32_t passes = 0;
    PROF_TAIL(
    if (a.prof && lane == 0)
        atomicMax(&a.prof[kProfTail], ~(unsigned long long)wall_clock64());
    )
#ifdef SNAPMI_TESTING
    uint32_t multi_rounds = 0; // rounds above the launch's own depth
#endif
    // where token idx goes; the first token of a page takes the page
    auto tok_at = [&](uint32_t idx) -> g_tok * {
        if (idx % kTokPage == 0)
            tpage = tok_page_take(a, b, idx / kTokPage, spare, spilled);
        return (g_tok *)a.tok_pool + (uint64_t)tpage * kTokPage +
               idx % kTokPage;
    };
    auto exc_put = [&](unsigned long long v) {
        if (nexc % kExcPage == 0)
            epage = tok_page_take(a, b, kTokPagesPerBlock + nexc / kExcPage,
                                  spare, spilled);
        if (!spilled)
            ((g_u64 *)((g_tok *)a.tok_pool + (uint64_t)epage * kTokPage))
                [nexc % kExcPage] = v;
        nexc++;
    };

    for (;;) {
        if (kTail && seen_idle && depth < a.lane_tail_depth &&
            (++passes & 63) == 0) {
            const uint32_t idle = __hip_atomic_load(
                &a.ticket[kTicketIdle], __ATOMIC_RELAXED,
                __HIP_MEMORY_SCOPE_AGENT);
            if (uni(idle) >= a.lane_tail_idle)
                depth = a.lane_tail_depth;
        }
        // token pages for the lanes that used theirs in the last round (the
        // loop's top is convergent: the run's bounds stay uniform)
        {
            const uint64_t M_pg = __ballot(spare == kNoPage);
            if (M_pg) {
                const uint32_t cnt = (uint32_t)__builtin_popcountll(M_pg);
                const uint32_t rank = __builtin_amdgcn_mbcnt_hi(
                    (uint32_t)(M_pg >> 32),
                    __builtin_amdgcn_mbcnt_lo((uint32_t)M_pg, 0));
                const uint32_t left = run_end - run_next;
                if (left < cnt) {
                    // what is left of the run goes to the first of them, a
                    // new run serves the others (lanes that work on blocks
                    // of one kind fill their pages in step: a remainder
                    // dropped here was a tenth of the pages of a batch
                    // sorted by file)
                    const uint32_t leader = (uint32_t)__builtin_ctzll(M_pg);
                    const uint32_t more = cnt - left;
                    const uint32_t take = more > kTokRun ? more : kTokRun;
                    uint32_t base = 0;
                    if (lane == leader)
                        base = atomicAdd(&a.tok_ctl[0], take);
                    base = rdlane(base, leader);
                    if (spare == kNoPage)
                        spare = rank < left ? run_next + rank
                                            : base + (rank - left);
                    run_next = base + more;
                    run_end = base + take;
                } else {
                    if (spare == kNoPage)
                        spare = run_next + rank;
                    run_next += cnt;
                }
            }
        }
        // Tickets are taken for the whole wavefront at once: the lanes that
        // need a block count themselves (ballot) and ONE of them adds the
        // count to the device-wide counter.  (One atomic per lane on one
        // address is 3.7 ns each, one after the other in the L2: 0.97 ms for
        // a launch of 262 144 tiny blocks, all of its duration.)
        const bool need = !have && !out_of_work;
        const uint64_t M_need = __ballot(need);
        unsigned long long tbase = 0;
        if (M_need) {
            const uint32_t leader = (uint32_t)__builtin_ctzll(M_need);
            if (lane == leader)
                tbase = atomicAdd((unsigned long long *)a.ticket,
                                  (unsigned long long)__builtin_popcountll(
                                      M_need));
            tbase = ((unsigned long long)rdlane((uint32_t)(tbase >> 32),
                                                leader)
                     << 32) |
                    rdlane((uint32_t)tbase, leader);
        }
        if (need) {
            const unsigned long long old =
                tbase + __builtin_amdgcn_mbcnt_hi(
                            (uint32_t)(M_need >> 32),
                            __builtin_amdgcn_mbcnt_lo((uint32_t)M_need, 0));
            b = a.blk_lo + (uint32_t)old;
            if ((uint64_t)b + (uint32_t)(old >> 32) >= nblocks) {
                out_of_work = true;
            } else {
                const BlockAt blk = locate_block(a, b);
                src = (gcptr)blk.in + blk.off();
                n = blk.n;
                spilled = false;
                ntok = 0;
                nexc = 0;
                csize = 0;
                next_emit = 0;
                have = true;
                if (n <= a.cls_lo || n > a.cls_hi) {
                    have = false; // another launch's block
                } else if (n < kMinNonLiteral) { // src/compress.rs:140-146
                    g_tok *const at = tok_at(0);
                    if (!spilled)
                        *at = tok_pack(n, 0, 0);
                    a.ntok[b] = spilled ? kTokSpilled : 1u;
                    a.blk_size[b] = token_bytes(n, 0, 0);
                    have = false;
                } else {
                    // fresh table = new epoch (src/compress.rs:491-518)
                    first8 = ld64p(src);
                    first4b = ld32u(src + 8);
                    epoch = (epoch + 1) & 0xFFFFu;
                    if (epoch == 0) { // wrapped: really clear this lane's table
                        for (uint32_t i = 0; i < kMaxTable; i++)
                            tab[i] = (u64x2){0, 0};
                        epoch = 1;
                    }
                    shift = table_shift(n, kMaxTable).shift;
                    s_limit = n - kInputMargin; // >= 2
                    // first trip of the skip loop: s = 1, s_next = 2
                    s = 1;
                    s_next = 2;
                    skip = 33;
                    mode = kProbe;
                    mis = (uint32_t)(uintptr_t)src & 127u;
                    src_al = src - mis;
                    hi = 0;
                }
            }
        }
        // the lanes that went out of work in this pass count themselves for
        // the launch's other wavefronts: one atomic
        if ((kTail || kProfTailBuild) && M_need) {
            const uint64_t M_out = __ballot(need && out_of_work);
            if (M_out) {
                if (kTail && lane == (uint32_t)__builtin_ctzll(M_out))
                    atomicAdd(&a.ticket[kTicketIdle],
                              (uint32_t)__builtin_popcountll(M_out));
                seen_idle = true;
                PROF_TAIL(
                if (a.prof) {
                    const unsigned long long t = wall_clock64();
                    if (need && out_of_work)
                        a.prof[kProfTailLanes + g] = t;
                    if (lane == (uint32_t)__builtin_ctzll(M_out))
                        atomicMax(&a.prof[kProfTail + 2], ~t);
                }
                )
            }
        }
        if (__ballot(have) == 0) {
            if (__ballot(!out_of_work) == 0)
                break;
            continue;
        }
        if (!have)
            continue;
#ifdef SNAPMI_TESTING
        if (kTail && depth > a.lane_depth)
            multi_rounds++;
#endif

        // ---- one round ----------------------------------------------------
        // The 17 bytes at pos-1 come from the window (pos = s, or p while a
        // match is open).  The next line is fetched while at least 64 bytes
        // of look-ahead remain, in the same round as the table access; only
        // a lane that jumped past its window (long match, large skip) has
        // to sit a round out.
        const uint32_t y0 = (mode == kExtend ? p : s) - 1 + mis;
        if (y0 >= hi)
            hi = y0 & ~127u; // jumped past the frontier: restart there
        const bool stall = y0 + 17 > hi;
        // (never fetch past the block's own last line: the next line may be
        // the first one behind the caller's allocation)
        const bool fill = y0 + 81 > hi && hi < ((n + mis + 127u) & ~127u);
        uint32_t q0, q1, q2, q3, r0, r1, r2, r3;
        {
            const uint32_t w0 = y0 >> 2, sh = y0 & 3;
            const uint32_t d0 = win[w0 & 63], d1 = win[(w0 + 1) & 63],
                           d2 = win[(w0 + 2) & 63], d3 = win[(w0 + 3) & 63],
                           d4 = win[(w0 + 4) & 63];
            q0 = __builtin_amdgcn_alignbyte(d1, d0, sh); // bytes at pos-1
            q1 = __builtin_amdgcn_alignbyte(d2, d1, sh);
            q2 = __builtin_amdgcn_alignbyte(d3, d2, sh);
            q3 = __builtin_amdgcn_alignbyte(d4, d3, sh);
            const uint32_t q4 = d4 >> (8 * sh);
            r0 = __builtin_amdgcn_alignbyte(q1, q0, 1); // bytes at pos
            r1 = __builtin_amdgcn_alignbyte(q2, q1, 1);
            r2 = __builtin_amdgcn_alignbyte(q3, q2, 1);
            r3 = __builtin_amdgcn_alignbyte(q4, q3, 1);
        }
        const uint32_t hprev = hash32(q0, shift), hcur = hash32(r0, shift);
        // the one random access of the round: table entry or candidate bytes
        gcptr pa = mode == kExtend ? src + c : (gcptr)(tab + hcur);
        pa = stall ? src_al + hi : pa;
        B16 A = ld128u(pa);
        // depth > 1: the up to three probes behind this one, should it and
        // they miss.  Probe k + 1 lies dx[k] bytes on: the skip schedule
        // (src/compress.rs:207-216; after a copy s + 1, then skip = 32) says
        // so at the start of the round, and its 12 bytes are in the registers
        // while dx[k] <= 3 (r3 ends at pos + 15).  Their entries are read
        // here, in front of everything the round writes.
        uint32_t hx[3] = {0, 0, 0}, dx[3] = {0, 0, 0};
        bool okx[3] = {false, false, false};
        B16 Ax[3] = {{{0, 0, 0, 0}}, {{0, 0, 0, 0}}, {{0, 0, 0, 0}}};
        if (kSpec || D() > 1) {
            uint32_t d = mode == kChain ? 1 : s_next - s;
            uint32_t sk = mode == kChain ? 32 : skip;
            bool ok = mode <= kChain && !stall;
#pragma unroll
            for (uint32_t k = 0; k < 3; k++) {
                if (k + 1 < D()) { // (uniform)
                    ok = ok && d <= 3;
                    dx[k] = d;
                    okx[k] = ok;
                    hx[k] = hash32(__builtin_amdgcn_alignbyte(r1, r0, d), shift);
                    if (ok)
                        Ax[k] = ld128u((gcptr)(tab + hx[k]));
                    const uint32_t step = sk >> 5;
                    d += step;
                    sk += step;
                }
            }
        }
        // (the load is issued HERE, in front of the window's line: a compiler
        // barrier, or it may be sunk behind the fill's wait - two latencies
        // in every round that fills)
        asm volatile("" ::: "memory");
        if (fill) {
            const g_u32x4 *lp = (const g_u32x4 *)(src_al + hi);
            const u32x4 f0 = lp[0], f1 = lp[1], f2 = lp[2], f3 = lp[3],
                        f4 = lp[4], f5 = lp[5], f6 = lp[6], f7 = lp[7];
            l_u32x4 *dst = (l_u32x4 *)(win + ((hi >> 2) & 63));
            dst[0] = f0; dst[1] = f1; dst[2] = f2; dst[3] = f3;
            dst[4] = f4; dst[5] = f5; dst[6] = f6; dst[7] = f7;
            hi += 128;
        }
        // one wait for the whole round: A is materialised before the branch
        // that uses it (the fill's wait, when there was one, covered it)
        asm volatile("" : "+v"(A.w[0]));
        if (kSpec || D() > 1) {
#pragma unroll
            for (uint32_t k = 0; k < 3; k++)
                if (k + 1 < D())
                    asm volatile("" : "+v"(Ax[k].w[0]));
        }
        if (stall)
            continue;

        bool matched = false;  // a copy ends in this round at mend
        bool advance = false;  // next trip of the skip loop
        bool tail = false;     // open match within 16 bytes of the block end
        bool finished = false;
        uint32_t mend = 0;
        const bool was_chain = mode == kChain;
        const uint32_t s0 = s;
        if (mode <= kChain) {
            if (mode == kChain) {
                // src/compress.rs:290-297: insert s-1 first; the lookup of s
                // must see it when both hash to the same slot
                const unsigned long long b8 =
                    ((unsigned long long)q1 << 32) | q0;
                const unsigned long long by =
                    (epoch << 48) | ((unsigned long long)(s - 1) << 32) | q2;
                tab[hprev] = (u64x2){b8, by};
                if (hprev == hcur) {
                    A.w[0] = q0;
                    A.w[1] = q1;
                    A.w[2] = q2;
                    A.w[3] = (uint32_t)(by >> 32);
                }
            }
            const unsigned long long p8 = ((unsigned long long)r1 << 32) | r0;
            const uint32_t p4 = r2;
            const bool live = (A.w[3] >> 16) == (uint32_t)epoch;
            const uint32_t cand = live ? A.w[3] & 0xFFFFu : 0;
            const unsigned long long c8 =
                live ? ((unsigned long long)A.w[1] << 32) | A.w[0] : first8;
            const uint32_t c4 = live ? A.w[2] : first4b;
            tab[hcur] = (u64x2){
                p8, (epoch << 48) | ((unsigned long long)s << 32) | p4};
            if ((uint32_t)c8 == r0) {
                // the entry holds the candidate's first 12 bytes, so most
                // matches are measured without touching the candidate's line
                const unsigned long long d8 = c8 ^ p8;
                const uint32_t d4 = c4 ^ p4;
                const uint32_t m =
                    d8 ? (uint32_t)__builtin_ctzll(d8) >> 3
                       : 8 + (d4 ? (uint32_t)__builtin_ctz(d4) >> 3 : 4);
                mpos = s;
                mcand = cand;
                if (m < 12) {
                    matched = true;
                    mend = s + m;
                } else {
                    p = s + 12;
                    c = cand + 12;
                    mode = kExtend;
                    tail = p + 16 > n;
                }
            } else {
                if (mode == kChain) { // src/compress.rs:310-312
                    s_next = s + 1;
                    skip = 32;
                }
                advance = true;
            }
        } else { // kExtend
            B16 Bv;
            Bv.w[0] = r0; Bv.w[1] = r1; Bv.w[2] = r2; Bv.w[3] = r3;
            const uint32_t m = common16(A, Bv);
            if (m < 16) {
                matched = true;
                mend = p + m;
            } else {
                p += 16;
                c += 16;
                tail = p + 16 > n;
            }
        }
        if (kSpec || D() > 1) {
#pragma unroll
            for (uint32_t k = 0; k < 3; k++) {
                if (k + 1 < D() && advance && okx[k]) {
                    // the probe in front missed: its advance
                    // (src/compress.rs:207-216), then the probe at the new s
                    // with the entry fetched for it
                    s = s_next;
                    const uint32_t step = skip >> 5;
                    s_next = s + step;
                    skip += step;
                    mode = kProbe;
                    advance = false;
                    if (s_next > s_limit) {
                        finished = true;
                    } else {
                        const uint32_t t0 =
                            __builtin_amdgcn_alignbyte(r1, r0, dx[k]);
                        const uint32_t t1 =
                            __builtin_amdgcn_alignbyte(r2, r1, dx[k]);
                        const uint32_t t2 =
                            __builtin_amdgcn_alignbyte(r3, r2, dx[k]);
                        // what this round wrote is newer than what it read:
                        // the chain insert, probe 0, the probes in between -
                        // the newest of them counts
                        B16 E = Ax[k];
                        if (was_chain && hx[k] == hprev) {
                            E.w[0] = q0;
                            E.w[1] = q1;
                            E.w[2] = q2;
                            E.w[3] = ((uint32_t)epoch << 16) | (s0 - 1);
                        }
                        if (hx[k] == hcur) {
                            E.w[0] = r0;
                            E.w[1] = r1;
                            E.w[2] = r2;
                            E.w[3] = ((uint32_t)epoch << 16) | s0;
                        }
#pragma unroll
                        for (uint32_t j = 0; j < k; j++) {
                            if (hx[k] == hx[j]) {
                                E.w[0] = __builtin_amdgcn_alignbyte(r1, r0, dx[j]);
                                E.w[1] = __builtin_amdgcn_alignbyte(r2, r1, dx[j]);
                                E.w[2] = __builtin_amdgcn_alignbyte(r3, r2, dx[j]);
                                E.w[3] = ((uint32_t)epoch << 16) | (s0 + dx[j]);
                            }
                        }
                        const unsigned long long p8 =
                            ((unsigned long long)t1 << 32) | t0;
                        const uint32_t p4 = t2;
                        const bool live = (E.w[3] >> 16) == (uint32_t)epoch;
                        const uint32_t cand = live ? E.w[3] & 0xFFFFu : 0;
                        const unsigned long long c8 =
                            live ? ((unsigned long long)E.w[1] << 32) | E.w[0]
                                 : first8;
                        const uint32_t c4 = live ? E.w[2] : first4b;
                        tab[hx[k]] = (u64x2){
                            p8,
                            (epoch << 48) | ((unsigned long long)s << 32) | p4};
                        if ((uint32_t)c8 == t0) {
                            const unsigned long long d8 = c8 ^ p8;
                            const uint32_t d4 = c4 ^ p4;
                            const uint32_t m =
                                d8 ? (uint32_t)__builtin_ctzll(d8) >> 3
                                   : 8 + (d4 ? (uint32_t)__builtin_ctz(d4) >> 3
                                             : 4);
                            mpos = s;
                            mcand = cand;
                            if (m < 12) {
                                matched = true;
                                mend = s + m;
                            } else {
                                p = s + 12;
                                c = cand + 12;
                                mode = kExtend;
                                tail = p + 16 > n;
                            }
                        } else {
                            advance = true;
                        }
                    }
                }
            }
        }
        if (tail) { // rare: finish the match bytewise up to the block end
            while (p < n && src[p] == src[c]) {
                p++;
                c++;
            }
            matched = true;
            mend = p;
        }
        bool flush = false;
        if (matched) {
            // token: literal next_emit..mpos, copy (mpos - mcand, mend - mpos)
            {
                // token_bytes(), short form for the usual token (literal of
                // at most 60 bytes, copy of at most 64): the round loop is
                // not free of VALU cost
                const uint32_t tl = mpos - next_emit, tc = mend - mpos,
                               to = mpos - mcand;
                tbuf[ntok & 31] = tok_pack(tl, tc, to);
                ntok++;
                if (tl > 60 || tc > 64) {
                    csize += token_bytes(tl, tc, to);
                    if (!tok_fits(tl, tc)) // rare: its numbers in full
                        exc_put(tok_pack64(tl, tc, to));
                } else {
                    csize += tl + 3 + (tl != 0) - (tc <= 11 && to <= 2047);
                }
            }
            flush = (ntok & 31) == 0;
            s = mend;
            next_emit = mend;
            mode = kChain;
            if (s >= s_limit) // src/compress.rs:275-277
                finished = true;
        }
        if (advance) { // src/compress.rs:207-216
            s = s_next;
            const uint32_t step = skip >> 5;
            s_next = s + step;
            skip += step;
            mode = kProbe;
            if (s_next > s_limit)
                finished = true;
        }
        if (finished)
            flush = flush || (ntok & 31) != 0;
        if (flush) { // the token group that holds token ntok-1
            g_u32x4 *to = (g_u32x4 *)tok_at((ntok - 1) & ~31u);
            const l_u32x4 *from = (const l_u32x4 *)tbuf;
            const u32x4 t0 = from[0], t1 = from[1], t2 = from[2], t3 = from[3],
                        t4 = from[4], t5 = from[5], t6 = from[6], t7 = from[7];
            // (a spilled block stores nothing: tens of thousands of lanes
            // writing one dump page wait for one another in its L2 channel -
            // 3.9 s for a launch of 64 000 spilled blocks)
            if (!spilled) {
                to[0] = t0; to[1] = t1; to[2] = t2; to[3] = t3;
                to[4] = t4; to[5] = t5; to[6] = t6; to[7] = t7;
            }
        }
        if (finished) { // done(): src/compress.rs:417-426
            if (next_emit < n) {
                const uint32_t tl = n - next_emit;
                // (behind a flushed group in that group's page; the first
                // token of a group of its own may open a page)
                g_tok *const at =
                    ntok % 32 ? (g_tok *)a.tok_pool +
                                    (uint64_t)tpage * kTokPage + ntok % kTokPage
                              : tok_at(ntok);
                if (!spilled)
                    *at = tok_pack(tl, 0, 0);
                ntok++;
                if (!tok_fits(tl, 0))
                    exc_put(tok_pack64(tl, 0, 0));
                csize += token_bytes(tl, 0, 0);
            }
            a.ntok[b] = spilled ? kTokSpilled : ntok;
            a.blk_size[b] = csize;
            have = false;
        }
    }
    a.lane_epochs[g] = epoch;
    PROF_TAIL(
    if (a.prof && lane == 0)
        atomicMax(&a.prof[kProfTail + 1], (unsigned long long)wall_clock64());
    )
#ifdef SNAPMI_TESTING
    if (kTail && lane == 0 && multi_rounds)
        atomicAdd(&a.tok_ctl[kTokCtlMultiRounds], multi_rounds);
#endif
}
} // namespace

#define SNAPMI_LANE_KERNEL(name, spec, tail)                                  \
    __global__ __launch_bounds__(64) void name(CompressArgs a)                \
    {                                                                         \
        __shared__ __attribute__((aligned(16))) uint32_t ring[kLaneRingWords]; \
        __shared__ __attribute__((aligned(16)))                               \
        unsigned long long tokbuf[kLaneTokWords];                             \
        match_blocks<spec, tail>(                                             \
            a, threadIdx.x, blockIdx.x * 64 + threadIdx.x,                    \
            (__attribute__((address_space(3))) uint32_t *)ring,               \
            (__attribute__((address_space(3))) unsigned long long *)tokbuf);  \
    }
// k_match_blocks has the run-time depth (CompressArgs::lane_depth says where
// it starts); the two with the round as compiled run where the options ask
// for no more probes than the launch starts with
SNAPMI_LANE_KERNEL(k_match_blocks, false, true)
SNAPMI_LANE_KERNEL(k_match_blocks_plain, false, false)
SNAPMI_LANE_KERNEL(k_match_blocks_spec, true, false)
#undef SNAPMI_LANE_KERNEL

// Both match finders on every CU (round 5): three wavefronts of the lane
// kernel - as many as reach the DRAM-transaction ceiling it is bound by
// (tests/hw/sweep.sh: 3 waves per CU 123 ms, 6 waves 122) - and two of the
// window kernel, which is bound by the instructions and latencies of a lone
// wavefront and touches HBM for little more than its input, in one persistent
// workgroup per CU: 3 x 24 KiB of lane windows and token lines + 2 x 32 KiB of
// tables.  One two-ended ticket: the lanes take blocks from the front of the
// segment, the windows from its back, until they meet; both write tokens for
// k_encode_tokens.  (Round 4 split the CUs between the two kernels and gained
// nothing; here the lanes keep every CU.)  k_match_both's lane wavefronts
// have the run-time depth, k_match_both_plain's the plain round alone.
namespace {
template <bool kTail>
__device__ __forceinline__ void match_both(
    const CompressArgs &a,
    __attribute__((address_space(3))) uint32_t *const ring,
    __attribute__((address_space(3))) unsigned long long *const tokbuf,
    const lptr16 tables)
{
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t wave = uni(threadIdx.x >> 6);
    if (wave < kBothLaneWaves) {
        match_blocks<false, kTail>(
            a, lane, (blockIdx.x * kBothLaneWaves + wave) * 64 + lane,
            ring + wave * kLaneRingWords, tokbuf + wave * kLaneTokWords);
        return;
    }
    const lptr16 table = tables + (wave - kBothLaneWaves) * kMaxTable;
    const uint32_t tbase = (uint32_t)(uintptr_t)table;
    const uint32_t nblocks = segment_blocks(a);
    for (;;) {
        const uint32_t b =
            uni(next_back_ticket(a.ticket, lane, a.blk_lo, nblocks));
        if (b == 0xFFFFFFFFu)
            break;
        compress_one_block_span<false, true>(a, b, lane, table, tbase);
    }
    PROF_TAIL(
    if (a.prof && lane == 0)
        atomicMax(&a.prof[kProfTail + 1], (unsigned long long)wall_clock64());
    )
}
} // namespace
#define SNAPMI_BOTH_KERNEL(name, tail)                                        \
    __global__ __launch_bounds__(kBothWaves * 64) void name(CompressArgs a)   \
    {                                                                         \
        __shared__ __attribute__((aligned(16)))                               \
        uint32_t ring[kBothLaneWaves][kLaneRingWords];                        \
        __shared__ __attribute__((aligned(16)))                               \
        unsigned long long tokbuf[kBothLaneWaves][kLaneTokWords];             \
        __shared__ __attribute__((aligned(16)))                               \
        uint16_t tables[kBothWaves - kBothLaneWaves][kMaxTable];              \
        match_both<tail>(                                                     \
            a, (__attribute__((address_space(3))) uint32_t *)&ring[0][0],     \
            (__attribute__((address_space(3))) unsigned long long *)          \
                &tokbuf[0][0],                                                \
            (lptr16)&tables[0][0]);                                           \
    }
SNAPMI_BOTH_KERNEL(k_match_both, true)
SNAPMI_BOTH_KERNEL(k_match_both_plain, false)
#undef SNAPMI_BOTH_KERNEL

} // namespace snapmi
