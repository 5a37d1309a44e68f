// snapmi_steps.hip -- the one-copy-per-step wavefront kernels of rounds 1-3,
// k_compress_blocks and k_compress_block_lds: the test build's cross-check of
// the window kernels (option span_kernel 0; the product library has neither).
// One wavefront owns one 64 KiB block at a time, its u16 hash table in LDS.
// The 64 lanes evaluate the next 64 positions of the reference's probe
// schedule (src/compress.rs:207-245) at once: ONE lane-ordered
// ds_mskor_rtn_b32 reproduces "candidate = table[h]; table[h] = s" in probe
// order (k_probe_lds_order, snapmi_window.hip), every lane compares 16 bytes
// at its candidate, the first hit wins and the entries of the lanes behind it
// are rolled back: one LDS atomic and one candidate gather per emitted copy.
#ifdef SNAPMI_TESTING
#include <type_traits>

#include "snapmi_compress_dev.hpp"

namespace snapmi {

// One 64 KiB block, by one wavefront.  kLds: the match finder reads the block
// from a copy in LDS at `lblock` (filled here) instead of HBM / L2 - every
// load on the per-copy dependency chain is then an LDS access.
template <bool kLds>
__device__ __forceinline__ void compress_one_block(
    const CompressArgs &a, const uint32_t b, const uint32_t lane,
    const lptr16 table, const uint32_t tbase, const uint32_t c2,
    const uint32_t c3, const uint32_t cB, const uint32_t cBn,
    __attribute__((address_space(3))) uint8_t *lblock = nullptr)
{
    const BlockAt at = locate_block(a, b);
    gcptr src = (gcptr)at.in + at.off();
    const uint32_t n = at.n;
    // (these kernels run in launches with scratch slots only)
    gptr dst;
    if (!block_dest<true>(a, at, b, lane == 0, dst))
        return; // stream rejected by k_plan_compress (E_ARGUMENT)
    TokenSink out;
    out.init(src, n, dst, lane);

    if (n < kMinNonLiteral) { // reference src/compress.rs:140-146
        out.record(0, n, 0, 0);
        out.flush();
        if (lane == 0)
            a.blk_size[b] = out.d;
        return;
    }
    // what the match finder reads: the block itself, or its copy in LDS
    typename std::conditional<kLds, lcptr, gcptr>::type msrc;
    if constexpr (kLds) {
        // 1 KiB per wave instruction, coalesced; the tail bytewise
        typedef __attribute__((address_space(3))) u32x4 l_u32x4;
        typedef __attribute__((address_space(1))) u32x4 g_u32x4c;
        const uint32_t mis = (uint32_t)(uintptr_t)src & 15u; // 16-byte lines
        l_u32x4 *to = (l_u32x4 *)lblock;
        // LDS copy starts at the 16-byte line that holds src[0]
        const g_u32x4c *from = (const g_u32x4c *)(src - mis);
        const uint32_t lines = (n + mis + 15) / 16;
        for (uint32_t i = lane; i < lines; i += kWave)
            to[i] = from[i]; // (never past the line that holds the last byte)
        __builtin_amdgcn_wave_barrier();
        msrc = (lcptr)lblock + mis;
    } else {
        msrc = src;
    }

    // table sizing + zero fill: reference src/compress.rs:491-518
    const TableShape ts = table_shift(n, kMaxTable);
    const uint32_t shift = ts.shift;
    for (uint32_t i = 8 * lane; i < ts.size; i += 8 * kWave)
        *(__attribute__((address_space(3))) u32x4 *)&table[i] =
            (u32x4){0, 0, 0, 0};
    // LDS operations of one wavefront execute in order: no barrier needed
    // between the zero fill and the first table access of this wavefront
    __builtin_amdgcn_wave_barrier();

    // reference Block::compress, src/compress.rs:195-317.
    //  chain == false: probing started at position 1 (block start);
    //  chain == true : a copy just ended at s (s < s_limit): lane 0 inserts
    //                  s-1, lane 1 is the check at s (:290-306), lanes 2..
    //                  are the probe loop restarted at s+1 (:310-312,:204).
    //  q: probes of the current run already done by earlier batches.
    const uint32_t s_limit = n - kInputMargin;
    uint32_t s = 0, next_emit = 0, q = 0;
    bool chain = false;
    // Register window of the input for hashing: wv0/1/2[lane] = the dword at
    // block offset wbase + {0,64,128} + lane.  After a copy the next batch's
    // hash inputs are a lane rotation of these (3 ds_bpermute), so the HBM/L2
    // round trip for "the 4 bytes at each probed position" leaves the chain.
    // wv3 is the prefetch slot: loaded one slide ahead of its first use.
    uint32_t wbase = 0x80000000u, wv0 = 0, wv1 = 0, wv2 = 0, wv3 = 0;
    const uint32_t cI = cB + 1; // offset of this lane's probe from s - 1
    PROF(
    uint64_t pt[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    uint64_t t_last = __builtin_readcyclecounter();
    uint64_t n_batches = 0, n_copies = 0;
    )
    for (;;) {
        PROF(
        n_batches++;
        )
        TICK(0);
        uint32_t p, nextp;
        bool active = true, probe = true;
        const uint32_t run0 = chain ? s + 1 : 1; // where the probe run began
        if (q == 0) {
            if (!chain) {
                p = lane ? run0 + c2 : 0;
                nextp = run0 + c3;
                active = lane != 0; // lane 0 only fetches bytes 0..15
            } else {
                p = s + cB;
                nextp = s + cBn;
                probe = lane != 0;
            }
        } else {
            p = run0 + kDelta.d[q + lane];
            nextp = run0 + kDelta.d[q + lane + 1];
        }
        // reference: "if s_next > s_limit return done()", :212-214
        const bool valid = active && nextp <= s_limit;
        const uint32_t pc = p < n - 16 ? p : n - 16;
        uint32_t hx = 0; // the 4 bytes at p, for the hash
        if (chain && q == 0) {
            // from the register window: no memory round trip before the hash
            const uint32_t idx = s - 1 - wbase + cI; // < 192
            const int sel = (int)((idx & 63) << 2);
            const uint32_t g0 =
                (uint32_t)__builtin_amdgcn_ds_bpermute(sel, (int)wv0);
            const uint32_t g1 =
                (uint32_t)__builtin_amdgcn_ds_bpermute(sel, (int)wv1);
            const uint32_t g2 =
                (uint32_t)__builtin_amdgcn_ds_bpermute(sel, (int)wv2);
            hx = idx < 64 ? g0 : (idx < 128 ? g1 : g2);
        }
        // issued after the window reads so that its latency overlaps the
        // hash, the LDS atomic and the candidate gather
        const B16 x = ld128u(msrc + pc);
        if (!(chain && q == 0)) {
            hx = x.w[0];
            // keep this a real (uniform) branch: as a select it would make
            // the hash wait for x on the window path too
            asm volatile("" : "+v"(hx));
        }
        TICK(1);
        const uint32_t h = hash32(hx, shift);
        uint32_t cand = 0;
        if (valid) {
            const uint32_t sh = (h & 1) * 16;
            const uint32_t old = lds_mskor_rtn(tbase + (h >> 1) * 4,
                                               0xFFFFu << sh, p << sh);
            cand = (old >> sh) & 0xFFFFu;
        }
        TICK(2);
        const B16 y = ld128u(msrc + cand);
        TICK(3);
        const uint32_t m = common16(x, y);
        // (cand < p always holds when the DS atomic applies lanes in ascending
        // order, which snapmi_ctx_create verifies; the test keeps the output
        // a valid stream even if that ever failed)
        const uint64_t hits = __ballot(valid && probe && m >= 4 && cand < p);
        if (hits == 0) {
            if (__ballot(active && !valid) != 0)
                break; // ran into s_limit: done
            q += q ? kWave : (chain ? kWave - 2 : kWave - 1);
            continue;
        }
        const uint32_t kh = (uint32_t)__builtin_ctzll(hits);
        const uint32_t pk = rdlane(p, kh);
        const uint32_t ck = rdlane(cand, kh);
        uint32_t len = rdlane(m, kh);
        // lanes past the hit never ran in the reference: give the table
        // back the value that was there before the first of them
        if (valid && lane > kh && cand <= pk)
            table[h] = (uint16_t)cand;

        TICK(4);
        TICK(5);
        if (len == 16)
            len += extend_match(msrc, n, ck + 16, pk + 16, lane);
        TICK(6);
        // literal next_emit..pk (reference :250-257) + copy (:272-273)
        out.record(next_emit, pk - next_emit, pk - ck, len);
        TICK(7);
        PROF(
        n_copies++;
        )
        s = pk + len;
        next_emit = s;
        chain = true;
        q = 0;
        // keep the window covering s-1 .. s+158: slide by 64 positions when
        // s-1 has moved past the first register, restart after a long jump
        {
            const uint32_t D = s - 1 - wbase;
            if (D >= 64) {
                if (D < 128) {
                    wv0 = wv1;
                    wv1 = wv2;
                    wv2 = wv3;
                    wbase += 64;
                    const uint32_t wp = wbase + 192 + lane;
                    wv3 = ld32u(msrc + (wp < n - 4 ? wp : n - 4));
                } else {
                    wbase = s - 1;
                    const uint32_t w0 = wbase + lane;
                    const uint32_t n4 = n - 4;
                    wv0 = ld32u(msrc + (w0 < n4 ? w0 : n4));
                    wv1 = ld32u(msrc + (w0 + 64 < n4 ? w0 + 64 : n4));
                    wv2 = ld32u(msrc + (w0 + 128 < n4 ? w0 + 128 : n4));
                    wv3 = ld32u(msrc + (w0 + 192 < n4 ? w0 + 192 : n4));
                }
            }
        }
        if (s >= s_limit) // reference :275-277
            break;
    }
    if (next_emit < n) // reference done(), src/compress.rs:417-426
        out.record(next_emit, n - next_emit, 0, 0);
    if (out.t)
        out.flush();
    if (lane == 0)
        a.blk_size[b] = out.d;
    PROF(
    TICK(8);
    if (lane == 0 && a.prof) {
        for (int i = 0; i < 9; i++)
            atomicAdd(&a.prof[i], (unsigned long long)pt[i]);
        atomicAdd(&a.prof[10], (unsigned long long)n_batches);
        atomicAdd(&a.prof[11], (unsigned long long)n_copies);
        atomicAdd(&a.prof[12], 1ull);
    }
    )
}

// ---------------------------------------------------------------------
// K1: persistent workgroups of five wavefronts, one 32 KiB table each.
// ---------------------------------------------------------------------
__global__ __launch_bounds__(kCompressWaves * 64) void k_compress_blocks(
    CompressArgs a)
{
    __shared__ __attribute__((aligned(16)))
    uint16_t tables[kCompressWaves][kMaxTable];

    const uint32_t lane = threadIdx.x & 63;
    const uint32_t wave = uni(threadIdx.x >> 6);
    const lptr16 table = (lptr16)&tables[wave][0];
    const uint32_t tbase = (uint32_t)(uintptr_t)table; // LDS byte offset
    const uint32_t nblocks = launch_blocks(a);

    // this lane's slice of the probe schedule
    const uint32_t c2 = lane >= 1 ? kDelta.d[lane - 1] : 0;
    const uint32_t c3 = kDelta.d[lane];
    // after a copy ending at s: lane 0 -> s-1, lane 1 -> s, lane j -> s+1+d[j-2]
    const uint32_t cB = lane >= 2 ? 1 + kDelta.d[lane - 2] : lane - 1;
    const uint32_t cBn = lane >= 2 ? 1 + c2 : 0; // offset of the next probe

    // one ticket per wavefront per block
    // (the helper's result comes back in a VGPR: re-pin it to an SGPR so the
    // whole block state stays scalar)
    uint32_t b = uni(next_ticket(a.ticket, lane, nblocks));
    while (b != 0xFFFFFFFFu) {
        if (lane == 0 && a.ntok)
            a.ntok[b] = 0xFFFFFFFFu; // encoded here, not by k_encode_tokens
        compress_one_block<false>(a, b, lane, table, tbase, c2, c3, cB, cBn);
        b = uni(next_ticket(a.ticket, lane, nblocks));
    }
}

// ---------------------------------------------------------------------
// K1 with ONE wavefront per CU, the hash table AND the 64 KiB input block in
// LDS (32 KiB + 64 KiB + a line of slack: one such workgroup per CU): every
// load on the per-copy dependency chain is an LDS access - the shape
// BASELINE.json's north_star describes, for batches of a couple of blocks per
// CU at most.
// ---------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_compress_block_lds(CompressArgs a)
{
    __shared__ __attribute__((aligned(16))) uint16_t table_mem[kMaxTable];
    __shared__ __attribute__((aligned(16))) uint8_t block_mem[kMaxBlock + 32];

    const uint32_t lane = threadIdx.x;
    const lptr16 table = (lptr16)&table_mem[0];
    const uint32_t tbase = (uint32_t)(uintptr_t)table;
    const uint32_t nblocks = launch_blocks(a);
    const uint32_t c2 = lane >= 1 ? kDelta.d[lane - 1] : 0;
    const uint32_t c3 = kDelta.d[lane];
    const uint32_t cB = lane >= 2 ? 1 + kDelta.d[lane - 2] : lane - 1;
    const uint32_t cBn = lane >= 2 ? 1 + c2 : 0;
    uint32_t b = uni(next_ticket(a.ticket, lane, nblocks));
    while (b != 0xFFFFFFFFu) {
        if (lane == 0 && a.ntok)
            a.ntok[b] = 0xFFFFFFFFu;
        compress_one_block<true>(
            a, b, lane, table, tbase, c2, c3, cB, cBn,
            (__attribute__((address_space(3))) uint8_t *)block_mem);
        b = uni(next_ticket(a.ticket, lane, nblocks));
    }
}

} // namespace snapmi
#endif // SNAPMI_TESTING
