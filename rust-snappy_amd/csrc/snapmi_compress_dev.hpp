// snapmi_compress_dev.hpp -- device-only helpers that more than one of the
// compressor's files use: the reference's hash and probe schedule, 16-byte
// loads and compares, the LDS exchange the window kernels rest on, the wave
// scan, what a token encodes to and the wavefront's token encoder (TokenSink),
// the wave-wide match extension, and the block tickets.
#pragma once

#include "snapmi_device.hpp"
#include "snapmi_kernels.hpp"

namespace snapmi {

namespace {

__device__ __forceinline__ uint32_t hash32(uint32_t x, uint32_t shift)
{
    return (x * 0x1E35A7BDu) >> shift; // reference src/compress.rs:523-525
}

// Offsets of the reference's probe schedule from the position where the
// probe loop is (re)entered: skip = 32; step = skip >> 5; skip += step
// (reference src/compress.rs:204-211).  d[i] is the i-th probed offset.
struct DeltaTable {
    uint32_t d[448];
};
constexpr DeltaTable make_delta()
{
    DeltaTable t{};
    uint32_t skip = 32, p = 0;
    for (int i = 0; i < 448; i++) {
        t.d[i] = p < 0x100000u ? p : 0x100000u;
        const uint32_t step = skip >> 5;
        p += step;
        skip += step;
    }
    return t;
}
__device__ const DeltaTable kDelta = make_delta();

// 16 unaligned bytes.
struct B16 {
    uint32_t w[4];
};
__device__ __forceinline__ B16 ld128u(gcptr p)
{
    B16 v;
    __builtin_memcpy(&v, p, 16);
    return v;
}

// the same loads from a copy of the block in LDS (k_compress_span_lds, the
// small-stream kernels of snapmi_compress.hip)
typedef const l_u8 *lcptr;
__device__ __forceinline__ B16 ld128u(lcptr p)
{
    B16 v;
    __builtin_memcpy(&v, p, 16);
    return v;
}
using snapmi::ld32u; // (the global-memory overload of snapmi_device.hpp)
__device__ __forceinline__ uint32_t ld32u(lcptr p)
{
    uint32_t v;
    __builtin_memcpy(&v, p, 4);
    return v;
}

// number of equal leading bytes of two 16-byte values (0..16)
__device__ __forceinline__ uint32_t common16(const B16 &a, const B16 &b)
{
    const uint64_t d0 = (((uint64_t)(a.w[1] ^ b.w[1])) << 32) | (a.w[0] ^ b.w[0]);
    const uint64_t d1 = (((uint64_t)(a.w[3] ^ b.w[3])) << 32) | (a.w[2] ^ b.w[2]);
    // branch-free on purpose: both halves are always needed, so the compiler
    // keeps the candidate read as one 16-byte load
    const uint32_t m0 = d0 ? (uint32_t)__builtin_ctzll(d0) >> 3 : 8u;
    const uint32_t m1 = d1 ? (uint32_t)__builtin_ctzll(d1) >> 3 : 8u;
    return m0 == 8 ? 8 + m1 : m0;
}

// ds_mskor_rtn_b32: MEM = (MEM & ~mask) | data, returns the old dword.
__device__ __forceinline__ uint32_t lds_mskor_rtn(uint32_t byte_addr,
                                                  uint32_t mask, uint32_t data)
{
    uint32_t old;
    asm volatile("ds_mskor_rtn_b32 %0, %1, %2, %3\n\ts_waitcnt lgkmcnt(0)"
                 : "=&v"(old)
                 : "v"(byte_addr), "v"(mask), "v"(data)
                 : "memory");
    return old;
}

// DPP helpers: wave64 inclusive add-scan without LDS (row_shr within rows of
// 16, then row_bcast:15 / row_bcast:31 across rows).
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ uint32_t dpp_add(uint32_t v)
{
    // lanes without a source (bound_ctrl) and rows outside ROW_MASK add 0
    const uint32_t t = (uint32_t)__builtin_amdgcn_update_dpp(
        0, (int)v, CTRL, ROW_MASK, 0xF, false);
    return v + t;
}
__device__ __forceinline__ uint32_t wave_inclusive_scan(uint32_t v)
{
    v = dpp_add<0x111, 0xF>(v); // row_shr:1
    v = dpp_add<0x112, 0xF>(v); // row_shr:2
    v = dpp_add<0x114, 0xF>(v); // row_shr:4
    v = dpp_add<0x118, 0xF>(v); // row_shr:8
    v = dpp_add<0x142, 0xA>(v); // row_bcast:15 -> rows 1,3
    v = dpp_add<0x143, 0xC>(v); // row_bcast:31 -> rows 2,3
    return v;
}

// Tokens of the greedy parse, one per lane, encoded 64 at a time.
//   a = literal length | copy offset << 16
//   b = copy length    | literal start << 16      (copy length 0: no copy)
// A token with neither literal nor copy is never recorded, so the pattern
// "both zero" encodes the one length that does not fit 16 bits: a 65536-byte
// literal (a whole block without a single match).
// Encoded size of one token = literal of L bytes, then a copy of C bytes at
// offset O (C = 0: none): reference emit_literal (src/compress.rs:433-474)
// and emit_copy (:323-369).  The match finder adds these up per block so the
// encoder can write every block at its final position.
__device__ __forceinline__ uint32_t token_bytes(uint32_t L, uint32_t C,
                                                uint32_t O)
{
    const uint32_t lt = L == 0 ? 0 : (L <= 60 ? 1 : (L <= 256 ? 2 : 3));
    const uint32_t n64 = C >= 68 ? (C - 4) >> 6 : 0;
    const uint32_t rem = C - (n64 << 6);
    const uint32_t mid = rem > 64 ? 1 : 0;
    const uint32_t fin_len = rem - 60 * mid;
    const uint32_t fin = C == 0 ? 0 : (fin_len <= 11 && O <= 2047 ? 2 : 3);
    return lt + L + 3 * (n64 + mid) + fin;
}

struct TokenSink {
    gcptr src;          // block input
    uint32_t n;         // block length
    gptr dst;           // block output
    uint32_t d;         // bytes written so far
    uint32_t a, b;      // this lane's token
    uint32_t t;         // tokens pending (uniform)
    uint32_t lane;

    __device__ __forceinline__ void init(gcptr s, uint32_t len, gptr o,
                                         uint32_t l)
    {
        src = s;
        n = len;
        dst = o;
        d = 0;
        a = b = 0;
        t = 0;
        lane = l;
    }

    __device__ __forceinline__ void record(uint32_t lit_start,
                                           uint32_t lit_len, uint32_t offset,
                                           uint32_t copy_len)
    {
        const bool me = lane == t;
        a = me ? ((lit_len & 0xFFFFu) | (offset << 16)) : a;
        b = me ? (copy_len | (lit_start << 16)) : b;
        t++;
        if (t == kWave)
            flush();
    }

    // the same without the flush: for a caller that makes room itself
    // (k_compress_spans: at most 17 tokens per step, one flush site)
    __device__ __forceinline__ void record_nf(uint32_t lit_start,
                                              uint32_t lit_len,
                                              uint32_t offset,
                                              uint32_t copy_len)
    {
        const bool me = lane == t;
        a = me ? ((lit_len & 0xFFFFu) | (offset << 16)) : a;
        b = me ? (copy_len | (lit_start << 16)) : b;
        t++;
    }

    // Encode the pending tokens: reference emit_literal (src/compress.rs:
    // 433-474) and emit_copy / emit_copy2 (:323-369), one token per lane.
    __device__ __forceinline__ void flush()
    {
        const bool act = lane < t;
        const uint32_t C = act ? (b & 0xFFFFu) : 0; // copy length
        uint32_t L = act ? (a & 0xFFFFu) : 0;       // literal length
        if (act && L == 0 && C == 0)
            L = kMaxBlock;
        const uint32_t O = a >> 16;                 // copy offset
        const uint32_t P = b >> 16;                 // literal start
        // literal tag size (:436-463)
        const uint32_t lt = L == 0 ? 0 : (L <= 60 ? 1 : (L <= 256 ? 2 : 3));
        // copy pieces (:339-356): n64 x copy2(64), maybe copy2(60), then the
        // tail as copy1 or copy2
        const uint32_t n64 = C >= 68 ? (C - 4) >> 6 : 0;
        const uint32_t rem = C - (n64 << 6);
        const uint32_t mid = rem > 64 ? 1 : 0;
        const uint32_t fin_len = rem - 60 * mid;
        const bool c1 = fin_len <= 11 && O <= 2047;
        const uint32_t fin = C == 0 ? 0 : (c1 ? 2 : 3);
        const uint32_t size = lt + L + 3 * (n64 + mid) + fin;
        const uint32_t incl = wave_inclusive_scan(size);
        gptr o = dst + d + (incl - size);
        d += rdlane(incl, kWave - 1);
        t = 0;

        // literal tag
        if (lt) {
            const uint32_t n1 = L - 1;
            if (lt == 1) {
                o[0] = (uint8_t)(n1 << 2);
            } else {
                o[0] = lt == 2 ? (60u << 2) : (61u << 2);
                o[1] = (uint8_t)n1;
                if (lt == 3)
                    o[2] = (uint8_t)(n1 >> 8);
            }
        }
        o += lt;
        // literal bytes, one lane per literal while they are short: up to
        // four 16-byte pieces, ALL loads first (one memory latency for the
        // whole literal instead of one per 4 bytes: the encoder's passes are
        // a chain of such latencies), then the stores - whole pieces as one
        // 16-byte store, the last one dword- and bytewise
        gcptr in = src + P;
        const uint32_t Lp = (L + 15u) & ~15u;
        if (L && L <= 64 && P + Lp <= n) {
            u32x4 v0 = {0, 0, 0, 0}, v1 = v0, v2 = v0, v3 = v0;
            v0 = ld128g(in);
            if (L > 16)
                v1 = ld128g(in + 16);
            if (L > 32)
                v2 = ld128g(in + 32);
            if (L > 48)
                v3 = ld128g(in + 48);
            typedef __attribute__((address_space(1))) u32x4 g_u32x4;
            typedef g_u32x4 __attribute__((aligned(1))) g_u32x4u;
            if (L >= 16)
                *(g_u32x4u *)o = v0;
            if (L >= 32)
                *(g_u32x4u *)(o + 16) = v1;
            if (L >= 48)
                *(g_u32x4u *)(o + 32) = v2;
            if (L >= 64)
                *(g_u32x4u *)(o + 48) = v3;
            // the last, partial piece (L & 15 bytes at o + (L & ~15))
            const uint32_t pk = L >> 4; // piece that holds it
            const u32x4 pv = pk == 0 ? v0 : (pk == 1 ? v1 : (pk == 2 ? v2 : v3));
            gptr po = o + (L & ~15u);
            const uint32_t r = L & 15u;
            if (r >= 4)
                st32u(po, pv.x);
            if (r >= 8)
                st32u(po + 4, pv.y);
            if (r >= 12)
                st32u(po + 8, pv.z);
            const uint32_t tl = r & 3u, tb = r & ~3u;
            const uint32_t ti = r >> 2; // dword holding the tail
            const uint32_t tw =
                ti == 0 ? pv.x : (ti == 1 ? pv.y : (ti == 2 ? pv.z : pv.w));
            if (tl >= 1)
                po[tb] = (uint8_t)tw;
            if (tl >= 2)
                po[tb + 1] = (uint8_t)(tw >> 8);
            if (tl >= 3)
                po[tb + 2] = (uint8_t)(tw >> 16);
        } else if (L && L <= 64) { // within 16 bytes of the block's end
            uint32_t i = 0;
            for (; i + 4 <= L; i += 4)
                st32u(o + i, ld32u(in + i));
            for (; i < L; i++)
                o[i] = in[i];
        }
        // copies
        gptr oc = o + L;
        const uint8_t olo = (uint8_t)O, ohi = (uint8_t)(O >> 8);
        for (uint32_t i = 0; i < n64; i++) {
            oc[0] = (uint8_t)((63u << 2) | 2u);
            oc[1] = olo;
            oc[2] = ohi;
            oc += 3;
        }
        if (mid) {
            oc[0] = (uint8_t)((59u << 2) | 2u);
            oc[1] = olo;
            oc[2] = ohi;
            oc += 3;
        }
        if (fin == 2) {
            oc[0] = (uint8_t)(((O >> 8) << 5) | ((fin_len - 4) << 2) | 1u);
            oc[1] = olo;
        } else if (fin == 3) {
            oc[0] = (uint8_t)(((fin_len - 1) << 2) | 2u);
            oc[1] = olo;
            oc[2] = ohi;
        }
        // long literals: the whole wave copies each (wave_copy)
        uint64_t longs = __ballot(L > 64);
        while (longs) {
            const uint32_t j = (uint32_t)__builtin_ctzll(longs);
            longs &= longs - 1;
            const uint32_t Lj = rdlane(L, j);
            const uint32_t Pj = rdlane(P, j);
            const uint64_t oj = ((uint64_t)rdlane((uint32_t)((uintptr_t)o >> 32), j) << 32) |
                                rdlane((uint32_t)(uintptr_t)o, j);
            wave_copy<true>((gptr)(uintptr_t)oj, src + Pj, Lj, lane);
        }
    }
};

// Continue a match past its first 16 bytes: common prefix of src[c..] and
// src[p..] bounded by the block end n, 256 bytes per wave instruction
// (reference extend_match, src/compress.rs:378-412).
template <class P>
__device__ __forceinline__ uint32_t extend_match(P src, uint32_t n,
                                                 uint32_t c, uint32_t p,
                                                 uint32_t lane)
{
    uint32_t len = 0;
    const uint32_t room = n - p;
    for (uint32_t pos = 0;; pos += 4 * kWave) {
        const uint32_t off = pos + 4 * lane;
        uint32_t eq = 0;
        if (off < room) {
            // dword loads clamped to the block; a clamped load is shifted so
            // the wanted bytes sit at the bottom (the rest is cut by `lim`)
            const uint32_t pa = c + off, pb = p + off;
            const uint32_t ca = pa < n - 4 ? pa : n - 4;
            const uint32_t cb = pb < n - 4 ? pb : n - 4;
            const uint32_t va = ld32u(src + ca) >> (8 * (pa - ca));
            const uint32_t vb = ld32u(src + cb) >> (8 * (pb - cb));
            const uint32_t x = va ^ vb;
            eq = x ? ((uint32_t)__builtin_ctz(x) >> 3) : 4u;
            const uint32_t lim = room - off;
            eq = eq < lim ? eq : lim;
        }
        const uint64_t stop = __ballot(eq < 4);
        if (stop == 0) {
            len += 4 * kWave;
            continue;
        }
        const uint32_t f = (uint32_t)__builtin_ctzll(stop);
        return len + 4 * f + rdlane(eq, f);
    }
}

} // namespace

// Device-wide block ticket, one 64-bit word: low half = blocks claimed from
// the front of the list (lane-per-block kernel), high half = blocks claimed
// from the back (a wavefront-per-block kernel).  The two kernels run
// concurrently and meet in the middle; a claim is valid while front + back
// < nblocks.  Lane 0 takes the ticket, the wavefront shares it.  Returns the
// block index or 0xFFFFFFFF.
inline __device__ __noinline__ uint32_t next_ticket(uint32_t *ticket,
                                                    uint32_t lane,
                                                    uint32_t nblocks)
{
    uint32_t blk = 0;
    if (lane == 0) {
        const unsigned long long old =
            atomicAdd((unsigned long long *)ticket, 1ull << 32);
        const uint32_t front = (uint32_t)old, back = (uint32_t)(old >> 32);
        blk = (uint64_t)front + back < nblocks ? nblocks - 1 - back
                                               : 0xFFFFFFFFu;
    }
    return uni(blk);
}

// the same for a kernel that takes blocks from the front only
inline __device__ __noinline__ uint32_t next_front_ticket(uint32_t *ticket,
                                                          uint32_t lane)
{
    uint32_t t = 0;
    if (lane == 0)
        t = atomicAdd(ticket, 1u);
    return uni(t);
}
// the two-ended ticket over the blocks [lo, hi) of a segment: the next block
// from the BACK (the lane kernel counts the low word up from the front)
inline __device__ __noinline__ uint32_t next_back_ticket(uint32_t *ticket,
                                                         uint32_t lane,
                                                         uint32_t lo,
                                                         uint32_t hi)
{
    uint32_t blk = 0;
    if (lane == 0) {
        const unsigned long long old =
            atomicAdd((unsigned long long *)ticket, 1ull << 32);
        const uint32_t front = (uint32_t)old, back = (uint32_t)(old >> 32);
        blk = hi > lo && (uint64_t)front + back < hi - lo ? hi - 1 - back
                                                          : 0xFFFFFFFFu;
    }
    return uni(blk);
}

// ds_mskor_b32: the same exchange without the old value
__device__ __forceinline__ void lds_mskor(uint32_t byte_addr, uint32_t mask,
                                          uint32_t data)
{
    asm volatile("ds_mskor_b32 %0, %1, %2"
                 :
                 : "v"(byte_addr), "v"(mask), "v"(data)
                 : "memory");
}

} // namespace snapmi
