// snapmi_device.hpp -- shared device-side helpers for the gfx950 Snappy codec.
//
// Everything here is written for CDNA4 wave64: one wavefront executes the
// sequential Snappy semantics of one block / one stream with its state in
// SGPRs (wave-uniform values), and uses the 64 lanes for the byte work
// (match extension, literal copies, back-reference copies).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "snapmi.h"
#include "snapmi_block.hpp"
#include "snapmi_element.hpp"
#include "snapmi_piecelist.hpp"

namespace snapmi {

constexpr uint32_t kWave = 64;
// (the codec's constants - kMaxBlock, kMaxTable, kSlotBytes ... - with
// max_compress_len_u64 and varint_len: snapmi_block.hpp)

// Explicit address spaces.  Pointers fetched from the descriptor arrays are
// generic to the compiler; without these it emits flat_load/flat_store, which
// count against both vmcnt and lgkmcnt and so serialise LDS and HBM waits.
typedef __attribute__((address_space(1))) uint8_t g_u8;
typedef g_u8 *gptr;        // global (HBM) bytes
typedef const g_u8 *gcptr; // global (HBM) bytes, read only
typedef __attribute__((address_space(3))) uint8_t l_u8; // LDS
typedef __attribute__((address_space(3))) uint16_t l_u16x;
typedef __attribute__((address_space(3))) uint32_t l_u32;
typedef __attribute__((address_space(3))) uint16_t l_u16;
typedef l_u16 *lptr16; // LDS u16
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ uint32_t uni(uint32_t v)
{
    return __builtin_amdgcn_readfirstlane(v);
}

// v_readlane_b32 with a wave-uniform lane index.  The builtin returns int:
// always go through this wrapper so the value is never sign-extended.
__device__ __forceinline__ uint32_t rdlane(uint32_t v, uint32_t lane)
{
    return (uint32_t)__builtin_amdgcn_readlane((int)v, (int)lane);
}

__device__ __forceinline__ uint64_t uni64(uint64_t v)
{
    uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v);
    uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
    return ((uint64_t)hi << 32) | lo;
}

// gfx950 global memory takes unaligned dword accesses; the compiler emits a
// single global_load_dword / global_store_dword for these.
__device__ __forceinline__ uint32_t ld32u(gcptr p)
{
    uint32_t v;
    __builtin_memcpy(&v, p, 4);
    return v;
}

__device__ __forceinline__ void st32u(gptr p, uint32_t v)
{
    __builtin_memcpy(p, &v, 4);
}

// 16 bytes from global memory at any alignment (one global_load_dwordx4)
__device__ __forceinline__ u32x4 ld128g(gcptr p)
{
    u32x4 v;
    __builtin_memcpy(&v, p, 16);
    return v;
}

// The whole wave copies len bytes (a long literal), touching exactly
// from[0..len) and to[0..len): the destination is brought to a 16-byte
// boundary, then 16 bytes per lane, 1 KiB per instruction - and with kRows4
// four such rows in flight per trip, for a kernel that has the registers (the
// decoders run 8 waves per SIMD and get their loads in flight from that) -
// the rest bytewise.  Long literals are the whole of an incompressible
// stream.  The source may have any alignment.
template <bool kRows4>
__device__ __forceinline__ void wave_copy(gptr to, gcptr from, uint64_t len,
                                          uint32_t lane)
{
    uint32_t head = (uint32_t)((16 - ((uintptr_t)to & 15)) & 15);
    if (head > len)
        head = (uint32_t)len;
    if (lane < head)
        to[lane] = from[lane];
    const uint64_t body = (len - head) & ~15ull;
    gptr t = to + head;
    gcptr f = from + head;
    typedef __attribute__((address_space(1))) u32x4 g_u32x4;
    uint64_t i = 16 * lane;
    for (; kRows4 && i + 3072 < body; i += 4096) {
        const u32x4 v0 = ld128g(f + i), v1 = ld128g(f + i + 1024),
                    v2 = ld128g(f + i + 2048), v3 = ld128g(f + i + 3072);
        *(g_u32x4 *)(t + i) = v0;
        *(g_u32x4 *)(t + i + 1024) = v1;
        *(g_u32x4 *)(t + i + 2048) = v2;
        *(g_u32x4 *)(t + i + 3072) = v3;
    }
    for (; i < body; i += 1024) {
        *(g_u32x4 *)(t + i) = ld128g(f + i);
    }
    const uint32_t tail = (uint32_t)(len - head - body);
    if (lane < tail)
        t[body + lane] = f[body + lane];
}

// Dword at base[pos..pos+4) where only base[0..avail) may be touched; bytes
// past `avail` read as zero.
__device__ __forceinline__ uint32_t ld32g(gcptr base, uint64_t pos,
                                          uint64_t avail)
{
    if (pos + 4 <= avail)
        return ld32u(base + pos);
    uint32_t v = 0;
    for (uint32_t k = 0; k < 3; k++)
        if (pos + k < avail)
            v |= (uint32_t)base[pos + k] << (8 * k);
    return v;
}

__device__ __forceinline__ void set_error(snapmi_error *errs, uint64_t i,
                                          int kind, uint64_t a, uint64_t b,
                                          uint64_t c)
{
    elem_fail(errs, i, kind, a, b, c);
}

// A stream of the batch decoder is finished: its error (or SNAPMI_OK) and the
// bytes it produced - none where it failed.
__device__ __forceinline__ void stream_done(snapmi_error *errs,
                                            uint64_t *out_lens, uint64_t i,
                                            int kind, uint64_t a, uint64_t b,
                                            uint64_t c, uint64_t out_len)
{
    set_error(errs, i, kind, a, b, c);
    out_lens[i] = out_len;
}

// ... with an error, inside a decoder that has `a` and `st`: `who` writes it
// (lane 0 of a wavefront; a lane with a stream of its own), all return `ret`.
#define SNAPMI_FAIL(who, ret, kind, fa, fb, fc)                               \
    do {                                                                      \
        if (who)                                                              \
            stream_done(a.errs, a.out_lens, st, (kind), (fa), (fb), (fc), 0); \
        return ret;                                                           \
    } while (0)

// Slot k of a piece-descriptor list (snapmi_piecelist.hpp) as whoever cuts
// the pieces hands it to the batch decoder: these in_len bytes into this room
// of cap bytes, mode m, nothing produced yet and no error.  piece_put stores
// the error's kind alone (a decoder that reports another kind writes the other
// fields beside it); piece_put_err a whole error of the caller's.
__device__ __forceinline__ void piece_put_fields(const PieceList &l,
                                                 uint64_t k, const void *in,
                                                 uint64_t in_len, void *out,
                                                 uint64_t cap, uint8_t mode)
{
    l.c_in[k] = in;
    l.c_inlen[k] = in_len;
    l.c_out[k] = out;
    l.c_cap[k] = cap;
    l.c_outlen[k] = 0;
    l.c_mode[k] = mode;
}

__device__ __forceinline__ void piece_put(const PieceList &l, uint64_t k,
                                          const void *in, uint64_t in_len,
                                          void *out, uint64_t cap,
                                          uint8_t mode)
{
    piece_put_fields(l, k, in, in_len, out, cap, mode);
    l.c_err[k].kind = SNAPMI_OK;
}

__device__ __forceinline__ void piece_put_err(const PieceList &l, uint64_t k,
                                              const void *in, uint64_t in_len,
                                              void *out, uint64_t cap,
                                              uint8_t mode,
                                              const snapmi_error &err)
{
    piece_put_fields(l, k, in, in_len, out, cap, mode);
    l.c_err[k] = err;
}

// The piece of slot k came out whole: it was the decoder's (mode 2), reports
// OK and filled its room.
__device__ __forceinline__ bool piece_whole(const PieceList &l, uint64_t k)
{
    return l.c_mode[k] == 2 && l.c_err[k].kind == SNAPMI_OK &&
           l.c_outlen[k] == l.c_cap[k];
}

// varint_read / header_read of snapmi_element.hpp over global memory
// (executed redundantly by every lane on uniform data)
__device__ __forceinline__ uint32_t read_varint(gcptr p, uint64_t n,
                                                uint64_t *value)
{
    return varint_read(bytes_at(p), n, value);
}

__device__ __forceinline__ int read_header(gcptr in, uint64_t in_len,
                                           uint32_t *hdr, uint64_t *dlen,
                                           snapmi_error *errs, uint64_t i)
{
    return header_read(bytes_at(in), in_len, hdr, dlen, errs, i);
}

// A 256-byte window of a byte stream held in one VGPR: lane i owns the dword
// at stream offset base + 4*i.  A wave-uniform position inside the window is
// read with two v_readlane + one 64-bit scalar shift, i.e. without a memory
// round trip.  Refills are one coalesced 256-byte global load.
struct ByteWindow {
    gcptr src;          // stream start
    uint64_t avail;     // readable bytes from src
    uint64_t base;      // stream offset of lane 0's dword
    uint32_t v;         // this lane's dword

    __device__ __forceinline__ void init(gcptr s, uint64_t a)
    {
        src = s;
        avail = a;
        base = ~0ull;
        v = 0;
    }
    __device__ __forceinline__ void refill(uint64_t pos)
    {
        base = pos;
        v = ld32g(src, pos + 4 * (threadIdx.x & 63), avail);
    }
    // dwords idx, idx+1 (idx uniform)
    __device__ __forceinline__ uint64_t pair(uint32_t idx) const
    {
        uint32_t lo = rdlane(v, idx);
        uint32_t hi = rdlane(v, idx + 1);
        return ((uint64_t)hi << 32) | lo;
    }
    // u32 at uniform stream offset p (bytes past avail read as zero)
    __device__ __forceinline__ uint32_t get32(uint64_t p)
    {
        if (p < base || p - base > 248)
            refill(p);
        uint32_t o = (uint32_t)(p - base);
        return (uint32_t)(pair(o >> 2) >> (8 * (o & 3)));
    }
};

} // namespace snapmi
