// snapmi_crc.hpp -- the arithmetic of masked CRC32C over buffers of any
// length (snapmi_crc32c_masked_batch), in plain C++ that the kernels, the host
// code and a CPU test (tests/crc_host.cpp) compile alike:
//
//   gf_mul            product of two polynomials over GF(2) mod P
//   crc_pow2_table    x^(8 * 2^k) mod P for k = 0..63, by repeated squaring
//   crc_pow8          x^(8 * t) mod P for a 64-bit t, from that table
//   crc_advance       a CRC state moved past t more bytes of message
//   crc_segments      segments of a buffer (0: the one-wavefront route has it)
//   crc_first_len     bytes of a buffer's first segment
//   crc_find_segment  segment number -> (buffer, segment, offset, bytes, tail)
//   crc_init_term     what the initial state 0xFFFFFFFF adds to a CRC
//   crc_mask          CheckSummer::crc32c_masked's last line
//
// A CRC state is a polynomial in the reflected representation (bit 31 = x^0),
// and the CRC register is linear over GF(2): with a zero initial state
//     state(A || B) = state(A) * x^(8 * |B|)  xor  state(B)        (mod P),
// and the initial state 0xFFFFFFFF adds 0xFFFFFFFF * x^(8 * len).  So a buffer
// cut into segments is the XOR, in any order, of every segment's own state
// advanced past the bytes behind it (its tail), plus the initial-state term.
//
// The cut: a buffer of more than kCrcShort bytes has k = ceil(len / S)
// segments; segment 0 is the first len - (k - 1) * S bytes (1..S of them),
// every later one is exactly S bytes.  Buffers of at most kCrcShort bytes have
// no segments: k_crc32c computes them on one wavefront.
//
// No HIP types, no allocation.
#pragma once

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define SNAPMI_CRC_HD __host__ __device__
#else
#define SNAPMI_CRC_HD
#endif

namespace snapmi {

constexpr uint32_t kCrcPoly = 0x82F63B78u; // reference build.rs:6
// longest buffer of the one-wavefront route (a frame chunk's 64 KiB)
constexpr uint64_t kCrcShort = 65536;
// S, a multiple of the 256 bytes a wavefront takes per step.  A step waits
// for its global load (about 0.4 us: 16 384 buffers of 64 KiB, 256 steps
// each, take 0.25 ms in two rounds of 8 192 resident wavefronts), so the rate
// is the number of wavefronts in flight: a device of 256 CUs wants 8 192
// segments, 8 per SIMD.  128 KiB gives 1 GiB that many, in one buffer or in
// sixteen; at 256 KiB (4 096 in flight) both ran at 0.61 of the short route's
// rate, at 128 KiB at 0.77.  What a segment costs on top of its 512 steps of
// 25 instructions - a power of x in six rounds of products and one more
// product, up to 32 rounds of 14 instructions each: 3 100 beside 13 000, and
// a search and an atomic - is what a smaller S would buy its parallelism
// with; 64 KiB doubles that share for buffers that fill the device anyway.
// (profiles/crc_long.json)
constexpr uint64_t kCrcSegment = 128 * 1024;
static_assert(kCrcSegment % 256 == 0 && kCrcSegment >= kCrcShort,
              "a segment is whole steps, and a split buffer is a long one");
constexpr uint32_t kCrcX0 = 0x80000000u; // the polynomial 1

// a * b mod P: a's coefficients from x^0 up, b times x on the way; ends with
// a's last coefficient, at once for a == 0 (the state of a segment of zero
// bytes is 0)
SNAPMI_CRC_HD inline uint32_t gf_mul(uint32_t a, uint32_t b)
{
    uint32_t p = 0;
    while (a) {
        if (a & kCrcX0)
            p ^= b;
        a <<= 1;
        b = (b & 1) ? (b >> 1) ^ kCrcPoly : b >> 1;
    }
    return p;
}

// pow2[k] = x^(8 * 2^k) mod P
inline void crc_pow2_table(uint32_t (&pow2)[64])
{
    pow2[0] = kCrcX0 >> 8; // x^8
    for (int k = 1; k < 64; k++)
        pow2[k] = gf_mul(pow2[k - 1], pow2[k - 1]);
}

// x^(8 * t) mod P: the product of the table's entries at t's set bits
SNAPMI_CRC_HD inline uint32_t crc_pow8(const uint32_t *pow2, uint64_t t)
{
    uint32_t p = kCrcX0;
    for (uint32_t k = 0; t; k++, t >>= 1)
        if (t & 1)
            p = gf_mul(p, pow2[k]);
    return p;
}

// the state `s` after t more bytes that are all zero - by linearity, what
// the bytes seen so far contribute to the state t bytes later
SNAPMI_CRC_HD inline uint32_t crc_advance(uint32_t s, uint32_t pow8_t)
{
    return gf_mul(s, pow8_t);
}

// the initial state's contribution to the state after len bytes
SNAPMI_CRC_HD inline uint32_t crc_init_term(uint32_t pow8_len)
{
    return gf_mul(0xFFFFFFFFu, pow8_len);
}

// reference src/crc32.rs:35-38, from the final state (before its complement)
SNAPMI_CRC_HD inline uint32_t crc_mask(uint32_t state)
{
    const uint32_t c = ~state;
    return ((c >> 15) | (c << 17)) + 0xA282EAD8u;
}

SNAPMI_CRC_HD inline uint64_t crc_segments(uint64_t len, uint64_t seg)
{
    return len > kCrcShort ? len / seg + (len % seg ? 1 : 0) : 0;
}

// (of a buffer that has segments: 1..seg bytes)
SNAPMI_CRC_HD inline uint64_t crc_first_len(uint64_t len, uint64_t seg)
{
    return len - (crc_segments(len, seg) - 1) * seg;
}

struct CrcSeg {
    uint32_t buffer;  // the buffer that owns the segment
    uint64_t segment; // its number inside the buffer
    uint64_t off;     // its first byte
    uint64_t len;     // its bytes
    uint64_t tail;    // the buffer's bytes behind it
};

// Segment s of the call, 0 <= s < first[n]: first[0..n] is the exclusive scan
// of the buffers' segment counts.  Its buffer is the last i with
// first[i] <= s - buffers without segments (short ones, empty ones) share
// their first[] with the buffer behind them and are never the last.
SNAPMI_CRC_HD inline CrcSeg crc_find_segment(const uint64_t *first,
                                             const uint64_t *lens, uint32_t n,
                                             uint64_t s, uint64_t seg)
{
    uint32_t lo = 0, hi = n - 1;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo + 1) / 2;
        if (first[mid] <= s)
            lo = mid;
        else
            hi = mid - 1;
    }
    CrcSeg r;
    const uint64_t len = lens[lo];
    const uint64_t head = crc_first_len(len, seg);
    r.buffer = lo;
    r.segment = s - first[lo];
    r.off = r.segment ? head + (r.segment - 1) * seg : 0;
    r.len = r.segment ? seg : head;
    r.tail = len - r.off - r.len;
    return r;
}

} // namespace snapmi
