// snapmi_hostbatch.hpp -- the plan of the host-memory batch calls
// (snapmi_compress_batch_host / snapmi_decompress_batch_host and their
// frame_ forms, snapmi_hostbatch.hip), in plain C++ that the host code, the pack kernel and
// a CPU test (tests/hostbatch_host.cpp) compile alike:
//
//   hb_plan_slice   which streams form the next slice of a batch, where each
//                   of them lies in the slice's device input slab and in its
//                   device output slab, and how large both slabs are
//   hb_find_stream  the tile -> stream mapping of k_hb_pack: the stream a byte
//   hb_tile         of the packed output belongs to, the streams a tile
//   hb_unit         covers, and what the thread that owns a 16-byte unit of
//                   it copies
//
// No HIP types, no allocation.
#pragma once

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define SNAPMI_HB_HD __host__ __device__
#else
#define SNAPMI_HB_HD
#endif

namespace snapmi {

// every stream starts on a 16-byte boundary, in every slab and in the packed
// output: k_hb_pack's loads and stores are 16 bytes wide
constexpr uint64_t kHbAlign = 16;
// bytes the codec kernels may read behind an input stream (their wide loads)
constexpr uint64_t kHbInSlack = 16;
// k_hb_pack: packed bytes per tile = one 16-byte unit per thread of a
// workgroup of 256
constexpr uint32_t kHbTile = 4096;
constexpr uint32_t kHbUnit = 16;
// most streams of one slice whatever their lengths (a million empty streams
// must not make one slice's descriptors unbounded)
constexpr size_t kHbMaxSliceStreams = (size_t)1 << 20;

SNAPMI_HB_HD inline uint64_t hb_align(uint64_t x)
{
    return (x + (kHbAlign - 1)) & ~(kHbAlign - 1);
}

// One slice: streams [s0, s1) of the batch.
struct HbSlice {
    size_t s0, s1;
    uint64_t in_raw;    // sum of the streams' input lengths
    uint64_t in_bytes;  // device input slab (every stream + kHbInSlack, aligned)
    uint64_t out_bytes; // device output slab (every stream's room, aligned)
};

// The slice that starts at stream s0 (s0 < n).  in_lens[i]: input bytes of
// stream i; rooms[i]: bytes the codec may write for it (compress:
// max_compress_len / frame_max_len, decompress: the header's length / what
// the chunk headers announce; 0 for a stream that will be refused).  Streams are added in order while the slice's input
// stays within in_limit and its rooms within out_limit; a stream that alone
// exceeds either is a slice of its own.  in_offs / out_offs (each s1 - s0
// values when not NULL, indexed i - s0) receive the streams' offsets in the
// two slabs.
inline HbSlice hb_plan_slice(const size_t *in_lens, const uint64_t *rooms,
                             size_t n, size_t s0, uint64_t in_limit,
                             uint64_t out_limit, uint64_t *in_offs,
                             uint64_t *out_offs)
{
    HbSlice x{s0, s0, 0, 0, 0};
    uint64_t out_raw = 0;
    while (x.s1 < n && x.s1 - x.s0 < kHbMaxSliceStreams) {
        const uint64_t len = in_lens[x.s1], room = rooms[x.s1];
        if (x.s1 > x.s0 &&
            (x.in_raw + len > in_limit || out_raw + room > out_limit))
            break;
        if (in_offs)
            in_offs[x.s1 - x.s0] = x.in_bytes;
        if (out_offs)
            out_offs[x.s1 - x.s0] = x.out_bytes;
        x.in_raw += len;
        out_raw += room;
        x.in_bytes += hb_align(len + kHbInSlack);
        x.out_bytes += hb_align(room);
        x.s1++;
    }
    return x;
}

// ---------------------------------------------------------------------
// The packed output of a compress slice: stream i's bytes at offs[i], where
// offs is the exclusive scan of hb_align(out_len) of the streams that
// succeeded and 0 for those that failed (offs[n] = the packed total).  The
// work unit is a tile of kHbTile packed bytes, not a stream: a tile finds the
// streams it covers by binary search, a thread the stream of its own 16-byte
// unit.  Every unit begins inside exactly one stream (streams start on unit
// boundaries and their padding is shorter than a unit).
// ---------------------------------------------------------------------

// the largest s in [lo, hi) with offs[s] <= p; needs offs[lo] <= p, lo < hi.
// Streams of size 0 (empty, failed) share their offset with the stream
// behind them and are never the answer for a p below the total.
SNAPMI_HB_HD inline uint32_t hb_find_stream(const uint64_t *offs, uint32_t lo,
                                            uint32_t hi, uint64_t p)
{
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (offs[mid] <= p)
            lo = mid;
        else
            hi = mid;
    }
    return lo;
}

// tile t of the packed output (t * kHbTile < total = offs[n]): its first and
// last byte and the streams they lie in
struct HbTile {
    uint64_t start, last;
    uint32_t s_lo, s_hi;
};

SNAPMI_HB_HD inline HbTile hb_tile(const uint64_t *offs, uint32_t n,
                                   uint64_t total, uint64_t t)
{
    HbTile x;
    x.start = t * kHbTile;
    x.last = (x.start + kHbTile < total ? x.start + kHbTile : total) - 1;
    x.s_lo = hb_find_stream(offs, 0, n, x.start);
    x.s_hi = hb_find_stream(offs, x.s_lo, n, x.last);
    return x;
}

struct HbUnit {
    uint32_t stream;  // the stream the unit at packed offset p lies in
    uint32_t bytes;   // 1..16: what of the unit is that stream's
    uint64_t src_off; // offset inside the stream (a multiple of 16)
};

// the unit at packed offset p (a multiple of 16 below offs[n]); [s_lo, s_hi]
// are the streams of the first and the last byte of its tile
SNAPMI_HB_HD inline HbUnit hb_unit(const uint64_t *offs, const uint64_t *lens,
                                   uint32_t s_lo, uint32_t s_hi, uint64_t p)
{
    HbUnit u;
    u.stream = hb_find_stream(offs, s_lo, s_hi + 1, p);
    u.src_off = p - offs[u.stream];
    const uint64_t rem = lens[u.stream] - u.src_off;
    u.bytes = rem < kHbUnit ? (uint32_t)rem : kHbUnit;
    return u;
}

} // namespace snapmi
