// snapmi - the plan of the long-stream decoder (scan, levels, chain, cuts,
// pieces: the k_bstream_* kernels) for one raw stream or the long streams of
// a small batch: geometry, workgroups, and where every table and descriptor
// lies in the scratch.  Plain functions, no HIP, so that
// tests/test_streamplan_cpu.py can pin them on the CPU; with them what the
// launches are handed (StreamArgs, BatchStreams) and the rule that sends a
// stream this way (long_stream_rule; LongItem).  Its users in the library:
// snapmi_longstream.hip (the kernels, snapmi_decompress_stream,
// decompress_batch_long), snapmi_index.hip (snapmi_build_block_index) and
// snapmi_api.hip (the rule, for the scalar calls).
#pragma once
#include <cstddef>
#include <cstdint>

#include "snapmi_piecelist.hpp"

#if defined(__HIPCC__)
#define SNAPMI_SP_HD __host__ __device__
#else
#define SNAPMI_SP_HD
#endif

namespace snapmi {

// The element chain is sequential, so it is resolved hierarchically first:
// per 4 KiB segment and per 256 KiB super-segment, "if an element starts at
// offset o (< kEntry) of this piece, where does the chain leave it and how many
// bytes has it produced".
constexpr uint32_t kSeg = 4096;           // bytes of compressed input
// Entry offsets tabulated per segment / child: a chain is followed from the
// first kEntry bytes behind a boundary.  8 instead of a full wavefront of 64:
// the 64 chains of a segment merge within a few elements, so most of the
// scan's hops were duplicates; a wavefront now scans eight segments (one raw
// stream of 3 GiB: 52 -> 119 GiB/s; 16 entries gave 103, 4 gave 123 within
// noise of 8).  A literal of 9-60 bytes that straddles a boundary jumps over
// the landing zone and costs one more segment of hops: rare next to the 8x.
constexpr uint32_t kEntry = 8;
constexpr uint32_t kSegPerSuper = 64;
constexpr uint32_t kCutSegs = 512; // segments per wavefront of k_bstream_cuts
constexpr uint32_t kScanSegs = 64; // ... of k_bstream_scan, at most
// wavefronts a scan launch should have before its wavefronts own that many
// segments each (StreamArgs::scan_segs)
constexpr uint32_t kScanFill = 1024;
constexpr uint32_t kStreamChunk = 65536;  // output bytes per piece: the
                                          // encoders' block size, so pieces
                                          // of their streams are independent

// Segment size of the scan of long streams (k_bstream_scan and the levels
// above it): 4 KiB when there is enough of them to fill the chip with walks
// (one 2 GiB stream: 2.0 ms of scan at 280 GiB/s), 1 KiB below that - the
// scan of a few hundred KiB is then a wait for the longest walk of ONE
// wavefront, ~1 200 hops of ~630 cycles in a 4 KiB segment (0.5 ms whatever
// the size), and a quarter of that with four times the lanes.  `forced`: the
// context's test option (0 = by size).
inline uint32_t stream_seg_log2(uint32_t forced, uint64_t long_bytes)
{
    if (forced)
        return forced;
    return long_bytes < ((uint64_t)256 << 20) ? 10u : 12u;
}

// Segments per wavefront of k_bstream_scan (StreamArgs::scan_segs) for a call
// whose long streams hold `nseg` segments together: the kernel's full group of
// 64 when that still makes kScanFill wavefronts, else halved until it does
// (not below 8).  A scan wavefront of 64 segments of 1 KiB hands its 64 lanes
// eight rounds of entry walks and then trunks of which the longest is three
// to four times the average - ~1 100 hops of ~630 cycles, 280 us, whoever
// else is on the chip - and 32 MiB of long streams are 506 such wavefronts,
// two per CU.  Measured (profiles/r5_scan_groups.txt): 64 MiB of the corpus
// round 1.359 -> 1.301 ms per call with 16 (8: 1.357 - the groups are a
// second wave of workgroups then), one 126 MB stream as a batch of one 1.690
// -> 1.585 with 32, Decoder::decompress of lcet10.txt 1.076 -> 0.993 with 8,
// 256 MiB 1.622 with 64 and 1.702 with 32: hence 1 024.  (The cuts kernel's
// 512 segments per wavefront were measured the same way: 64 .. 512 are equal,
// its time is the one walk every lane has.)  `forced`: the context's test
// option (0 = by size).
inline uint32_t stream_scan_segs(uint32_t forced, uint64_t nseg)
{
    if (forced)
        return forced;
    uint32_t segs = kScanSegs;
    while (segs > 8 && nseg / segs < kScanFill)
        segs /= 2;
    return segs;
}

// Output bound of a lone stream (snapmi_decompress_stream), which has not been
// looked at: the caller's buffer, and no more than ~21.4x the input (a 3-byte
// copy element yields at most 64 bytes).  A batch's long streams have their
// announced length instead (k_long_plan).
inline uint64_t lone_stream_bound(uint64_t in_len, uint64_t out_cap)
{
    if (in_len < (1ull << 40) && in_len * 22 < out_cap)
        return in_len * 22;
    return out_cap;
}

// Is a raw stream of `len` compressed bytes that announces `dl` bytes of
// output worth cutting into pieces (ten small launches, ~0.5 ms, instead of
// one wavefront at 0.14 GiB/s of elements or 0.85 GB/s of literal bytes)?
// From min_len (32 KiB) on when it expands by half and fills a piece and a
// half; from 256 KiB on whatever it holds (profiles/r4_scalar_latency.txt).
SNAPMI_SP_HD inline bool long_stream_rule(unsigned long long len,
                                          unsigned long long dl,
                                          unsigned long long min_len)
{
    const bool sane = dl / 22 <= len && 2 * dl >= 3ull * kStreamChunk;
    return sane && len >= min_len &&
           (2 * dl >= 3 * len || len >= (256ull << 10));
}
struct LongItem { // what k_long_plan hands to the host
    uint32_t idx, pad;
    unsigned long long in_len, dlen;
    const void *in;
    void *out;
    unsigned long long out_cap;
};

// the kernels with more than one workgroup per stream; the launch of each has
// an exclusive prefix of its workgroups over the streams (BatchStreams::pre)
enum StreamKernel { kPScan, kPSuper, kPSuper3, kPSpread3, kPSpread2, kPCuts,
                    kPPieces, kPre };

// One long raw stream decoded by many wavefronts (snapmi_decompress_stream,
// and the long streams of a small batch): what every k_bstream_* kernel is
// handed of it.
struct StreamArgs {
    const uint8_t *in;
    unsigned long long in_len;
    uint8_t *out;
    unsigned long long out_cap;
    unsigned long long *out_len; // [1]
    snapmi_error *err;           // [1]
    // meta[0] header bytes, [1] decoded length, [2] 0 = pieces decode it,
    // 1 = the sequential decoder must (error, or a stream whose pieces are
    // not independent), [3] pieces
    unsigned long long *meta;
    // per level (4 KiB, 256 KiB, 16 MiB blocks): tables of (exit, produced)
    // per entry offset < kEntry - level 1 [segments * kEntry], levels 2 and 3
    // [blocks * 64 children * 64] - and entries [blocks] of (position,
    // produced) where the chain enters each block (~0 = it does not)
    unsigned long long *s1, *s2, *s3;
    unsigned long long *e1, *e2, *e3;
    unsigned long long *cuts;     // [(kmax + 1) * 2] (src, dst) of piece k
    uint32_t nseg, nsuper, nsuper3, kmax;
    // log2 of the segment size of this call (12 = kSeg; 10 for streams that
    // are short enough for the scan to be a wait for its longest walk: a
    // quarter of the hops per lane, four times the lanes - round 5)
    uint32_t seg_log2;
    // segments a wavefront of k_bstream_scan owns: kScanSegs when that still
    // makes kScanFill wavefronts, fewer (a power of two from 8) when it does
    // not - a scan wavefront is as slow as the chain of walks its lanes are
    // handed, ~630 cycles a hop whoever else is on the chip
    // (stream_scan_segs)
    uint32_t scan_segs;
    // its piece descriptors, [kmax], for the batch decoder
    PieceList c;
    // a long stream of a batch: where k_bstream_finish says whether the
    // launch behind it must decode the stream (0) or not (3); else nullptr
    uint8_t *fb_mode;
};
// (plan_streams sizes the descriptor block of a launch with it)
static_assert(sizeof(StreamArgs) == 200, "StreamArgs sizes the descriptor block");
// the long streams of a batch (a lone stream is a batch of one): their
// descriptors and, per kernel, the first workgroup of every stream (nullptr:
// one workgroup each)
struct BatchStreams {
    const StreamArgs *descs;
    const uint32_t *pre; // [n + 1]
    uint32_t n;
};

// One stream of a plan.  in_len and bound are the caller's; plan_streams
// fills in the rest.
struct StreamSlot {
    uint64_t in_len, bound;
    uint32_t nseg, nsuper, nsuper3, kmax; // pieces: one per 64 KiB of bound
    // byte offsets into sd_tables: meta [8], e-tables [blocks * 2] per level,
    // (exit, produced) tables, cuts [(kmax + 1) * 2] (unsigned long long)
    size_t meta, e1, e2, e3, s1, s2, s3, cuts;
    size_t entry; // its first piece in the descriptor arrays of sd_desc
};

// Its PieceOffsets base lays out sd_desc: the piece descriptors of all
// streams, an array per field (snapmi_piecelist.hpp).
struct StreamPlan : PieceOffsets {
    uint32_t n;
    uint32_t seg_log2, scan_segs;
    bool fits; // every nseg and kmax under 2^30 (else nothing below is set)
    uint32_t grid[kPre];   // workgroups of each prefixed launch
    // sd_tables: the meta of all streams, the e-tables of all streams (one
    // 0xFF fill of e_bytes from e_off), then per stream s1, s2, s3, cuts
    size_t e_off, e_bytes, t_bytes;
    // sd_desc: `pieces` slots at the offsets of the base; d_bytes is its
    // `total`, named like the other sizes to reserve
    size_t pieces, d_bytes;
    // descriptor block: n descriptors of desc_size bytes, then the prefixes
    // [kPre][n + 1] (uint32_t)
    size_t pre_off, desc_bytes;
};

// Plans the n streams of slot[] (in_len, bound set) and writes the exclusive
// workgroup prefixes of every prefixed kernel to pre[kPre * (n + 1)], each
// with its total last.  The scan's groups follow the lone stream's segments
// when `lone`, and the batch's long bytes per segment plus one per stream
// otherwise - the two callers' rules, which differ by one segment for a
// single stream that is not a multiple of a segment long.
inline StreamPlan plan_streams(StreamSlot *slot, uint32_t n, bool lone,
                               uint32_t forced_seg_log2,
                               uint32_t forced_scan_segs, size_t desc_size,
                               uint32_t *pre)
{
    StreamPlan p = {};
    p.n = n;
    uint64_t long_bytes = 0;
    for (uint32_t j = 0; j < n; j++)
        long_bytes += slot[j].in_len;
    p.seg_log2 = stream_seg_log2(forced_seg_log2, long_bytes);
    const uint64_t seg = 1ull << p.seg_log2;
    p.fits = true;
    for (uint32_t j = 0; j < n; j++) {
        const uint64_t nseg = (slot[j].in_len + seg - 1) / seg + 1;
        const uint64_t kmax = slot[j].bound / kStreamChunk + 2;
        if (nseg > 0x3FFFFFFFu || kmax > 0x3FFFFFFFu) {
            p.fits = false;
            return p;
        }
        StreamSlot &g = slot[j];
        g.nseg = (uint32_t)nseg;
        g.nsuper = (g.nseg + kSegPerSuper - 1) / kSegPerSuper;
        g.nsuper3 = (g.nsuper + kSegPerSuper - 1) / kSegPerSuper;
        g.kmax = (uint32_t)kmax;
    }
    p.scan_segs = stream_scan_segs(forced_scan_segs,
                                   lone ? slot[0].nseg : long_bytes / seg + n);
    p.e_off = (size_t)n * 64;
    for (uint32_t j = 0; j < n; j++) {
        const StreamSlot &g = slot[j];
        p.e_bytes += ((size_t)g.nseg + g.nsuper + g.nsuper3) * 16;
    }

    const size_t st = (size_t)n + 1;
    size_t e = p.e_off, t = p.e_off + p.e_bytes;
    for (uint32_t j = 0; j < n; j++) {
        StreamSlot &g = slot[j];
        const uint32_t wgs[kPre] = {(g.nseg + p.scan_segs - 1) / p.scan_segs,
                                    g.nsuper,
                                    g.nsuper3,
                                    (g.nsuper3 + 63) / 64,
                                    (g.nsuper + 63) / 64,
                                    (g.nseg + kCutSegs - 1) / kCutSegs,
                                    (g.kmax + 255) / 256};
        for (int k = 0; k < kPre; k++) { // exclusive prefix, total last
            pre[k * st + j] = p.grid[k];
            p.grid[k] += wgs[k];
        }
        g.meta = (size_t)j * 64;
        g.e1 = e;
        g.e2 = g.e1 + (size_t)g.nseg * 16;
        g.e3 = g.e2 + (size_t)g.nsuper * 16;
        e = g.e3 + (size_t)g.nsuper3 * 16;
        g.s1 = t;
        g.s2 = g.s1 + (size_t)g.nseg * kEntry * 16;
        g.s3 = g.s2 + (size_t)g.nsuper * kSegPerSuper * kEntry * 16;
        g.cuts = g.s3 + (size_t)g.nsuper3 * kSegPerSuper * kEntry * 16;
        t = g.cuts + ((size_t)g.kmax + 1) * 16;
        g.entry = p.pieces;
        p.pieces += g.kmax;
    }
    for (int k = 0; k < kPre; k++)
        pre[k * st + n] = p.grid[k];
    p.t_bytes = t + 64;

    static_cast<PieceOffsets &>(p) = piece_offsets(p.pieces);
    p.d_bytes = p.total;

    p.pre_off = (size_t)n * desc_size;
    p.desc_bytes = p.pre_off + (size_t)kPre * st * sizeof(uint32_t);
    return p;
}

} // namespace snapmi
