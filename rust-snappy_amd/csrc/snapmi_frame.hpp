// snapmi_frame.hpp -- private: what the files of the frame layer share.
//
//   snapmi_crc.hip       masked CRC32C (launch_crc32c)
//   snapmi_frame.hip     compress side (frame_compress_list)
//   snapmi_framedec.hip  decode side (frame_decompress_batch_listed)
//   snapmi_hostpipe.hip  the host-buffer calls over the two
//
// The first part is plain C++ that a host compiler takes as well
// (tests/test_carve_cpu.py): the kernels' argument blocks and, for each
// scratch buffer that holds their arrays, the one layout function that both
// sizes and places them (snapmi_carve.hpp).  The second part, under hipcc
// only, declares the functions one file offers the others.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "snapmi.h"
#include "snapmi_carve.hpp"
#include "snapmi_framewalk.hpp"

namespace snapmi {

constexpr uint32_t kFrameSlot = 76496;          // kMaxChunk rounded to 16
// (kMaxChunk, FrameChunk and the chunk-header walk: snapmi_framewalk.hpp)

// candidates kept per segment of the parallel header walk (k_fw_*)
constexpr uint32_t kFwCands = 32;

// ---------------------------------------------------------------------
// decode side: the fronts of a lone stream
// ---------------------------------------------------------------------
// The fronts of a lone stream's decode (snapmi_frame_decompress[_ex]): the
// side-index check, the parallel header walk and the sequential walk.  Each
// leaves the stream's chunk table as a batch of one stream, in the layout of
// FrameBatchDecodeArgs below, for the kernels behind it.
struct FrameDecodeArgs {
    const uint8_t *in;
    uint64_t in_len;
    uint8_t *out; // may be nullptr (lengths only)
    uint64_t out_cap;
    const uint64_t *index; // optional chunk header offsets
    uint32_t n_index;
    uint32_t cap_chunks; // capacity of chunks[]
    uint32_t flags;      // SNAPMI_FRAME_CONTINUATION: identifier already seen
    // first 10 bytes of the reference decoder's `src` scratch buffer when
    // this call starts (all zero for a fresh decoder): see frame_short_varint
    uint8_t stale[10];
    uint32_t *meta; // for the host: [0] data chunks found, [1] overflow flag,
                    // [2] 1: the side index met a chunk only a walk can
                    // judge, 2: so did the parallel walk; a no-wait decode's
                    // own: [3] kFrontWalk when its sequential walk ran
    // 1: the sequential walk of a no-wait decode, enqueued behind another
    // front (snapmi_framewalk.hpp); 0 in every other launch
    uint32_t chained;
    // the batch of one
    FrameChunk *chunks;
    uint32_t *c_stream; // [cap_chunks], all 0
    uint64_t *counts;   // [1] data chunks
    uint64_t *first;    // {0, data chunks}
    snapmi_error *serr; // [1] structural error of the walk
    uint32_t *sidx;     // [1] the data chunk it precedes (0xFFFFFFFF = none)
    uint32_t *first_bad; // [1] 0xFFFFFFFF: no chunk has failed yet
    const void **in_ptrs; // [1] each: the call's scalars
    uint64_t *in_lens;
    void **out_ptrs;
    uint64_t *out_caps;
    // parallel header walk (k_fw_*): per 32 MiB segment of the stream, the
    // chains that start at a plausible header inside its first 76 494 bytes
    // and reach the segment's end: {entry, exit, data chunks on the way}
    unsigned long long *fw_cand; // [nseg * kFwCands * 3]
    uint32_t *fw_ncand;          // [nseg]
    unsigned long long *fw_entry; // [nseg + 1] the real chain's entry per segment
    uint32_t *fw_base;           // [nseg + 1] data chunks in front of the segment
    uint32_t nseg;
    unsigned long long fw_seg; // segment bytes (32 MiB; smaller in tests)
};

struct FrameBatchDecodeArgs {
    const void *const *in_ptrs;
    const uint64_t *in_lens;
    void *const *out_ptrs; // nullptr = lengths only
    const uint64_t *out_caps;
    uint64_t *out_lens;
    snapmi_error *errs; // nullptr = not reported
    uint32_t n, total;  // streams, data chunks of all streams
    // per stream
    uint64_t *counts;     // [n] data chunks in front of the walk's error
    uint64_t *first;      // [n+1] exclusive scan of counts
    snapmi_error *serr;   // [n] the walk's structural error
    uint32_t *sidx;       // [n] data chunk it precedes (0xFFFFFFFF = none)
    uint32_t *first_bad;  // [n] first chunk with an error (0xFFFFFFFF = none,
                          // set with serr and sidx, not by a memset a call)
    // per data chunk of the list
    FrameChunk *chunks;
    uint32_t *c_stream;
    uint64_t *dlens;
    uint64_t *offs; // [total+1] exclusive scan of dlens
    snapmi_error *cerrs;
    snapmi_error *derrs;
    const void **c_in;
    uint64_t *c_in_len;
    void **c_out;
    uint64_t *c_caps;
    uint64_t *c_out_lens;
    uint8_t *modes;
    uint32_t *crcs;
};

// ctx->fb_streams: the per-stream arrays of a decode of a.n streams
inline void fbd_streams_layout(Carver &c, FrameBatchDecodeArgs &a)
{
    const size_t n = a.n;
    a.counts = c.take<uint64_t>(n);
    a.first = c.take<uint64_t>(n + 1);
    a.serr = c.take<snapmi_error>(n);
    a.sidx = c.take<uint32_t>(n);
    a.first_bad = c.take<uint32_t>(n);
}

// ctx->fb_streams of a lone stream's decode: the batch of one (b.n = 1, and
// a's view of the same five arrays), then the call's scalars in the places of
// the batch's arrays, the fronts' words for the host and the parallel walk's
// state for a.nseg segments
inline void frame_lone_layout(Carver &c, FrameBatchDecodeArgs &b,
                              FrameDecodeArgs &a)
{
    const size_t nseg = a.nseg;
    fbd_streams_layout(c, b);
    a.counts = b.counts;
    a.first = b.first;
    a.serr = b.serr;
    a.sidx = b.sidx;
    a.first_bad = b.first_bad;
    a.in_ptrs = c.take<const void *>(1);
    a.in_lens = c.take<uint64_t>(1);
    a.out_ptrs = c.take<void *>(1);
    a.out_caps = c.take<uint64_t>(1);
    a.meta = c.take<uint32_t>(4);
    a.fw_cand = c.take<unsigned long long>(nseg * kFwCands * 3);
    a.fw_entry = c.take<unsigned long long>(nseg + 1);
    a.fw_ncand = c.take<uint32_t>(nseg);
    a.fw_base = c.take<uint32_t>(nseg + 1);
}

// ctx->fb_chunks: the per-chunk arrays of a decode, for a list of a.total
// data chunks
inline void fbd_chunks_layout(Carver &c, FrameBatchDecodeArgs &a)
{
    const size_t t = a.total;
    a.chunks = c.take<FrameChunk>(t);
    a.c_stream = c.take<uint32_t>(t);
    a.dlens = c.take<uint64_t>(t);
    a.offs = c.take<uint64_t>(t + 1);
    a.cerrs = c.take<snapmi_error>(t);
    a.derrs = c.take<snapmi_error>(t);
    a.c_in = c.take<const void *>(t);
    a.c_in_len = c.take<uint64_t>(t);
    a.c_out = c.take<void *>(t);
    a.c_caps = c.take<uint64_t>(t);
    a.c_out_lens = c.take<uint64_t>(t);
    a.modes = c.take<uint8_t>(t);
    a.crcs = c.take<uint32_t>(t);
}

// ---------------------------------------------------------------------
// The chunk list.  The chunks of all streams of a call form one list (stream
// i owns chunks [first[i], first[i+1])), the codec kernels run over that
// list, and the results map back to each stream: a chunk's output position
// is its offset in the list's output minus the offset of its stream's first
// chunk.
// ---------------------------------------------------------------------
struct FrameBatchCompressArgs {
    const void *const *in_ptrs;
    const uint64_t *in_lens;
    void *const *out_ptrs;
    const uint64_t *out_caps; // nullptr = not checked
    uint64_t *out_lens;
    snapmi_error *errs; // nullptr = not reported
    uint32_t n, total, seg; // streams, chunks, chunks per segment
    // a list of one stream may have these:
    // [total+1] input offset of every chunk (the caller decides where chunks
    // end); nullptr = 65536-byte multiples
    const uint64_t *chunk_in_off;
    // [total+1] out: where every chunk's header lies, and the frame's length
    uint64_t *chunk_offsets;
    uint32_t ident; // 10 when streams begin with the identifier, 0 when not
    uint64_t *counts;       // [n] chunks per stream
    uint64_t *first;        // [n+1] exclusive scan of counts
    uint8_t *refused;       // [n] stream fails the capacity check
    uint64_t *sbase;        // [n] list offset of the stream's first chunk
    const void **c_in;      // [total] chunk input
    uint64_t *c_len;
    uint32_t *c_stream;
    // the segment [lo, lo + cnt) of the list (per-segment scratch below)
    uint32_t lo, cnt;
    uint64_t *carry; // [1] list bytes of the segments in front
    void **slot_ptrs;
    uint64_t *clens;
    uint32_t *crcs;
    uint64_t *sizes; // 8 + payload; 0 for a refused stream's chunks
    uint64_t *offs;  // [cnt+1] exclusive scan of sizes
    uint8_t *slots;
};

// a lone stream's scalars, where k_fb_lone puts them
struct FrameLonePlaces {
    const void **in;
    uint64_t *len;
    void **out;
};

// ctx->fr_desc: the arrays of a compress of a.n streams, a.total chunks and
// segments of a.seg chunks.  A lone stream's scalars take the places of the
// per-stream input arrays, which the layout then points a at (k_fb_lone
// fills them).
inline FrameLonePlaces fb_desc_layout(Carver &c, FrameBatchCompressArgs &a,
                                      bool lone)
{
    const size_t n = a.n, total = a.total, seg = a.seg;
    FrameLonePlaces l;
    l.in = c.take<const void *>(lone ? 1 : 0);
    l.len = c.take<uint64_t>(lone ? 1 : 0);
    l.out = c.take<void *>(lone ? 1 : 0);
    if (lone) {
        a.in_ptrs = l.in;
        a.in_lens = l.len;
        a.out_ptrs = l.out;
    }
    a.counts = c.take<uint64_t>(n);
    a.first = c.take<uint64_t>(n + 1);
    a.refused = c.take<uint8_t>(n);
    a.sbase = c.take<uint64_t>(n);
    a.c_in = c.take<const void *>(total);
    a.c_len = c.take<uint64_t>(total);
    a.c_stream = c.take<uint32_t>(total);
    a.carry = c.take<uint64_t>(1);
    a.slot_ptrs = c.take<void *>(seg);
    a.clens = c.take<uint64_t>(seg);
    a.crcs = c.take<uint32_t>(seg);
    a.sizes = c.take<uint64_t>(seg);
    a.offs = c.take<uint64_t>(seg + 1);
    return l;
}

// ctx->fr_crc: what snapmi_crc32c_masked_batch keeps for the long buffers
// among its n (k_crc_plan writes both)
struct CrcLong {
    uint64_t *seg_first; // [n+1] exclusive scan of the buffers' segments
    uint32_t *acc;       // [n] the segments' states, XORed together
};

inline void crc_long_layout(Carver &c, CrcLong &l, size_t n)
{
    l.seg_first = c.take<uint64_t>(n + 1);
    l.acc = c.take<uint32_t>(n);
}

} // namespace snapmi

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>

struct snapmi_ctx;

namespace snapmi {

// ---- snapmi_crc.hip ----------------------------------------------------
// the CRC32C tables of the context, computed and uploaded on its first use:
// one blocking copy, which the callers keep in front of a call's first
// enqueue
int ensure_tables(snapmi_ctx *ctx);
// masked CRC32C of n buffers of at most 65536 bytes each, on `st`
// (k_crc32c; a longer buffer's place in out[] is left alone)
int launch_crc32c(snapmi_ctx *ctx, hipStream_t st, const void *const *ptrs,
                  const uint64_t *lens, uint32_t *out, uint32_t n);

// ---- snapmi_frame.hip --------------------------------------------------
// k_scan_u64 (the strided one-workgroup scan of snapmi_scan.hpp):
// out[0..n) = exclusive scan of in[0..n), out[n] = total
int launch_scan_u64(snapmi_ctx *ctx, hipStream_t st, const uint64_t *in,
                    uint64_t *out, uint32_t n);

// What frame_compress_list frames: n streams by arrays in device memory, or
// (lone) the one stream [in, in + in_len) -> out.
struct FrameList {
    bool lone = false;
    size_t n = 1;
    uint64_t total = 0;                  // chunks of all streams
    const uint64_t *h_in_lens = nullptr; // [n] the streams' lengths, host
    uint64_t *out_lens = nullptr;        // device, [n]
    // n streams
    const void *const *in_ptrs = nullptr;
    const uint64_t *in_lens = nullptr;
    void *const *out_ptrs = nullptr;
    const uint64_t *out_caps = nullptr; // nullptr = not checked
    snapmi_error *errs = nullptr;       // nullptr = not reported
    // the lone stream
    const void *in = nullptr;
    uint64_t in_len = 0;
    void *out = nullptr;
    // and what only a lone stream may have:
    // [total+1] where the caller cut the chunks, device-readable (device or
    // pinned host memory), and [total] their lengths on the host;
    // nullptr = 65536-byte multiples
    const uint64_t *chunk_in_off = nullptr;
    const uint32_t *h_chunk_lens = nullptr;
    bool ident = true; // streams begin with the stream identifier
    uint64_t *chunk_offsets = nullptr; // device, [total+1] out (k_fb_emit)
};

// The one place that frames chunks: descriptors of the list, then per segment
// the checksums, the raw compressor, sizes, their scan and the emit.
int frame_compress_list(snapmi_ctx *ctx, const FrameList &l);

// ---- snapmi_framedec.hip -----------------------------------------------
// n_words (at most 64) words of a result, from device memory into pinned
// (device-mapped) host memory, by a kernel store on `st` (k_post_words)
int post_words(snapmi_ctx *ctx, hipStream_t st, uint32_t *host_mapped,
               const uint32_t *dev, uint32_t n_words);
// snapmi_frame_scan_host, stopping in front of data chunk number `max_data`
// (status 3: the caller's output buffer is full)
int frame_scan(const void *h_in, uint64_t in_len, uint32_t flags,
               uint8_t *stale10, uint64_t *h_offsets, uint64_t cap,
               uint64_t max_data, uint64_t *n_chunks, uint64_t *consumed);
// snapmi_frame_decompress_batch of n streams the host has walked: d_first
// [n + 1] and d_list [total] (FwEntry, snapmi_framewalk.hpp) replace the
// device's walk and its wait; *d_bad (cleared by the caller) is raised when
// the list disagrees with the bytes
int frame_decompress_batch_listed(snapmi_ctx *ctx,
                                  const void *const *d_in_ptrs,
                                  const uint64_t *d_in_lens,
                                  void *const *d_out_ptrs,
                                  const uint64_t *d_out_caps,
                                  uint64_t *d_out_lens, snapmi_error *d_errs,
                                  size_t n, const uint64_t *d_first,
                                  const void *d_list, uint64_t total,
                                  uint32_t *d_bad);

} // namespace snapmi
#endif // __HIPCC__
