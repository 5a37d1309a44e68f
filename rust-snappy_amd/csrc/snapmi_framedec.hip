// snapmi_framedec.hip -- Snappy frame format on the device (gfx950): the
// decode side (the format and the compress side: snapmi_frame.hip; the rules
// of the reference's reader, src/read.rs: snapmi_framewalk.hpp).  The data
// chunks of all the streams of a call form one list, the raw decompressor
// runs on a batch whose "streams" are the chunks, and a call for one stream
// is a batch of one whose chunk table one of three fronts fills.
//
// Kernels here:
//   k_frame_walk      one stream: sequential walk over the chunk headers (the
//                     format has no index) with the reference's checks
//   k_fw_candidates, k_fw_resolve, k_fw_emit
//                     the headers of a long stream, found in parallel
//   k_frame_meta_init, k_frame_index
//                     one stream with a side index, checked
//   k_frame_nowait_seal   behind the fronts of a no-wait decode
//   k_fbd_walk_count, k_fbd_walk_fill
//                     many streams: one thread walks a stream
//   k_fbd_from_list   many streams the host has walked: its list, checked
//   k_fbd_lens        decompressed length of every data chunk
//   k_fbd_desc        descriptors for the raw decompressor
//   k_fbd_verify_chunks, k_fbd_verify_streams
//                     CRC comparison, first error in stream order
//   k_post_words      a few words of a result into pinned host memory
//                     (post_words, for the host pipeline as well)
#include <hip/hip_runtime.h>

#include <string.h>

#include "snapmi.h"
#include "snapmi_ctx.hpp"
#include "snapmi_launch.hpp"
#include "snapmi_device.hpp"
#include "snapmi_kernels.hpp"
#include "snapmi_frame.hpp"

using namespace snapmi;

namespace snapmi {

// ---------------------------------------------------------------------
// Parallel header walk.  The frame format is a linked list without an index:
// k_frame_walk below hops from header to header, 0.7 us per hop (1.1 s for the
// 1 048 576 chunks of a 64 GiB stream).  But a header is easy to recognise
// (type byte, 24-bit length within the format's limits, chunk inside the
// stream: 0.2 % of random positions pass) and a chain that starts at a wrong
// position dies within a hop or two.  So, per 32 MiB segment of the stream:
//   k_fw_candidates  every position of the segment's first 76 494 bytes (the
//                    real chain must touch down there) that looks like a
//                    header is followed to the segment's end; the survivors
//                    are recorded as {entry, exit, data chunks};
//   k_fw_resolve     one thread strings the segments together: the real
//                    chain enters segment k where it left segment k-1;
//   k_fw_emit        one thread per segment walks its real chain again and
//                    writes the chunk records at their final index.
// Only well-formed stretches are decided here: the first header that the
// reference's reader would reject (or a chunk the stale-buffer rule applies
// to) makes the chain "die", the resolve step then finds no continuation and
// sets meta[2] = 2, and the sequential walk runs and reports the error.
// ---------------------------------------------------------------------

// What a front found, by its one deciding thread: nd data chunks, and the
// structural error e in front of data chunk `sidx` (0xFFFFFFFF = none).
__device__ inline void frame_front_result(const FrameDecodeArgs &a,
                                          uint32_t nd, const snapmi_error &e,
                                          uint32_t sidx)
{
    a.meta[0] = nd;
    a.counts[0] = nd;
    a.first[0] = 0;
    a.first[1] = nd;
    a.serr[0] = e;
    a.sidx[0] = sidx;
    a.first_bad[0] = 0xFFFFFFFFu;
    a.in_ptrs[0] = a.in;
    a.in_lens[0] = a.in_len;
    a.out_ptrs[0] = a.out;
    a.out_caps[0] = a.out_cap;
}
constexpr uint32_t kFwScan = 4 + kMaxChunk; // longest chunk, header included

// One hop of a well-formed chain: the chunk at r (header checks of
// src/read.rs:119-187 that need no history).  Returns false if the reader
// would stop here; *data = 1 for a compressed / stored chunk.
__device__ inline bool fw_hop(const FrameDecodeArgs &a, uint64_t &r,
                              uint32_t &data)
{
    gcptr in = (gcptr)a.in;
    if (a.in_len - r < 4)
        return false;
    const uint32_t hd = ld32u(in + r);
    const uint32_t ty = hd & 0xFF;
    const uint64_t len = hd >> 8;
    data = 0;
    if (len > kMaxChunk || (ty >= 0x02 && ty <= 0x7F) ||
        a.in_len - r - 4 < len)
        return false;
    if (ty == 0xFF) {
        if (len != 6)
            return false;
        const uint8_t body[6] = {'s', 'N', 'a', 'P', 'p', 'Y'};
        for (int k = 0; k < 6; k++)
            if (in[r + 4 + k] != body[k])
                return false;
    } else if (ty <= 0x01) {
        if (len < 4 || (ty == 0x01 && len - 4 > kMaxBlock))
            return false;
        if (ty == 0x00 && short_varint(in + r + 8, len - 4))
            return false; // read.rs:216: the sequential walk's business
        data = 1;
    }
    r += 4 + len;
    return true;
}

__global__ __launch_bounds__(256) void k_fw_candidates(FrameDecodeArgs a)
{
    const uint64_t seg = blockIdx.y;
    const uint64_t lo = seg * a.fw_seg;
    uint64_t end = lo + a.fw_seg; // the chain leaves the segment at or past it
    if (end > a.in_len)
        end = a.in_len;
    const uint64_t off = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (off >= kFwScan || lo + off >= a.in_len)
        return;
    if (seg == 0 && off != 0)
        return; // the stream starts at its first byte
    uint64_t r = lo + off;
    uint32_t n = 0, data = 0;
    while (r < end) {
        if (!fw_hop(a, r, data))
            return; // not a chain (or the real one's first bad chunk)
        n += data;
    }
    const uint32_t k = atomicAdd(&a.fw_ncand[seg], 1u);
    if (k < kFwCands) {
        unsigned long long *c = a.fw_cand + (seg * kFwCands + k) * 3;
        c[0] = lo + off;
        c[1] = r;
        c[2] = n;
    }
}

__global__ void k_fw_resolve(FrameDecodeArgs a)
{
    gcptr in = (gcptr)a.in;
    frame_front_result(a, 0, frame_err(SNAPMI_OK, 0, 0), 0xFFFFFFFFu);
    a.meta[1] = 0;
    a.meta[2] = 2; // until proven well-formed: the sequential walk decides
    // the first chunk must be the stream identifier (src/read.rs:123-128)
    if (!(a.flags & SNAPMI_FRAME_CONTINUATION) &&
        (a.in_len < 4 || in[0] != 0xFF))
        return;
    uint64_t cur = 0;
    uint32_t total = 0;
    for (uint32_t seg = 0; seg < a.nseg; seg++) {
        a.fw_entry[seg] = ~0ull;
        a.fw_base[seg] = total;
        if (cur >= ((uint64_t)seg + 1) * a.fw_seg)
            continue; // (a chunk of <= 76 KiB spans a whole small test segment)
        const uint32_t nc =
            a.fw_ncand[seg] < kFwCands ? a.fw_ncand[seg] : kFwCands;
        bool found = false;
        for (uint32_t k = 0; k < nc && !found; k++) {
            const unsigned long long *c =
                a.fw_cand + ((uint64_t)seg * kFwCands + k) * 3;
            if (c[0] == cur) {
                a.fw_entry[seg] = cur;
                cur = c[1];
                total += (uint32_t)c[2];
                found = true;
            }
        }
        if (!found)
            return; // the real chain does not survive this segment
    }
    if (cur != a.in_len)
        return;
    a.fw_base[a.nseg] = total;
    frame_front_result(a, total, frame_err(SNAPMI_OK, 0, 0), 0xFFFFFFFFu);
    a.meta[1] = total > a.cap_chunks ? 1 : 0;
    a.meta[2] = 0;
}

__global__ void k_fw_emit(FrameDecodeArgs a)
{
    const uint32_t seg = blockIdx.x * blockDim.x + threadIdx.x;
    if (seg >= a.nseg || a.meta[2] != 0 || a.meta[1] != 0)
        return;
    uint64_t r = a.fw_entry[seg];
    if (r == ~0ull)
        return;
    gcptr in = (gcptr)a.in;
    uint64_t end = ((uint64_t)seg + 1) * a.fw_seg;
    if (end > a.in_len)
        end = a.in_len;
    uint32_t idx = a.fw_base[seg];
    while (r < end) {
        const uint32_t hd = ld32u(in + r);
        const uint32_t ty = hd & 0xFF;
        const uint32_t len = hd >> 8;
        if (ty <= 0x01) {
            FrameChunk c;
            c.payload_off = r + 8;
            c.payload_len = len - 4;
            c.crc = ld32u(in + r + 4);
            c.type = ty;
            c.pad = 0;
            a.c_stream[idx] = 0;
            a.chunks[idx++] = c;
        }
        r += 4 + (uint64_t)len;
    }
}

// the walk of the one stream of snapmi_frame_decompress[_ex]
__global__ void k_frame_walk(FrameDecodeArgs a)
{
    if (blockIdx.x || threadIdx.x)
        return;
    if (a.chained) { // the front before this launch may have decided
        const bool decided = frame_front_decided(a.meta[2]);
        a.meta[3] = decided ? 0 : kFrontWalk;
        if (decided)
            return;
    }
    a.meta[1] = 0;
    a.meta[2] = 0;
    uint32_t nd;
    const snapmi_error e = frame_walk(
        (gcptr)a.in, a.in_len, a.flags, a.stale, nd,
        [&](uint32_t k, const FrameChunk &c) {
            if (k < a.cap_chunks) {
                a.chunks[k] = c;
                a.c_stream[k] = 0;
            } else {
                a.meta[1] = 1; // overflow: caller reruns with more room
            }
        });
    frame_front_result(a, nd, e, e.kind != SNAPMI_OK ? nd : 0xFFFFFFFFu);
}

// With a side index: chunk i's header is at index[i]; all chunks must be
// data chunks written by snapmi_frame_compress (the stream identifier is
// checked here as well).
__global__ void k_frame_index(FrameDecodeArgs a)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    gcptr in = (gcptr)a.in;
    // (k_frame_meta_init runs before this launch)
    // (the rules: snapmi_framewalk.hpp; whatever fails them sends the whole
    // stream to the walk, which owns every error report)
    if (i == 0 && !frame_index_start(in, a.in_len, a.flags, a.n_index))
        a.meta[2] = 1;
    if (i >= a.n_index)
        return;
    FrameChunk c;
    if (!frame_index_entry(in, a.in_len, a.flags, a.index, a.n_index, i, c))
        a.meta[2] = 1;
    a.chunks[i] = c;
    a.c_stream[i] = 0;
}

// Behind the fronts of a no-wait decode (rules: snapmi_framewalk.hpp).  The
// host has sized the chunk table and every launch behind this one for
// cap_chunks records; the deciding front left meta[0] of them.  A broken
// promise becomes the stream's one verdict, over a stream of no chunks; what
// is left of the table is filled with records that decode to nothing (and
// that k_fbd_verify_chunks passes over).  One thread per record; thread 0
// also notes the front for info "frame_nowait_front".
__global__ __launch_bounds__(256) void k_frame_nowait_seal(
    FrameDecodeArgs a, uint32_t first_front, uint32_t *front_out)
{
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    // (thread 0 writes neither word: every block reads the same two)
    const FrameNowait x = frame_nowait_rule(
        first_front, a.chained && a.meta[3] == kFrontWalk, a.meta[0],
        a.cap_chunks);
    if (t >= x.pad_lo && t < a.cap_chunks) {
        a.chunks[t] = frame_no_chunk();
        a.c_stream[t] = 0;
    }
    if (t != 0)
        return;
    front_out[0] = x.front;
    if (x.exceeded) {
        a.counts[0] = 0;
        a.first[1] = 0;
        a.serr[0] = frame_nowait_exceeded(a.meta[0], a.cap_chunks);
        a.sidx[0] = 0;
    }
}

// Final verdict of one framed stream of n data chunks: its first error in
// stream order (the reference processes chunk by chunk: length checks, raw
// decode, checksum :225-232 / :189-196) and the output bytes reported with
// it.  first_bad: first chunk with an error in cerrs[] (0xFFFFFFFF = none);
// sidx: the data chunk the walk's structural error serr precedes; offs[0..n]:
// output offsets of the chunks (offs[0] need not be 0); has_out: not a
// lengths-only call; cap: the output's capacity.
__device__ inline void frame_verdict(uint32_t first_bad, uint32_t sidx,
                                     uint32_t n, const snapmi_error *cerrs,
                                     const snapmi_error &serr, bool has_out,
                                     uint64_t cap, const uint64_t *offs,
                                     snapmi_error &e, uint64_t &out_len)
{
    const uint64_t total = offs[n] - offs[0];
    const bool decoded = has_out && total <= cap;
    e = frame_err(SNAPMI_OK, 0, 0);
    if (first_bad != 0xFFFFFFFFu && first_bad < sidx)
        e = cerrs[first_bad];
    else if (serr.kind != SNAPMI_OK)
        e = serr;
    else if (has_out && total > cap)
        e = frame_err(SNAPMI_BUFFER_TOO_SMALL, cap, total);
    // On an error the chunks in front of the failing one are decoded and
    // checked: the reference's reader has handed them out by then
    // (src/read.rs:112-118), so their byte count is reported.
    uint32_t upto = n;
    if (e.kind != SNAPMI_OK) {
        upto = first_bad < sidx ? first_bad : (sidx < n ? sidx : n);
        if (!decoded)
            upto = 0;
    }
    out_len = offs[upto] - offs[0];
}

// the decode stage's verdict on data chunk i (already decoded, not failed
// before): raw decoder error, else checksum mismatch; false if it is good
__device__ inline bool frame_chunk_decode_err(const snapmi_error &derr,
                                              uint32_t stored_crc,
                                              uint32_t crc, snapmi_error &e)
{
    if (derr.kind != SNAPMI_OK) {
        e = derr;
        return true;
    }
    if (crc != stored_crc) {
        e = frame_err(SNAPMI_CHECKSUM, stored_crc, crc);
        return true;
    }
    return false;
}

// pass 1: one thread per stream (a wavefront walks 64 streams) counts the
// data chunks in front of the stream's first structural error
__global__ __launch_bounds__(64) void k_fbd_walk_count(FrameBatchDecodeArgs a)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n)
        return;
    const uint8_t fresh[10] = {0}; // every stream of a batch starts fresh
    uint32_t nd;
    const snapmi_error e =
        frame_walk((gcptr)a.in_ptrs[i], a.in_lens[i], 0, fresh, nd,
                   [](uint32_t, const FrameChunk &) {});
    a.counts[i] = nd;
    a.serr[i] = e;
    a.sidx[i] = e.kind != SNAPMI_OK ? nd : 0xFFFFFFFFu;
    a.first_bad[i] = 0xFFFFFFFFu;
}

// pass 2: the same walk writes the chunk records at the stream's place
__global__ __launch_bounds__(64) void k_fbd_walk_fill(FrameBatchDecodeArgs a)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n || a.counts[i] == 0)
        return;
    const uint8_t fresh[10] = {0};
    const uint64_t base = a.first[i];
    const uint64_t cnt = a.counts[i];
    uint32_t nd;
    frame_walk((gcptr)a.in_ptrs[i], a.in_lens[i], 0, fresh, nd,
               [&](uint32_t k, const FrameChunk &c) {
                   if (k < cnt) {
                       a.chunks[base + k] = c;
                       a.c_stream[base + k] = i;
                   }
               });
}

// From the last chunk the reader accepted (or the stream's start) to `to`:
// true when in[r, to) is a run of chunks the walk skips - the identifier,
// skippable and padding chunks - that ends exactly at `to`.
__device__ inline bool fbd_gap(gcptr in, uint64_t in_len, uint64_t r,
                               bool seen_ident, uint64_t to)
{
    const uint8_t fresh[10] = {0};
    if (to > in_len)
        return false;
    while (r < to) {
        bool data;
        FrameChunk c;
        if (frame_hop(in, in_len, fresh, r, seen_ident, data, c).kind !=
                SNAPMI_OK ||
            data)
            return false;
    }
    return r == to;
}

// The walk kernels' work for streams the HOST has walked already
// (snapmi_frame_decompress_batch_listed): list[t] names data chunk t of the
// batch and l_first[i] the first chunk of stream i, both written by the host
// from the bytes it staged.  The list is a hint that is checked, never
// trusted: thread t < total hops with the walk's own rules from the chunk in
// front of its chunk (the stream's start for a first chunk) to its header and
// over it, thread total + i from stream i's last chunk to the stream's end,
// so together they are one walk of every stream.  Whatever does not come out
// as listed raises *bad (the call fails) and leaves a chunk that decodes to
// nothing.
__global__ __launch_bounds__(256) void k_fbd_from_list(FrameBatchDecodeArgs a,
                                                       const uint64_t *l_first,
                                                       const FwEntry *list,
                                                       uint32_t *bad)
{
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    const uint8_t fresh[10] = {0};
    bool good = true;
    if (t < a.total) {
        const FwEntry x = list[t];
        const uint32_t s = x.stream < a.n ? x.stream : 0;
        FrameChunk c;
        c.payload_off = 0;
        c.payload_len = 0;
        c.crc = 0;
        c.type = 0xFF;
        c.pad = 0xFF;
        good = x.stream < a.n && l_first[s] <= t && t < l_first[s + 1];
        if (good) {
            gcptr in = (gcptr)a.in_ptrs[s];
            const uint64_t in_len = a.in_lens[s];
            uint64_t r = 0;
            bool seen = false, data = false;
            if (t > l_first[s]) {
                r = list[t - 1].off + 4 + (list[t - 1].hd >> 8);
                seen = true;
            }
            FrameChunk got;
            good = fbd_gap(in, in_len, r, seen, x.off) && x.off < in_len;
            r = x.off;
            seen = true; // (a first chunk lies behind the identifier: r > 0)
            good = good && x.off > 0 &&
                   frame_hop(in, in_len, fresh, r, seen, data, got).kind ==
                       SNAPMI_OK &&
                   data && fw_ld32(in + x.off) == x.hd;
            if (good)
                c = got;
        }
        a.chunks[t] = c;
        a.c_stream[t] = s;
    } else if (t - a.total < a.n) {
        const uint32_t i = t - a.total;
        const uint64_t b = l_first[i], e = l_first[i + 1];
        // (stored in front of the walk below: behind it the six pointers
        // stay live across it and the kernel spills SGPRs)
        a.counts[i] = e - b;
        a.first[i] = b;
        if (i + 1 == a.n)
            a.first[a.n] = e;
        a.serr[i] = frame_err(SNAPMI_OK, 0, 0);
        a.sidx[i] = 0xFFFFFFFFu;
        a.first_bad[i] = 0xFFFFFFFFu;
        uint64_t r = 0;
        if (e > b)
            r = list[e - 1].off + 4 + (list[e - 1].hd >> 8);
        good = fbd_gap((gcptr)a.in_ptrs[i], a.in_lens[i], r, e > b,
                       a.in_lens[i]);
    }
    if (!good)
        *bad = 1;
}

__global__ void k_fbd_lens(FrameBatchDecodeArgs a)
{
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= a.total)
        return;
    const FrameChunk ch = a.chunks[c];
    gcptr in = (gcptr)a.in_ptrs[a.c_stream[c]];
    snapmi_error e;
    a.dlens[c] = frame_chunk_len(in + ch.payload_off, ch, e);
    a.cerrs[c] = e;
}

// does stream s's output fit its buffer?
__device__ inline bool fbd_fits(const FrameBatchDecodeArgs &a, uint32_t s)
{
    const uint64_t b = a.first[s], e = a.first[s + 1];
    return a.offs[e] - a.offs[b] <= a.out_caps[s];
}

// descriptors for the raw decompressor (one "stream" per data chunk)
__global__ void k_fbd_desc(FrameBatchDecodeArgs a)
{
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= a.total)
        return;
    const uint32_t s = a.c_stream[c];
    const FrameChunk ch = a.chunks[c];
    // a chunk that already failed (or an output that does not fit) is
    // decoded as an empty stored chunk: nothing is written
    const bool skip = a.cerrs[c].kind != SNAPMI_OK || !fbd_fits(a, s);
    a.c_in[c] = (const uint8_t *)a.in_ptrs[s] + ch.payload_off;
    a.c_in_len[c] = skip ? 0 : ch.payload_len;
    a.modes[c] = skip ? 1 : (uint8_t)ch.type;
    a.c_out[c] = (uint8_t *)a.out_ptrs[s] + (a.offs[c] - a.offs[a.first[s]]);
    a.c_caps[c] = a.dlens[c];
    a.c_out_lens[c] = 0;
}

// per chunk: the decode stage's verdict, and the first bad chunk per stream
__global__ void k_fbd_verify_chunks(FrameBatchDecodeArgs a)
{
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= a.total)
        return;
    const uint32_t s = a.c_stream[c];
    // A record behind its stream's chunks is no chunk of it: the padding of
    // a no-wait decode (k_frame_nowait_seal), whose error kind is not OK,
    // must not become the stream's first bad chunk.
    if (c - a.first[s] >= a.first[s + 1] - a.first[s])
        return;
    bool bad = a.cerrs[c].kind != SNAPMI_OK;
    if (!bad && a.out_ptrs && fbd_fits(a, s))
        bad = frame_chunk_decode_err(a.derrs[c], a.chunks[c].crc, a.crcs[c],
                                     a.cerrs[c]);
    if (bad)
        atomicMin(&a.first_bad[s], (uint32_t)(c - a.first[s]));
}

__global__ void k_fbd_verify_streams(FrameBatchDecodeArgs a)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n)
        return;
    const uint64_t b = a.first[i];
    snapmi_error e;
    uint64_t len;
    frame_verdict(a.first_bad[i], a.sidx[i], (uint32_t)(a.first[i + 1] - b),
                  a.cerrs + b, a.serr[i], a.out_ptrs != nullptr,
                  a.out_ptrs ? a.out_caps[i] : 0, a.offs + b, e, len);
    if (a.errs)
        a.errs[i] = e;
    a.out_lens[i] = len;
}

} // namespace snapmi

extern "C" {

int snapmi_frame_index_host(const void *h_in, uint64_t in_len,
                            uint64_t *h_offsets, uint64_t cap,
                            uint64_t *n_chunks)
{
    // the regular cases of k_frame_walk (reference src/read.rs:111-236);
    // anything else is left to the device walk, which owns the error report
    if (!n_chunks || (in_len && !h_in))
        return 1;
    return frame_index_walk((const uint8_t *)h_in, in_len, h_offsets, cap,
                            n_chunks);
}

// the index kernel's result if its threads find nothing wrong (they only
// ever raise meta[2])
__global__ void k_frame_meta_init(FrameDecodeArgs a)
{
    frame_front_result(a, a.n_index, frame_err(SNAPMI_OK, 0, 0), 0xFFFFFFFFu);
    a.meta[1] = 0;
    a.meta[2] = 0;
}

static int mailbox(snapmi_ctx *ctx)
{
    if (!ctx->h_mail)
        HIP_TRY(ctx, hipHostMalloc((void **)&ctx->h_mail, 256,
                                   hipHostMallocDefault));
    return SNAPMI_OK;
}

// A few words of a result, from device memory into pinned (device-mapped)
// host memory.  A hipMemcpyAsync of 16 bytes would do the same - through the
// copy engine, where it waits behind whatever bulk copy is under way in that
// direction (20 ms behind a 1 GiB result): a kernel store does not queue.
__global__ void k_post_words(uint32_t *host_mapped, const uint32_t *dev,
                             uint32_t n)
{
    if (threadIdx.x < n)
        host_mapped[threadIdx.x] = dev[threadIdx.x];
    __threadfence_system();
}

} // extern "C"

int snapmi::post_words(snapmi_ctx *ctx, hipStream_t st, uint32_t *host_mapped,
                       const uint32_t *dev, uint32_t n_words)
{
    hipLaunchKernelGGL(k_post_words, dim3(1), dim3(64), 0, st, host_mapped,
                       dev, n_words);
    HIP_TRY(ctx, hipGetLastError());
    return SNAPMI_OK;
}

// snapmi_frame_scan_host, stopping in front of data chunk number `max_data`
// (status 3: the caller's output buffer is full)
int snapmi::frame_scan(const void *h_in, uint64_t in_len, uint32_t flags,
                       uint8_t *stale10, uint64_t *h_offsets, uint64_t cap,
                       uint64_t max_data, uint64_t *n_chunks,
                       uint64_t *consumed)
{
    if (!n_chunks || !consumed || (in_len && !h_in))
        return SNAPMI_E_ARGUMENT;
    const uint8_t *in = (const uint8_t *)h_in;
    uint64_t r = 0, nd = 0;
    bool seen_ident = (flags & SNAPMI_FRAME_CONTINUATION) != 0;
    int status = 0;
    while (r != in_len) {
        if (in_len - r < 4) {
            status = 2;
            break;
        }
        const uint32_t ty = in[r];
        const uint64_t len = (uint64_t)in[r + 1] | ((uint64_t)in[r + 2] << 8) |
                             ((uint64_t)in[r + 3] << 16);
        if ((!seen_ident && ty != 0xFF) || len > kMaxChunk ||
            (ty >= 0x02 && ty <= 0x7F) || (ty == 0xFF && len != 6) ||
            (ty <= 0x01 && (len < 4 || (ty == 0x01 && len - 4 > kMaxBlock)))) {
            status = 1;
            break;
        }
        if (in_len - r - 4 < len) {
            status = 2;
            break;
        }
        if (ty == 0xFF && memcmp(in + r + 4, "sNaPpY", 6) != 0) {
            status = 1;
            break;
        }
        seen_ident = true;
        if (ty <= 0x01) {
            if (nd == max_data) {
                status = 3;
                break;
            }
            if (h_offsets) {
                if (nd + 1 >= cap)
                    return SNAPMI_E_ARGUMENT;
                h_offsets[nd] = r;
            }
            nd++;
        }
        if (stale10) { // the reference reader's src[0..10), see frame_short_varint
            memcpy(stale10, in + r, 4);
            const uint64_t body = ty == 0x00 ? r + 8 : r + 4;
            const uint64_t blen = ty == 0x00 ? len - 4 : (ty == 0x01 ? 0 : len);
            memcpy(stale10, in + body, (size_t)(blen < 10 ? blen : 10));
        }
        r += 4 + len;
    }
    if (h_offsets) {
        if (nd + 1 > cap)
            return SNAPMI_E_ARGUMENT;
        h_offsets[nd] = r;
    }
    *n_chunks = nd;
    *consumed = r;
    return status;
}

extern "C" {

int snapmi_frame_scan_host(const void *h_in, uint64_t in_len, uint32_t flags,
                           uint8_t *stale10, uint64_t *h_offsets,
                           uint64_t cap, uint64_t *n_chunks,
                           uint64_t *consumed)
{
    return frame_scan(h_in, in_len, flags, stale10, h_offsets, cap,
                      ~0ull, n_chunks, consumed);
}

// The per-stream scratch of a decode of n streams; for a lone stream's decode
// (n = 1, `lone` with its nseg set) the fronts' places lie behind it.
static int fbd_streams(snapmi_ctx *ctx, FrameBatchDecodeArgs &a, size_t n,
                       FrameDecodeArgs *lone)
{
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    int rc = ensure_tables(ctx);
    if (rc)
        return rc;
    a.n = (uint32_t)n;
    a.total = 0;
    auto layout = [&](Carver &c) {
        if (lone)
            frame_lone_layout(c, a, *lone);
        else
            fbd_streams_layout(c, a);
    };
    // per-stream scratch and per-chunk scratch in two buffers: the second is
    // sized after the walk, and growing it must not drop the first
    Carver measure;
    layout(measure);
    if ((rc = reserve(ctx, ctx->fb_streams, measure.bytes())))
        return rc;
    Carver place(ctx->fb_streams.p);
    layout(place);
    return SNAPMI_OK;
}

// A batch call's arguments (false ones are reported) and per-stream scratch.
static int fbd_begin(snapmi_ctx *ctx, const char *what,
                     const void *const *d_in_ptrs, const uint64_t *d_in_lens,
                     void *const *d_out_ptrs, const uint64_t *d_out_caps,
                     uint64_t *d_out_lens, snapmi_error *d_errs, size_t n,
                     FrameBatchDecodeArgs &a)
{
    if (!d_in_ptrs || !d_in_lens || !d_out_lens || (d_out_ptrs && !d_out_caps))
        return fail_ctx(ctx, SNAPMI_E_ARGUMENT, "%s: bad args", what);
    if (n > 0x7FFFFFFFu)
        return fail_ctx(ctx, SNAPMI_E_ARGUMENT,
                        "%s: %zu streams (at most 2^31 - 1)", what, n);
    a.in_ptrs = d_in_ptrs;
    a.in_lens = d_in_lens;
    a.out_ptrs = d_out_ptrs;
    a.out_caps = d_out_caps;
    a.out_lens = d_out_lens;
    a.errs = d_errs;
    return fbd_streams(ctx, a, n, nullptr);
}

// The per-chunk scratch of a decode, for a list of `total` data chunks.
static int fbd_table(snapmi_ctx *ctx, const char *what,
                     FrameBatchDecodeArgs &a, uint64_t total)
{
    if (total > 0x7FFFFFFFu)
        return fail_ctx(ctx, SNAPMI_E_ARGUMENT,
                        "%s: %llu chunks (at most 2^31 - 1)", what,
                        (unsigned long long)total);
    a.total = (uint32_t)total;
    Carver measure;
    fbd_chunks_layout(measure, a);
    int rc = reserve(ctx, ctx->fb_chunks, measure.bytes());
    if (rc)
        return rc;
    Carver place(ctx->fb_chunks.p);
    fbd_chunks_layout(place, a);
    return SNAPMI_OK;
}

// Everything behind the chunk table (chunks[], c_stream[] of a.total data
// chunks; first[], serr[], sidx[], first_bad[] per stream): lengths,
// descriptors, the codec, the checksums and the verdicts.
static int fbd_finish(snapmi_ctx *ctx, FrameBatchDecodeArgs &a)
{
    hipStream_t s = ctx->stream;
    const size_t n = a.n;
    const uint32_t tb = 256;
    const uint32_t gc = a.total ? (a.total + tb - 1) / tb : 1;
    if (a.total)
        hipLaunchKernelGGL(k_fbd_lens, dim3(gc), dim3(tb), 0, s, a);
    int rc = launch_scan_u64(ctx, s, a.dlens, a.offs, a.total);
    if (rc)
        return rc;
    if (a.out_ptrs && a.total) {
        hipLaunchKernelGGL(k_fbd_desc, dim3(gc), dim3(tb), 0, s, a);
        rc = launch_decompress(ctx, a.c_in, a.c_in_len, a.c_out, a.c_caps,
                               a.c_out_lens, a.derrs, a.modes, a.total);
        if (rc)
            return rc;
        // CRC of what was produced (chunks that were skipped have c_out_lens
        // 0: their CRC is never compared)
        if ((rc = launch_crc32c(ctx, s, (const void *const *)a.c_out,
                                a.c_out_lens, a.crcs, a.total)))
            return rc;
    }
    if (a.total)
        hipLaunchKernelGGL(k_fbd_verify_chunks, dim3(gc), dim3(tb), 0, s, a);
    hipLaunchKernelGGL(k_fbd_verify_streams,
                       dim3((uint32_t)((n + tb - 1) / tb)), dim3(tb), 0, s, a);
    HIP_TRY(ctx, hipGetLastError());
    return SNAPMI_OK;
}

// One front of a lone stream's decode, enqueued: the side index, the parallel
// header walk or the sequential walk (kFront*, snapmi_framewalk.hpp).  It
// leaves its findings in a.meta and the batch of one; nothing here waits.
static int frame_front(snapmi_ctx *ctx, const FrameDecodeArgs &a,
                       uint32_t front)
{
    hipStream_t s = ctx->stream;
    const uint32_t tb = 256;
    const uint32_t gb = a.cap_chunks ? (a.cap_chunks + tb - 1) / tb : 1;
    if (front == kFrontIndex) {
        hipLaunchKernelGGL(k_frame_meta_init, dim3(1), dim3(1), 0, s, a);
        hipLaunchKernelGGL(k_frame_index, dim3(gb), dim3(tb), 0, s, a);
    } else if (front == kFrontParallel) {
        HIP_TRY(ctx, hipMemsetAsync(a.fw_ncand, 0, a.nseg * 4, s));
        hipLaunchKernelGGL(k_fw_candidates,
                           dim3((kFwScan + 255) / 256, a.nseg), dim3(256), 0,
                           s, a);
        hipLaunchKernelGGL(k_fw_resolve, dim3(1), dim3(1), 0, s, a);
        hipLaunchKernelGGL(k_fw_emit, dim3((a.nseg + 63) / 64), dim3(64), 0,
                           s, a);
    } else {
        hipLaunchKernelGGL(k_frame_walk, dim3(1), dim3(64), 0, s, a);
    }
    return SNAPMI_OK;
}

int snapmi_frame_decompress_ex(snapmi_ctx *ctx, const void *d_in,
                               uint64_t in_len, void *d_out, uint64_t out_cap,
                               uint64_t *d_out_len, snapmi_error *d_err,
                               const uint64_t *d_chunk_offsets,
                               uint64_t n_chunks, uint32_t flags,
                               const uint8_t *stale10)
{
    const char *what = "frame";
    if (!ctx || !d_out_len || !d_err || (in_len && !d_in) ||
        (flags &
         ~(uint32_t)(SNAPMI_FRAME_CONTINUATION | SNAPMI_FRAME_NO_WAIT)))
        return SNAPMI_E_ARGUMENT;
    const bool nowait = (flags & SNAPMI_FRAME_NO_WAIT) != 0;
    if (nowait && n_chunks > 0x7FFFFFFFu)
        return fail_ctx(ctx, SNAPMI_E_ARGUMENT,
                        "frame: a bound of %llu chunks (at most 2^31 - 1)",
                        (unsigned long long)n_chunks);
    flags &= SNAPMI_FRAME_CONTINUATION; // what the kernels know
    // capacity for the chunk table: exact with an index, else an estimate
    // that is retried once with the exact count (no-wait: the caller's bound)
    bool use_index = d_chunk_offsets != nullptr;
    // long streams without an index: find the headers in parallel (k_fw_*)
    bool parallel_walk =
        in_len >= ctx->frame_parallel_walk_min && !(nowait && use_index);
    uint64_t cap = use_index ? n_chunks : in_len / 2048 + 64;
    const uint64_t fw_seg = ctx->frame_walk_segment;
    const uint64_t nseg64 = (in_len + fw_seg - 1) / fw_seg;
    if (nseg64 == 0 || nseg64 > 65535)
        parallel_walk = false; // (empty; grid limit: 2 TiB at the default)
    const uint32_t nseg = parallel_walk ? (uint32_t)nseg64 : 0;
    // The stream is a batch of one: the call's scalars go where the batch's
    // arrays lie (frame_front_result), beside the fronts' own state.  All of
    // it is sized here, once: a retry below grows the chunk table only.
    FrameDecodeArgs a;
    FrameBatchDecodeArgs b;
    a.in = (const uint8_t *)d_in;
    a.in_len = in_len;
    a.out = (uint8_t *)d_out;
    a.out_cap = out_cap;
    a.flags = flags;
    a.chained = 0;
    for (int k = 0; k < 10; k++)
        a.stale[k] = stale10 ? stale10[k] : 0;
    a.nseg = nseg;
    a.fw_seg = fw_seg;
    int rc = fbd_streams(ctx, b, 1, &a);
    if (rc || (!nowait && (rc = mailbox(ctx))))
        return rc;
    hipStream_t s = ctx->stream;
    b.in_ptrs = a.in_ptrs;
    b.in_lens = a.in_lens;
    b.out_ptrs = d_out ? a.out_ptrs : nullptr; // nullptr = lengths only
    b.out_caps = a.out_caps;
    b.out_lens = d_out_len;
    b.errs = d_err;
    if (nowait) {
        // Nothing comes back to the host: the table, the fronts and every
        // launch behind them are sized from in_len and the caller's bound,
        // the fronts are enqueued back to back and the order on the stream
        // lets the first that decides win (snapmi_framewalk.hpp).  Scratch
        // that must grow is the only wait, here and in fbd_finish.
        if ((rc = reserve(ctx, ctx->fr_nowait, sizeof(uint32_t))) ||
            (rc = fbd_table(ctx, what, b, n_chunks)))
            return rc;
        a.chunks = b.chunks;
        a.c_stream = b.c_stream;
        a.index = d_chunk_offsets;
        a.n_index = use_index ? (uint32_t)n_chunks : 0;
        a.cap_chunks = (uint32_t)n_chunks;
        const uint32_t tb = 256;
        const uint32_t gb =
            n_chunks ? (uint32_t)((n_chunks + tb - 1) / tb) : 1;
        const uint32_t first_front = use_index        ? kFrontIndex
                                     : parallel_walk ? kFrontParallel
                                                     : kFrontWalk;
        if (first_front != kFrontWalk) {
            if ((rc = frame_front(ctx, a, first_front)))
                return rc;
            a.chained = 1;
        }
        if ((rc = frame_front(ctx, a, kFrontWalk)))
            return rc;
        hipLaunchKernelGGL(k_frame_nowait_seal, dim3(gb), dim3(tb), 0, s, a,
                           first_front, (uint32_t *)ctx->fr_nowait.p);
        HIP_TRY(ctx, hipGetLastError());
        ctx->fr_nowait_live = true;
        b.total = (uint32_t)n_chunks;
        return fbd_finish(ctx, b);
    }
    for (int attempt = 0; attempt < 4; attempt++) {
        if (cap > 0x7FFFFFFFu)
            return fail_ctx(ctx, SNAPMI_E_ARGUMENT, "frame: too many chunks");
        const size_t n = (size_t)cap;
        if ((rc = fbd_table(ctx, what, b, cap)))
            return rc;
        a.chunks = b.chunks;
        a.c_stream = b.c_stream;
        a.index = use_index ? d_chunk_offsets : nullptr;
        a.n_index = use_index ? (uint32_t)n_chunks : 0;
        a.cap_chunks = (uint32_t)n;
        if ((rc = frame_front(ctx, a,
                              use_index       ? kFrontIndex
                              : parallel_walk ? kFrontParallel
                                              : kFrontWalk)))
            return rc;
        // the number of data chunks decides the launch sizes below
        uint32_t meta[3];
        if ((rc = post_words(ctx, s, (uint32_t *)ctx->h_mail, a.meta, 3u)))
            return rc;
        HIP_TRY(ctx, hipStreamSynchronize(s));
        memcpy(meta, (const void *)ctx->h_mail, sizeof meta);
        if (use_index && meta[2]) { // the index does not tile the stream with
            use_index = false;      // plain data chunks: the walk decides
            cap = n_chunks + in_len / 65536 + 64;
            continue;
        }
        if (parallel_walk && meta[2] == 2) { // something in the stream that
            parallel_walk = false;           // only the sequential walk judges
            continue;
        }
        if (meta[1] && !use_index && cap < meta[0]) { // table too small
            cap = meta[0];
            continue;
        }
        b.total = meta[0] < n ? meta[0] : (uint32_t)n;
        return fbd_finish(ctx, b);
    }
    return fail_ctx(ctx, SNAPMI_E_DEVICE, "frame: chunk table retry failed");
}

int snapmi_frame_decompress(snapmi_ctx *ctx, const void *d_in,
                            uint64_t in_len, void *d_out, uint64_t out_cap,
                            uint64_t *d_out_len, snapmi_error *d_err,
                            const uint64_t *d_chunk_offsets,
                            uint64_t n_chunks)
{
    return snapmi_frame_decompress_ex(ctx, d_in, in_len, d_out, out_cap,
                                      d_out_len, d_err, d_chunk_offsets,
                                      n_chunks, 0, nullptr);
}

int snapmi_frame_decompress_batch(snapmi_ctx *ctx,
                                  const void *const *d_in_ptrs,
                                  const uint64_t *d_in_lens,
                                  void *const *d_out_ptrs,
                                  const uint64_t *d_out_caps,
                                  uint64_t *d_out_lens, snapmi_error *d_errs,
                                  size_t n)
{
    const char *what = "frame_decompress_batch";
    if (!ctx)
        return SNAPMI_E_ARGUMENT;
    if (n == 0)
        return SNAPMI_OK;
    FrameBatchDecodeArgs a;
    int rc = fbd_begin(ctx, what, d_in_ptrs, d_in_lens, d_out_ptrs, d_out_caps,
                       d_out_lens, d_errs, n, a);
    if (rc || (rc = mailbox(ctx)))
        return rc;
    hipStream_t s = ctx->stream;
    const uint32_t gs = (uint32_t)((n + 63) / 64);
    hipLaunchKernelGGL(k_fbd_walk_count, dim3(gs), dim3(64), 0, s, a);
    if ((rc = launch_scan_u64(ctx, s, a.counts, a.first, (uint32_t)n)))
        return rc;
    // the one wait: the number of data chunks sizes everything below
    if ((rc = post_words(ctx, s, (uint32_t *)ctx->h_mail,
                         (const uint32_t *)(a.first + n), 2u)))
        return rc;
    HIP_TRY(ctx, hipStreamSynchronize(s));
    const uint64_t total =
        (uint64_t)ctx->h_mail[0] | ((uint64_t)ctx->h_mail[1] << 32);
    if ((rc = fbd_table(ctx, what, a, total)))
        return rc;
    // the same walk again, now with a place for every chunk record
    if (total)
        hipLaunchKernelGGL(k_fbd_walk_fill, dim3(gs), dim3(64), 0, s, a);
    return fbd_finish(ctx, a);
}

} // extern "C"

// snapmi_frame_decompress_batch of streams the host has walked
// (snapmi_framewalk.hpp: frame_walk_host found every one of them well-formed
// from start to end): d_first[i] is the first data chunk of stream i
// (d_first[n] = total), d_list the chunks.  k_fbd_from_list stands in for the
// two walk kernels, the scan of their counts and the wait for the total, so
// this call only enqueues; a list that disagrees with the bytes sets *d_bad
// (device memory the caller has cleared) and leaves nothing decoded from the
// chunks in question.  Verdicts, lengths and error fields come from the
// kernels behind it, as ever.
int snapmi::frame_decompress_batch_listed(
    snapmi_ctx *ctx, const void *const *d_in_ptrs, const uint64_t *d_in_lens,
    void *const *d_out_ptrs, const uint64_t *d_out_caps, uint64_t *d_out_lens,
    snapmi_error *d_errs, size_t n, const uint64_t *d_first,
    const void *d_list, uint64_t total, uint32_t *d_bad)
{
    const char *what = "frame_decompress_batch (listed)";
    if (!ctx || !d_first || !d_list || !d_bad)
        return fail_ctx(ctx, SNAPMI_E_ARGUMENT, "%s: bad args", what);
    if (n == 0)
        return SNAPMI_OK;
    FrameBatchDecodeArgs a;
    int rc = fbd_begin(ctx, what, d_in_ptrs, d_in_lens, d_out_ptrs, d_out_caps,
                       d_out_lens, d_errs, n, a);
    if (rc || (rc = fbd_table(ctx, what, a, total)))
        return rc;
    const uint32_t tb = 256;
    hipLaunchKernelGGL(k_fbd_from_list,
                       dim3((uint32_t)((total + n + tb - 1) / tb)), dim3(tb), 0,
                       ctx->stream, a, d_first, (const FwEntry *)d_list,
                       d_bad);
    return fbd_finish(ctx, a);
}
