// snapmi_frame.hip -- Snappy frame format on the device (gfx950).
//
// Reference: src/frame.rs (chunk layout, compress_frame), src/crc32.rs
// (masked CRC32C), src/write.rs (chunking of write::FrameEncoder),
// src/read.rs (read::FrameDecoder state machine).  A framed stream is a
// 10-byte stream identifier followed by chunks
//     type(1) | len24 LE (= 4 + payload) | masked crc32c(uncompressed) LE | payload
// and every data chunk (<= 64 KiB of input) is an independent raw stream, so
// the chunk is the parallel unit: the raw codec kernels run unchanged on a
// batch whose "streams" are the chunks.  The chunks of all the streams of a
// call form one list (stream i owns chunks [first[i], first[i+1])); a call
// for one stream is a list of one stream.
//
// Kernels here:
//   k_crc32c          masked CRC32C, one wavefront per buffer, 64 interleaved
//                     partial CRCs advanced 256 bytes per step with 4 LDS
//                     table lookups, combined by GF(2) multiplication
//   k_crc_plan, k_crc_segments, k_crc_finish
//                     the same of buffers of more than 64 KiB, cut into
//                     segments that the whole device shares (snapmi_crc.hpp)
//   k_scan_u64        exclusive scan (one workgroup; snapmi_scan.hpp)
//   k_fb_chunks       compress side: chunk descriptors for the raw compressor
//   k_fb_sizes        compressed-vs-stored decision (src/frame.rs:85) + sizes
//   k_fb_emit         headers + payloads into the framed streams
//   k_frame_walk      decode side, one stream: sequential walk over the chunk
//                     headers (the format has no index) with the reference's
//                     checks; k_fw_* find the headers of a long stream in
//                     parallel, k_frame_index checks a side index
//   k_fbd_walk_*      decode side, many streams: one thread walks a stream
//   k_fbd_lens        decompressed length of every data chunk
//   k_fbd_desc        descriptors for the raw decompressor
//   k_fbd_verify_*    CRC comparison, first error in stream order
#include <hip/hip_runtime.h>

#include <string.h>
#include <vector>

#include <chrono>

#include "snapmi.h"
#include "snapmi_ctx.hpp"
#include "snapmi_hostpipe.hpp"
#include "snapmi_device.hpp"
#include "snapmi_kernels.hpp"
#include "snapmi_scan.hpp"
#include "snapmi_crc.hpp"
#include "snapmi_framewalk.hpp"

using namespace snapmi;

namespace snapmi {

constexpr uint32_t kFrameSlot = 76496;          // kMaxChunk rounded to 16
// (kMaxChunk, FrameChunk and the chunk-header walk: snapmi_framewalk.hpp)
static_assert(kFwMaxBlock == kMaxBlock && kFwMaxInput == kMaxInput,
              "snapmi_framewalk.hpp restates the codec's limits");

// Tables for k_crc32c, generated once per context on the host (the
// reference generates its tables at build time, build.rs:97-124).
struct CrcTables {
    uint32_t z256[4][256]; // state advanced by 256 zero bytes, per input byte
    uint32_t lane_mul[64]; // x^(8*4*(64-j)) mod P: final advance of lane j
    uint32_t init_adv[65537]; // 0xFFFFFFFF advanced by n zero bytes
    uint32_t pow2[64];        // x^(8 * 2^k) mod P (crc_pow2_table)
};
// (gf_mul, the powers of x and the cut of a long buffer: snapmi_crc.hpp)

// The zero-initial-state CRC state of m[0, len), len <= kCrcSegment, by one
// wavefront; z = the four z256 tables in LDS.  The message is zero-padded at
// the FRONT to a multiple of 256 bytes (leading zeros do not move a zero
// state); lane j owns dwords j, j+64, ... and keeps a_j = Z256(a_j) ^ dword,
// where Z256 = "advance 256 zero bytes".  The 64 partial states are advanced
// to the end (one GF(2) product each) and XOR-reduced: every lane returns the
// state, without the initial state's term and before the mask.  Reads
// m[0, len) and nothing else (the dword that straddles the front bytewise).
__device__ __forceinline__ uint32_t crc_wave_state(const uint32_t *z, gcptr m,
                                                   uint32_t len, uint32_t lane,
                                                   const CrcTables *tab)
{
    const uint32_t pad = (256 - (len & 255)) & 255;
    const uint32_t steps = (len + pad) >> 8;
    uint32_t a = 0;
    for (uint32_t t = 0; t < steps; t++) {
        const uint32_t pos = 256 * t + 4 * lane; // in the padded message
        uint32_t w;
        if (pos >= pad) {
            w = ld32u(m + (pos - pad));
        } else if (pos + 4 <= pad) {
            w = 0;
        } else { // the dword that straddles the start of the data
            w = 0;
            for (uint32_t b = pad - pos; b < 4; b++)
                w |= (uint32_t)m[pos + b - pad] << (8 * b);
        }
        a = z[a & 255] ^ z[256 + ((a >> 8) & 255)] ^
            z[512 + ((a >> 16) & 255)] ^ z[768 + (a >> 24)] ^ w;
    }
    uint32_t f = gf_mul(tab->lane_mul[lane], a);
    for (uint32_t o = 32; o; o >>= 1)
        f ^= __shfl_xor(f, o);
    return f;
}

// x^(8 * t) mod P in every lane of a wavefront: lane k holds x^(8 * 2^k) when
// bit k of t is set and 1 otherwise, six shuffle rounds multiply the 64
// together (crc_pow8 is the same product, one factor after the other).
__device__ __forceinline__ uint32_t crc_wave_pow8(const CrcTables *tab,
                                                  uint64_t t, uint32_t lane)
{
    uint32_t p = ((t >> lane) & 1) ? tab->pow2[lane] : kCrcX0;
    for (uint32_t o = 32; o; o >>= 1)
        p = gf_mul(p, __shfl_xor(p, o));
    return p;
}

// ---------------------------------------------------------------------
// K4: masked CRC32C of n buffers (<= 65536 bytes each), one wavefront each:
// crc_wave_state above, and the contribution of the initial state 0xFFFFFFFF
// from a table.  Equals crc32c_slice16 / the SSE4.2 instruction of reference
// src/crc32.rs:59-111; mask :35-38.  A longer buffer is not this kernel's:
// its wavefront writes nothing (k_crc_plan / k_crc_segments / k_crc_finish
// behind snapmi_crc32c_masked_batch; the frame codec's chunks are never
// longer).
// ---------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_crc32c(const void *const *ptrs,
                                               const uint64_t *lens,
                                               uint32_t *out, uint32_t n,
                                               const CrcTables *tab)
{
    __shared__ uint32_t z[4 * 256];
    const uint32_t lane = threadIdx.x;
    const uint32_t i = blockIdx.x;
    if (i >= n || lens[i] > kCrcShort)
        return;
    for (uint32_t k = lane; k < 1024; k += 64)
        z[k] = tab->z256[k >> 8][k & 255];
    __syncthreads();
    const uint32_t len = (uint32_t)lens[i];
    const uint32_t f = crc_wave_state(z, (gcptr)ptrs[i], len, lane, tab);
    if (lane == 0)
        out[i] = crc_mask(f ^ tab->init_adv[len]); // src/crc32.rs:37
}

// ---------------------------------------------------------------------
// Buffers of more than 65536 bytes (snapmi_crc32c_masked_batch only), cut
// into segments of kCrcSegment bytes as snapmi_crc.hpp says; three launches
// behind k_crc32c, sized from n and the CU count alone:
//   k_crc_plan      one workgroup: segments per buffer, their scan
//                   seg_first[0..n], and a zero accumulator per buffer;
//   k_crc_segments  a fixed grid of wavefronts strides over the segments
//                   0 .. seg_first[n]: the segment's state, advanced past
//                   its tail, goes into its buffer's accumulator by a global
//                   atomic XOR (linear: no order); the wavefront of a
//                   buffer's segment 0 adds the initial state's term;
//   k_crc_finish    one thread per buffer: complement, rotate, mask, store -
//                   of the long buffers only.
// ---------------------------------------------------------------------
// k_crc_segments' grid: wavefronts per CU - all a CU holds, 8 per SIMD (each
// has 4 KiB of LDS): a step waits for memory, the rate is the wavefronts in
// flight (kCrcSegment, snapmi_crc.hpp)
constexpr uint32_t kCrcWavesPerCu = 32;
// buffers per item of k_crc_plan's scan: 16 384 buffers are one stride of the
// workgroup, and a thread's 16 loads are in flight together
constexpr uint32_t kCrcPlanGroup = 16;

__global__ __launch_bounds__(1024) void k_crc_plan(const uint64_t *lens,
                                                   uint32_t n,
                                                   uint64_t *seg_first,
                                                   uint32_t *acc)
{
    uint64_t carry[1] = {0};
    const uint32_t groups = (n + kCrcPlanGroup - 1) / kCrcPlanGroup;
    wg_scan_strided(
        groups, carry,
        [&](uint32_t g, uint64_t (&x)[1]) {
            const uint32_t lo = g * kCrcPlanGroup;
            for (uint32_t i = lo; i < n && i - lo < kCrcPlanGroup; i++)
                x[0] += crc_segments(lens[i], kCrcSegment);
        },
        [&](uint32_t g, const uint64_t (&)[1], const uint64_t (&ex)[1]) {
            const uint32_t lo = g * kCrcPlanGroup;
            uint64_t at = ex[0];
            for (uint32_t i = lo; i < n && i - lo < kCrcPlanGroup; i++) {
                seg_first[i] = at;
                acc[i] = 0;
                at += crc_segments(lens[i], kCrcSegment);
            }
        });
    if (threadIdx.x == 0)
        seg_first[n] = carry[0];
}

__global__ __launch_bounds__(64) void k_crc_segments(
    const void *const *ptrs, const uint64_t *lens, uint32_t n,
    const uint64_t *seg_first, uint32_t *acc, const CrcTables *tab)
{
    __shared__ uint32_t z[4 * 256];
    const uint32_t lane = threadIdx.x;
    const uint64_t total = seg_first[n];
    if (blockIdx.x >= total)
        return; // (a call without a long buffer: every wavefront, at once)
    for (uint32_t k = lane; k < 1024; k += 64)
        z[k] = tab->z256[k >> 8][k & 255];
    __syncthreads();
    for (uint64_t s = blockIdx.x; s < total; s += gridDim.x) {
        const CrcSeg g = crc_find_segment(seg_first, lens, n, s, kCrcSegment);
        const uint32_t f = crc_wave_state(z, (gcptr)ptrs[g.buffer] + g.off,
                                          (uint32_t)g.len, lane, tab);
        uint32_t v = crc_advance(f, crc_wave_pow8(tab, g.tail, lane));
        if (g.segment == 0)
            v ^= crc_init_term(crc_wave_pow8(tab, lens[g.buffer], lane));
        if (lane == 0)
            atomicXor(&acc[g.buffer], v);
    }
}

__global__ void k_crc_finish(const uint64_t *lens, uint32_t n,
                             const uint32_t *acc, uint32_t *out)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && lens[i] > kCrcShort)
        out[i] = crc_mask(acc[i]);
}

// exclusive scan of n u64 values, out[n] = total; one workgroup
__global__ __launch_bounds__(1024) void k_scan_u64(const uint64_t *in,
                                                   uint64_t *out, uint32_t n)
{
    uint64_t carry[1] = {0};
    wg_scan_strided(
        n, carry, [&](uint32_t i, uint64_t (&x)[1]) { x[0] = in[i]; },
        [&](uint32_t i, const uint64_t (&)[1], const uint64_t (&ex)[1]) {
            out[i] = ex[0];
        });
    if (threadIdx.x == 0)
        out[n] = carry[0];
}

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
constexpr uint32_t kFwCands = 32;

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

__device__ inline uint64_t frame_max_len_dev(uint64_t n)
{
    return 10 + n + 8 * ((n + kMaxBlock - 1) / kMaxBlock);
}

// stream i has no room: cap_i < snapmi_frame_max_len(len_i) (an empty input
// writes nothing and needs none, as snapmi_frame_compress)
__device__ inline bool fb_refused(const FrameBatchCompressArgs &a, uint32_t i)
{
    const uint64_t len = a.in_lens[i];
    return a.out_caps && len && a.out_caps[i] < frame_max_len_dev(len);
}

// A lone stream as a list of one stream: the call's scalars in the places of
// the per-stream arrays (chunks: as the caller cut them, or one per 65536
// bytes); its first chunk is the list's first.
__global__ void k_fb_lone(const void **in_ptrs, uint64_t *in_lens,
                          void **out_ptrs, uint64_t *first, uint64_t *sbase,
                          const void *in, uint64_t in_len, void *out,
                          uint64_t chunks)
{
    in_ptrs[0] = in;
    in_lens[0] = in_len;
    out_ptrs[0] = out;
    first[0] = 0;
    first[1] = chunks;
    sbase[0] = 0;
}

__global__ void k_fb_counts(FrameBatchCompressArgs a)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < a.n)
        a.counts[i] = (a.in_lens[i] + kMaxBlock - 1) / kMaxBlock;
}

// the stream owning list entry t: the last i with first[i] <= t
__device__ inline uint32_t fb_stream_of(const uint64_t *first, uint32_t n,
                                        uint32_t t)
{
    uint32_t lo = 0, hi = n - 1;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo + 1) / 2;
        if (first[mid] <= t)
            lo = mid;
        else
            hi = mid - 1;
    }
    return lo;
}

// thread t: stream t's capacity check and result slots, list entry t's
// chunk descriptor, segment slot t's pointer; thread 0 clears the carry (here,
// not by a memset: a memset a call costs a one-stream call 4 us)
__global__ void k_fb_chunks(FrameBatchCompressArgs a)
{
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t == 0)
        a.carry[0] = 0;
    if (t < a.n) {
        const bool r = fb_refused(a, t);
        a.refused[t] = r;
        a.out_lens[t] = 0;
        if (a.errs)
            a.errs[t] = r ? frame_err(SNAPMI_BUFFER_TOO_SMALL, a.out_caps[t],
                                      frame_max_len_dev(a.in_lens[t]))
                          : frame_err(SNAPMI_OK, 0, 0);
    }
    if (t < a.total) {
        const uint32_t i = fb_stream_of(a.first, a.n, t);
        uint64_t off, len;
        if (a.chunk_in_off) {
            off = a.chunk_in_off[t];
            len = a.chunk_in_off[t + 1] - off;
        } else {
            off = (t - a.first[i]) * (uint64_t)kMaxBlock;
            len = a.in_lens[i] - off < kMaxBlock ? a.in_lens[i] - off
                                                 : kMaxBlock;
        }
        a.c_in[t] = (const uint8_t *)a.in_ptrs[i] + off;
        a.c_len[t] = len;
        a.c_stream[t] = i;
    }
    if (t < a.seg)
        a.slot_ptrs[t] = a.slots + (uint64_t)t * kFrameSlot;
}

// reference compress_frame, src/frame.rs:83-89; nothing for a refused stream
__global__ void k_fb_sizes(FrameBatchCompressArgs a)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.cnt)
        return;
    const uint32_t gi = a.lo + i;
    const uint64_t len = a.c_len[gi];
    const uint64_t clen = a.clens[i];
    const bool stored = clen >= len - len / 8;
    a.sizes[i] = a.refused[a.c_stream[gi]] ? 0 : 8 + (stored ? len : clen);
}

// The list offset of every stream whose first chunk lies in this segment,
// fixed before the segment's emit (which reads it in other workgroups; a
// stream that started in an earlier segment has it already).
__global__ void k_fb_base(FrameBatchCompressArgs a)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.cnt)
        return;
    const uint32_t gi = a.lo + i;
    const uint32_t s = a.c_stream[gi];
    if (a.first[s] == gi)
        a.sbase[s] = a.carry[0] + a.offs[i];
}

// one chunk at o: header (src/frame.rs:91-93) by thread 0, then the payload
// from `from` by the whole workgroup
__device__ inline void frame_put_chunk(gptr o, bool stored, uint64_t payload,
                                       uint32_t crc, gcptr from)
{
    if (threadIdx.x == 0) {
        const uint32_t cl = 4 + (uint32_t)payload;
        o[0] = stored ? 0x01 : 0x00;
        o[1] = (uint8_t)cl;
        o[2] = (uint8_t)(cl >> 8);
        o[3] = (uint8_t)(cl >> 16);
        o[4] = (uint8_t)crc;
        o[5] = (uint8_t)(crc >> 8);
        o[6] = (uint8_t)(crc >> 16);
        o[7] = (uint8_t)(crc >> 24);
    }
    gptr to = o + 8;
    for (uint64_t k = 4 * threadIdx.x; k + 4 <= payload; k += 4 * blockDim.x)
        st32u(to + k, ld32u(from + k));
    const uint64_t t = payload & ~3ull;
    if (threadIdx.x < (payload & 3))
        to[t + threadIdx.x] = from[t + threadIdx.x];
}

// one workgroup per chunk of the segment: the stream identifier (first
// chunk), header (src/frame.rs:91-93) and payload at the chunk's offset in
// its stream; the stream's last chunk writes its length
__global__ __launch_bounds__(256) void k_fb_emit(FrameBatchCompressArgs a)
{
    const uint32_t i = blockIdx.x;
    const uint32_t gi = a.lo + i;
    const uint32_t s = a.c_stream[gi];
    if (a.refused[s])
        return;
    const uint64_t len = a.c_len[gi];
    const uint64_t clen = a.clens[i];
    const bool stored = clen >= len - len / 8;
    const uint64_t payload = stored ? len : clen;
    const uint64_t at = a.ident + a.carry[0] + a.offs[i] - a.sbase[s];
    gptr base = (gptr)a.out_ptrs[s];
    gptr o = base + at;
    if (gi == a.first[s] && threadIdx.x < a.ident) {
        const uint8_t ident[10] = {0xFF, 0x06, 0x00, 0x00, 's',
                                   'N',  'a',  'P',  'p',  'Y'};
        base[threadIdx.x] = ident[threadIdx.x];
    }
    frame_put_chunk(o, stored, payload, a.crcs[i],
                    stored ? (gcptr)a.c_in[gi]
                           : (gcptr)(a.slots + (uint64_t)i * kFrameSlot));
    if (threadIdx.x == 0) {
        if (a.chunk_offsets) {
            a.chunk_offsets[gi] = at;
            if (gi + 1 == a.total)
                a.chunk_offsets[a.total] = at + 8 + payload;
        }
        if (gi + 1 == a.first[s + 1])
            a.out_lens[s] = at + 8 + payload;
    }
}

__global__ void k_fb_advance(FrameBatchCompressArgs a)
{
    a.carry[0] += a.offs[a.cnt];
}

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

// ---------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------
static int ensure_tables(snapmi_ctx *ctx)
{
    if (ctx->fr_tables_ready)
        return SNAPMI_OK;
    int rc = reserve(ctx, ctx->fr_tables, sizeof(CrcTables));
    if (rc)
        return rc;
    std::vector<uint8_t> buf(sizeof(CrcTables));
    CrcTables *t = (CrcTables *)buf.data();
    uint32_t byte_tab[256];
    for (uint32_t i = 0; i < 256; i++) { // reference build.rs:110-124
        uint32_t c = i;
        for (int k = 0; k < 8; k++)
            c = (c & 1) ? (c >> 1) ^ kCrcPoly : c >> 1;
        byte_tab[i] = c;
    }
    auto adv1 = [&](uint32_t s) { return byte_tab[s & 255] ^ (s >> 8); };
    for (int k = 0; k < 4; k++)
        for (uint32_t b = 0; b < 256; b++) {
            uint32_t s = b << (8 * k);
            for (int z = 0; z < 256; z++)
                s = adv1(s);
            t->z256[k][b] = s;
        }
    // x^(8*n) mod P = the state 0x80000000 (x^0) advanced by n zero bytes
    for (uint32_t j = 0; j < 64; j++) {
        uint32_t s = 1u << 31;
        for (uint32_t z = 0; z < 4 * (64 - j); z++)
            s = adv1(s);
        t->lane_mul[j] = s;
    }
    uint32_t s = 0xFFFFFFFFu;
    for (uint32_t n = 0; n <= 65536; n++) {
        t->init_adv[n] = s;
        s = adv1(s);
    }
    crc_pow2_table(t->pow2);
    HIP_TRY(ctx, hipMemcpyAsync(ctx->fr_tables.p, buf.data(),
                                sizeof(CrcTables), hipMemcpyHostToDevice,
                                ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    ctx->fr_tables_ready = true;
    return SNAPMI_OK;
}

template <class T> static T *carve(uint8_t *&p, size_t count)
{
    uintptr_t a = ((uintptr_t)p + 15) & ~(uintptr_t)15;
    T *r = (T *)a;
    p = (uint8_t *)(a + count * sizeof(T));
    return r;
}

} // namespace snapmi

extern "C" {

size_t snapmi_frame_max_len(size_t n)
{
    const size_t chunks = (n + kMaxBlock - 1) / kMaxBlock;
    return 10 + n + 8 * chunks;
}

int snapmi_crc32c_masked_batch(snapmi_ctx *ctx, const void *const *d_ptrs,
                               const uint64_t *d_lens, uint32_t *d_out,
                               size_t n)
{
    if (!ctx || (n && (!d_ptrs || !d_lens || !d_out)) || n > 0x7FFFFFFFu)
        return SNAPMI_E_ARGUMENT;
    if (n == 0)
        return SNAPMI_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    int rc = ensure_tables(ctx);
    if (rc)
        return rc;
    // the long route's scratch: seg_first[n + 1] and an accumulator per
    // buffer - a matter of n alone; the lengths stay on the device
    if ((rc = reserve(ctx, ctx->fr_crc, (n + 1) * 8 + n * 4 + 16)))
        return rc;
    uint8_t *p = (uint8_t *)ctx->fr_crc.p;
    uint64_t *seg_first = carve<uint64_t>(p, n + 1);
    uint32_t *acc = carve<uint32_t>(p, n);
    const CrcTables *tab = (const CrcTables *)ctx->fr_tables.p;
    hipStream_t s = ctx->stream;
    hipLaunchKernelGGL(k_crc32c, dim3((uint32_t)n), dim3(64), 0, s, d_ptrs,
                       d_lens, d_out, (uint32_t)n, tab);
    hipLaunchKernelGGL(k_crc_plan, dim3(1), dim3(1024), 0, s, d_lens,
                       (uint32_t)n, seg_first, acc);
    hipLaunchKernelGGL(k_crc_segments,
                       dim3(kCrcWavesPerCu *
                            (uint32_t)(ctx->num_cus > 0 ? ctx->num_cus : 256)),
                       dim3(64),
                       0, s, d_ptrs, d_lens, (uint32_t)n, seg_first, acc, tab);
    hipLaunchKernelGGL(k_crc_finish, dim3((uint32_t)((n + 255) / 256)),
                       dim3(256), 0, s, d_lens, (uint32_t)n, acc, d_out);
    HIP_TRY(ctx, hipGetLastError());
    return SNAPMI_OK;
}

} // extern "C"

namespace snapmi {
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
static int frame_compress_list(snapmi_ctx *ctx, const FrameList &l)
{
    hipStream_t s = ctx->stream;
    const size_t n = l.n;
    const uint64_t total = l.total;
    const bool lone = l.lone;
    // segments of at most lane_segment_blocks chunks (16 GiB of input by
    // default): 76 KiB of slot + 72 KiB of tokens per chunk of a segment;
    // per segment the chunks of at most 8 KiB for the compressor's routing
    // (chunks cut short by the caller - flushes, short reads -, else only a
    // stream's last chunk can be one)
    const uint32_t seg = total < ctx->lane_segment_blocks
                             ? (uint32_t)total
                             : ctx->lane_segment_blocks;
    std::vector<uint64_t> c8(seg ? (total + seg - 1) / seg : 0, 0);
    if (l.h_chunk_lens) {
        for (uint64_t t = 0; t < total; t++)
            c8[t / seg] += l.h_chunk_lens[t] <= 8192;
    } else {
        for (uint64_t i = 0, at = 0; i < n; i++) {
            const uint64_t len = l.h_in_lens[i];
            const uint64_t k = (len + kMaxBlock - 1) / kMaxBlock;
            if (k && len - (k - 1) * kMaxBlock <= 8192)
                c8[(at + k - 1) / seg]++;
            at += k;
        }
    }
    int rc = ensure_tables(ctx);
    if (rc)
        return rc;
    const size_t bytes = n * (8 + 8 + 1 + 8) + 8 + 3 * 8 +
                         total * (8 + 8 + 4) +
                         (size_t)seg * (8 + 8 + 4 + 8 + 8) + 8 + 8 + 16 * 16;
    if ((rc = reserve(ctx, ctx->fr_desc, bytes)) ||
        (seg && (rc = reserve(ctx, ctx->fr_slots, (size_t)seg * kFrameSlot))))
        return rc;
    FrameBatchCompressArgs a;
    uint8_t *p = (uint8_t *)ctx->fr_desc.p;
    // (a lone stream's scalars take the places of the arrays: k_fb_lone)
    const void **lone_in = carve<const void *>(p, lone ? 1 : 0);
    uint64_t *lone_len = carve<uint64_t>(p, lone ? 1 : 0);
    void **lone_out = carve<void *>(p, lone ? 1 : 0);
    a.in_ptrs = lone ? lone_in : l.in_ptrs;
    a.in_lens = lone ? lone_len : l.in_lens;
    a.out_ptrs = lone ? lone_out : l.out_ptrs;
    a.out_caps = l.out_caps;
    a.out_lens = l.out_lens;
    a.errs = l.errs;
    a.n = (uint32_t)n;
    a.total = (uint32_t)total;
    a.seg = seg;
    a.chunk_in_off = l.chunk_in_off;
    a.chunk_offsets = l.chunk_offsets;
    a.ident = l.ident ? 10 : 0;
    a.counts = carve<uint64_t>(p, n);
    a.first = carve<uint64_t>(p, n + 1);
    a.refused = carve<uint8_t>(p, n);
    a.sbase = carve<uint64_t>(p, n);
    a.c_in = carve<const void *>(p, total);
    a.c_len = carve<uint64_t>(p, total);
    a.c_stream = carve<uint32_t>(p, total);
    a.carry = carve<uint64_t>(p, 1);
    a.slot_ptrs = carve<void *>(p, seg);
    a.clens = carve<uint64_t>(p, seg);
    a.crcs = carve<uint32_t>(p, seg);
    a.sizes = carve<uint64_t>(p, seg);
    a.offs = carve<uint64_t>(p, (size_t)seg + 1);
    a.slots = (uint8_t *)ctx->fr_slots.p;
    a.lo = a.cnt = 0;

    const uint32_t tb = 256;
    uint64_t most = total > n ? total : n;
    if (lone) {
        hipLaunchKernelGGL(k_fb_lone, dim3(1), dim3(1), 0, s, lone_in,
                           lone_len, lone_out, a.first, a.sbase, l.in,
                           l.in_len, l.out, total);
    } else {
        hipLaunchKernelGGL(k_fb_counts, dim3((uint32_t)((n + tb - 1) / tb)),
                           dim3(tb), 0, s, a);
        hipLaunchKernelGGL(k_scan_u64, dim3(1), dim3(1024), 0, s, a.counts,
                           a.first, (uint32_t)n);
    }
    hipLaunchKernelGGL(k_fb_chunks, dim3((uint32_t)((most + tb - 1) / tb)),
                       dim3(tb), 0, s, a);
    for (uint32_t lo = 0; lo < total; lo += seg) {
        const uint32_t cnt = total - lo < seg ? (uint32_t)total - lo : seg;
        a.lo = lo;
        a.cnt = cnt;
        const uint32_t gb = (cnt + tb - 1) / tb;
        // The checksums only need the input: they run on the side stream,
        // under the match finder (which waits on HBM round trips and leaves
        // 16 KiB of LDS per CU free - room for three CRC workgroups).  Fusing
        // the CRC into the match finder's own block loads would add ~380
        // vector instructions per 128-byte line to a loop of ~150 per round
        // to save a kernel of 1 % of the pass: not done.
        const bool side = ctx->frame_crc_side_stream;
        if (side) {
            HIP_TRY(ctx, hipEventRecord(ctx->ev_crc[0], s));
            HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream2, ctx->ev_crc[0], 0));
        }
        hipLaunchKernelGGL(k_crc32c, dim3(cnt), dim3(64), 0,
                           side ? ctx->stream2 : s, a.c_in + lo, a.c_len + lo,
                           a.crcs, cnt, (const CrcTables *)ctx->fr_tables.p);
        if (side)
            HIP_TRY(ctx, hipEventRecord(ctx->ev_crc[1], ctx->stream2));
        // every chunk is a one-block raw stream: cnt blocks, no scratch slots
        rc = launch_compress(ctx, a.c_in + lo, a.c_len + lo, a.slot_ptrs,
                             nullptr, a.clens, nullptr, cnt, cnt, 0, 0xF,
                             c8[lo / seg]);
        if (rc)
            return rc;
        if (side)
            HIP_TRY(ctx, hipStreamWaitEvent(s, ctx->ev_crc[1], 0));
        hipLaunchKernelGGL(k_fb_sizes, dim3(gb), dim3(tb), 0, s, a);
        hipLaunchKernelGGL(k_scan_u64, dim3(1), dim3(1024), 0, s, a.sizes,
                           a.offs, cnt);
        if (!lone) // (a lone stream's first chunk is the list's: k_fb_lone)
            hipLaunchKernelGGL(k_fb_base, dim3(gb), dim3(tb), 0, s, a);
        hipLaunchKernelGGL(k_fb_emit, dim3(cnt), dim3(256), 0, s, a);
        hipLaunchKernelGGL(k_fb_advance, dim3(1), dim3(1), 0, s, a);
    }
    HIP_TRY(ctx, hipGetLastError());
    return SNAPMI_OK;
}
} // namespace snapmi

extern "C" {

int snapmi_frame_compress(snapmi_ctx *ctx, const void *d_in, uint64_t in_len,
                          void *d_out, uint64_t out_cap, uint64_t *d_out_len,
                          uint64_t *d_chunk_offsets)
{
    if (!ctx || !d_out_len || (in_len && (!d_in || !d_out)))
        return SNAPMI_E_ARGUMENT;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    if (in_len == 0) { // the identifier is written lazily: src/write.rs:154-170
        HIP_TRY(ctx, hipMemsetAsync(d_out_len, 0, sizeof(uint64_t), s));
        return SNAPMI_OK;
    }
    if (out_cap < snapmi_frame_max_len(in_len))
        return fail_ctx(ctx, SNAPMI_E_ARGUMENT,
                        "frame_compress: out_cap %llu < frame_max_len %zu",
                        (unsigned long long)out_cap,
                        snapmi_frame_max_len(in_len));
    const uint64_t n64 = (in_len + kMaxBlock - 1) / kMaxBlock;
    if (n64 > 0x7FFFFFFFu)
        return fail_ctx(ctx, SNAPMI_E_ARGUMENT, "frame_compress: too long");
    FrameList l;
    l.lone = true;
    l.in = d_in;
    l.in_len = in_len;
    l.out = d_out;
    l.out_lens = d_out_len;
    l.h_in_lens = &in_len;
    l.total = n64;
    l.chunk_offsets = d_chunk_offsets;
    return frame_compress_list(ctx, l);
}

int snapmi_frame_compress_chunks(snapmi_ctx *ctx, const void *d_in,
                                 const uint32_t *h_chunk_lens, size_t n,
                                 uint32_t flags, void *d_out, uint64_t out_cap,
                                 uint64_t *d_out_len,
                                 uint64_t *d_chunk_offsets)
{
    if (!ctx || !d_out_len || (n && (!d_in || !d_out || !h_chunk_lens)) ||
        n > 0x7FFFFFFFu || (flags & ~(uint32_t)SNAPMI_FRAME_NO_IDENT))
        return SNAPMI_E_ARGUMENT;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    if (n == 0) {
        HIP_TRY(ctx, hipMemsetAsync(d_out_len, 0, sizeof(uint64_t), s));
        return SNAPMI_OK;
    }
    // input offsets of the chunks: chunk i = d_in[off[i], off[i+1])
    std::vector<uint64_t> off(n + 1);
    off[0] = 0;
    for (size_t i = 0; i < n; i++) {
        if (h_chunk_lens[i] == 0 || h_chunk_lens[i] > kMaxBlock)
            return fail_ctx(ctx, SNAPMI_E_ARGUMENT,
                            "frame_compress_chunks: chunk %zu has %u bytes "
                            "(1..65536)", i, h_chunk_lens[i]);
        off[i + 1] = off[i] + h_chunk_lens[i];
    }
    const bool ident = !(flags & SNAPMI_FRAME_NO_IDENT);
    const uint64_t need = (ident ? 10 : 0) + off[n] + 8 * (uint64_t)n;
    if (out_cap < need)
        return fail_ctx(ctx, SNAPMI_E_ARGUMENT,
                        "frame_compress_chunks: out_cap %llu < %llu",
                        (unsigned long long)out_cap, (unsigned long long)need);
    int rc = reserve(ctx, ctx->fr_chunk_off, (n + 1) * sizeof(uint64_t));
    if (rc)
        return rc;
    HIP_TRY(ctx, hipMemcpyAsync(ctx->fr_chunk_off.p, off.data(),
                                (n + 1) * sizeof(uint64_t),
                                hipMemcpyHostToDevice, s));
    HIP_TRY(ctx, hipStreamSynchronize(s)); // `off` is pageable host memory
    FrameList l;
    l.lone = true;
    l.in = d_in;
    l.in_len = off[n];
    l.out = d_out;
    l.out_lens = d_out_len;
    l.total = n;
    l.chunk_in_off = (const uint64_t *)ctx->fr_chunk_off.p;
    l.h_chunk_lens = h_chunk_lens;
    l.ident = ident;
    l.chunk_offsets = d_chunk_offsets;
    return frame_compress_list(ctx, l);
}

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

// Device memory -> pinned (device-mapped) host memory by a kernel: 16-byte
// stores over the host link.  On this platform a hipMemcpyAsync to the host
// and one from the host, on two streams of one process, ran one after the
// other (SNAPMI_PIPE_TRACE: a 0.55 GB copy in took 26 ms behind a 1 GiB copy
// out) although the link is full duplex (tests/hw/pcie_duplex.py: 2 x 48
// GB/s); a copy kernel beside a copy-engine transfer the other way does
// overlap.  The destination is brought to a 16-byte boundary first.
__global__ __launch_bounds__(256) void k_to_host(uint8_t *host,
                                                 const uint8_t *dev,
                                                 uint64_t n)
{
    gptr to = (gptr)host;
    gcptr from = (gcptr)dev;
    const uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t nthr = (uint64_t)gridDim.x * blockDim.x;
    uint64_t head = (16 - ((uintptr_t)host & 15)) & 15;
    if (head > n)
        head = n;
    if (tid < head)
        to[tid] = from[tid];
    const uint64_t body = (n - head) & ~15ull;
    typedef __attribute__((address_space(1))) u32x4 g_u32x4;
    for (uint64_t i = 16 * tid; i < body; i += 16 * nthr)
        *(g_u32x4 *)(to + head + i) = ld128g(from + head + i);
    const uint64_t tail = n - head - body;
    if (tid < tail)
        to[head + body + tid] = from[head + body + tid];
}

// is [p, p + n) host memory a kernel may write (pinned and mapped)?
static bool device_visible_at(const void *p)
{
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, p) != hipSuccess) {
        (void)hipGetLastError(); // plain malloc memory: not an error here
        return false;
    }
    // (the copy kernel stores through the HOST address: memory that is
    // mapped at another device address - hipHostRegister without unified
    // addressing - goes home by hipMemcpyAsync instead)
    return at.type == hipMemoryTypeHost && at.devicePointer == p;
}
// k_to_host may store to [p, p + n): both ends pinned and mapped at their
// host address (a buffer that starts in a pinned region and leaves it - a
// caller's offset into a smaller registration - must not reach the kernel)
static bool device_visible(const void *p, size_t n)
{
    if (!p || !n)
        return false;
    return device_visible_at(p) &&
           device_visible_at((const uint8_t *)p + (n - 1));
}

static int copy_home(snapmi_ctx *ctx, hipStream_t st, uint8_t *h_dst,
                     const void *d_src, uint64_t n, bool by_kernel)
{
    if (by_kernel) {
        // enough workgroups to keep the link busy, few enough to leave the
        // codec its CUs
        hipLaunchKernelGGL(k_to_host, dim3(128), dim3(256), 0, st, h_dst,
                           (const uint8_t *)d_src, n);
        HIP_TRY(ctx, hipGetLastError());
        return SNAPMI_OK;
    }
    HIP_TRY(ctx, hipMemcpyAsync(h_dst, d_src, n, hipMemcpyDeviceToHost, st));
    return SNAPMI_OK;
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

// snapmi_frame_scan_host, stopping in front of data chunk number `max_data`
// (status 3: the caller's output buffer is full)
static int frame_scan(const void *h_in, uint64_t in_len, uint32_t flags,
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

int snapmi_frame_scan_host(const void *h_in, uint64_t in_len, uint32_t flags,
                           uint8_t *stale10, uint64_t *h_offsets,
                           uint64_t cap, uint64_t *n_chunks,
                           uint64_t *consumed)
{
    return frame_scan(h_in, in_len, flags, stale10, h_offsets, cap,
                      ~0ull, n_chunks, consumed);
}

// The per-stream scratch of a decode of n streams, and `extra` bytes behind
// it that are the caller's (*rest).
static int fbd_streams(snapmi_ctx *ctx, FrameBatchDecodeArgs &a, size_t n,
                       size_t extra, uint8_t **rest)
{
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    int rc = ensure_tables(ctx);
    if (rc)
        return rc;
    // per-stream scratch and per-chunk scratch in two buffers: the second is
    // sized after the walk, and growing it must not drop the first
    if ((rc = reserve(ctx, ctx->fb_streams,
                      n * (8 + 8 + sizeof(snapmi_error) + 4 + 4) + 8 +
                          16 * 8 + extra)))
        return rc;
    uint8_t *p = (uint8_t *)ctx->fb_streams.p;
    a.n = (uint32_t)n;
    a.total = 0;
    a.counts = carve<uint64_t>(p, n);
    a.first = carve<uint64_t>(p, n + 1);
    a.serr = carve<snapmi_error>(p, n);
    a.sidx = carve<uint32_t>(p, n);
    a.first_bad = carve<uint32_t>(p, n);
    if (rest)
        *rest = p;
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
    return fbd_streams(ctx, a, n, 0, nullptr);
}

// The per-chunk scratch of a decode, for a list of `total` data chunks.
static int fbd_table(snapmi_ctx *ctx, const char *what,
                     FrameBatchDecodeArgs &a, uint64_t total)
{
    if (total > 0x7FFFFFFFu)
        return fail_ctx(ctx, SNAPMI_E_ARGUMENT,
                        "%s: %llu chunks (at most 2^31 - 1)", what,
                        (unsigned long long)total);
    const size_t t = (size_t)total;
    int rc;
    if ((rc = reserve(ctx, ctx->fb_chunks,
                      t * (sizeof(FrameChunk) + 4 + 8 + 8 +
                           2 * sizeof(snapmi_error) + 8 + 8 + 8 + 8 + 8 + 1 +
                           4) + 8 + 16 * 16)))
        return rc;
    uint8_t *p = (uint8_t *)ctx->fb_chunks.p;
    a.total = (uint32_t)total;
    a.chunks = carve<FrameChunk>(p, t);
    a.c_stream = carve<uint32_t>(p, t);
    a.dlens = carve<uint64_t>(p, t);
    a.offs = carve<uint64_t>(p, t + 1);
    a.cerrs = carve<snapmi_error>(p, t);
    a.derrs = carve<snapmi_error>(p, t);
    a.c_in = carve<const void *>(p, t);
    a.c_in_len = carve<uint64_t>(p, t);
    a.c_out = carve<void *>(p, t);
    a.c_caps = carve<uint64_t>(p, t);
    a.c_out_lens = carve<uint64_t>(p, t);
    a.modes = carve<uint8_t>(p, t);
    a.crcs = carve<uint32_t>(p, t);
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
    hipLaunchKernelGGL(k_scan_u64, dim3(1), dim3(1024), 0, s, a.dlens, a.offs,
                       a.total);
    if (a.out_ptrs && a.total) {
        hipLaunchKernelGGL(k_fbd_desc, dim3(gc), dim3(tb), 0, s, a);
        int rc = launch_decompress(ctx, a.c_in, a.c_in_len, a.c_out, a.c_caps,
                                   a.c_out_lens, a.derrs, a.modes, a.total);
        if (rc)
            return rc;
        // CRC of what was produced (chunks that were skipped have c_out_lens
        // 0: their CRC is never compared)
        hipLaunchKernelGGL(k_crc32c, dim3(a.total), dim3(64), 0, s,
                           (const void *const *)a.c_out, a.c_out_lens, a.crcs,
                           a.total, (const CrcTables *)ctx->fr_tables.p);
    }
    if (a.total)
        hipLaunchKernelGGL(k_fbd_verify_chunks, dim3(gc), dim3(tb), 0, s, a);
    hipLaunchKernelGGL(k_fbd_verify_streams,
                       dim3((uint32_t)((n + tb - 1) / tb)), dim3(tb), 0, s, a);
    HIP_TRY(ctx, hipGetLastError());
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
    uint8_t *p;
    const size_t front_bytes = 4 * 8 + 16 + 16 * 16 +
                               (size_t)(nseg + 2) * (kFwCands * 24 + 4 + 8 + 4);
    a.in = (const uint8_t *)d_in;
    a.in_len = in_len;
    a.out = (uint8_t *)d_out;
    a.out_cap = out_cap;
    a.flags = flags;
    a.chained = 0;
    for (int k = 0; k < 10; k++)
        a.stale[k] = stale10 ? stale10[k] : 0;
    int rc = fbd_streams(ctx, b, 1, front_bytes, &p);
    if (rc || (!nowait && (rc = mailbox(ctx))))
        return rc;
    hipStream_t s = ctx->stream;
    a.in_ptrs = carve<const void *>(p, 1);
    a.in_lens = carve<uint64_t>(p, 1);
    a.out_ptrs = carve<void *>(p, 1);
    a.out_caps = carve<uint64_t>(p, 1);
    a.meta = carve<uint32_t>(p, 4);
    a.nseg = nseg;
    a.fw_seg = fw_seg;
    a.fw_cand = carve<unsigned long long>(p, (size_t)nseg * kFwCands * 3);
    a.fw_entry = carve<unsigned long long>(p, (size_t)nseg + 1);
    a.fw_ncand = carve<uint32_t>(p, nseg);
    a.fw_base = carve<uint32_t>(p, (size_t)nseg + 1);
    a.counts = b.counts;
    a.first = b.first;
    a.serr = b.serr;
    a.sidx = b.sidx;
    a.first_bad = b.first_bad;
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
        uint32_t first_front = kFrontWalk;
        if (use_index) {
            first_front = kFrontIndex;
            hipLaunchKernelGGL(k_frame_meta_init, dim3(1), dim3(1), 0, s, a);
            hipLaunchKernelGGL(k_frame_index, dim3(gb), dim3(tb), 0, s, a);
        } else if (parallel_walk) {
            first_front = kFrontParallel;
            HIP_TRY(ctx, hipMemsetAsync(a.fw_ncand, 0, a.nseg * 4, s));
            hipLaunchKernelGGL(k_fw_candidates,
                               dim3((kFwScan + 255) / 256, a.nseg), dim3(256),
                               0, s, a);
            hipLaunchKernelGGL(k_fw_resolve, dim3(1), dim3(1), 0, s, a);
            hipLaunchKernelGGL(k_fw_emit, dim3((a.nseg + 63) / 64), dim3(64),
                               0, s, a);
        }
        a.chained = first_front != kFrontWalk;
        hipLaunchKernelGGL(k_frame_walk, dim3(1), dim3(64), 0, s, a);
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

        const uint32_t tb = 256;
        const uint32_t gb = n ? (uint32_t)((n + tb - 1) / tb) : 1;
        if (use_index) {
            hipLaunchKernelGGL(k_frame_meta_init, dim3(1), dim3(1), 0, s, a);
            hipLaunchKernelGGL(k_frame_index, dim3(gb), dim3(tb), 0, s, a);
        } else if (parallel_walk) {
            HIP_TRY(ctx, hipMemsetAsync(a.fw_ncand, 0, a.nseg * 4, s));
            hipLaunchKernelGGL(k_fw_candidates,
                               dim3((kFwScan + 255) / 256, a.nseg), dim3(256),
                               0, s, a);
            hipLaunchKernelGGL(k_fw_resolve, dim3(1), dim3(1), 0, s, a);
            hipLaunchKernelGGL(k_fw_emit, dim3((a.nseg + 63) / 64), dim3(64),
                               0, s, a);
        } else {
            hipLaunchKernelGGL(k_frame_walk, dim3(1), dim3(64), 0, s, a);
        }
        // the number of data chunks decides the launch sizes below
        uint32_t meta[3];
        hipLaunchKernelGGL(k_post_words, dim3(1), dim3(64), 0, s,
                           (uint32_t *)ctx->h_mail, a.meta, 3u);
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

int snapmi_frame_compress_batch(snapmi_ctx *ctx, const void *const *d_in_ptrs,
                                const uint64_t *d_in_lens,
                                const uint64_t *h_in_lens,
                                void *const *d_out_ptrs,
                                const uint64_t *d_out_caps,
                                uint64_t *d_out_lens, snapmi_error *d_errs,
                                size_t n)
{
    if (!ctx)
        return SNAPMI_E_ARGUMENT;
    if (n == 0)
        return SNAPMI_OK;
    if (!d_in_ptrs || !d_in_lens || !d_out_ptrs || !d_out_lens)
        return fail_ctx(ctx, SNAPMI_E_ARGUMENT,
                        "frame_compress_batch: bad args");
    if (n > 0x7FFFFFFFu)
        return fail_ctx(ctx, SNAPMI_E_ARGUMENT,
                        "frame_compress_batch: %zu streams (at most 2^31 - 1)",
                        n);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    std::vector<uint64_t> fetched;
    if (!h_in_lens) {
        fetched.resize(n);
        HIP_TRY(ctx, hipMemcpyAsync(fetched.data(), d_in_lens,
                                    n * sizeof(uint64_t),
                                    hipMemcpyDeviceToHost, s));
        HIP_TRY(ctx, hipStreamSynchronize(s));
        h_in_lens = fetched.data();
    }
    uint64_t total = 0;
    for (size_t i = 0; i < n; i++)
        total += (h_in_lens[i] + kMaxBlock - 1) / kMaxBlock;
    if (total > 0x7FFFFFFFu)
        return fail_ctx(ctx, SNAPMI_E_ARGUMENT,
                        "frame_compress_batch: %llu chunks (at most 2^31 - 1)",
                        (unsigned long long)total);
    FrameList l;
    l.in_ptrs = d_in_ptrs;
    l.in_lens = d_in_lens;
    l.out_ptrs = d_out_ptrs;
    l.out_caps = d_out_caps;
    l.out_lens = d_out_lens;
    l.errs = d_errs;
    l.n = n;
    l.h_in_lens = h_in_lens;
    l.total = total;
    return frame_compress_list(ctx, l);
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
    hipLaunchKernelGGL(k_scan_u64, dim3(1), dim3(1024), 0, s, a.counts,
                       a.first, (uint32_t)n);
    // the one wait: the number of data chunks sizes everything below
    hipLaunchKernelGGL(k_post_words, dim3(1), dim3(64), 0, s,
                       (uint32_t *)ctx->h_mail, (const uint32_t *)(a.first + n),
                       2u);
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

extern "C" {

// ----------------------------------------------------------------------
// Host-buffer forms (H2D + kernels + D2H, blocking): what a host-language
// FrameEncoder / FrameDecoder (the Rust shim, the Python mirror, tools/szip)
// calls per batch of chunks.
// ----------------------------------------------------------------------
size_t snapmi_frame_encode_bound(size_t total_bytes, size_t n_chunks)
{
    return 10 + total_bytes + 8 * n_chunks;
}

} // extern "C"

// ---- the pipeline behind the two host-buffer calls -----------------------
// The staging pipeline of the host-buffer calls: snapmi_hostpipe.hpp.
namespace snapmi {
void host_pipe_destroy(snapmi_ctx *ctx)
{
    snapmi_host_pipe *p = ctx->pipe;
    if (!p)
        return;
    if (p->s_in) {
        (void)hipStreamSynchronize(p->s_in);
        (void)hipStreamDestroy(p->s_in);
    }
    if (p->s_out) {
        (void)hipStreamSynchronize(p->s_out);
        (void)hipStreamDestroy(p->s_out);
    }
    for (PipeSlot &sl : p->slot) {
        for (DevBuf *b : {&sl.in, &sl.out, &sl.desc, &sl.home})
            if (b->p)
                (void)hipFree(b->p);
        for (PinBuf *b : {&sl.hb_in, &sl.hb_home})
            if (b->p)
                (void)hipHostFree(b->p);
        for (hipEvent_t e : {sl.ev_h2d, sl.ev_k, sl.ev_d2h})
            if (e)
                (void)hipEventDestroy(e);
        if (sl.h_res)
            (void)hipHostFree(sl.h_res);
        if (sl.h_off)
            (void)hipHostFree(sl.h_off);
    }
    delete p;
    ctx->pipe = nullptr;
}
} // namespace snapmi

int snapmi::host_pipe(snapmi_ctx *ctx, snapmi_host_pipe **out)
{
    if (!ctx->pipe) {
        snapmi_host_pipe *p = new snapmi_host_pipe;
        ctx->pipe = p; // (freed with the context whatever fails below)
        HIP_TRY(ctx, hipStreamCreateWithFlags(&p->s_in, hipStreamNonBlocking));
        HIP_TRY(ctx, hipStreamCreateWithFlags(&p->s_out, hipStreamNonBlocking));
        for (PipeSlot &sl : p->slot) {
            HIP_TRY(ctx, hipEventCreate(&sl.ev_h2d));
            HIP_TRY(ctx, hipEventCreate(&sl.ev_k));
            HIP_TRY(ctx, hipEventCreate(&sl.ev_d2h));
            HIP_TRY(ctx, hipHostMalloc((void **)&sl.h_res, sizeof *sl.h_res,
                                       hipHostMallocDefault));
        }
    }
    *out = ctx->pipe;
    return SNAPMI_OK;
}

static int slot_offsets(snapmi_ctx *ctx, PipeSlot &sl, size_t n)
{
    if (n <= sl.h_off_cap)
        return SNAPMI_OK;
    if (sl.h_off)
        HIP_TRY(ctx, hipHostFree(sl.h_off));
    sl.h_off = nullptr;
    sl.h_off_cap = 0;
    const size_t want = n + n / 4 + 64;
    HIP_TRY(ctx, hipHostMalloc((void **)&sl.h_off, want * sizeof(uint64_t),
                               hipHostMallocDefault));
    sl.h_off_cap = want;
    return SNAPMI_OK;
}

// a slot's device buffer grows only when nothing of the slot is in flight
int snapmi::slot_reserve(snapmi_ctx *ctx, snapmi::DevBuf &b, size_t bytes)
{
    if (bytes <= b.cap)
        return SNAPMI_OK;
    if (b.p) {
        HIP_TRY(ctx, hipDeviceSynchronize());
        HIP_TRY(ctx, hipFree(b.p));
        b.p = nullptr;
        b.cap = 0;
    }
    const size_t want = bytes + bytes / 8 + 256;
    HIP_TRY(ctx, hipMalloc(&b.p, want));
    b.cap = want;
#ifdef SNAPMI_TESTING
    return fill_new_dev(ctx, b);
#else
    return SNAPMI_OK;
#endif
}

int snapmi::pipe_copy_home(snapmi_ctx *ctx, hipStream_t st, uint8_t *h_dst,
                           const void *d_src, uint64_t n, bool by_kernel)
{
    return copy_home(ctx, st, h_dst, d_src, n, by_kernel);
}

int snapmi::launch_scan_u64(snapmi_ctx *ctx, hipStream_t st,
                            const uint64_t *in, uint64_t *out, uint32_t n)
{
    hipLaunchKernelGGL(k_scan_u64, dim3(1), dim3(1024), 0, st, in, out, n);
    HIP_TRY(ctx, hipGetLastError());
    return SNAPMI_OK;
}

extern "C" {

int snapmi_frame_encode_host(snapmi_ctx *ctx, const uint8_t *h_in,
                             const uint32_t *h_chunk_lens, size_t n,
                             uint32_t flags, uint8_t *h_out, size_t out_cap,
                             size_t *written)
{
    if (!ctx || !written || (n && (!h_in || !h_chunk_lens || !h_out)) ||
        n > 0x7FFFFFFFu || (flags & ~(uint32_t)SNAPMI_FRAME_NO_IDENT))
        return SNAPMI_E_ARGUMENT;
    *written = 0;
    if (n == 0)
        return SNAPMI_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    uint64_t total = 0;
    for (size_t i = 0; i < n; i++) {
        if (h_chunk_lens[i] == 0 || h_chunk_lens[i] > kMaxBlock)
            return fail_ctx(ctx, SNAPMI_E_ARGUMENT,
                            "frame_encode_host: chunk %zu has %u bytes "
                            "(1..65536)", i, h_chunk_lens[i]);
        total += h_chunk_lens[i];
    }
    const size_t need = snapmi_frame_encode_bound(total, n);
    if (out_cap < need - ((flags & SNAPMI_FRAME_NO_IDENT) ? 10 : 0))
        return fail_ctx(ctx, SNAPMI_E_ARGUMENT,
                        "frame_encode_host: out_cap %zu < %zu", out_cap, need);
    snapmi_host_pipe *P;
    int rc = host_pipe(ctx, &P);
    if (rc)
        return rc;
    hipStream_t sK = ctx->stream;
    PipeDrain drain{ctx, P};
    // Slices: the match finder wants large launches (its latency floor is
    // ~35 ms whatever the size: DESIGN 4.1), the pipeline wants several
    // slices; by default a batch of 1 GiB or more is cut in two to three.
    const uint64_t slice_bytes = ctx->host_encode_slice;
    struct Slice {
        size_t c0, c1;      // chunks [c0, c1)
        uint64_t b0, bytes; // input bytes
    };
    std::vector<Slice> sl;
    {
        const uint64_t k = total <= slice_bytes
                               ? 1
                               : (total + slice_bytes - 1) / slice_bytes;
        const uint64_t per = (total + k - 1) / k;
        size_t c = 0;
        uint64_t b = 0;
        while (c < n) {
            Slice x{c, c, b, 0};
            while (x.c1 < n && (x.bytes < per || x.c1 == x.c0)) {
                x.bytes += h_chunk_lens[x.c1];
                x.c1++;
            }
            c = x.c1;
            b += x.bytes;
            sl.push_back(x);
        }
    }
    const size_t ns = sl.size();
    uint64_t out_off = 0;
    const bool out_by_kernel =
        (ctx->host_copy_kernel & 2) && device_visible(h_out, out_cap);
    // step t: copy slice t in, start the kernels of slice t-1, send the
    // result of slice t-2 home
    for (size_t t = 0; t < ns + 2; t++) {
        if (t < ns) {
            PipeSlot &s = P->slot[t % kSlots];
            const Slice &x = sl[t];
            const size_t cn = x.c1 - x.c0;
            if ((rc = slot_reserve(ctx, s.in, x.bytes + 16)) ||
                (rc = slot_reserve(ctx, s.out,
                                   snapmi_frame_encode_bound(x.bytes, cn) +
                                       64)) ||
                (rc = slot_reserve(ctx, s.desc, 64 + (cn + 1) * 8)) ||
                (rc = slot_offsets(ctx, s, cn + 1)))
                return rc;
            HIP_TRY(ctx, hipMemcpyAsync(s.in.p, h_in + x.b0, x.bytes,
                                        hipMemcpyHostToDevice, P->s_in));
            HIP_TRY(ctx, hipEventRecord(s.ev_h2d, P->s_in));
        }
        if (t >= 1 && t - 1 < ns) {
            PipeSlot &s = P->slot[(t - 1) % kSlots];
            const Slice &x = sl[t - 1];
            const size_t cn = x.c1 - x.c0;
            s.h_off[0] = 0;
            for (size_t i = 0; i < cn; i++)
                s.h_off[i + 1] = s.h_off[i] + h_chunk_lens[x.c0 + i];
            uint64_t *d_len = (uint64_t *)s.desc.p;
            HIP_TRY(ctx, hipStreamWaitEvent(sK, s.ev_h2d, 0));
            if (t - 1 >= kSlots) // the slot's last result has left
                HIP_TRY(ctx, hipStreamWaitEvent(sK, s.ev_d2h, 0));
            const bool ident =
                t - 1 == 0 && !(flags & SNAPMI_FRAME_NO_IDENT);
            // (the chunk offsets are read where they lie, in pinned host
            // memory: a copy would wait behind the bulk copy of the next
            // slice; so would one of the result)
            FrameList l;
            l.lone = true;
            l.in = s.in.p;
            l.in_len = x.bytes;
            l.out = s.out.p;
            l.out_lens = d_len;
            l.total = cn;
            l.chunk_in_off = s.h_off;
            l.h_chunk_lens = h_chunk_lens + x.c0;
            l.ident = ident;
            rc = frame_compress_list(ctx, l);
            if (rc)
                return rc;
            hipLaunchKernelGGL(k_post_words, dim3(1), dim3(64), 0, sK,
                               (uint32_t *)&s.h_res->len,
                               (const uint32_t *)d_len, 2u);
            HIP_TRY(ctx, hipEventRecord(s.ev_k, sK));
        }
        if (t >= 2) {
            PipeSlot &s = P->slot[(t - 2) % kSlots];
            HIP_TRY(ctx, hipEventSynchronize(s.ev_k));
            const uint64_t flen = s.h_res->len;
            if (out_off + flen > out_cap)
                return fail_ctx(ctx, SNAPMI_E_DEVICE,
                                "frame_encode_host: %llu > cap",
                                (unsigned long long)(out_off + flen));
            if ((rc = copy_home(ctx, P->s_out, h_out + out_off, s.out.p,
                                flen, out_by_kernel)))
                return rc;
            HIP_TRY(ctx, hipEventRecord(s.ev_d2h, P->s_out));
            out_off += flen;
        }
    }
    HIP_TRY(ctx, hipStreamSynchronize(P->s_out));
    drain.armed = false; // (every copy in and every kernel lies in front)
    *written = (size_t)out_off;
    return SNAPMI_OK;
}

int snapmi_frame_decode_host(snapmi_ctx *ctx, const uint8_t *h_in,
                             size_t in_len, uint32_t flags, uint8_t *stale10,
                             uint8_t *h_out, size_t out_cap, size_t *written,
                             size_t *consumed, snapmi_error *err)
{
    if (!ctx || !written || !consumed || (in_len && !h_in) ||
        (out_cap && !h_out) ||
        (flags & ~(uint32_t)(SNAPMI_FRAME_CONTINUATION | SNAPMI_FRAME_FINAL)))
        return SNAPMI_E_ARGUMENT;
    *written = 0;
    *consumed = 0;
    if (err)
        memset(err, 0, sizeof *err);
    if (in_len == 0)
        return SNAPMI_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    snapmi_host_pipe *P;
    int rc = host_pipe(ctx, &P);
    if (rc)
        return rc;
    hipStream_t sK = ctx->stream;
    PipeDrain drain{ctx, P};
    const bool final = (flags & SNAPMI_FRAME_FINAL) != 0;
    uint32_t cflag = flags & SNAPMI_FRAME_CONTINUATION;
    uint8_t stale[10] = {0}; // the reader's src[0..10) in front of `pos`
    if (stale10)
        memcpy(stale, stale10, 10);
    const uint64_t slice_chunks = ctx->host_decode_slice_chunks;
    const bool out_by_kernel =
        (ctx->host_copy_kernel & 1) && device_visible(h_out, out_cap);

    static const bool trace = getenv("SNAPMI_PIPE_TRACE") != nullptr;
    static hipEvent_t ev_base = nullptr;
    if (trace) {
        if (!ev_base)
            (void)hipEventCreate(&ev_base);
        (void)hipEventRecord(ev_base, sK);
    }
    const auto t_start = std::chrono::steady_clock::now();
    auto now_us = [&] {
        return (long)std::chrono::duration_cast<std::chrono::microseconds>(
                   std::chrono::steady_clock::now() - t_start)
            .count();
    };
    // what a slice in flight is
    struct Flight {
        bool live = false, clean = false;
        uint64_t used = 0;
    } fl[kSlots];
    uint64_t pos = 0;      // input consumed by the slices issued so far
    uint64_t wrote = 0;    // output bytes of the slices retired so far
    uint64_t budget = out_cap / kMaxBlock; // chunks the output still holds
    bool more = true;      // another slice may follow
    int result = SNAPMI_OK;
    snapmi_error first_err;
    memset(&first_err, 0, sizeof first_err);
    bool disagree = false;

    // the result of the slice in slot k goes home
    auto retire = [&](int k) -> int {
        PipeSlot &s = P->slot[k];
        Flight &f = fl[k];
        if (!f.live)
            return SNAPMI_OK;
        f.live = false;
        HIP_TRY(ctx, hipEventSynchronize(s.ev_k));
        if (trace) {
            float a = 0, b = 0;
            (void)hipEventElapsedTime(&a, ev_base, s.ev_h2d);
            (void)hipEventElapsedTime(&b, ev_base, s.ev_k);
            fprintf(stderr, "[pipe] slot %d: h2d done %.1f ms, kernels done "
                            "%.1f ms (device clock)\n", k, a, b);
        }
        const uint64_t len = s.h_res->len;
        if (wrote + len > out_cap)
            return fail_ctx(ctx, SNAPMI_E_DEVICE,
                            "frame_decode_host: %llu > cap",
                            (unsigned long long)(wrote + len));
        if (result == SNAPMI_OK && !disagree) {
            // (nothing behind a failed slice is delivered)
            if (len) {
                if (int e = copy_home(ctx, P->s_out, h_out + wrote, s.out.p,
                                      len, out_by_kernel))
                    return e;
                HIP_TRY(ctx, hipEventRecord(s.ev_d2h, P->s_out));
            }
            wrote += len;
            if (s.h_res->e.kind != SNAPMI_OK) {
                result = s.h_res->e.kind;
                first_err = s.h_res->e;
            } else if (!f.clean) {
                disagree = true; // the host scan saw a bad or cut-off chunk
            }
        }
        return SNAPMI_OK;
    };

    // step t: slice t is issued (copy in on one stream, kernels behind it on
    // the context's); then slice t-1 is retired - its kernels lie in front of
    // slice t's on the same stream and snapmi_frame_decompress_ex waits for
    // its own header pass, so they are done - and its output goes home on the
    // third stream while slice t decodes
    for (uint64_t t = 0;; t++) {
        const int k = (int)(t % kSlots);
        // the slot's previous slice (t - 3) is retired by now (see below)
        if (more && result == SNAPMI_OK && !disagree) {
            PipeSlot &s = P->slot[k];
            const uint64_t maxc = budget < slice_chunks ? budget : slice_chunks;
            uint8_t stale_in[10], stale_work[10];
            memcpy(stale_in, stale, 10);
            memcpy(stale_work, stale, 10);
            uint64_t nd = 0, used = 0;
            const uint8_t *in = h_in + pos;
            const uint64_t left = in_len - pos;
            // the scan stops at the first cut-off (2) or rejected (1) chunk,
            // or in front of the first data chunk beyond the slice (3)
            int status = frame_scan(in, left, cflag, nullptr, nullptr, 0, maxc,
                                    &nd, &used);
            if (status > 3)
                return status;
            if ((rc = slot_offsets(ctx, s, nd + 1)))
                return rc;
            status = frame_scan(in, left, cflag, stale_work, s.h_off, nd + 1,
                                maxc, &nd, &used);
            if (status > 3)
                return status;
            if (status == 3 && used == 0 && budget == 0) {
                if (pos == 0 && out_cap < kMaxBlock)
                    return fail_ctx(ctx, SNAPMI_E_ARGUMENT,
                                    "frame_decode_host: out_cap below 65536");
                more = false; // the output buffer is full: call again
            } else if (used == 0 && status == 2 && !final) {
                more = false; // not one whole chunk here: supply more input
            } else if (left == 0) {
                more = false;
            } else {
                const bool clean =
                    status == 3 || status == 0 || (status == 2 && !final);
                const uint64_t dec_len = clean ? used : left;
                if ((rc = slot_reserve(ctx, s.in, dec_len + 16)) ||
                    (rc = slot_reserve(ctx, s.out, nd * kMaxBlock + 64)) ||
                    (rc = slot_reserve(ctx, s.desc, 128 + (nd + 1) * 8)))
                    return rc;
                if (trace)
                    fprintf(stderr, "[pipe] t=%lu scanned %ld us\n",
                            (unsigned long)t, now_us());
                HIP_TRY(ctx, hipMemcpyAsync(s.in.p, in, dec_len,
                                            hipMemcpyHostToDevice, P->s_in));
                HIP_TRY(ctx, hipEventRecord(s.ev_h2d, P->s_in));
                if (trace)
                    fprintf(stderr, "[pipe] t=%lu h2d issued %ld us (%llu B)\n",
                            (unsigned long)t, now_us(),
                            (unsigned long long)dec_len);
                uint64_t *d_len = (uint64_t *)s.desc.p;
                snapmi_error *d_err =
                    (snapmi_error *)((uint8_t *)s.desc.p + 64);
                HIP_TRY(ctx, hipStreamWaitEvent(sK, s.ev_h2d, 0));
                if (t >= kSlots) // the slot's last result has left
                    HIP_TRY(ctx, hipStreamWaitEvent(sK, s.ev_d2h, 0));
                const bool with_index = clean && nd > 0;
                // (the side index is read where it lies, in pinned host
                // memory, and the result is posted by a kernel: copies on
                // this stream would wait behind the bulk copies)
                rc = snapmi_frame_decompress_ex(
                    ctx, s.in.p, dec_len, s.out.p, nd * kMaxBlock, d_len,
                    d_err, with_index ? s.h_off : nullptr, nd, cflag,
                    stale_in);
                if (rc)
                    return rc;
                static_assert(sizeof(PipeSlot::Result) == 40, "len + error");
                hipLaunchKernelGGL(k_post_words, dim3(1), dim3(64), 0, sK,
                                   (uint32_t *)&s.h_res->len,
                                   (const uint32_t *)d_len, 2u);
                hipLaunchKernelGGL(k_post_words, dim3(1), dim3(64), 0, sK,
                                   (uint32_t *)&s.h_res->e,
                                   (const uint32_t *)d_err, 8u);
                HIP_TRY(ctx, hipEventRecord(s.ev_k, sK));
                if (trace)
                    fprintf(stderr, "[pipe] t=%lu kernels issued %ld us\n",
                            (unsigned long)t, now_us());
                fl[k].live = true;
                fl[k].clean = clean;
                fl[k].used = used;
                if (clean) {
                    pos += used;
                    budget -= nd;
                    cflag = SNAPMI_FRAME_CONTINUATION;
                    memcpy(stale, stale_work, 10);
                }
                // 3: the slice was full, the next one follows; anything else
                // ends the batch (all consumed / a cut-off tail / an error
                // the device is about to name)
                more = status == 3;
            }
        } else {
            more = false;
        }
        if (t >= 1 && (rc = retire((int)((t - 1) % kSlots))))
            return rc;
        if (trace)
            fprintf(stderr, "[pipe] t=%lu retired %ld us\n", (unsigned long)t,
                    now_us());
        if (!more)
            break;
    }
    for (int k = 0; k < kSlots; k++)
        if ((rc = retire(k)))
            return rc;
    HIP_TRY(ctx, hipStreamSynchronize(P->s_out));
    drain.armed = false; // all slices retired, their copies home are done
    if (trace) {
        for (int k = 0; k < kSlots; k++) {
            float a = 0;
            if (hipEventElapsedTime(&a, ev_base, P->slot[k].ev_d2h) ==
                hipSuccess)
                fprintf(stderr, "[pipe] slot %d: last d2h done %.1f ms\n", k,
                        a);
        }
        fprintf(stderr, "[pipe] done %ld us\n", now_us());
    }
    *written = (size_t)wrote;
    if (result != SNAPMI_OK) {
        if (err)
            *err = first_err;
        return result;
    }
    if (disagree)
        return fail_ctx(ctx, SNAPMI_E_DEVICE,
                        "frame_decode_host: host scan and device walk "
                        "disagree");
    *consumed = (size_t)pos;
    if (stale10)
        memcpy(stale10, stale, 10);
    return SNAPMI_OK;
}

} // extern "C"
