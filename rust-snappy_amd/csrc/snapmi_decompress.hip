// snapmi_decompress.hip -- Snappy raw stream decompressor for gfx950 (CDNA4):
// the pipeline of a batch, and the lane-per-stream kernels.
//
// Semantics (element order, every bounds check, which error wins and with
// which field values) follow the reference src/decompress.rs exactly; the
// element format is written once, in snapmi_element.hpp.  A raw stream has no
// block index (src/compress.rs:128-153), so the stream is the parallel unit;
// a batch supplies thousands of them, sorted longest first
// (k_plan_decompress*), and every size class has its kernel: one wavefront
// per stream (snapmi_wide.hip), or - k_decompress_tiny / _small, here - one
// LANE per stream of under 256 / 512 compressed bytes whose output is no
// larger.  (What cuts one long stream or an indexed one into pieces for these
// kernels decodes nothing: snapmi_longstream.hip, snapmi_index.hip.)
// DESIGN.md section 4.2 has the history and what bounds each of them.
#include "snapmi_device.hpp"
#include "snapmi_element.hpp"
#include "snapmi_kernels.hpp"
#include "snapmi_scan.hpp"

namespace snapmi {

// decompress_len, reference src/decompress.rs:30-35: one thread per stream.
__global__ __launch_bounds__(256) void k_decompress_len(DecompressArgs a)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n_streams)
        return;
    const uint64_t in_len = a.in_lens[i];
    a.out_lens[i] = 0;
    if (in_len == 0) {
        set_error(a.errs, i, SNAPMI_OK, 0, 0, 0);
        return;
    }
    uint32_t hdr;
    uint64_t dlen;
    if (read_header((gcptr)a.in_ptrs[i], in_len, &hdr, &dlen,
                    a.errs, i) != SNAPMI_OK)
        return;
    a.out_lens[i] = dlen;
    set_error(a.errs, i, SNAPMI_OK, 0, 0, 0);
}

// Streams of fewer than kTiny = 2^kTinyLog2 compressed bytes are decoded one
// per LANE (k_decompress_tiny below), streams of under kSmallDec bytes whose
// output is no larger on half the lanes of a wavefront (k_decompress_small,
// round 5); the sort puts both classes last, and the plan leaves the number
// of streams in front of them in bucket_pos[64] and [65].
constexpr uint32_t kTinyLog2 = 8;
constexpr uint32_t kSmallDecLog2 = 9;
constexpr uint32_t kSmallDec = 1u << kSmallDecLog2;
// sort classes, descending in the dispatch order: kFirstWide + floor(log2
// (compressed length)) - 8 for the wavefront decoder, kSmallClass, then
// floor(log2(length)) of the tiny ones
constexpr uint32_t kSmallClass = kTinyLog2;
constexpr uint32_t kFirstWide = kTinyLog2 + 1;

// The size class a stream is sorted by: floor(log2(compressed length)) -
// except that a raw stream of under kTiny bytes whose header promises MORE
// than kTiny bytes of output (a run of zeros: 200 bytes of copies are 4 KiB)
// (or a piece of a long stream with as much) is not the lane-per-stream
// kernel's: it keeps its output in LDS, kTiny bytes per lane; what does not
// fit would be left to one lane moving bytes through global memory.  Such a
// stream, and any of 256 .. 511 compressed bytes, whose output is at most
// kSmallDec bytes is k_decompress_small's; the rest goes with the first class
// of the wavefront decoder.
__device__ __forceinline__ uint32_t plan_class(const DecompressArgs &a,
                                               uint32_t i)
{
    const uint64_t len = a.in_lens[i];
    if (a.modes && a.modes[i] == 3) // not this launch's: behind everything
        return 0;
    const uint32_t bk = len ? 63 - (uint32_t)__builtin_clzll(len) : 0;
    if (len == 0 || bk > kSmallDecLog2 - 1)
        return len ? (bk < 62 ? bk + 1 : 63) : 0;
    const uint32_t mode = a.modes ? a.modes[i] : 0;
    uint64_t dl = 0;
    bool header = true;
    if (mode == 2) // a piece of a long stream: its output is out_caps
        dl = a.out_caps[i];
    else if (mode == 0 && read_varint((gcptr)a.in_ptrs[i], len, &dl) == 0)
        header = false; // the lane-per-stream kernel reports it
    if (bk < kTinyLog2 && (!header || dl <= (1u << kTinyLog2)))
        return bk;
    if (mode == 0 && header && dl <= kSmallDec)
        return kSmallClass;
    return kFirstWide;
}

// ---------------------------------------------------------------------
// Plan: dispatch order.  Streams differ in size by orders of magnitude and a
// stream is decoded by one wavefront, so the longest streams must start
// first or they become the tail of the launch.  One workgroup sorts the
// stream indices by floor(log2(compressed length)), largest bucket first
// (counting sort: histogram, bucket offsets, scatter).
// ---------------------------------------------------------------------
// Bucket counts -> bucket offsets, in place (one thread), with the two marks
// the decoders read: bucket_pos[64] and [65].
__device__ __forceinline__ void plan_offsets(const DecompressArgs &a,
                                             uint32_t *counts)
{
    uint32_t run = 0;
    for (uint32_t k = 0; k < 64; k++) {
        if (k == 64 - kFirstWide) // the wavefront decoder's streams
            a.bucket_pos[64] = run;
        if (k == 64 - kSmallClass) // ... and k_decompress_small's
            a.bucket_pos[65] = run;
        const uint32_t c = counts[k];
        counts[k] = run;
        run += c;
    }
}

__global__ __launch_bounds__(1024) void k_plan_decompress(DecompressArgs a)
{
    __shared__ uint32_t hist[64];
    if (a.gate && *a.gate != a.gate_value)
        return;
    if (threadIdx.x < 64)
        hist[threadIdx.x] = 0;
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < a.n_streams; i += blockDim.x) {
        const uint32_t bk = plan_class(a, i);
        atomicAdd(&hist[63 - bk], 1u); // reversed: big buckets first
    }
    __syncthreads();
    if (threadIdx.x == 0)
        plan_offsets(a, hist);
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < a.n_streams; i += blockDim.x) {
        const uint32_t bk = plan_class(a, i);
        a.order[atomicAdd(&hist[63 - bk], 1u)] = i;
    }
}

// The same sort on many workgroups (10.7 M streams: 19 ms of a 33 ms pass in
// the one-workgroup kernel): histogram, offsets, scatter.  bucket_pos[0, 64)
// = counts, then cursors.
__global__ __launch_bounds__(1024) void k_plan_decompress_a(DecompressArgs a)
{
    __shared__ uint32_t hist[64];
    if (a.gate && *a.gate != a.gate_value)
        return;
    if (threadIdx.x < 64)
        hist[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < a.n_streams) {
        const uint32_t bk = plan_class(a, i);
        atomicAdd(&hist[63 - bk], 1u); // reversed: big buckets first
    }
    __syncthreads();
    if (threadIdx.x < 64 && hist[threadIdx.x])
        atomicAdd(&a.bucket_pos[threadIdx.x], hist[threadIdx.x]);
}

__global__ __launch_bounds__(64) void k_plan_decompress_b(DecompressArgs a)
{
    if (a.gate && *a.gate != a.gate_value)
        return;
    if (threadIdx.x == 0)
        plan_offsets(a, a.bucket_pos);
}

__global__ __launch_bounds__(1024) void k_plan_decompress_c(DecompressArgs a)
{
    __shared__ uint32_t hist[64], base[64];
    if (a.gate && *a.gate != a.gate_value)
        return;
    if (threadIdx.x < 64)
        hist[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t bk = 0, mine = 0;
    if (i < a.n_streams) {
        bk = 63 - plan_class(a, i);
        mine = atomicAdd(&hist[bk], 1u); // my place among this workgroup's
    }
    __syncthreads();
    // one range per bucket and workgroup
    if (threadIdx.x < 64 && hist[threadIdx.x])
        base[threadIdx.x] = atomicAdd(&a.bucket_pos[threadIdx.x],
                                      hist[threadIdx.x]);
    __syncthreads();
    if (i < a.n_streams)
        a.order[base[bk] + mine] = i;
}

// Tiny streams, one per LANE: a wavefront per stream spends ten microseconds
// of dependent round trips (descriptors, header, first window, flush) on a
// stream of 150 bytes; here 64 streams share them.  Errors and their fields
// are the reference's, lane by lane.
namespace {
// A stream on global memory: lane_decode of snapmi_element.hpp.
__device__ __forceinline__ void decode_tiny(const DecompressArgs &a,
                                            const uint64_t st)
{
    const uint32_t mode = a.modes ? a.modes[st] : 0;
    uint64_t produced;
    if (lane_decode((gcptr)a.in_ptrs[st], a.in_lens[st], mode,
                    (gptr)a.out_ptrs[st], a.out_caps[st], &produced, a.errs,
                    st)) {
        if (mode != 3) // (another launch decodes that one)
            stream_done(a.errs, a.out_lens, st, SNAPMI_OK, 0, 0, 0, produced);
    } else {
        a.out_lens[st] = 0;
    }
}
} // namespace

// Tiny streams (fewer than kTiny compressed bytes), one per LANE.  A stream
// whose output is tiny as well (the usual case) is staged in LDS - input and
// output dword-interleaved across the lanes, so that lane l's byte k is at
// ((k >> 2) * kLanes + l) * 4 + (k & 3) and the lanes of an access fall on
// different banks - decoded there with the reference's loop, and stored with
// 16-byte accesses: four LDS latencies per byte moved instead of two HBM
// round trips.  The others run the same loop on global memory.
// k_decompress_small (round 5) is the same body with 512 bytes of input and of
// output per lane on 32 lanes of a wavefront, for the streams between the
// tiny ones and the wavefront decoder's (400-byte pages decoded at 106 GiB/s
// a wavefront each, between 290 and 170 for their neighbours).
template <uint32_t kLog2, uint32_t kLanes>
__device__ __forceinline__ void decompress_lane_streams(
    const DecompressArgs &a, const uint64_t first, const uint64_t end)
{
    constexpr uint32_t kT = 1u << kLog2;
    __shared__ __attribute__((aligned(16))) uint32_t tin[kT / 4 * kLanes];
    __shared__ __attribute__((aligned(16))) uint32_t tout[kT / 4 * kLanes];
    const uint32_t lane = threadIdx.x;
    if (first + (uint64_t)blockIdx.x * kLanes >= end)
        return;
    const uint64_t i = first + (uint64_t)blockIdx.x * kLanes + lane;
    if (lane >= kLanes || i >= end)
        return;
    const uint64_t st = a.order[i];
    gcptr in = (gcptr)a.in_ptrs[st];
    const uint32_t in_len = (uint32_t)a.in_lens[st]; // < kT
    const uint32_t mode = a.modes ? a.modes[st] : 0;
    // the header decides: a stream with a tiny output goes through LDS
    uint64_t dl = 0;
    uint32_t hdr = 0;
    bool small = mode == 0 && in_len > 0;
    if (small) {
        hdr = read_varint(in, in_len, &dl);
        small = hdr != 0 && dl <= kT && dl <= a.out_caps[st];
    }
    if (!small) {
        decode_tiny(a, st);
        return;
    }
    typedef __attribute__((address_space(3))) uint32_t l_u32t;
    l_u8 *const bin = (l_u8 *)(l_u32t *)tin;
    l_u8 *const bout = (l_u8 *)(l_u32t *)tout;
    auto at = [lane](uint32_t k) {
        return ((k >> 2) * kLanes + lane) * 4 + (k & 3);
    };
    // stage the elements: whole dwords (reads stay inside the stream: the
    // last partial dword bytewise)
    const uint32_t slen = in_len - hdr;
    gcptr src = in + hdr;
    {
        uint32_t k = 0;
        for (; k + 4 <= slen; k += 4)
            *(l_u32t *)(bin + at(k)) = ld32u(src + k);
        for (; k < slen; k++)
            bin[at(k)] = src[k];
    }
    const uint32_t dlen = (uint32_t)dl;
    // lane_decode's loop (snapmi_element.hpp: its checks, order and fields)
    // over the staged bytes, WRITTEN OUT: as one function over a memory policy
    // these kernels take more VGPRs than the parent's.
    uint32_t s = 0, d = 0;
    while (s < slen) {
        const uint32_t tag = bin[at(s)];
        s += 1;
        if ((tag & 3) == 0) {
            uint32_t len = (tag >> 2) + 1;
            if (len >= 61) {
                if (s + 4 > slen)
                    SNAPMI_FAIL(true, , SNAPMI_LITERAL, 4, slen - s, dlen - d);
                const uint32_t nb = len - 60;
                uint32_t raw = 0;
                for (uint32_t k = 0; k < 4; k++)
                    raw |= (uint32_t)bin[at(s + k)] << (8 * k);
                // (u64: a length field of 0xFFFFFFFF + 1 must not wrap)
                const uint64_t l64 =
                    (uint64_t)(nb == 4 ? raw : raw & ((1u << (8 * nb)) - 1)) +
                    1;
                s += nb;
                if (slen - s < l64 || dlen - d < l64)
                    SNAPMI_FAIL(true, , SNAPMI_LITERAL, l64, slen - s,
                                dlen - d);
                len = (uint32_t)l64;
            } else if (slen - s < len || dlen - d < len) {
                SNAPMI_FAIL(true, , SNAPMI_LITERAL, len, slen - s, dlen - d);
            }
            for (uint32_t k = 0; k < len; k++)
                bout[at(d + k)] = bin[at(s + k)];
            s += len;
            d += len;
        } else {
            const uint32_t kind = tag & 3;
            const uint32_t nb = copy_offset_bytes(kind);
            const uint32_t len = copy_length(tag);
            uint64_t offset = kind == 1 ? copy1_high(tag) : 0;
            if (s + nb > slen)
                SNAPMI_FAIL(true, , SNAPMI_COPY_READ, nb, slen - s, 0);
            uint32_t v = 0;
            for (uint32_t k = 0; k < nb; k++)
                v |= (uint32_t)bin[at(s + k)] << (8 * k);
            offset |= v;
            s += nb;
            if (d <= offset - 1) // wrapping, also catches offset == 0
                SNAPMI_FAIL(true, , SNAPMI_OFFSET, offset, d, 0);
            if (d + len > dlen)
                SNAPMI_FAIL(true, , SNAPMI_COPY_WRITE, len, dlen - d, 0);
            const uint32_t from = d - (uint32_t)offset;
            for (uint32_t k = 0; k < len; k++)
                bout[at(d + k)] = bout[at(from + k)];
            d += len;
        }
    }
    if (d != dlen)
        SNAPMI_FAIL(true, , SNAPMI_HEADER_MISMATCH, dlen, d, 0);
    gptr dst = (gptr)a.out_ptrs[st];
    {
        uint32_t k = 0;
        for (; k + 4 <= dlen; k += 4)
            st32u(dst + k, *(const l_u32t *)(bout + at(k)));
        for (; k < dlen; k++)
            dst[k] = bout[at(k)];
    }
    stream_done(a.errs, a.out_lens, st, SNAPMI_OK, 0, 0, 0, dlen);
}

__global__ __launch_bounds__(64) void k_decompress_tiny(DecompressArgs a)
{
    if (a.gate && uni64(*a.gate) != a.gate_value)
        return;
    decompress_lane_streams<kTinyLog2, kWave>(a, uni(a.bucket_pos[65]),
                                               a.n_streams);
}

// The libsnappy seam's single-launch path (snapmi_seam.hip, seam_tiny): ONE
// stream of under 256 compressed bytes; descriptor, input and output in
// pinned host memory, *done polled by the host (k_seam_compress_tiny).
__global__ __launch_bounds__(64) void k_seam_decompress_tiny(
    DecompressArgs a, uint32_t *done, uint32_t seq)
{
    decompress_lane_streams<kTinyLog2, kWave>(a, 0, 1);
    if (threadIdx.x == 0) {
        __threadfence_system();
        __hip_atomic_store(done, seq, __ATOMIC_RELEASE,
                           __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

__global__ __launch_bounds__(64) void k_decompress_small(DecompressArgs a)
{
    if (a.gate && uni64(*a.gate) != a.gate_value)
        return;
    decompress_lane_streams<kSmallDecLog2, 32>(a, uni(a.bucket_pos[64]),
                                               uni(a.bucket_pos[65]));
}

} // namespace snapmi
