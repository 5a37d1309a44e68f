// snapmi_decompress.hip -- Snappy raw stream decompressor for gfx950 (CDNA4).
//
// Semantics (element order, every bounds check, which error wins and with
// which field values) follow the reference src/decompress.rs exactly.  The
// reference walks one element at a time (tag dispatch loop, :130-148).  A raw
// stream has no block index (src/compress.rs:128-153), so the stream is the
// parallel unit; a batch supplies thousands of them, sorted longest first
// (k_plan_decompress*), and every size class has its kernel:
//
//   k_decompress_streams3 (+ _many)   one wavefront per stream, the default.
//       decode_windows3 (third generation): 256 compressed bytes per window;
//       the lanes look at tag bytes only to find the element starts (four
//       rounds of pointer jumping per 64-byte group), the starts are
//       compacted so that lane t holds the t-th ELEMENT of the window, which
//       is then decoded, checked and placed (DPP scan) per lane; elements
//       whose source is complete are copied in one lane-parallel step of
//       whole 16-byte pieces (lane order of one DS instruction resolves the
//       overlaps), far sources requested for the whole window at once; the
//       elements that read the window's own output follow one by one, by
//       the whole wave.  A 4 KiB ring of recent output lives in LDS, the
//       ring goes to HBM 256 bytes at a time.  The last 337 bytes of a
//       stream are decode_windows2's (second generation: 64-byte windows, an
//       element per lane that sits on its first byte), which is also
//       k_decompress_streams2, the cross-check of the test build.
//   k_decompress_tiny / _small   streams of under 256 / 512 compressed bytes
//       whose output is no larger: one per LANE (64 / 32 per wavefront),
//       input and output staged in LDS, the reference's loop per lane.
//   k_decompress_sequential   the reference's loop, one element at a time:
//       what names every error (any failed check of the wide paths hands the
//       stream over), and the fallback of a device that fails the LDS
//       store-order self-check.
// (What cuts ONE long stream into pieces for these kernels, on many
// wavefronts - k_long_plan, k_bstream_* -, decodes nothing and lives beside
// its host code: snapmi_longstream.hip.  What cuts pieces from a block index,
// and what builds one from the scan's cuts, decodes nothing and lives beside
// its host code: snapmi_index.hip.)
//
// DESIGN.md section 4.2 has the history (byte-per-lane kernel of round 1,
// gone; 354 -> 16 ms at cfg2) and what bounds each of them.
#include "snapmi_device.hpp"
#include "snapmi_kernels.hpp"
#include "snapmi_scan.hpp"

namespace snapmi {

namespace {


#define SNAPMI_FAIL(kind, fa, fb, fc)                                         \
    do {                                                                      \
        if (lane == 0) {                                                      \
            set_error(a.errs, st, (kind), (fa), (fb), (fc));                  \
            a.out_lens[st] = 0;                                               \
        }                                                                     \
        return;                                                               \
    } while (0)

// The reference's element-at-a-time loop (src/decompress.rs:130-343), state
// in SGPRs, bytes moved by the lanes.  Used to finish a stream once the wide
// path has met something irregular; resumes at (s, d).
__device__ __forceinline__ void decode_sequential(const DecompressArgs &a,
                                               uint64_t st, uint32_t lane,
                                               gcptr src,
                                               uint64_t src_len, gptr dst,
                                               uint64_t dst_len, uint64_t s,
                                               uint64_t d)
{
    ByteWindow win;
    win.init(src, src_len);
    uint64_t pend = 0; // dst[pend..d) may still be in flight (stores)

    while (s < src_len) {
        const uint32_t w = win.get32(s); // tag + the 3 bytes after it
        const uint32_t tag = w & 0xFF;
        s += 1;
        if ((tag & 3) == 0) {
            // reference read_literal, src/decompress.rs:161-228
            uint64_t len = (tag >> 2) + 1;
            if (len >= 61) {
                if (s + 4 > src_len)
                    SNAPMI_FAIL(SNAPMI_LITERAL, 4, src_len - s, dst_len - d);
                const uint32_t nb = (uint32_t)len - 60;
                const uint32_t raw = win.get32(s);
                len = (uint64_t)(nb == 4 ? raw
                                         : raw & ((1u << (8 * nb)) - 1)) +
                      1;
                s += nb;
            }
            if (src_len - s < len || dst_len - d < len)
                SNAPMI_FAIL(SNAPMI_LITERAL, len, src_len - s, dst_len - d);
            gcptr from = src + s;
            gptr to = dst + d;
            for (uint64_t i = 4 * lane; i + 4 <= len; i += 4 * kWave)
                st32u(to + i, ld32u(from + i));
            const uint64_t t = len & ~3ull;
            if (lane < (len & 3))
                to[t + lane] = from[t + lane];
            s += len;
            d += len;
        } else {
            // reference read_copy + TagEntry::offset,
            // src/decompress.rs:233-343,433-474
            const uint32_t kind = tag & 3;
            const uint32_t nb = kind == 1 ? 1 : (kind == 2 ? 2 : 4);
            const uint32_t len =
                kind == 1 ? 4 + ((tag >> 2) & 7) : 1 + (tag >> 2);
            uint64_t offset = kind == 1 ? (uint64_t)(tag >> 5) << 8 : 0;
            if (s + 4 <= src_len) {
                if (nb == 1)
                    offset |= (w >> 8) & 0xFF;
                else if (nb == 2)
                    offset |= (w >> 8) & 0xFFFF;
                else
                    offset |= win.get32(s);
            } else if (nb == 1) {
                if (s >= src_len)
                    SNAPMI_FAIL(SNAPMI_COPY_READ, 1, src_len - s, 0);
                offset |= (w >> 8) & 0xFF;
            } else if (nb == 2) {
                if (s + 1 >= src_len)
                    SNAPMI_FAIL(SNAPMI_COPY_READ, 2, src_len - s, 0);
                offset |= (w >> 8) & 0xFFFF;
            } else {
                SNAPMI_FAIL(SNAPMI_COPY_READ, 4, src_len - s, 0);
            }
            s += nb;
            if (d <= offset - 1) // wrapping, also catches offset == 0
                SNAPMI_FAIL(SNAPMI_OFFSET, offset, d, 0);
            const uint64_t end = d + len;
            if (end > dst_len)
                SNAPMI_FAIL(SNAPMI_COPY_WRITE, len, dst_len - d, 0);

            // Source bytes are dst[d-offset .. min(d, d-offset+len)).  If
            // any of them may still be an in-flight store of this wave,
            // drain the stores first.
            const uint64_t from0 = d - offset;
            const uint64_t src_end = offset < len ? d : from0 + len;
            if (src_end > pend) {
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
                pend = d;
            }
            if (lane < len) {
                uint32_t i = lane;
                if (offset < len) {
                    // pattern replication: i mod offset, exact for i,offset<64
                    const uint32_t o = (uint32_t)offset;
                    const uint32_t q =
                        (uint32_t)(((float)lane + 0.5f) *
                                   __builtin_amdgcn_rcpf((float)o));
                    i = lane - q * o;
                }
                dst[d + lane] = dst[from0 + i];
            }
            d = end;
        }
    }
    if (d != dst_len)
        SNAPMI_FAIL(SNAPMI_HEADER_MISMATCH, dst_len, d, 0);
    if (lane == 0) {
        set_error(a.errs, st, SNAPMI_OK, 0, 0, 0);
        a.out_lens[st] = dst_len;
    }
}

// wave64 DPP helpers (row_shr inside rows of 16, row_bcast across rows)
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ uint32_t dpp_get(uint32_t v)
{
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, ROW_MASK,
                                                 0xF, false);
}
// Inclusive prefix sum over the wave: six v_add_u32_dpp.  (Through the
// update_dpp builtin every step is a v_mov_dpp plus an add - the compiler
// does not fold them - and the decoders' window loop is bound by VALU issue.)
// A DPP operand written by the instruction in front needs two wait states;
// the compiler cannot see into the asm, so the first pad also covers the
// worst case in front of it (a VALU write of EXEC: five wait states).
__device__ __forceinline__ uint32_t wave_inclusive_add(uint32_t v)
{
    asm volatile(
        "s_nop 4\n\t"
        "v_add_u32_dpp %0, %0, %0 row_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
        "s_nop 1\n\t"
        "v_add_u32_dpp %0, %0, %0 row_shr:2 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
        "s_nop 1\n\t"
        "v_add_u32_dpp %0, %0, %0 row_shr:4 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
        "s_nop 1\n\t"
        "v_add_u32_dpp %0, %0, %0 row_shr:8 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
        "s_nop 1\n\t"
        "v_add_u32_dpp %0, %0, %0 row_bcast:15 row_mask:0xa bank_mask:0xf\n\t"
        "s_nop 1\n\t"
        "v_add_u32_dpp %0, %0, %0 row_bcast:31 row_mask:0xc bank_mask:0xf\n\t"
        "s_nop 1"
        : "+v"(v));
    return v;
}
// OR of v over all lanes (uniform result)
__device__ __forceinline__ uint32_t wave_or(uint32_t v)
{
    v |= dpp_get<0x111, 0xF>(v);
    v |= dpp_get<0x112, 0xF>(v);
    v |= dpp_get<0x114, 0xF>(v);
    v |= dpp_get<0x118, 0xF>(v);
    v |= dpp_get<0x142, 0xA>(v);
    v |= dpp_get<0x143, 0xC>(v);
    return rdlane(v, 63);
}

__device__ __forceinline__ uint32_t popc_below(uint64_t mask)
{
    // number of set bits of `mask` strictly below this lane
    return __builtin_amdgcn_mbcnt_hi(
        (uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0));
}

// 8 bytes at src[pos..] with bytes at or past `avail` read as zero
__device__ __forceinline__ uint64_t ld64g(gcptr src, uint64_t pos,
                                          uint64_t avail)
{
    if (pos + 8 <= avail) {
        uint64_t v;
        __builtin_memcpy(&v, src + pos, 8);
        return v;
    }
    uint64_t v = 0;
    for (uint32_t k = 0; k < 7; k++)
        if (pos + k < avail)
            v |= (uint64_t)src[pos + k] << (8 * k);
    return v;
}

// 16 bytes as two qwords
struct B16x {
    uint64_t lo, hi;
};


// 8 bytes at src[pos..] for a stream of avail >= 8 readable bytes; bytes at
// or past `avail` read as zero.  Branch-free: the load address is clamped
// into the stream and the value shifted back into place.
__device__ __forceinline__ uint64_t ld64c(gcptr src, uint64_t pos,
                                          uint64_t avail)
{
    const uint64_t pc = pos < avail - 8 ? pos : avail - 8;
    uint64_t v;
    __builtin_memcpy(&v, src + pc, 8);
    const uint64_t sh = pos - pc; // 0 inside the stream
    return sh < 8 ? v >> (8 * sh) : 0;
}

} // namespace

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
    if (threadIdx.x == 0) {
        uint32_t run = 0;
        for (uint32_t k = 0; k < 64; k++) {
            if (k == 64 - kFirstWide) // the wavefront decoder's streams
                a.bucket_pos[64] = run;
            if (k == 64 - kSmallClass) // ... and k_decompress_small's
                a.bucket_pos[65] = run;
            const uint32_t c = hist[k];
            hist[k] = run;
            run += c;
        }
    }
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
    if (threadIdx.x == 0) {
        uint32_t run = 0;
        for (uint32_t k = 0; k < 64; k++) {
            if (k == 64 - kFirstWide)
                a.bucket_pos[64] = run;
            if (k == 64 - kSmallClass)
                a.bucket_pos[65] = run;
            const uint32_t c = a.bucket_pos[k];
            a.bucket_pos[k] = run;
            run += c;
        }
    }
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

// ---------------------------------------------------------------------
// One wavefront per raw stream: the wide path.
//
// Two window loops share the stream prologue, a 4 KiB ring of recent output
// in LDS and the hand-over to the sequential decoder:
//
// decode_windows2 (second generation; k_decompress_streams2 and the last
// bytes of every stream in k_decompress_streams3) - 64 compressed bytes per
// window, an element is copied by the lane that sits on its first byte:
//
//   1. every lane decodes the element that would start at its byte of the
//      64-byte window, and loads 16 literal bytes speculatively;
//   2. the real element starts are the orbit of lane 0 under "next element"
//      (one ds_bpermute per round, see the loop) - no compaction, the
//      records stay where they were decoded;
//   3. a DPP scan of the output lengths over the start lanes places every
//      element; the window is cut after 2048 output bytes (kWinMax), so a
//      4 KiB ring of recent output in LDS always keeps 2 KiB of history that
//      the window's own writes cannot touch;
//   4. ONE lane-parallel copy step: every element whose source is complete
//      before the window (literals; copies from in front of it) is copied by
//      its lane, 16 bytes per trip - source: the speculative literal bytes,
//      the ring, or HBM for what the ring no longer holds - and stored to
//      the ring as WHOLE 16-byte pieces, last piece first: overlapping lanes
//      of one DS store are applied in ascending lane order, so the excess
//      bytes of a short element are overwritten by the elements that follow;
//   5. the few elements that read the window's own output or repeat a short
//      period are swept in stream order, each by the whole wave (lane k =
//      byte k, k mod offset for overlaps);
//   6. the ring goes to HBM 256 bytes at a time (one dword per lane), so
//      global stores are whole aligned lines instead of 64 byte stores.
//
// decode_windows3 (third generation, the default) - 256 compressed bytes per
// window and one ELEMENT per lane; described at the function.
//
// Both loops are bound by instruction issue - VALU (a wave64 integer
// instruction holds its SIMD for four cycles) and the CU's one scalar unit
// about equally, the LDS pipeline third (tests/hw/lds_cost.hip) - so they are
// written for few instructions: predicates are 64-bit lane masks in SGPRs,
// combined with scalar ALU operations and handed back to the vector side as
// they are (inverse ballot); positions are 32-bit (no scalar 64-bit compare
// exists); tests that only matter near the end of the input sit behind one
// uniform branch; addresses are a uniform base plus a 32-bit lane offset.
//
// Everything irregular - a failed check, an element cut off by the end of
// the input - stops the wide path at a window boundary: the ring is stored
// and the sequential decoder above finishes the stream from (s, d) with the
// reference's exact error.  tests/model_decoder.py and tests/model_decoder3.py
// restate the two loops lane by lane on the CPU (test infrastructure, not
// used here).
// ---------------------------------------------------------------------
namespace {
#define SNAPMI_RING 4096 // experiment builds: 8192 / 16384 (make ring_variants)
constexpr uint32_t kRing2 = SNAPMI_RING;
constexpr uint32_t kWinMax = 2048;

__device__ __forceinline__ uint32_t lds_ld32(const l_u8 *p)
{
    uint32_t v;
    __builtin_memcpy(&v, p, 4);
    return v;
}
__device__ __forceinline__ uint64_t lds_ld64(const l_u8 *p)
{
    uint64_t v;
    __builtin_memcpy(&v, p, 8);
    return v;
}
__device__ __forceinline__ void lds_st64(l_u8 *p, uint64_t v)
{
    __builtin_memcpy(p, &v, 8);
}
__device__ __forceinline__ void lds_st32(l_u8 *p, uint32_t v)
{
    __builtin_memcpy(p, &v, 4);
}
__device__ __forceinline__ void lds_st16(l_u8 *p, uint16_t v)
{
    __builtin_memcpy(p, &v, 2);
}

struct Ring2 {
    l_u8 *rg;       // kRing2 bytes + a 16-byte mirror of its first 16
    gptr dst;
    uint32_t lane;
    uint32_t gflush; // dst[0, gflush) has been stored
    uint32_t fenced; // ... and those stores are known to be complete

    // ring[0,16) again behind the end: unaligned reads may run past it
    __device__ __forceinline__ void mirror() const
    {
        if (lane < 4)
            lds_st32(rg + kRing2 + 4 * lane, lds_ld32(rg + 4 * lane));
    }
    // whole 256-byte pieces of dst[gflush, d), one dword per lane
    __device__ __forceinline__ void flush_chunks(uint32_t d)
    {
        while (gflush + 256 <= d) {
            const uint32_t p = gflush + 4 * lane;
            st32u(dst + p, lds_ld32(rg + (p & (kRing2 - 1))));
            gflush += 256;
        }
    }
    // everything up to `upto`, bytewise (before a long literal, at the end,
    // when the sequential decoder takes over)
    __device__ __forceinline__ void flush_partial(uint32_t upto)
    {
        for (uint32_t p = gflush + lane; p < upto; p += kWave)
            dst[p] = rg[p & (kRing2 - 1)];
        gflush = upto;
    }
    // a far source must be a completed store
    __device__ __forceinline__ void fence_for(uint32_t limit)
    {
        if (limit > fenced) {
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
            fenced = gflush;
        }
    }
};
} // namespace

namespace {
#define SNAPMI_FAIL_V(ret, kind, fa, fb, fc)                                  \
    do {                                                                      \
        if (lane == 0) {                                                      \
            set_error(a.errs, st, (kind), (fa), (fb), (fc));                  \
            a.out_lens[st] = 0;                                               \
        }                                                                     \
        return ret;                                                           \
    } while (0)

// The wide path's state: everything uniform (SGPRs).
struct Wide {
    gcptr src;        // elements (behind the varint header)
    gptr dst;
    uint64_t src_len, dst_len;
    uint64_t st;      // stream index
    // Positions are 32-bit: there is no scalar 64-bit compare, each one in
    // a window loop would be two VALU instructions.  dst_len < 2^32 by the
    // format; a compressed stream of 4 GiB or more (legal, if every element
    // is tiny) is left to the sequential decoder as a whole, and so is an
    // output within 4 KiB of 2^32 (window arithmetic like d + W + 16 must
    // not wrap).
    uint32_t slen, dlen;
    uint32_t s, d;    // positions in src / dst
    uint32_t ring_lo; // the ring holds dst[max(ring_lo, d - 4096), d)
    Ring2 R;
    PROF(
    uint64_t n_win = 0, n_elem = 0, n_dep = 0, n_fence = 0, n_far = 0,
             n_trip = 0, n_run = 0, n_win3 = 0;
    )
    __device__ __forceinline__ bool too_big() const
    {
        return src_len > 0xFFE00000ull || dst_len > 0xFFFFF000ull;
    }
};

// Stored chunk, header, capacity (reference Decoder::decompress,
// src/decompress.rs:75-95).  False: the stream is finished (copied, or its
// error is written).
__device__ __forceinline__ bool open_stream(const DecompressArgs &a,
                                            const uint32_t lane, Wide &x,
                                            l_u8 *ring_mem,
                                            const uint32_t slot)
{
    const uint64_t st = a.order[slot]; // slot: position in the sorted order
    gcptr in = (gcptr)a.in_ptrs[st];
    const uint64_t in_len = a.in_lens[st];
    const bool piece = a.modes && a.modes[st] == 2;

    if (a.modes && a.modes[st] == 3)
        return false; // another launch decodes this stream
    if (a.modes && a.modes[st] == 1) {
        // stored frame chunk (reference src/read.rs:173-199): the payload is
        // the data (wave_copy)
        const uint64_t cap0 = a.out_caps[st];
        if (in_len > cap0)
            SNAPMI_FAIL_V(false, SNAPMI_BUFFER_TOO_SMALL, cap0, in_len, 0);
        wave_copy<false>((gptr)a.out_ptrs[st], in, in_len, lane);
        if (lane == 0) {
            set_error(a.errs, st, SNAPMI_OK, 0, 0, 0);
            a.out_lens[st] = in_len;
        }
        return false;
    }
    uint32_t hdr = 0;
    uint64_t dst_len = 0;
    if (piece) { // elements [in, in + in_len) produce exactly out_caps bytes
        dst_len = a.out_caps[st];
    } else {
        if (in_len == 0)
            SNAPMI_FAIL_V(false, SNAPMI_EMPTY, 0, 0, 0);
        snapmi_error *e = lane == 0 ? a.errs : nullptr;
        if (read_header(in, in_len, &hdr, &dst_len, e, st) != SNAPMI_OK) {
            if (lane == 0)
                a.out_lens[st] = 0;
            return false;
        }
    }
    // the header came through vector loads: pin it (and everything derived
    // from it) to SGPRs so the decoder state is scalar
    hdr = uni(hdr);
    dst_len = uni64(dst_len);
    const uint64_t cap = a.out_caps[st];
    if (dst_len > cap)
        SNAPMI_FAIL_V(false, SNAPMI_BUFFER_TOO_SMALL, cap, dst_len, 0);
    x.st = st;
    x.src = in + hdr;
    x.src_len = in_len - hdr;
    x.dst = (gptr)a.out_ptrs[st];
    x.dst_len = dst_len;
    x.slen = (uint32_t)x.src_len;
    x.dlen = (uint32_t)dst_len;
    x.s = x.d = x.ring_lo = 0;
    x.R.rg = ring_mem;
    x.R.dst = x.dst;
    x.R.lane = lane;
    x.R.gflush = 0;
    x.R.fenced = 0;
    return true;
}

// The end of a stream: what the wide path has in the ring is stored; an
// irregular stream is finished (and its error named) by the sequential
// decoder; HeaderMismatch, reference src/decompress.rs:149-157.
__device__ __forceinline__ void close_stream(const DecompressArgs &a,
                                             const uint32_t lane, Wide &x,
                                             const bool irregular)
{
    const uint64_t st = x.st;
    x.R.flush_partial(x.d);
    if (irregular) {
        decode_sequential(a, st, lane, x.src, x.src_len, x.dst, x.dst_len,
                          x.s, x.d);
        return;
    }
    PROF(
    if (lane == 0 && a.prof) {
        atomicAdd(&a.prof[7], (unsigned long long)x.n_win3);
        atomicAdd(&a.prof[8], (unsigned long long)x.n_run);
        atomicAdd(&a.prof[9], (unsigned long long)x.n_far);
        atomicAdd(&a.prof[10], (unsigned long long)x.n_win);
        atomicAdd(&a.prof[11], (unsigned long long)x.n_trip);
        atomicAdd(&a.prof[12], (unsigned long long)x.n_elem);
        atomicAdd(&a.prof[13], (unsigned long long)x.n_fence);
        atomicAdd(&a.prof[14], (unsigned long long)x.n_dep);
        atomicAdd(&a.prof[15], 1ull);
    }
    )
    if (x.d != x.dst_len)
        SNAPMI_FAIL(SNAPMI_HEADER_MISMATCH, x.dst_len, x.d, 0);
    if (lane == 0) {
        set_error(a.errs, st, SNAPMI_OK, 0, 0, 0);
        a.out_lens[st] = x.dst_len;
    }
}

// The second-generation window loop from (x.s, x.d) to the end of the
// input.  True: something irregular, the sequential decoder takes over.
__device__ __forceinline__ bool decode_windows2(Wide &x, const uint32_t lane)
{
    gcptr src = x.src;
    gptr dst = x.dst;
    const uint64_t src_len = x.src_len;
    const uint32_t slen = x.slen, dlen = x.dlen;
    uint32_t s = x.s, d = x.d, ring_lo = x.ring_lo;
    Ring2 &R = x.R;
    l_u8 *const rg = R.rg;
    // streams too short for the 8-byte window loads go to the sequential
    // decoder at once; so does the first failed check
    bool irregular = src_len < 8;
    uint64_t w = irregular || s >= slen
                     ? 0
                     : ld64c(src, (uint64_t)s + lane, src_len); // src[s+lane..]
    while (!irregular && s < slen) {
        COUNT(x.n_win);
        // bytes of input left, as far as this window can see (<= 2^20)
        const uint32_t rem = slen - s < (1u << 20) ? slen - s : 1u << 20;
        // ---- 1. the element that would start at src[s + lane] ------------
        const uint32_t tag = (uint32_t)w & 0xFF;
        const uint32_t b14 = (uint32_t)(w >> 8); // the 4 bytes after the tag
        const uint32_t type = tag & 3, n6 = tag >> 2;
        const bool is_lit = type == 0;
        // The bytes behind the tag hold a little-endian number of nb bytes:
        // the rest of a literal's length (nb = 0..4, reference read_literal,
        // src/decompress.rs:161-228) or a copy's offset (nb = 1, 2, 4,
        // TagEntry::offset / read_copy, :233-250,433-474) - one extraction
        // for both (this loop is bound by VALU issue: every instruction that
        // goes is 0.4 % of the kernel)
        const uint32_t lnb = (n6 > 59 ? n6 : 59) - 59; // extra length bytes
        const uint32_t cnb = type + (type == 3);        // 1, 2, 4
        const uint32_t sh = 32 - 8 * (is_lit ? lnb : cnb);
        const uint32_t ext = (b14 << (sh & 31)) >> (sh & 31); // (nb = 0: unused)
        const uint32_t lraw = lnb ? ext : n6; // length - 1
        const uint32_t hd = 1 + lnb;
        // Predicates live as 64-bit lane masks in SGPRs and are combined
        // there: a __ballot of a compound per-lane bool costs two VALU
        // instructions on top of its compares (the bool is materialised and
        // compared again), a scalar AND of two simple ballots costs none.
        const uint64_t M_lit = __ballot(is_lit);
        // literals of more than 64 bytes: not in a window
        const uint64_t M_lng = M_lit & __ballot(lraw >= 64);
        const uint32_t clen = type == 1 ? 4 + (n6 & 7) : 1 + n6;
        const uint32_t off = ext | (type == 1 ? (tag & 0xE0u) << 3 : 0);
        const uint32_t olen = is_lit ? lraw + 1 : clen;      // if !lng
        const uint32_t enc = is_lit ? hd + lraw + 1 : 1 + cnb; // if !lng
        // the whole element lies inside the input (:189-217 src side, CopyRead)
        // (an extended literal length is read as 4 bytes: :189-198)
        // (a window with 160 bytes of input in front of it - all but the
        // last two or three of a stream - needs none of the per-lane tests:
        // lane + 5 + 64 + 16 <= rem whatever the element)
        const bool deep = rem >= 160;
        const uint64_t M_fits =
            deep ? ~M_lng
                 : ~M_lng & __ballot(lane < rem && enc <= rem - lane &&
                                     !(is_lit && lnb && lane + 5 > rem));
        // 16 literal bytes, speculatively (only windows well inside the input)
        const bool inner = rem >= 64 + 5 + 16;
        B16x lit16;
        // (uniform base + 32-bit lane offset: the load takes the base from
        // SGPRs and no 64-bit vector adds are spent on the address)
        const gcptr win_src = src + s;
        if (inner) {
            __builtin_memcpy(&lit16, win_src + (lane + hd), 16);
        } else {
            lit16.lo = lit16.hi = 0;
        }
        // ---- 2. element starts: the orbit of lane 0 under "next" ----------
        // A ds_bpermute costs the CU's one LDS pipeline about as much as
        // seven VALU instructions cost its four SIMDs (tests/hw/lds_cost.hip:
        // 6.4 cycles), so the discovery moves ONE dword per round: the wave
        // is two halves of 32 positions, and a lane's set R (32 bits, its own
        // half) holds the first nodes of its chain INCLUDING the frontier -
        // the node not yet expanded, which is the set's highest bit because
        // chains run forward.  One round: R |= R[frontier].  After k rounds a
        // set holds 2^k + 1 nodes; a half has at most 16 (every element has
        // two bytes or more), so four rounds finish it.  A lane whose element
        // ends its chain - long literal, behind the input, or reaching into
        // the other half / out of the window - has no frontier beyond itself
        // and fetches its own set.  The two halves are strung together by
        // the scalar unit afterwards.
        const uint32_t nx = lane + enc;
        const uint64_t T = M_lng | (deep ? 0 : __ballot(lane >= rem));
        const uint64_t M_stay = ~T & __ballot((nx ^ lane) < 32);
        uint32_t Rr = (1u << (lane & 31)) |
                      (__builtin_amdgcn_inverse_ballot_w64(M_stay)
                           ? 1u << (nx & 31)
                           : 0);
        const int c4 = (int)((lane | 31) << 2);
#pragma unroll
        for (uint32_t k = 0; k < 4; k++) {
            const int sel = c4 - 4 * (int)__builtin_clz(Rr);
            Rr |= (uint32_t)__builtin_amdgcn_ds_bpermute(sel, (int)Rr);
        }
        uint64_t S = rdlane(Rr, 0);
        {
            // the last start of the lower half: does its element lead into
            // the upper half?
            const uint32_t t0 = 31 - (uint32_t)__builtin_clz((uint32_t)S);
            const uint32_t nx0 = rdlane(nx, t0);
            if (!((T >> t0) & 1) && nx0 < kWave)
                S |= (uint64_t)rdlane(Rr, nx0) << 32;
        }
        // ---- 3. placement, window cut, checks ------------------------------
        const uint64_t M_elem = S & M_fits;
        const uint32_t o =
            __builtin_amdgcn_inverse_ballot_w64(M_elem) ? olen : 0;
        const uint32_t incl = wave_inclusive_add(o);
        // the window ends in front of the first start that is a long literal
        // or does not fit, and after kWinMax output bytes
        const uint64_t stop = S & ~M_fits;
        const uint64_t below =
            stop ? ((1ull << __builtin_ctzll(stop)) - 1) : ~0ull;
        const uint64_t K = M_elem & __ballot(incl <= kWinMax) & below;
        if (K == 0) {
            // lane 0 is a literal of more than 64 bytes: wave_copy
            const uint32_t lng0 = (uint32_t)M_lng & 1u;
            const uint64_t Lq = (uint64_t)rdlane(lraw, 0) + 1;
            const uint32_t h0 = rdlane(hd, 0);
            if (!lng0 || rem < h0 || slen - (s + h0) < Lq || dlen - d < Lq) {
                irregular = true; // the sequential decoder names the error
                break;
            }
            R.flush_partial(d);
            wave_copy<false>(dst + d, src + s + h0, Lq, lane);
            s += h0 + (uint32_t)Lq;
            d += (uint32_t)Lq;
            R.gflush = d;
            ring_lo = d; // these bytes are not in the ring
            if (s < slen)
                w = ld64c(src, (uint64_t)s + lane, src_len);
            continue;
        }
        const uint32_t last = 63 - (uint32_t)__builtin_clzll(K);
        const uint32_t W = rdlane(incl, last);         // output of the window
        const uint32_t cur = last + rdlane(enc, last); // input consumed
        const uint32_t dstp = d + (incl - o);          // element's position
        // reference checks :209-217 (dst side), :245-250, :327-332
        const uint64_t M_cpy = K & ~M_lit;
        if (W > dlen - d ||
            (M_cpy & (__ballot(off == 0) | __ballot(off > dstp))) != 0) {
            irregular = true;
            break;
        }
        PROF(
        x.n_elem += __builtin_popcountll(K);
        )
        // next window's bytes: issued now, consumed after the expand
        // (plain unaligned loads while the next window lies inside the
        // input - a uniform test; the clamped form only at the stream's end)
        uint64_t w_next;
        if (slen - s >= cur + kWave + 8)
            __builtin_memcpy(&w_next, src + (s + cur) + lane, 8);
        else
            w_next = ld64c(src, (uint64_t)s + cur + lane, src_len);

        // ---- 4. the lane-parallel copy step --------------------------------
        const uint32_t q = dstp - off;               // copy source (if cpy)
        // (a copy that a lane moves by itself does not overlap its source:
        // olen <= off, it reads olen bytes)
        const uint32_t qe = q + olen;
        // (whole 16-byte pieces are stored: up to 15 bytes behind the window's
        // output may be clobbered too)
        const uint32_t dW = d + W + 16;
        uint32_t safe_lo = dW > kRing2 ? dW - kRing2 : 0;
        safe_lo = safe_lo > ring_lo ? safe_lo : ring_lo;
        const uint64_t M_ring = __ballot(q >= safe_lo);
        // 16-byte loads from HBM must stay inside the buffers: an element
        // that ends within 15 bytes of the input's / the output's end is
        // left to the sweep, which moves exactly its bytes
        // (for a literal near the end of the input the exact figure, for a
        // copy from HBM 64: elements of a window have at most 64 bytes)
        // lanes that copy their element themselves: literals (with their 16
        // speculative bytes inside the input), copies whose whole source lies
        // in front of the window, in the ring's safe part or stored already
        const uint64_t M_litok =
            deep ? M_lit
                 : (inner ? M_lit & __ballot(lane + hd + ((olen + 15) & ~15u) <=
                                             rem)
                          : 0);
        const uint64_t M_src = __ballot(qe <= d) & __ballot(olen <= off);
        const uint64_t M_farok =
            dlen >= 64 ? __ballot(qe <= R.gflush) & __ballot(q <= dlen - 64)
                       : 0;
        const uint64_t M_lw =
            K &
            (M_litok | (~M_lit & M_src & (M_ring | M_farok)));
        const uint64_t M_far = M_lw & ~M_lit & ~M_ring; // source in HBM
        const uint64_t M_rng = M_lw & ~M_lit & M_ring;  // source in the ring
        {
            if (M_far) {
                PROF(
                x.n_far += __builtin_popcountll(M_far);
                )
                if ((M_far & __ballot(qe > R.fenced)) != 0) {
                    R.fence_for(0xFFFFFFFFu);
                    COUNT(x.n_fence);
                }
            }
            // Every lane stores WHOLE 16-byte pieces with one ds_write_b128:
            // the bytes past an element's end land on the following elements,
            // whose lanes are higher and whose stores of the same instruction
            // therefore win (overlapping lanes of one DS store are applied in
            // ascending lane order: tests/hw/lds_write_order.hip, checked at
            // context creation).  The pieces go last to first, so the excess
            // of an element's last piece is repaired by the first pieces of
            // its successors, which are all written by the last trip.
            const uint64_t M_g16 = M_lw & __ballot(olen > 16);
            const uint32_t top =
                M_g16 == 0 ? 0
                           : ((M_g16 & __ballot(olen > 48))
                                  ? 48
                                  : ((M_g16 & __ballot(olen > 32)) ? 32 : 16));
            // an element's own bytes wrap around the ring's end only in a
            // window whose output does (uniform)
            const bool wraps = (d & (kRing2 - 1)) + W > kRing2;
            for (uint32_t c = top;; c -= 16) {
                const uint64_t M_act = c == 0 ? M_lw : M_lw & __ballot(c < olen);
                if (M_act != 0) {
                    COUNT(x.n_trip);
                    // source: 16 bytes from the literal, the ring, or HBM
                    // (a lane that loads nothing below stores nothing either:
                    // whatever v starts with - the literal bytes of trip 0 -
                    // is never seen)
                    B16x v = lit16;
                    if (c != 0 && __builtin_amdgcn_inverse_ballot_w64(
                                      M_act & M_lit)) {
                        __builtin_memcpy(&v, win_src + (lane + hd + c), 16);
                    }
                    if ((M_act & M_far) != 0 &&
                        __builtin_amdgcn_inverse_ballot_w64(M_act & M_far))
                        __builtin_memcpy(&v, dst + (q + c), 16);
                    if (__builtin_amdgcn_inverse_ballot_w64(M_act & M_rng)) {
                        // (only the lanes that need it: the LDS serves a wave's
                        // scattered unaligned reads a few lanes per cycle)
                        // (one unaligned 16-byte read costs the LDS one
                        // cycle per lane, two 8-byte reads two:
                        // tests/hw/lds_cost.hip; it may run into the mirror)
                        __builtin_memcpy(&v, rg + ((q + c) & (kRing2 - 1)), 16);
                    }
                    const uint32_t wa = (dstp + c) & (kRing2 - 1);
                    // (rare) the element's own bytes wrap around the ring's
                    // end: those lanes store bytewise, after the others
                    uint64_t M_strad = 0;
                    uint32_t m = 16;
                    if (wraps) {
                        m = olen - c < 16 ? olen - c : 16;
                        M_strad = M_act & __ballot(wa + m > kRing2);
                    }
                    if (__builtin_amdgcn_inverse_ballot_w64(M_act & ~M_strad))
                        __builtin_memcpy(rg + wa, &v, 16); // may reach the mirror
                    if (M_strad != 0 &&
                        __builtin_amdgcn_inverse_ballot_w64(M_strad)) {
                        for (uint32_t j = 0; j < m; j++) {
                            const uint64_t part = j < 8 ? v.lo : v.hi;
                            rg[(wa + j) & (kRing2 - 1)] =
                                (uint8_t)(part >> (8 * (j & 7)));
                        }
                    }
                }
                if (c == 0)
                    break;
            }
        }
        // ---- 5. the sweep: elements that depend on this window -------------
        uint64_t dep = K & ~M_lw;
        while (dep) {
            COUNT(x.n_dep);
            const uint32_t i = (uint32_t)__builtin_ctzll(dep);
            dep &= dep - 1;
            const uint32_t ni = rdlane(olen, i), di = rdlane(dstp, i);
            uint32_t val = 0;
            if ((M_lit >> i) & 1) {
                // (only windows at the very end of the input, `inner` false)
                if (lane < ni)
                    val = src[s + i + rdlane(hd, i) + lane];
            } else {
                const uint32_t qi = rdlane(q, i), oi = rdlane(off, i);
                const uint32_t nsrc = ni < oi ? ni : oi;
                uint32_t kk = lane;
                if (oi < ni) { // overlapping: byte k repeats byte k mod oi
                    const uint32_t quo = (uint32_t)(
                        ((float)lane + 0.5f) *
                        __builtin_amdgcn_rcpf((float)oi));
                    kk = lane - quo * oi;
                }
                const bool in_ring = qi >= safe_lo;
                if (!in_ring) {
                    // bytes the ring has lost that are not stored yet (only
                    // right after a long literal): store them first
                    if (qi + nsrc > R.gflush)
                        R.flush_partial(di);
                    if (qi + nsrc > R.fenced) {
                        R.fence_for(0xFFFFFFFFu);
                        COUNT(x.n_fence);
                    }
                }
                if (lane < ni)
                    val = in_ring ? (uint32_t)rg[(qi + kk) & (kRing2 - 1)]
                                  : (uint32_t)dst[qi + kk];
            }
            if (lane < ni)
                rg[(di + lane) & (kRing2 - 1)] = (uint8_t)val;
        }
        // The mirror of ring[0,16) behind the ring's end, once per window (a
        // uniform test): the window's stores - whole 16-byte pieces, so up to
        // d + W + 16 - touched ring[0,16), or spilled over the end into the
        // mirror.  Within the window nobody reads through it what these
        // stores changed: such a source lies below safe_lo; the sweep and the
        // flush address the ring bytewise / dword-aligned.
        {
            const uint32_t a0 = d & (kRing2 - 1);
            if (a0 < 16 || a0 + W + 16 > kRing2)
                R.mirror();
        }
        // ---- 6. advance; whole 256-byte pieces go to HBM -------------------
        d += W;
        s += cur;
        w = w_next;
        R.flush_chunks(d);
    }
    x.s = s;
    x.d = d;
    x.ring_lo = ring_lo;
    return irregular;
}

// ---------------------------------------------------------------------
// The third-generation window loop: kG3 x 64 compressed bytes per window,
// one ELEMENT per lane.
//
// The second generation spends its instructions on lanes that hold no
// element: every lane decodes "the element that would start at my byte" in
// full (offset, length, checks, source classes), and one lane in four or five
// is a real start.  Instruction issue - vector and scalar - is what bounds
// the loop, so here the expensive part runs on real elements only:
//
//   1. LENGTHS.  A window is kG3 groups of 64 input bytes; lane l looks at
//      the TAG bytes at s + 64 g + l, just far enough to know how many
//      compressed bytes the element there would take (tag only: a literal
//      with length bytes - 61 bytes or more - always ends a window).
//   2. STARTS.  Per group one ds_bpermute per round, four rounds (a lane's
//      32-bit set of its 32-byte sub-window, frontier as the highest bit:
//      R |= R[frontier]); the 2 kG3 sub-windows are strung together by the
//      scalar unit (two v_readlane each).
//   3. COMPACTION.  The t-th start of the window goes to lane t: rank by
//      population count, position through a 64 kG3-byte table in LDS.
//   4. DECODE, PLACEMENT, CHECKS as in the second generation, but every lane
//      below the element count holds a real element (40 of 64 lanes on the
//      corpus instead of 14).
//   5. COPY.  Every element whose source is complete before the window -
//      literals, copies from in front of it - is copied by its lane, as in
//      the second generation: 16 bytes per trip, whole-piece stores resolved
//      by lane order, the far sources of the whole window requested at once.
//      Then the LATE elements - copies that read the window's own output
//      (2.3 per window on text, 8 on html) or overlap themselves - are moved
//      one by one, in stream order, by the whole wave (lane k = byte k).
//
// A window needs kTail3 bytes of input in front of it, so that none of its
// loads can leave the input; the last bytes of a stream (and streams shorter
// than that) are decode_windows2's.  True: something irregular.
// ---------------------------------------------------------------------
#define SNAPMI_G3 4
constexpr uint32_t kG3 = SNAPMI_G3;
static_assert(kG3 == 2 || kG3 == 4,
              "positions in a window are masked with 64 kG3 - 1; 8 groups do "
              "not fit 64 VGPRs");
// the last position (64 kG3 - 1), a tag, 60 literal bytes read as whole
// 16-byte pieces
constexpr uint32_t kTail3 = 64 * kG3 + 1 + 64 + 16;

__device__ __forceinline__ bool decode_windows3(Wide &x, const uint32_t lane,
                                                l_u8 *const postab)
{
    gcptr src = x.src;
    gptr dst = x.dst;
    const uint32_t slen = x.slen, dlen = x.dlen;
    uint32_t s = x.s, d = x.d, ring_lo = x.ring_lo;
    Ring2 &R = x.R;
    l_u8 *const rg = R.rg;
    bool irregular = false;
    uint32_t tg[kG3]; // tag bytes of the window at s, one per group
    bool have = false;
    const int c4 = (int)((lane | 31) << 2);
    const uint32_t self = 1u << (lane & 31);

    while (slen - s >= kTail3) {
        COUNT(x.n_win3);
        const gcptr win_src = src + s;
        if (!have) {
#pragma unroll
            for (uint32_t g = 0; g < kG3; g++)
                tg[g] = win_src[64 * g + lane];
        }
        // ---- 1. lengths, 2. starts -------------------------------------
        uint32_t nx[kG3], Rr[kG3];
#pragma unroll
        for (uint32_t g = 0; g < kG3; g++) {
            const uint32_t t = tg[g], type = t & 3;
            const uint32_t pos = 64 * g + lane;
            // copies take 2, 3, 5 bytes; a literal its tag and n6 + 1 bytes;
            // a literal with length bytes (n6 >= 60) ends every chain: its
            // "next" lies behind the window
            uint32_t enc =
                type ? (0x05030200u >> (8 * type)) & 0xFF : (t >> 2) + 2;
            enc = (t & 0xF3) == 0xF0 ? 255 : enc;
            nx[g] = pos + enc;
            // (the chain stays in this lane's 32-byte sub-window)
            Rr[g] = self | ((nx[g] ^ pos) < 32 ? 1u << (nx[g] & 31) : 0);
        }
#pragma unroll
        for (uint32_t k = 0; k < 4; k++) {
#pragma unroll
            for (uint32_t g = 0; g < kG3; g++) {
                const int sel = c4 - 4 * (int)__builtin_clz(Rr[g]);
                Rr[g] |= (uint32_t)__builtin_amdgcn_ds_bpermute(sel,
                                                                (int)Rr[g]);
            }
        }
        // the sub-windows, strung together: sub-window k is entered at its
        // byte e; its last start's element leads into a later one (or out
        // of the window)
        uint32_t S32[2 * kG3];
#pragma unroll
        for (uint32_t kk = 0; kk < 2 * kG3; kk++)
            S32[kk] = 0;
        {
            uint32_t k = 0, e = 0;
#pragma unroll
            for (uint32_t kk = 0; kk < 2 * kG3; kk++) {
                if (k == kk) {
                    const uint32_t g = kk >> 1, half = 32 * (kk & 1);
                    const uint32_t Sk = rdlane(Rr[g], half + e);
                    S32[kk] = Sk;
                    const uint32_t lt = 31 - (uint32_t)__builtin_clz(Sk);
                    const uint32_t nxa = rdlane(nx[g], half + lt);
                    k = nxa >> 5;
                    e = nxa & 31;
                }
            }
        }
        uint64_t S[kG3];
#pragma unroll
        for (uint32_t g = 0; g < kG3; g++)
            S[g] = ((uint64_t)S32[2 * g + 1] << 32) | S32[2 * g];
        // ---- 3. compaction ---------------------------------------------
        uint32_t base = 0;
#pragma unroll
        for (uint32_t g = 0; g < kG3; g++) {
            // (a lane that is no start writes behind the table: a select is
            // cheaper than an exec region - the scalar unit is what is short)
            const uint32_t r = __builtin_amdgcn_inverse_ballot_w64(S[g])
                                   ? base + popc_below(S[g])
                                   : 64 * kG3 + lane;
            postab[r] = (uint8_t)(64 * g + lane);
            base += (uint32_t)__builtin_popcountll(S[g]);
        }
        const uint32_t n_el = base < kWave ? base : kWave;
        const uint64_t M_act = n_el == kWave ? ~0ull : (1ull << n_el) - 1;
        // (lanes behind the last element read what an earlier window left:
        // any position in the window will do, they are masked by M_act)
        const uint32_t pos = postab[lane] & (64 * kG3 - 1);
        // ---- 4. the element, in full -----------------------------------
        uint64_t w;
        __builtin_memcpy(&w, win_src + pos, 8);
        B16x lit16;
        __builtin_memcpy(&lit16, win_src + (pos + 1), 16);
        const uint32_t tag = (uint32_t)w & 0xFF;
        const uint32_t b14 = (uint32_t)(w >> 8); // the 4 bytes after the tag
        const uint32_t type = tag & 3, n6 = tag >> 2;
        const uint64_t M_lit = __ballot(type == 0);
        const uint64_t M_lng = M_act & M_lit & __ballot(n6 >= 60);
        // a copy's offset: 1, 2 or 4 bytes behind the tag (TagEntry::offset /
        // read_copy, reference src/decompress.rs:233-250,433-474)
        const uint32_t cnb = type + (type == 3);
        const uint32_t sh = 32 - 8 * cnb;
        const uint32_t ext = (b14 << (sh & 31)) >> (sh & 31);
        const uint32_t off = ext | (type == 1 ? (tag & 0xE0u) << 3 : 0);
        // output bytes: a literal's and a long copy's n6 + 1, copy-1's 4..11
        const uint32_t olen = type == 1 ? 4 + (n6 & 7) : 1 + n6;
        const uint32_t enc = type == 0 ? n6 + 2 : 1 + cnb;
        const uint64_t M_el = M_act & ~M_lng;
        const uint32_t o =
            __builtin_amdgcn_inverse_ballot_w64(M_el) ? olen : 0;
        const uint32_t incl = wave_inclusive_add(o);
        // the window ends in front of a literal with length bytes, and after
        // kWinMax output bytes
        const uint64_t below =
            M_lng ? ((1ull << __builtin_ctzll(M_lng)) - 1) : ~0ull;
        const uint64_t K = M_el & __ballot(incl <= kWinMax) & below;
        if (K == 0) {
            // lane 0 is a literal with length bytes (reference read_literal,
            // src/decompress.rs:161-228): moved by the whole wave
            const uint32_t lnb = rdlane(n6, 0) - 59; // 1..4 length bytes
            const uint32_t b0 = rdlane(b14, 0);
            const uint64_t Lq =
                (uint64_t)(lnb == 4 ? b0 : b0 & ((1u << (8 * lnb)) - 1)) + 1;
            const uint32_t h0 = 1 + lnb;
            if (slen - (s + h0) < Lq || dlen - d < Lq) {
                irregular = true; // the sequential decoder names the error
                break;
            }
            R.flush_partial(d);
            wave_copy<false>(dst + d, src + s + h0, Lq, lane);
            s += h0 + (uint32_t)Lq;
            d += (uint32_t)Lq;
            R.gflush = d;
            ring_lo = d; // these bytes are not in the ring
            have = false;
            continue;
        }
        // (K is a prefix of the lanes)
        const uint32_t nK = (uint32_t)__builtin_popcountll(K);
        const uint32_t W = rdlane(incl, nK - 1);       // output of the window
        const uint32_t cur = rdlane(pos, nK - 1) + rdlane(enc, nK - 1);
        const uint32_t dstp = d + (incl - o);          // element's position
        // reference checks :209-217 (dst side), :245-250, :327-332
        const uint64_t M_cpy = K & ~M_lit;
        if (W > dlen - d ||
            (M_cpy & (__ballot(off == 0) | __ballot(off > dstp))) != 0) {
            irregular = true;
            break;
        }
        PROF(
        x.n_elem += nK;
        )
        // next window's tags: issued now, consumed after the copy step
        uint32_t tgn[kG3];
        const bool have_next = slen - (s + cur) >= kTail3;
        if (have_next) {
#pragma unroll
            for (uint32_t g = 0; g < kG3; g++)
                tgn[g] = win_src[cur + 64 * g + lane];
        } else {
#pragma unroll
            for (uint32_t g = 0; g < kG3; g++)
                tgn[g] = 0;
        }
        // ---- 5. the copy step, in in-order runs ------------------------
        const uint32_t q = dstp - off; // copy source (if cpy)
        const uint32_t qe = q + olen;  // (its end, for a copy that does not
                                       // overlap itself)
        // (whole 16-byte pieces are stored: up to 15 bytes behind the window's
        // output may be clobbered too)
        const uint32_t dW = d + W + 16;
        uint32_t safe_lo = dW > kRing2 ? dW - kRing2 : 0;
        safe_lo = safe_lo > ring_lo ? safe_lo : ring_lo;
        const uint64_t M_ring = __ballot(q >= safe_lo);
        // A source in HBM must have been stored, and its 16-byte loads must
        // stay inside the buffer.  Both hold by construction while the ring
        // is whole (a far source ends 1968 bytes or more in front of d, the
        // stores lag d by less than 256); only behind a long literal, whose
        // bytes are not in the ring, must the lanes be asked.
        const bool whole = ring_lo + kRing2 <= dW;
        const uint64_t M_farok =
            whole ? ~0ull
                  : (dlen >= 64 ? __ballot(qe <= R.gflush) &
                                      __ballot(q <= dlen - 64)
                                : 0);
        // LATE elements are moved one by one, in stream order, by the whole
        // wave, after everything else: copies that read this window's own
        // output (qe > d: that includes a copy that overlaps itself) and
        // sources neither in the ring nor stored.  (2.3 per window on text,
        // 8 on html: a loop of in-order RUNS of lanes - whole-piece stores
        // per run - was measured first and cost the scalar unit five times
        // as much per dependent element.)
        const uint64_t M_late =
            M_cpy & (__ballot(qe > d) | ~(M_ring | M_farok));
        const uint64_t M_lw = K & ~M_late; // copied by their own lanes, now
        // an element's own bytes wrap around the ring's end only in a
        // window whose output does (uniform)
        const uint32_t r0 = d & (kRing2 - 1);
        const bool wraps = r0 + W > kRing2;
        const uint64_t M_far = M_lw & M_cpy & ~M_ring; // source in HBM
        const uint64_t M_rng = M_lw & M_cpy & M_ring;  // ... in the ring
        // The first piece of every element whose source is not in the ring:
        // literal bytes are here already (lit16); far sources are an L2 miss
        // each (64 bytes from HBM or the MALL, a microsecond or two), and
        // that latency is what a wave waits for most - all of them at once.
        B16x v0 = lit16;
        if (M_far) {
            PROF(
            x.n_far += __builtin_popcountll(M_far);
            )
            // sources in HBM must be completed stores
            if ((M_far & __ballot(qe > R.fenced)) != 0) {
                R.fence_for(0xFFFFFFFFu);
                COUNT(x.n_fence);
            }
            if (__builtin_amdgcn_inverse_ballot_w64(M_far))
                __builtin_memcpy(&v0, dst + q, 16);
        }
        // Every lane stores WHOLE 16-byte pieces with one ds_write_b128 per
        // trip, last piece first; the excess of a short element lands on
        // the elements behind it - higher lanes of the same instruction,
        // which win (see decode_windows2), or late elements, which are
        // written afterwards.
        const uint64_t M_g16 = M_lw & __ballot(olen > 16);
        if (!wraps && M_g16 == 0) {
            // the usual window: one piece per element, no wrap
            COUNT(x.n_trip);
            B16x v = v0;
            if (__builtin_amdgcn_inverse_ballot_w64(M_rng))
                __builtin_memcpy(&v, rg + (q & (kRing2 - 1)), 16);
            if (__builtin_amdgcn_inverse_ballot_w64(M_lw))
                __builtin_memcpy(rg + (dstp & (kRing2 - 1)), &v, 16);
        } else {
            const uint32_t top =
                M_g16 == 0 ? 0
                           : ((M_g16 & __ballot(olen > 48))
                                  ? 48
                                  : ((M_g16 & __ballot(olen > 32)) ? 32 : 16));
            for (uint32_t c = top;; c -= 16) {
                const uint64_t M_actc =
                    c == 0 ? M_lw : M_lw & __ballot(c < olen);
                if (M_actc != 0) {
                    COUNT(x.n_trip);
                    B16x v = v0;
                    if (c != 0) {
                        if (__builtin_amdgcn_inverse_ballot_w64(M_actc & M_lit))
                            __builtin_memcpy(&v, win_src + (pos + 1 + c), 16);
                        if ((M_actc & M_far) != 0 &&
                            __builtin_amdgcn_inverse_ballot_w64(M_actc & M_far))
                            __builtin_memcpy(&v, dst + (q + c), 16);
                    }
                    if (__builtin_amdgcn_inverse_ballot_w64(M_actc & M_rng))
                        __builtin_memcpy(&v, rg + ((q + c) & (kRing2 - 1)),
                                         16);
                    const uint32_t wa = (dstp + c) & (kRing2 - 1);
                    // (rare) the element's own bytes wrap around the ring's
                    // end: those lanes store bytewise, after the others
                    uint64_t M_strad = 0;
                    uint32_t m = 16;
                    if (wraps) {
                        m = olen - c < 16 ? olen - c : 16;
                        M_strad = M_actc & __ballot(wa + m > kRing2);
                    }
                    if (__builtin_amdgcn_inverse_ballot_w64(M_actc & ~M_strad))
                        __builtin_memcpy(rg + wa, &v, 16); // may reach the mirror
                    if (M_strad != 0 &&
                        __builtin_amdgcn_inverse_ballot_w64(M_strad)) {
                        for (uint32_t j = 0; j < m; j++) {
                            const uint64_t part = j < 8 ? v.lo : v.hi;
                            rg[(wa + j) & (kRing2 - 1)] =
                                (uint8_t)(part >> (8 * (j & 7)));
                        }
                    }
                }
                if (c == 0)
                    break;
            }
        }
        // the late elements: lane k = byte k of the element (exactly its
        // bytes, addressed bytewise: no mirror)
        uint64_t late = M_late;
        if ((M_late & ~M_ring) == 0) {
            // (the usual case: every late source is in the ring)
            while (late) {
                COUNT(x.n_dep);
                const uint32_t i = (uint32_t)__builtin_ctzll(late);
                late &= late - 1;
                const uint32_t F = rdlane(dstp, i), ni = rdlane(olen, i);
                const uint32_t qi = rdlane(q, i), oi = F - qi;
                uint32_t kk = lane;
                if (oi < ni) { // overlapping: byte k repeats byte k mod oi
                    const uint32_t quo = (uint32_t)(
                        ((float)lane + 0.5f) *
                        __builtin_amdgcn_rcpf((float)oi));
                    kk = lane - quo * oi;
                }
                if (lane < ni)
                    rg[(F + lane) & (kRing2 - 1)] =
                        rg[(qi + kk) & (kRing2 - 1)];
            }
        }
        while (late) {
            COUNT(x.n_dep);
            const uint32_t i = (uint32_t)__builtin_ctzll(late);
            late &= late - 1;
            const uint32_t F = rdlane(dstp, i), ni = rdlane(olen, i);
            const uint32_t qi = rdlane(q, i), oi = F - qi;
            uint32_t kk = lane;
            if (oi < ni) { // overlapping: byte k repeats byte k mod oi
                const uint32_t quo = (uint32_t)(
                    ((float)lane + 0.5f) * __builtin_amdgcn_rcpf((float)oi));
                kk = lane - quo * oi;
            }
            const bool in_ring = qi >= safe_lo;
            if (!in_ring) {
                const uint32_t nsrc = ni < oi ? ni : oi;
                // bytes the ring has lost that are not stored yet (only
                // right after a long literal): store them first
                if (qi + nsrc > R.gflush)
                    R.flush_partial(F);
                if (qi + nsrc > R.fenced) {
                    R.fence_for(0xFFFFFFFFu);
                    COUNT(x.n_fence);
                }
            }
            if (lane < ni) {
                const uint32_t val =
                    in_ring ? (uint32_t)rg[(qi + kk) & (kRing2 - 1)]
                            : (uint32_t)dst[qi + kk];
                rg[(F + lane) & (kRing2 - 1)] = (uint8_t)val;
            }
        }
        // the mirror for the next window (see decode_windows2)
        if (r0 < 16 || r0 + W + 16 > kRing2)
            R.mirror();
        // ---- 6. advance; whole 256-byte pieces go to HBM -----------------
        d += W;
        s += cur;
#pragma unroll
        for (uint32_t g = 0; g < kG3; g++)
            tg[g] = tgn[g];
        have = have_next;
        R.flush_chunks(d);
    }
    x.s = s;
    x.d = d;
    x.ring_lo = ring_lo;
    return irregular;
}
} // namespace

// ---------------------------------------------------------------------
// Tiny streams, one per LANE: the reference's loop (src/decompress.rs:75-95,
// 130-343) as it stands, every lane on a stream of its own.  A wavefront per
// stream spends ten microseconds of dependent round trips (descriptors,
// header, first window, flush) on a stream of 150 bytes; here 64 streams
// share them.  Literals move 16 bytes at a time where both buffers allow it,
// copies bytewise (they may overlap).  Errors and their fields are the
// reference's, lane by lane.
// ---------------------------------------------------------------------
namespace {
#define SNAPMI_TINY_FAIL(kind, fa, fb, fc)                                    \
    do {                                                                      \
        set_error(a.errs, st, (kind), (fa), (fb), (fc));                      \
        a.out_lens[st] = 0;                                                   \
        return;                                                               \
    } while (0)

__device__ __forceinline__ void decode_tiny(const DecompressArgs &a,
                                            const uint64_t st)
{
    gcptr in = (gcptr)a.in_ptrs[st];
    const uint64_t in_len = a.in_lens[st];
    gptr dst = (gptr)a.out_ptrs[st];
    const uint32_t mode = a.modes ? a.modes[st] : 0;
    const uint64_t cap = a.out_caps[st];
    if (mode == 3)
        return; // another launch decodes this stream
    if (mode == 1) { // stored frame chunk (reference src/read.rs:173-199)
        if (in_len > cap)
            SNAPMI_TINY_FAIL(SNAPMI_BUFFER_TOO_SMALL, cap, in_len, 0);
        for (uint64_t i = 0; i < in_len; i++)
            dst[i] = in[i];
        set_error(a.errs, st, SNAPMI_OK, 0, 0, 0);
        a.out_lens[st] = in_len;
        return;
    }
    uint32_t hdr = 0;
    uint64_t dst_len = 0;
    if (mode == 2) { // headerless piece: exactly out_caps bytes
        dst_len = cap;
    } else {
        if (in_len == 0)
            SNAPMI_TINY_FAIL(SNAPMI_EMPTY, 0, 0, 0);
        if (read_header(in, in_len, &hdr, &dst_len, a.errs, st) != SNAPMI_OK) {
            a.out_lens[st] = 0;
            return;
        }
        if (dst_len > cap)
            SNAPMI_TINY_FAIL(SNAPMI_BUFFER_TOO_SMALL, cap, dst_len, 0);
    }
    gcptr src = in + hdr;
    const uint64_t src_len = in_len - hdr;
    uint64_t s = 0, d = 0;
    while (s < src_len) {
        const uint32_t tag = src[s];
        s += 1;
        if ((tag & 3) == 0) {
            // read_literal, src/decompress.rs:161-228
            uint64_t len = (tag >> 2) + 1;
            if (len >= 61) {
                if (s + 4 > src_len)
                    SNAPMI_TINY_FAIL(SNAPMI_LITERAL, 4, src_len - s,
                                     dst_len - d);
                const uint32_t nb = (uint32_t)len - 60;
                const uint32_t raw = ld32u(src + s);
                len = (uint64_t)(nb == 4 ? raw
                                         : raw & ((1u << (8 * nb)) - 1)) +
                      1;
                s += nb;
            }
            if (src_len - s < len || dst_len - d < len)
                SNAPMI_TINY_FAIL(SNAPMI_LITERAL, len, src_len - s,
                                 dst_len - d);
            uint64_t i = 0;
            for (; i + 16 <= len; i += 16) {
                const u32x4 t = ld128g(src + s + i);
                __builtin_memcpy(dst + d + i, &t, 16);
            }
            for (; i < len; i++)
                dst[d + i] = src[s + i];
            s += len;
            d += len;
        } else {
            // read_copy + TagEntry::offset, src/decompress.rs:233-343,433-474
            const uint32_t kind = tag & 3;
            const uint32_t nb = kind == 1 ? 1 : (kind == 2 ? 2 : 4);
            const uint32_t len =
                kind == 1 ? 4 + ((tag >> 2) & 7) : 1 + (tag >> 2);
            uint64_t offset = kind == 1 ? (uint64_t)(tag >> 5) << 8 : 0;
            if (s + nb > src_len)
                SNAPMI_TINY_FAIL(SNAPMI_COPY_READ, nb, src_len - s, 0);
            uint32_t v = 0;
            for (uint32_t k = 0; k < nb; k++)
                v |= (uint32_t)src[s + k] << (8 * k);
            offset |= v;
            s += nb;
            if (d <= offset - 1) // wrapping, also catches offset == 0
                SNAPMI_TINY_FAIL(SNAPMI_OFFSET, offset, d, 0);
            const uint64_t end = d + len;
            if (end > dst_len)
                SNAPMI_TINY_FAIL(SNAPMI_COPY_WRITE, len, dst_len - d, 0);
            // (bytewise and in order: the source may overlap the
            // destination; a lane's own stores are visible to its loads)
            for (uint32_t k = 0; k < len; k++)
                dst[d + k] = dst[d - offset + k];
            d = end;
        }
    }
    if (d != dst_len)
        SNAPMI_TINY_FAIL(SNAPMI_HEADER_MISMATCH, dst_len, d, 0);
    set_error(a.errs, st, SNAPMI_OK, 0, 0, 0);
    a.out_lens[st] = dst_len;
}
} // namespace

// 8 waves per SIMD (64 VGPRs, 5 KiB of LDS each): a window is a chain of
// LDS / HBM round trips, and two more waves to switch to are worth more than
// a few spilled dwords (36.0 -> 32.2 ms at cfg2 for the second generation).
#define SNAPMI_DEC2_WAVES 8
__attribute__((amdgpu_waves_per_eu(SNAPMI_DEC2_WAVES, SNAPMI_DEC2_WAVES)))
__global__ __launch_bounds__(64) void k_decompress_streams3(DecompressArgs a)
{
    // the ring, its 16-byte mirror, the compaction table (+ 64 bytes that
    // take the writes of lanes without an element)
    __shared__ __attribute__((aligned(16)))
    uint8_t ring_mem[kRing2 + 16 + 64 * kG3 + 64];
    const uint32_t lane = threadIdx.x;
    if (a.gate && uni64(*a.gate) != a.gate_value)
        return;
    // workgroups [0, n_big): one stream each; the tiny streams behind them
    // (the sort put them last) are k_decompress_tiny's, one per LANE
    if (blockIdx.x >= uni(a.bucket_pos[64]))
        return;
    Wide x;
    if (!open_stream(a, lane, x, (l_u8 *)ring_mem, blockIdx.x))
        return;
    bool irregular = x.too_big();
    if (!irregular)
        irregular = decode_windows3(x, lane, (l_u8 *)ring_mem + kRing2 + 16);
    if (!irregular)
        irregular = decode_windows2(x, lane);
    close_stream(a, lane, x, irregular);
}

// The same decoder for batches of millions of streams: a workgroup takes
// kManyStreams positions of the sorted order, so the dispatcher hands out a
// sixteenth of the workgroups - at 10.7 M streams of 200 bytes, all of them
// k_decompress_tiny's, the 10.7 M empty workgroups of the launch above were
// 1.1 ms of a 4.4 ms pass.  The positions are a whole grid apart (workgroup w:
// w, w + G, w + 2G ...): every workgroup starts with one of the G longest
// streams and gets one of every size stratum, so a few giant streams in such
// a batch do not end up behind each other in one wavefront.
// (No occupancy attribute: the loop around the body costs registers, and held
// to 64 VGPRs it spills; four wavefronts per SIMD are plenty for streams that
// small.)
__global__ __launch_bounds__(64) void k_decompress_streams3_many(
    DecompressArgs a)
{
    __shared__ __attribute__((aligned(16)))
    uint8_t ring_mem[kRing2 + 16 + 64 * kG3 + 64];
    const uint32_t lane = threadIdx.x;
    if (a.gate && uni64(*a.gate) != a.gate_value)
        return;
    const uint32_t n_big = uni(a.bucket_pos[64]);
    for (uint32_t j = 0; j < kManyStreams; j++) {
        const uint32_t slot = blockIdx.x + j * gridDim.x;
        if (slot >= n_big)
            return;
        Wide x;
        if (!open_stream(a, lane, x, (l_u8 *)ring_mem, slot))
            continue;
        bool irregular = x.too_big();
        if (!irregular)
            irregular =
                decode_windows3(x, lane, (l_u8 *)ring_mem + kRing2 + 16);
        if (!irregular)
            irregular = decode_windows2(x, lane);
        close_stream(a, lane, x, irregular);
    }
}

#ifdef SNAPMI_TESTING // (libsnapmi_test.so only)
// The second generation alone (option decode_kernel = 2): kept as the
// cross-check every decoder parity test also runs through.
__attribute__((amdgpu_waves_per_eu(SNAPMI_DEC2_WAVES, SNAPMI_DEC2_WAVES)))
__global__ __launch_bounds__(64) void k_decompress_streams2(DecompressArgs a)
{
    __shared__ __attribute__((aligned(16))) uint8_t ring_mem[kRing2 + 16];
    const uint32_t lane = threadIdx.x;
    if (a.gate && uni64(*a.gate) != a.gate_value)
        return;
    Wide x;
    if (!open_stream(a, lane, x, (l_u8 *)ring_mem, blockIdx.x))
        return;
    const bool irregular = x.too_big() || decode_windows2(x, lane);
    close_stream(a, lane, x, irregular);
}
#endif

// The reference's loop alone, one element at a time (option decode_kernel =
// 0): what a context falls back to when the self-check of the LDS store
// order fails, and a third opinion for the tests.
__global__ __launch_bounds__(64) void k_decompress_sequential(DecompressArgs a)
{
    __shared__ __attribute__((aligned(16))) uint8_t ring_mem[16];
    const uint32_t lane = threadIdx.x;
    if (a.gate && uni64(*a.gate) != a.gate_value)
        return;
    Wide x;
    if (!open_stream(a, lane, x, (l_u8 *)ring_mem, blockIdx.x))
        return;
    decode_sequential(a, x.st, lane, x.src, x.src_len, x.dst, x.dst_len, 0, 0);
}

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
    uint32_t s = 0, d = 0;
    while (s < slen) {
        const uint32_t tag = bin[at(s)];
        s += 1;
        if ((tag & 3) == 0) {
            uint32_t len = (tag >> 2) + 1;
            if (len >= 61) {
                if (s + 4 > slen)
                    SNAPMI_TINY_FAIL(SNAPMI_LITERAL, 4, slen - s, dlen - d);
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
                    SNAPMI_TINY_FAIL(SNAPMI_LITERAL, l64, slen - s, dlen - d);
                len = (uint32_t)l64;
            } else if (slen - s < len || dlen - d < len) {
                SNAPMI_TINY_FAIL(SNAPMI_LITERAL, len, slen - s, dlen - d);
            }
            for (uint32_t k = 0; k < len; k++)
                bout[at(d + k)] = bin[at(s + k)];
            s += len;
            d += len;
        } else {
            const uint32_t kind = tag & 3;
            const uint32_t nb = kind == 1 ? 1 : (kind == 2 ? 2 : 4);
            const uint32_t len =
                kind == 1 ? 4 + ((tag >> 2) & 7) : 1 + (tag >> 2);
            uint64_t offset = kind == 1 ? (uint64_t)(tag >> 5) << 8 : 0;
            if (s + nb > slen)
                SNAPMI_TINY_FAIL(SNAPMI_COPY_READ, nb, slen - s, 0);
            uint32_t v = 0;
            for (uint32_t k = 0; k < nb; k++)
                v |= (uint32_t)bin[at(s + k)] << (8 * k);
            offset |= v;
            s += nb;
            if (d <= offset - 1) // wrapping, also catches offset == 0
                SNAPMI_TINY_FAIL(SNAPMI_OFFSET, offset, d, 0);
            if (d + len > dlen)
                SNAPMI_TINY_FAIL(SNAPMI_COPY_WRITE, len, dlen - d, 0);
            const uint32_t from = d - (uint32_t)offset;
            for (uint32_t k = 0; k < len; k++)
                bout[at(d + k)] = bout[at(from + k)];
            d += len;
        }
    }
    if (d != dlen)
        SNAPMI_TINY_FAIL(SNAPMI_HEADER_MISMATCH, dlen, d, 0);
    gptr dst = (gptr)a.out_ptrs[st];
    {
        uint32_t k = 0;
        for (; k + 4 <= dlen; k += 4)
            st32u(dst + k, *(const l_u32t *)(bout + at(k)));
        for (; k < dlen; k++)
            dst[k] = bout[at(k)];
    }
    set_error(a.errs, st, SNAPMI_OK, 0, 0, 0);
    a.out_lens[st] = dlen;
}

__global__ __launch_bounds__(64) void k_decompress_tiny(DecompressArgs a)
{
    if (a.gate && uni64(*a.gate) != a.gate_value)
        return;
    decompress_lane_streams<kTinyLog2, kWave>(a, uni(a.bucket_pos[65]),
                                               a.n_streams);
}

// The libsnappy seam's single-launch path (snapmi_api.hip, seam_tiny): ONE
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
