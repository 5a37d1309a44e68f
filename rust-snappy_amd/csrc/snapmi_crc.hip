// snapmi_crc.hip -- masked CRC32C on the device (gfx950): the checksum of the
// frame format's chunks (reference src/crc32.rs) and, for buffers of any
// length, snapmi_crc32c_masked_batch.
//
// Kernels here:
//   k_crc32c          masked CRC32C, one wavefront per buffer, 64 interleaved
//                     partial CRCs advanced 256 bytes per step with 4 LDS
//                     table lookups, combined by GF(2) multiplication
//   k_crc_plan, k_crc_segments, k_crc_finish
//                     the same of buffers of more than 64 KiB, cut into
//                     segments that the whole device shares (snapmi_crc.hpp)
// The frame files reach k_crc32c through launch_crc32c (snapmi_frame.hpp).
#include <hip/hip_runtime.h>

#include <vector>

#include "snapmi.h"
#include "snapmi_ctx.hpp"
#include "snapmi_device.hpp"
#include "snapmi_scan.hpp"
#include "snapmi_crc.hpp"
#include "snapmi_frame.hpp"

using namespace snapmi;

namespace snapmi {

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

// ---------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------
int ensure_tables(snapmi_ctx *ctx)
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

// (a caller checks hipGetLastError behind the launches of its own call)
int launch_crc32c(snapmi_ctx *ctx, hipStream_t st, const void *const *ptrs,
                  const uint64_t *lens, uint32_t *out, uint32_t n)
{
    int rc = ensure_tables(ctx);
    if (rc)
        return rc;
    hipLaunchKernelGGL(k_crc32c, dim3(n), dim3(64), 0, st, ptrs, lens, out, n,
                       (const CrcTables *)ctx->fr_tables.p);
    return SNAPMI_OK;
}

} // namespace snapmi

extern "C" {

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
    CrcLong l;
    Carver measure;
    crc_long_layout(measure, l, n);
    if ((rc = reserve(ctx, ctx->fr_crc, measure.bytes())))
        return rc;
    Carver place(ctx->fr_crc.p);
    crc_long_layout(place, l, n);
    uint64_t *seg_first = l.seg_first;
    uint32_t *acc = l.acc;
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
