// snapmi_wide.hip -- the wavefront decoder's kernels: one wavefront per raw
// stream (snapmi_wide.hpp; the window loops: snapmi_wide2.hpp, _wide3.hpp).
#include "snapmi_wide.hpp"
#include "snapmi_wide2.hpp"
#include "snapmi_wide3.hpp"

namespace snapmi {

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

} // namespace snapmi
