// snapmi_launch.hpp -- private: what the host-side units of the raw codec
// share - the launchers (snapmi_launch.hip), the lane tables
// (snapmi_lanetables.hip), the long-stream plan on the device
// (snapmi_longstream.hip) - and what the frame layer calls of them.
#pragma once

#include "snapmi_ctx.hpp"
#include "snapmi_piecelist.hpp"
#include "snapmi_streamplan.hpp"

namespace snapmi {

struct CompressArgs;            // snapmi_kernels.hpp

static_assert(sizeof(snapmi_error) == kPieceErrBytes,
              "snapmi_piecelist.hpp sizes the piece descriptors with it");

#define LAUNCH_CHECK(name)                                                    \
    do {                                                                      \
        hipError_t _e = hipGetLastError();                                    \
        if (_e != hipSuccess)                                                 \
            return fail_ctx(ctx, SNAPMI_E_DEVICE, "launch of " #name ": %s",  \
                            hipGetErrorString(_e));                           \
    } while (0)

// batches of up to this many streams / blocks are planned and scanned by one
// workgroup (one launch instead of three)
constexpr size_t kPlanOneWg = 16384;
// A scan of n items (snapmi_scan.hpp): one() launches the one-workgroup
// kernel, three(parts) the (a) (b) (c) kernels over `parts` workgroups of 1024
// items, for more than kPlanOneWg of them.
template <class One, class Three>
inline void launch_scan(size_t n, One one, Three three)
{
    if (n > kPlanOneWg)
        three((uint32_t)((n + 1023) / 1024));
    else
        one();
}

// pinned host staging of a context (grow-only): pageable copies go through
// the runtime's own staging buffer one at a time, process-wide - eight
// threads calling snappy_compress would queue there
inline int pin_reserve(snapmi_ctx *ctx, PinBuf &b, size_t bytes)
{
    if (bytes <= b.cap)
        return SNAPMI_OK;
    if (b.p) {
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        HIP_TRY(ctx, hipHostFree(b.p));
        b.p = nullptr;
        b.cap = 0;
    }
    if (!b.listed) {
        ctx->pin_bufs.push_back(&b);
        b.listed = true;
    }
    const size_t want = bytes + bytes / 4 + 4096;
    HIP_TRY(ctx, hipHostMalloc(&b.p, want, hipHostMallocDefault));
    b.cap = want;
#ifdef SNAPMI_TESTING
    fill_new_pin(ctx, b);
#endif
    return SNAPMI_OK;
}

void host_pipe_destroy(snapmi_ctx *ctx); // snapmi_hostpipe.hip

// snapmi_api.hip
int release_batch_scratch(snapmi_ctx *ctx);
// reference bytes::read_varu64, src/bytes.rs:73-90
size_t host_varint(const uint8_t *p, size_t n, uint64_t *value);
// host buffers of up to this many bytes go through the context's pinned
// staging (one host memcpy each way, no pageable device copy)
constexpr size_t kPinStage = 8u << 20;
// the scalar calls (snapmi_raw_compress / snapmi_raw_decompress)
int run_one(snapmi_ctx *ctx, bool compress, const uint8_t *input,
            size_t input_len, uint8_t *output, size_t output_cap,
            size_t *written, snapmi_error *err);

// snapmi_lanetables.hip
void free_lane_tables(snapmi_ctx *ctx);
int place_lane_tables(snapmi_ctx *ctx, uint32_t lanes, bool top_of_memory);
int prepare_lane_tables(snapmi_ctx *ctx, uint64_t blocks, bool top);

// snapmi_index.hip: the block index of the batch launch_compress compressed
void launch_block_index(snapmi_ctx *ctx, const CompressArgs &a,
                        uint64_t *d_index_first, uint64_t *d_index,
                        uint64_t index_entries);

// snapmi_launch.hip
// raw compress of n streams; blocks/slots = launch geometry computed from
// the (host-known) stream lengths
int launch_compress(snapmi_ctx *ctx, const void *const *d_in_ptrs,
                    const uint64_t *d_in_lens, void *const *d_out_ptrs,
                    const uint64_t *d_out_caps, uint64_t *d_out_lens,
                    snapmi_error *d_errs, size_t n, uint64_t blocks,
                    uint64_t slots, uint32_t small_classes = 0xF,
                    uint64_t cnt8 = 0, uint64_t block_bytes = 0,
                    // the block index (snapmi_blockindex.hpp), or nullptr
                    uint64_t *d_index_first = nullptr,
                    uint64_t *d_index = nullptr, uint64_t index_entries = 0);
// raw decompress; d_modes optional (1 = stored chunk, plain copy)
int launch_decompress(snapmi_ctx *ctx, const void *const *d_in_ptrs,
                      const uint64_t *d_in_lens, void *const *d_out_ptrs,
                      const uint64_t *d_out_caps, uint64_t *d_out_lens,
                      snapmi_error *d_errs, const uint8_t *d_modes, size_t n,
                      const unsigned long long *d_gate = nullptr,
                      unsigned long long gate_value = 0,
                      // a launch beside the context's stream: its stream and
                      // its own dispatch-order scratch (no timing events)
                      hipStream_t side = nullptr, DevBuf *side_order = nullptr,
                      // no stream of the launch is of the lane-per-stream
                      // classes (under 512 bytes of output): their kernels
                      // are not launched
                      bool wide_only = false);
// ... of the first `count` slots of a piece-descriptor slab
inline int launch_pieces(snapmi_ctx *ctx, const PieceList &l, size_t count,
                         const unsigned long long *d_gate = nullptr,
                         unsigned long long gate_value = 0)
{
    return launch_decompress(ctx, l.c_in, l.c_inlen, l.c_out, l.c_cap,
                             l.c_outlen, l.c_err, l.c_mode, count, d_gate,
                             gate_value);
}

// snapmi_longstream.hip
size_t long_stream_min();
// a stream's own ends, as its descriptor holds them (StreamArgs)
struct StreamEnds {
    const void *in;
    void *out;
    uint64_t out_cap, *out_len;
    snapmi_error *err;
    uint8_t *fb_mode; // a long stream of a batch, else nullptr
};
StreamArgs stream_desc(snapmi_ctx *ctx, const StreamPlan &p,
                       const StreamSlot &g, const StreamEnds *io);
int launch_stream_cuts(snapmi_ctx *ctx, const StreamPlan &p, const void *dev);

} // namespace snapmi
