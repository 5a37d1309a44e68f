// snapmi_ctx.hpp -- private: the context object and helpers shared by the
// host-side translation units.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "snapmi.h"
#include "snapmi_options.hpp"

namespace snapmi {

struct DevBuf { // device memory of a context (grow-only)
    void *p = nullptr;
    size_t cap = 0;
    bool listed = false; // in snapmi_ctx::dev_bufs (reserve)
    bool kept = false;   // the class: KeptDev / ScratchDev below
};

struct PinBuf { // pinned, device-mapped host memory (grow-only)
    void *p = nullptr;
    size_t cap = 0;
    bool listed = false; // in snapmi_ctx::pin_bufs (pin_reserve)
    bool kept = false;   // the class: KeptPin / ScratchPin below
};

// Every buffer is declared as one of two classes (the table: DESIGN 4.2b;
// tests/test_scratch_classes_cpu.py holds the two together):
//   Scratch*  every word a call reads was written earlier in the same call -
//             by a memset or a copy on the call's stream, by the host, or by
//             a kernel of the call.  What the buffer held before does not
//             matter: the test build fills these with any byte between calls
//             (test option "scratch_fill") and every result stays the same.
//   Kept*     meaning survives a call.  The declaration says who initialises
//             the buffer and when; a buffer that grows is initialised again.
// reserve, pin_reserve and slot_reserve take the base type and see the class
// in `kept`.
struct ScratchDev : DevBuf {};
struct KeptDev : DevBuf {
    KeptDev() { kept = true; }
};
struct ScratchPin : PinBuf {};
struct KeptPin : PinBuf {
    KeptPin() { kept = true; }
};

// What a range write, or an append, of indexed streams keeps between calls
// (snapmi_update.hip): the device's copy of the host's lists, the named
// streams' states and the blocks' running sums, the two counters of its
// kernels; the pinned staging of the lists with the event of the copy that
// last read it - the next call waits for that event, never for the stream,
// before it writes there again; the blocks that went through the compressor
// and those that were decoded first in the last call; whether it ran its
// kernels.
struct UpdateScratch {
    ScratchDev meta, state, stat;
    ScratchPin pin;
    hipEvent_t ev = nullptr;
    bool ev_live = false;
    uint64_t blocks = 0, decoded = 0;
    bool stats_live = false;
};

} // namespace snapmi

struct snapmi_host_pipe; // snapmi_hostpipe.hip: staging of the host-buffer calls

// (the base: every knob, its default and what it means)
struct snapmi_ctx : snapmi::Options {
    int device = 0;
    snapmi_host_pipe *pipe = nullptr;
    // 256 bytes of pinned, device-mapped host memory: kernels post small
    // results here (no copy-engine round trip behind a bulk copy)
    volatile uint32_t *h_mail = nullptr;
    // what reserve / pin_reserve have given memory to, each once:
    // snapmi_ctx_destroy frees these, "scratch_bytes" sums the first
    std::vector<snapmi::DevBuf *> dev_bufs;
    std::vector<snapmi::PinBuf *> pin_bufs;
    // pinned host staging of the scalar (host-pointer) entry points
    snapmi::ScratchPin pin_in, pin_out, pin_desc;
    // what the last host batch call did: slices, bytes copied each way,
    // slices decoded from the host's chunk list
    uint64_t hb_slices = 0, hb_h2d_bytes = 0, hb_d2h_bytes = 0;
    uint64_t hb_listed_slices = 0;
    hipStream_t stream = nullptr;
    bool owns_stream = false;
    std::string last_error;
    // grow-only device scratch of the raw codec
    snapmi::ScratchDev blk_first, slot_first, blk_size, blk_off, slots,
        plan_part;
    // lane-per-block match finder: tokens, token counts
    snapmi::ScratchDev tokens, tok_pages, tok_stage, ntok;
    // ... and its HBM hash tables with every lane's epoch: kept - an entry of
    // an older epoch counts as empty, so a table is never cleared between
    // blocks.  place_lane_tables (snapmi_lanetables.hip) zeroes both whenever
    // it gives them memory.
    snapmi::KeptDev lane_tables, lane_epochs;
    // lane_tables made of physical chunks (hipMemCreate) mapped into one
    // address range (place_lane_tables, snapmi_lanetables.hip): the chunks and
    // the bytes of the range; empty / 0 when lane_tables.p came from hipMalloc
    std::vector<hipMemGenericAllocationHandle_t> lane_chunks;
    size_t lane_chunk_bytes = 0, lane_va_bytes = 0;
    uint32_t lane_chunk_count = 0, lane_per_chunk = 0; // lane -> table map
    uint32_t n_lanes = 0;
    uint64_t lane_stride = 0;      // 16-byte entries between two lanes' tables
    bool lane_tables_top = false;  // placed by snapmi_ctx_prepare(TOP_OF_MEMORY)
    snapmi::ScratchDev sched;
    const char *last_kernel = "";
    // the hint: pinned words the last token-path batch posted (compressed
    // bytes, input bytes, its number)
    volatile uint32_t *h_ratio = nullptr;
    uint32_t ratio_seq = 0; // batches posted so far
    // the token pool (CompressArgs::tok_pool): what option token_pool_pct has
    // grown to behind batches that spilled, and what k_redo_spilled posted of
    // the last launch it has finished: pages asked for | blocks spilled |
    // blocks | seq
    uint32_t token_pool_now = 0;
    volatile uint32_t *h_tokstat = nullptr;
    uint32_t tokstat_seq = 0, tokstat_seen = 0;
    uint32_t tok_pages_asked = 0, tok_blocks_spilled = 0;
    uint32_t tok_pool_pages_last = 0; // pages of the last launch's pool
    hipStream_t stream2 = nullptr; // the wavefront kernel's side stream
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    hipEvent_t ev_crc[2] = {nullptr, nullptr}; // frame encode: CRC on stream2
    // staging for the host-pointer (scalar) entry points
    snapmi::ScratchDev st_in, st_out, st_desc, st_prof, ticket, order;
    // long-stream decode scratch of snapmi_decompress_stream and of the long
    // streams of a batch (snapmi_streamplan.hpp lays them out): tables,
    // piece descriptors
    snapmi::ScratchDev sd_tables, sd_desc;
    // the long streams of a small batch get their pieces
    // (snapmi_decompress_batch, option batch_long_streams): modes of the
    // batch's own launch and of the one behind, what k_long_plan found; the
    // streams' descriptors and workgroup prefixes (a lone stream's too); pinned
    // staging of the list and of the batch's descriptors
    snapmi::ScratchDev bl_modes, bl_list, bl_descs, bl_order;
    snapmi::ScratchPin pin_bl;
    snapmi::ScratchPin pin_bl2; // descriptors of the long streams of a batch
    // snapmi_decompress_batch_indexed: the modes of the launch behind, the
    // descriptor list (a slot per stream and per index entry), and the gate /
    // counter words of its kernels
    // (IndexArgs::gate); calls so far; whether the last call ran them
    snapmi::ScratchDev ix_modes, ix_desc;
    // kept: gate[3] carries the ix_seq of the last call that handed a stream
    // back, and the launch behind compares it with its own.
    // snapmi_decompress_batch_indexed zeroes the 64 bytes when it first gives
    // them memory (fresh_gate); every call's k_index_plan resets the counters
    snapmi::KeptDev ix_gate;
    uint64_t ix_seq = 0;
    bool ix_stats_live = false;
    // snapmi_decompress_ranges_indexed: the piece descriptors of one group,
    // per-range slots and verdicts, the scans' partial sums, the edge rooms
    // (at most range_scratch_bytes of them) and the two counters of its
    // kernels; pieces the last call's ranges took; whether it ran them
    snapmi::ScratchDev rg_desc, rg_meta, rg_part, rg_room, rg_stat;
    uint64_t rg_pieces = 0;
    bool rg_stats_live = false;
    // snapmi_build_block_index: the device's copies of the host's arrays, the
    // streams' states and the walk list; its five counters; the pinned staging
    // of those copies and of one group's descriptors (two slots, taken in
    // turn), each with the event of the copy that last read it - the call
    // waits for that event, never for the stream, before it writes there
    // again; groups so far; whether the last call ran its kernels
    snapmi::ScratchDev ib_meta, ib_stat;
    snapmi::ScratchPin pin_ib, pin_ibg[2];
    hipEvent_t ev_ib = nullptr, ev_ibg[2] = {nullptr, nullptr};
    bool ev_ib_live = false, ev_ibg_live[2] = {false, false};
    uint64_t ib_groups = 0;
    bool ib_stats_live = false;
    // snapmi_write_ranges_indexed and snapmi_append_indexed
    // (snapmi_update.hip), each its own UpdateScratch: a write's list copy
    // and an append's never wait for each other's event.  What a group of
    // either runs in - the one-block streams of its compress launch, its
    // compress slots, its rooms (slots and rooms together at most
    // write_scratch_bytes a group, unless one stream takes more) and its piece
    // descriptors - is one set: the calls follow each other on the stream.
    snapmi::UpdateScratch wr, ap;
    snapmi::ScratchDev up_z, up_slot, up_room, up_desc;
    // frame layer scratch (snapmi_frame.hip, its layouts: snapmi_frame.hpp)
    snapmi::ScratchDev fr_desc, fr_slots, fr_chunk_off;
    // kept: the CRC32C tables, filled once by ensure_tables
    // (snapmi_crc.hip) when it gives them memory; fr_tables_ready says so
    snapmi::KeptDev fr_tables;
    // snapmi_crc32c_masked_batch: the long buffers' segment scan and
    // accumulators (sized from n alone)
    snapmi::ScratchDev fr_crc;
    // frame decode: per-stream and per-chunk scratch
    snapmi::ScratchDev fb_streams, fb_chunks;
    // the front that decided the last no-wait decode (info
    // "frame_nowait_front"); whether there has been one
    snapmi::ScratchDev fr_nowait;
    bool fr_nowait_live = false;
    bool fr_tables_ready = false;
    int num_cus = 0;
    hipEvent_t ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    std::string probe_log;          // k_probe_tables ms of every candidate
    // ds_mskor_rtn_b32 applies same-address lanes in ascending lane order on
    // this device (checked by k_probe_lds_order at context creation); the
    // wavefront-per-block kernel is only used when this holds
    bool lds_order_ok = false;
    bool lds_order_hw = false;
    // overlapping lanes of one plain DS store land in ascending lane order
    // (same self-check): k_decompress_streams2 needs it
    bool lds_store_order_ok = true; // what the self-check found (the option can only lower it)
    bool timing_valid = false;
    bool timing_is_compress = false;
    bool dominant_split = false; // ev[4]/ev[5] bracket k_match_blocks
    uint64_t codec_launches = 0;
    uint32_t seam_seq = 0; // the seam's single-launch path: its last ticket
    uint32_t prof_tail_lanes = 0; // SNAPMI_PROFILE=3: lanes of the last launch
    // test option "scratch_fill": what the last setting filled (buffers,
    // bytes) and how many of those buffers read back as filled (in the
    // product context too, always 0: kInfo is the same table in both builds)
    uint64_t fill_buffers = 0, fill_bytes = 0, fill_seen = 0;
};

namespace snapmi {

inline int fail_ctx(snapmi_ctx *ctx, int kind, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (ctx)
        ctx->last_error = buf;
    return kind;
}

#define HIP_TRY(ctx, expr)                                                    \
    do {                                                                      \
        hipError_t _e = (expr);                                               \
        if (_e != hipSuccess)                                                 \
            return snapmi::fail_ctx((ctx), SNAPMI_E_DEVICE, "%s failed: %s",  \
                                    #expr, hipGetErrorString(_e));            \
    } while (0)

#ifdef SNAPMI_TESTING
// Test option "scratch_fill": a new allocation of either class holds the
// byte before its owner sees it (a kept buffer's own initialisation comes
// after, as after a real hipMalloc).  Blocking.
inline int fill_new_dev(snapmi_ctx *ctx, DevBuf &b)
{
    if (ctx->scratch_fill < 0)
        return SNAPMI_OK;
    HIP_TRY(ctx, hipMemsetAsync(b.p, ctx->scratch_fill, b.cap, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return SNAPMI_OK;
}
inline void fill_new_pin(snapmi_ctx *ctx, PinBuf &b)
{
    if (ctx->scratch_fill >= 0)
        memset(b.p, ctx->scratch_fill, b.cap);
}
#endif

// (slack: an eighth more than asked for, so that batches that grow a little
// do not reallocate every time - or none, for the token pool, whose size is a
// stated share of the input)
// A buffer is listed in the context the first time it is given memory and
// stays listed, freed or grown: the context's own DevBufs only (a slot of the
// host pipeline has slot_reserve).
inline int reserve(snapmi_ctx *ctx, DevBuf &b, size_t bytes,
                   bool slack = true)
{
    if (bytes <= b.cap)
        return SNAPMI_OK;
    if (b.p) {
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        HIP_TRY(ctx, hipFree(b.p));
        b.p = nullptr;
        b.cap = 0;
    }
    if (!b.listed) {
        ctx->dev_bufs.push_back(&b);
        b.listed = true;
    }
    size_t want = bytes + (slack ? bytes / 8 : 0) + 256;
    HIP_TRY(ctx, hipMalloc(&b.p, want));
    b.cap = want;
#ifdef SNAPMI_TESTING
    return fill_new_dev(ctx, b);
#else
    return SNAPMI_OK;
#endif
}

} // namespace snapmi
