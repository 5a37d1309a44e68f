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

struct snapmi_host_pipe; // snapmi_frame.hip: staging of the host-buffer calls

struct snapmi_ctx {
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
    // slices of the host-buffer frame calls: input bytes per encode slice,
    // data chunks per decode slice
    // (measured, profiles/r3_host_pipeline.txt: the match finder's latency
    // floor wants two slices for 4 GiB, the decoder is happy from 0.5 GiB)
    uint64_t host_encode_slice = 2048ull << 20;
    uint64_t host_decode_slice_chunks = 8192;
    // results go home by a copy kernel (bit 0: decode, bit 1: encode) or by
    // hipMemcpyAsync: see k_to_host.  The kernel is used only when the
    // caller's buffer is pinned, device-mapped host memory
    // (snapmi_host_alloc).  Encode: off - the copy kernel would wait for the
    // match finder's persistent workgroups.
    int host_copy_kernel = 1;
    // the host-memory batch calls (snapmi_hostbatch.hip): input bytes per
    // slice; streams of at least host_batch_direct_min bytes are copied to
    // the device from where they lie instead of through the pinned staging;
    // 1: k_hb_pack stores a compress slice's packed output straight into
    // pinned host memory, 0: into device memory, followed by one D2H
    // (measured, profiles/host_batch.json; the last two are test options)
    uint64_t host_batch_slice = 16ull << 20;
    uint64_t host_batch_direct_min = 1ull << 20;
    int host_batch_pack_to_host = 1;
    // 1: a slice of snapmi_frame_decompress_batch_host whose streams the host
    // found well-formed sends its chunk list along and the device does not
    // walk (k_fbd_from_list); 0: the device always walks (test option)
    int host_batch_listed = 1;
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
    bool lane_table_spread = true; // spread the tables over free memory
    bool lane_tables_top = false;  // placed by snapmi_ctx_prepare(TOP_OF_MEMORY)
    // SNAPMI_COMPRESS=waves|lanes|both: 0 = wavefront kernel only, 1 = lane
    // kernel on large batches and the wavefront kernel on small ones
    // (default), 2 = on large batches both kernels at once, sharing one
    // two-ended ticket (no faster: the wavefront kernel takes whole CUs' LDS
    // away from the lanes' input windows; kept as a cross-check)
    int compress_mode = 1;
    // k_compress_spans on more blocks than it has wavefronts: 1 (default) the
    // order of the blocks is chosen as the launch goes (SpanSched,
    // snapmi_compress.hip), 0 ticket order, 2 scheduled whatever the count
    int span_schedule = 1;
    snapmi::ScratchDev sched;
    // 1: lane-kernel launches of at least lane_coresident_min_blocks blocks
    // run k_match_both - three lane wavefronts and two window wavefronts on
    // every CU, one two-ended ticket
    // (cfg2, 146 700 blocks: 115.6 -> 108.4 ms for the match finder; at 4 GiB
    // a draw, below that the lanes have taken every block before a window
    // wavefront has finished one: profiles/r5_coresident.txt)
    int lane_coresident = 1;
    uint64_t lane_coresident_min_blocks = 98304;
    const char *last_kernel = "";
    // 1: blocks of at most 8 KiB go to the window kernel with 16 KiB tables
    // (k_match_spans_8k: 10 wavefronts per CU) when the batch has at least
    // small_table_min_blocks of them
    int small_table_kernel = 1;
    uint64_t small_table_min_blocks = 256;
    // k_compress_block_lds (one block per CU, input block in LDS as well):
    // 1 = for batches of at most two blocks per CU (default), 0 = never,
    // 2 = whenever the wavefront kernel would run (tests)
    int small_batch_kernel = 1;
    // the wavefront-per-block kernels' step: 1 (default) = a window of 63
    // consecutive positions per step, every parse event inside it resolved
    // by a walk over registers (k_compress_spans / k_compress_span_lds);
    // 0 = one copy per step (k_compress_blocks / k_compress_block_lds, the
    // kernels of rounds 1-3: kept as the cross-check)
    int span_kernel = 1;
    // compress_mode 2 ("both"): CUs the wavefront kernel's persistent
    // workgroups take (each owns a CU's whole LDS, so the lane kernel's
    // wavefronts run on the others); 0 = half of the CUs
    uint32_t both_wave_cus = 0;
    // 1: the per-batch scratch of the compressor (token arrays: 128 KiB per
    // block of a lane-kernel segment, up to 34 GB; block slots of the
    // wavefront kernels) is given back when the batch's results are waited
    // for (snapmi_ctx_synchronize; the scalar and libsnappy entry points,
    // which wait for their own result) instead of being kept for the next
    // batch.  snapmi_last_timing waits for events only and the host frame
    // calls keep their pipeline's scratch: neither frees.  For a host
    // that compresses now and then and shares the GPU; costs a hipFree /
    // hipMalloc pair per batch.  The lane tables are not scratch: they are
    // bounded by lane_table_budget_pct.
    int release_scratch = 0;
    // the match finder of the token path (large batches, compress_mode 1):
    // 0 = k_match_blocks (a lane per block, hash tables in HBM), 1 =
    // k_match_spans (a wavefront per block, table in LDS, no tables in HBM
    // at all), 2 (default) = by what this context's last batch compressed
    // to: data that does not compress (ratio >= match_spans_ratio_pct) costs
    // a lane three HBM transactions per probe for nothing
    int match_kernel = 2;
    uint32_t match_spans_ratio_pct = 90;
    // the hint: pinned words the last token-path batch posted (compressed
    // bytes, input bytes, its number)
    volatile uint32_t *h_ratio = nullptr;
    uint32_t ratio_seq = 0; // batches posted so far
    // the token pool (CompressArgs::tok_pool): per cent of the worst case it
    // is sized to (option token_pool_pct), what that has grown to behind
    // batches that spilled, the floor in pages (64 MiB: small batches never
    // spill; test option token_pool_min_pages), and what k_redo_spilled
    // posted of the last launch it has finished: pages asked for | blocks
    // spilled | blocks | seq
    uint32_t token_pool_pct = 39, token_pool_now = 0;
    uint32_t token_pool_min_pages = 32768;
    volatile uint32_t *h_tokstat = nullptr;
    uint32_t tokstat_seq = 0, tokstat_seen = 0;
    uint32_t tok_pages_asked = 0, tok_blocks_spilled = 0;
    uint32_t tok_pool_pages_last = 0; // pages of the last launch's pool
    // 1 (default): a lane-kernel launch of at most lane_speculate_max_blocks
    // blocks (and no more blocks than lanes) runs k_match_blocks_spec (a
    // probe's round also fetches the entry of the probe that follows a
    // miss); 0: always the plain kernel.  Measured: -10..15 % at 2 048 ..
    // 16 384 blocks of text, nothing at 32 768 (test option to move the
    // limit: lane_speculate_max_blocks).
    int lane_speculate = 1;
    uint64_t lane_speculate_max_blocks = 24576;
    // The tail of a lane-kernel launch (k_match_blocks, k_match_blocks_spec,
    // the lane wavefronts of k_match_both): once the ticket has run out lanes
    // only finish, memory falls below its random-access rate and a round
    // costs its latency.  lane_tail_probes 2..4: a wavefront that has seen
    // the ticket run out resolves up to that many probes a round from the
    // moment lane_tail_idle_pct per cent of the launch's lanes are out of
    // work (0: from the first round); 0 or 1: never (the rounds of the launch
    // stay what lane_speculate makes them).  Same bytes at every setting.
    // Measured at cfg2, each time in one process on one table placement
    // (profiles/lane_tail.json, the timeline in
    // profiles/lane_tail_timeline.txt): 2 probes from 40 % idle take 2.6 ms
    // off k_match_both's 107.7 and 1.4 off 110.6 on a second box; 3 and 4
    // probes cost more than they save.
    uint32_t lane_tail_probes = 2;
    uint32_t lane_tail_idle_pct = 40;
    // k_compress_tiny (streams of fewer than 256 bytes, one per LANE, all of
    // their state in LDS): 1 = on (default), 0 = such streams are one-block
    // streams of the block kernels (cross-check, and what round 2 measured)
    int tiny_stream_kernel = 1;
    // k_compress_small (streams of 256 bytes and more, a few per wavefront,
    // state in LDS; needs tiny_stream_kernel): 1 = up to 1 023 bytes
    // (default), 2 = up to 2 047 (measured slower than the lane kernel from
    // 1 KiB on), 0 = off
    int small_stream_kernel = 1;
    // batches of more streams than this are decoded by
    // k_decompress_streams3_many (kManyStreams streams per workgroup)
    uint64_t decode_many_min = 1u << 20;
    // the lane kernel's segment is matched in two halves and the first
    // half's tokens are encoded on the side stream meanwhile: 1 = when the
    // segment has at least 1.4 blocks per lane, 0 = never (default: measured
    // SLOWER, 121.6 -> 135 ms at cfg2 - the encoder's streaming traffic under
    // the match finder costs its random accesses far more than the 3.3 ms
    // it hides), 2 = whenever the segment has two blocks (tests)
    int lane_overlap_encode = 0;
    // 1: the lane tables come from hipExtMallocWithFlags(hipDeviceMallocUncached)
    int lane_tables_uncached = 0;
    // 3: k_decompress_streams3 (element per lane, 128-byte windows; default);
    // 2: k_decompress_streams2 (64-byte windows), kept as a cross-check;
    // 0: the sequential decoder alone
    int decode_kernel = 3;
    hipStream_t stream2 = nullptr; // the wavefront kernel's side stream
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    hipEvent_t ev_crc[2] = {nullptr, nullptr}; // frame encode: CRC on stream2
    bool frame_crc_side_stream = true;
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
    int batch_long_streams = 1;
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
    uint64_t range_scratch_bytes = 1ull << 30;
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
    uint64_t write_scratch_bytes = 1ull << 30;
    // test options: "index_build_route" (BuildArgs::route) and the most
    // streams a group of the scan route holds
    uint32_t index_build_route = 0;
    uint32_t index_build_group_streams = 4096;
    // segment size of the long-stream scan: 0 = by size (1 KiB under 256 MiB
    // of long streams, 4 KiB from there), 10 / 12 forced (test option)
    uint32_t stream_seg_log2 = 0;
    uint32_t stream_scan_segs = 0; // test option: 0 = by size
    // frame layer scratch (snapmi_frame.hip)
    snapmi::ScratchDev fr_desc, fr_slots, fr_chunk_off;
    // kept: the CRC32C tables, filled once by ensure_tables
    // (snapmi_frame.hip) when it gives them memory; fr_tables_ready says so
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
    // framed streams of at least this many bytes without a side index get
    // their chunk headers found in parallel (k_fw_*); shorter ones are walked
    uint64_t frame_parallel_walk_min = 4ull << 20;
    uint64_t frame_walk_segment = 32ull << 20; // >= 128 KiB (test knob)
    int num_cus = 0;
    hipEvent_t ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    // measured crossover (profiles/r5_crossover.txt): the corpus round 1.7
    // GiB, alice29.txt 1.15, html 0.55 - 8 192 until the window kernel got
    // its lane-parallel walk in round 5
    uint32_t lane_min_blocks = 20480;
    // blocks per lane-kernel launch: bounds the token scratch (34 GB here)
    uint32_t lane_segment_blocks = 262144;
    uint32_t lane_waves_per_cu = 6; // 24 KiB of LDS per wave
    uint32_t lane_max_waves = 0;    // test knob: cap on lane-kernel waves (0 = none)
    // placements of the lane tables that are timed before one is kept
    // (place_lane_tables in snapmi_lanetables.hip: spread over the budget, then
    // packed behind that, then spread again; a candidate costs one hipMalloc
    // and a 3 ms probe, and the driver wipes what a loser gives back)
    uint32_t lane_table_tries = 2;
    // percent of the free device memory the lane tables (and, while a
    // placement is chosen, their candidates) may hold: the GPU may be shared
    uint32_t lane_table_budget_pct = 33;
    bool lane_table_probe = false; // experiment knob: probe even with 1 try
    uint32_t lane_table_stride_kib = 0; // experiment knob: bytes between tables
    std::string probe_log;          // k_probe_tables ms of every candidate
    // test knob: every lane's table epoch is set to this value before the
    // next lane-kernel launch (-1 = leave the epochs alone); lets a test
    // reach the 16-bit epoch wrap without 65 535 blocks per lane
    int64_t lane_epoch_preset = -1;
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
#ifdef SNAPMI_TESTING
    // test option "scratch_fill" (include/snapmi_test.h): the byte every new
    // allocation is born holding, -1 = off; what the last setting filled
    // (buffers, bytes) and how many of those buffers read back as filled
    int scratch_fill = -1;
    uint64_t fill_buffers = 0, fill_bytes = 0, fill_seen = 0;
#endif
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
