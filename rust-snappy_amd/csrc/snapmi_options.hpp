// snapmi_options.hpp -- the knobs of a context: their fields and defaults
// (Options, which snapmi_ctx derives from), the one table of the names the
// two setters accept with the values each takes, and the names of
// snapmi_ctx_get_info.  Host only, no HIP: tests/options_host.cpp walks them.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>

namespace snapmi {

struct Options {
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
    bool lane_table_spread = true; // spread the tables over free memory
    // SNAPMI_COMPRESS=waves|lanes|both: 0 = wavefront kernel only, 1 = lane
    // kernel on large batches and the wavefront kernel on small ones
    // (default), 2 = on large batches both kernels at once, sharing one
    // two-ended ticket (no faster: the wavefront kernel takes whole CUs' LDS
    // away from the lanes' input windows; kept as a cross-check)
    int compress_mode = 1;
    // k_compress_spans on more blocks than it has wavefronts: 1 (default) the
    // order of the blocks is chosen as the launch goes (SpanSched,
    // snapmi_window.hip), 0 ticket order, 2 scheduled whatever the count
    int span_schedule = 1;
    // 1: lane-kernel launches of at least lane_coresident_min_blocks blocks
    // run k_match_both - three lane wavefronts and two window wavefronts on
    // every CU, one two-ended ticket
    // (cfg2, 146 700 blocks: 115.6 -> 108.4 ms for the match finder; at 4 GiB
    // a draw, below that the lanes have taken every block before a window
    // wavefront has finished one: profiles/r5_coresident.txt)
    int lane_coresident = 1;
    uint64_t lane_coresident_min_blocks = 98304;
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
    // the token pool (CompressArgs::tok_pool): per cent of the worst case it
    // is sized to (what that has grown to behind batches that spilled is the
    // context's token_pool_now) and the floor in pages (64 MiB: small batches
    // never spill; a test option)
    uint32_t token_pool_pct = 39;
    uint32_t token_pool_min_pages = 32768;
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
    bool frame_crc_side_stream = true; // frame encode: CRC on the side stream
    int batch_long_streams = 1; // snapmi_decompress_batch: 0 = only enqueues
    uint64_t range_scratch_bytes = 1ull << 30; // of a range call's edge rooms
    uint64_t write_scratch_bytes = 1ull << 30; // of a group's slots and rooms
    // test options: "index_build_route" (BuildArgs::route) and the most
    // streams a group of the scan route holds
    uint32_t index_build_route = 0;
    uint32_t index_build_group_streams = 4096;
    // segment size of the long-stream scan: 0 = by size (1 KiB under 256 MiB
    // of long streams, 4 KiB from there), 10 / 12 forced (test option)
    uint32_t stream_seg_log2 = 0;
    uint32_t stream_scan_segs = 0; // test option: 0 = by size
    // framed streams of at least this many bytes without a side index get
    // their chunk headers found in parallel (k_fw_*); shorter ones are walked
    uint64_t frame_parallel_walk_min = 4ull << 20;
    uint64_t frame_walk_segment = 32ull << 20; // >= 128 KiB (test knob)
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
    // test knob: every lane's table epoch is set to this value before the
    // next lane-kernel launch (-1 = leave the epochs alone); lets a test
    // reach the 16-bit epoch wrap without 65 535 blocks per lane
    int64_t lane_epoch_preset = -1;
    // test option "scratch_fill": the byte every new allocation is born
    // holding, -1 = off (read by the test build only; a field of both builds)
    int scratch_fill = -1;
};

// One entry per accepted name.  A value is accepted when it lies in the
// build's interval - [lo, hi] in the product library, [test_lo, test_hi] in
// the test build (SNAPMI_TESTING), wider for the three cross-checks - and,
// where the accepted set is no interval, `member` agrees.  Two names have no
// field: "lds_order_ok" lowers a device fact of the context and
// "lane_tables_renew" acts at once (snapmi_api.hip).
struct OptionDesc {
    const char *name;
    void (*store)(Options &, int64_t);
    int64_t (*load)(const Options &);
    bool test_only; // a name of snapmi_ctx_set_test_option
    int64_t lo, hi, test_lo, test_hi;
    bool (*member)(int64_t value, bool test_build);
};

constexpr int64_t kOptAny = INT64_MAX; // no upper bound
// kSlotBytes + kMaxBlock, a block's slot and room (tied in snapmi_api.hip)
constexpr int64_t kOptWriteScratchMin = 142032;

#define FIELD(f)                                                              \
    #f, [](Options &o, int64_t v) { o.f = (decltype(o.f))v; },                \
        [](const Options &o) { return (int64_t)o.f; }
#define OPT(f, lo, hi) {FIELD(f), false, lo, hi, lo, hi, nullptr}
#define TEST_OPT(f, lo, hi) {FIELD(f), true, lo, hi, lo, hi, nullptr}
inline constexpr OptionDesc kOptions[] = {
    // snapmi_ctx_set_option (include/snapmi.h)
    {FIELD(compress_mode), false, 0, 1, 0, 2, nullptr},
    OPT(lane_min_blocks, 1, kOptAny),
    OPT(lane_segment_blocks, 64, 0x7FFFFFFF),
    OPT(lane_table_spread, 0, 1),
    OPT(lane_table_tries, 1, 16),
    OPT(lane_table_budget_pct, 1, 90),
    OPT(token_pool_pct, 1, 100),
    OPT(token_pool_min_pages, 0, 0x7FFFFFFF),
    OPT(span_schedule, 0, 2),
    OPT(lane_coresident, 0, 1),
    OPT(lane_coresident_min_blocks, 1, kOptAny),
    OPT(small_table_kernel, 0, 1),
    OPT(small_table_min_blocks, 1, kOptAny),
    OPT(small_batch_kernel, 0, 2),
    OPT(lane_speculate, 0, 1),
    OPT(lane_tail_probes, 0, 4),
    OPT(lane_tail_idle_pct, 0, 100),
    {FIELD(span_kernel), false, 1, 1, 0, 1, nullptr},
    OPT(match_kernel, 0, 2),
    OPT(match_spans_ratio_pct, 1, 200),
    OPT(release_scratch, 0, 1),
    OPT(batch_long_streams, 0, 1),
    OPT(both_wave_cus, 0, 4096),
    OPT(tiny_stream_kernel, 0, 1),
    OPT(small_stream_kernel, 0, 2),
    OPT(frame_parallel_walk_min, 0, kOptAny),
    OPT(host_copy_kernel, 0, 3),
    OPT(host_encode_slice, 65536, kOptAny),
    OPT(host_decode_slice_chunks, 1, kOptAny),
    OPT(host_batch_slice, 65536, kOptAny),
    OPT(range_scratch_bytes, 128 << 10, kOptAny),
    OPT(write_scratch_bytes, kOptWriteScratchMin, kOptAny),
    // (stored as 0 on a device that failed the DS store order self-check)
    {FIELD(decode_kernel), false, 0, 3, 0, 3,
     [](int64_t v, bool test) { return v == 0 || v == 3 || (v == 2 && test); }},
    // snapmi_ctx_set_test_option (include/snapmi_test.h)
    TEST_OPT(lane_waves_per_cu, 1, 32),
    TEST_OPT(decode_many_min, 0, kOptAny),
    TEST_OPT(lane_speculate_max_blocks, 0, kOptAny),
    TEST_OPT(lane_max_waves, 0, 0x7FFFFFFF),
    TEST_OPT(frame_crc_side_stream, 0, 1),
    TEST_OPT(lane_tables_uncached, 0, 1),
    TEST_OPT(lane_overlap_encode, 0, 2),
    TEST_OPT(frame_walk_segment, 128 << 10, kOptAny),
    {FIELD(lane_table_stride_kib), true, 0, 4096, 0, 4096,
     [](int64_t v, bool) { return v == 0 || (v >= 256 && v % 4 == 0); }},
    TEST_OPT(lane_table_probe, 0, 1), // time the placement even if 1 try
    {"lane_tables_renew", nullptr, nullptr, true, 1, 1, 1, 1, nullptr},
    TEST_OPT(lane_epoch_preset, -1, 0xFFFF),
    TEST_OPT(index_build_route, 0, 2),
    TEST_OPT(index_build_group_streams, 1, 4096),
    {FIELD(stream_seg_log2), true, 0, 12, 0, 12,
     [](int64_t v, bool) { return v == 0 || v == 10 || v == 12; }},
    {FIELD(stream_scan_segs), true, 0, 64, 0, 64,
     [](int64_t v, bool) { return v == 0 || (v >= 8 && (v & (v - 1)) == 0); }},
    {"lds_order_ok", nullptr, nullptr, true, 0, 1, 0, 1, nullptr},
    TEST_OPT(host_batch_direct_min, 0, kOptAny),
    TEST_OPT(host_batch_pack_to_host, 0, 1),
    TEST_OPT(host_batch_listed, 0, 1),
    TEST_OPT(scratch_fill, -1, 255),
};
#undef TEST_OPT
#undef OPT
#undef FIELD

template <class T, size_t N>
const T *find_named(const T (&table)[N], const char *name)
{
    for (const T &e : table)
        if (strcmp(name, e.name) == 0)
            return &e;
    return nullptr;
}

enum class OptionSet { accepted, unknown_name, refused_value };

// What both setters do with (name, value): test_entry_point says which of
// them is asking - each knows its own names only -, test_build which library.
// Stores an accepted value in its field, if the name has one.
inline OptionSet option_set(Options &o, const char *name, int64_t value,
                            bool test_entry_point, bool test_build)
{
    const OptionDesc *d = find_named(kOptions, name);
    if (!d || d->test_only != test_entry_point)
        return OptionSet::unknown_name;
    const int64_t lo = test_build ? d->test_lo : d->lo;
    const int64_t hi = test_build ? d->test_hi : d->hi;
    if (value < lo || value > hi ||
        (d->member && !d->member(value, test_build)))
        return OptionSet::refused_value;
    if (d->store)
        d->store(o, value);
    return OptionSet::accepted;
}

// The names snapmi_ctx_get_info answers (their sources need the context:
// snapmi_api.hip has them, in this order: a static_assert there).
struct InfoName {
    const char *name;
    bool test_only; // answered by the test build only
};
inline constexpr InfoName kInfoNames[] = {
    {"scratch_bytes", false}, {"token_scratch_bytes", false},
    {"token_pool_pages", false}, {"token_pool_pct_now", false},
    {"token_pages_asked", false}, {"token_blocks_spilled", false},
    {"host_batch_slices", false}, {"host_batch_h2d_bytes", false},
    {"host_batch_d2h_bytes", false}, {"host_batch_listed_slices", false},
    {"index_streams_pieced", false}, {"index_streams_fallback", false},
    {"range_pieces", false}, {"range_ranges_ok", false},
    {"range_ranges_failed", false}, {"write_blocks", false},
    {"write_blocks_decoded", false}, {"write_streams_ok", false},
    {"write_streams_failed", false}, {"append_blocks", false},
    {"append_blocks_decoded", false}, {"append_streams_ok", false},
    {"append_streams_failed", false}, {"index_build_built", false},
    {"index_build_unaligned", false}, {"index_build_corrupt", false},
    {"index_build_missized", false}, {"index_build_walked", false},
    {"frame_nowait_front", false}, {"lane_multi_rounds", true},
    {"scratch_fill_buffers", true}, {"scratch_fill_bytes", true},
    {"scratch_fill_seen", true},
};

} // namespace snapmi
