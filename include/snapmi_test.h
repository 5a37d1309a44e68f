/*
 * snapmi_test.h -- knobs of the test suite and of the experiment drivers
 * (tests/, tests/hw/).  Not part of the production ABI of snapmi.h: results
 * never depend on them, and a production host has no use for them.
 *
 * These exist in the TEST build of the library only (libsnapmi_test.so:
 * the same sources compiled with -DSNAPMI_TESTING; rust-snappy_amd/csrc/
 * Makefile).  The product library, libsnapmi.so, does not export
 * snapmi_ctx_set_test_option, ignores the environment, and does not contain
 * the cross-check kernels that only these options reach: snapmi_ctx_set_option
 * values "compress_mode" 2 (both compressors on one ticket), "span_kernel" 0
 * (k_compress_blocks / k_compress_block_lds, one copy per step) and
 * "decode_kernel" 2 (k_decompress_streams2 alone) are SNAPMI_E_ARGUMENT there.
 *
 * Environment: a process that sets SNAPMI_TESTING=1 may also steer a new
 * context with SNAPMI_LANE_WAVES, SNAPMI_LANE_SEGMENT_BLOCKS,
 * SNAPMI_LANE_TABLE_SPREAD, SNAPMI_LANE_MIN_BLOCKS, SNAPMI_FRAME_CRC_SIDE,
 * SNAPMI_LANE_UNCACHED, SNAPMI_HOST_COPY_KERNEL,
 * SNAPMI_HOST_ENCODE_SLICE, SNAPMI_HOST_DECODE_CHUNKS, SNAPMI_DECODE_KERNEL,
 * SNAPMI_COMPRESS (the experiment scripts under tests/hw/ do).  Without
 * SNAPMI_TESTING they are ignored.
 */
#ifndef SNAPMI_TEST_H
#define SNAPMI_TEST_H

#include "snapmi.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 *   "lane_waves_per_cu"    lanes in flight = 64 x this x CUs (default 6)
 *   "lane_max_waves"       cap on the lane kernel's wavefronts (0 = none), so
 *                          a small batch puts several blocks on one lane
 *   "lane_tables_uncached" 1: the lane tables come from an uncached
 *                          allocation (measured: no gain; default 0)
 *   "lane_overlap_encode"  0 (default) never; 1: a lane-kernel segment with
 *                          at least 1.4 blocks per lane is matched in two
 *                          halves, the first half's tokens encoded on a side
 *                          stream meanwhile (measured slower); 2: whenever it
 *                          has two blocks
 *   "lane_table_probe"     1: time the placement even with one try
 *   "lane_table_stride_kib"  bytes between two lanes' tables, in KiB: 0
 *                          (default) by the budget, or 256 .. 4096 in steps
 *                          of 4 (an experiment knob: no probing, no chunks)
 *   "lane_tables_renew"    1: free the lane tables now; the next large batch
 *                          allocates (and places) new ones
 *   "lane_epoch_preset"    0..65535: every lane's hash-table epoch is set to
 *                          this before the next lane-kernel launch (reaches
 *                          the 16-bit epoch wrap without 65 535 blocks/lane)
 *   "lds_order_ok"         0: behave as if the LDS atomic order self-check of
 *                          snapmi_ctx_create had failed (lane kernel only)
 *   "frame_crc_side_stream"  0: the frame encoder's CRC kernel runs on the
 *                          main stream
 *   "lane_speculate_max_blocks"  lane-kernel launches of at most this many
 *                          blocks run k_match_blocks_spec (default 24 576)
 *   "decode_many_min"      batches of more streams than this are decoded by
 *                          k_decompress_streams3_many, 16 streams of the
 *                          sorted order per workgroup (default 1 048 576; the
 *                          suite lowers it to reach the kernel with 40 000)
 *   "stream_seg_log2"      segment size of the long-stream scan: 0 (default)
 *                          by size - 1 KiB under 256 MiB of long streams,
 *                          4 KiB from there -, 10 or 12: forced
 *   "stream_scan_segs"     segments a scan workgroup of it takes: 0 (default)
 *                          by size, or 8, 16, 32, 64
 *   "frame_walk_segment"   segment of the parallel chunk-header walk (>= 128
 *                          KiB; default 32 MiB)
 *   "host_batch_direct_min"  the host batch calls copy a stream of at least
 *                          this many bytes to the device from where it lies
 *                          instead of through pinned staging (default 1 MiB)
 *   "host_batch_pack_to_host"  1 (default): k_hb_pack stores the packed
 *                          output of a compress slice straight into pinned
 *                          host memory; 0: into device memory, followed by
 *                          one D2H of exactly that much
 *   "host_batch_listed"    1 (default): a slice of
 *                          snapmi_frame_decompress_batch_host whose streams
 *                          are all well-formed is decoded from the host's
 *                          chunk list; 0: the device always walks
 *   "index_build_route"    snapmi_build_block_index: 0 (default) streams of
 *                          two blocks and more go through the parallel scan
 *                          and those it gives up on to the sequential walker;
 *                          1: all of them to the walker; 2: the scan alone,
 *                          and what it gives up on is reported CORRUPT (shows
 *                          a test which streams fell through)
 *   "index_build_group_streams"  most streams in one group of its scan route
 *                          (1 .. 4096, default 4096)
 *   "scratch_fill"         -1 (default): off.  0..255: waits for the context's
 *                          streams (its own two and the host pipe's), then
 *                          sets the whole capacity of every SCRATCH buffer of
 *                          the context - device, pinned, the host pipe's
 *                          slots (the classes: DESIGN 4.2b) - to that byte;
 *                          kept buffers are not touched.  While it is not -1
 *                          every new allocation of either class is filled
 *                          with the byte before its owner sees it.  No result
 *                          depends on it: tests/test_gpu_scratch.py.  The
 *                          counters a call left for snapmi_ctx_get_info in
 *                          such a buffer read as "no call yet" afterwards.
 *                          snapmi_ctx_get_info (test build): what the last
 *                          setting of 0..255 filled, "scratch_fill_buffers"
 *                          and "scratch_fill_bytes", and how many of those
 *                          buffers hold the byte in their first, middle and
 *                          last position, "scratch_fill_seen"
 * Returns SNAPMI_E_ARGUMENT for an unknown name.
 *
 * snapmi_ctx_get_info answers one more name in the test build (beside the
 * three of "scratch_fill"):
 *   "lane_multi_rounds"    rounds of the last token-path segment's lane
 *                          wavefronts that resolved more probes than the
 *                          launch's own depth (the test build's kernels
 *                          count them; waits for the launch)
 */
SNAPMI_API int snapmi_ctx_set_test_option(snapmi_ctx *ctx, const char *name,
                               int64_t value);

#ifdef __cplusplus
}
#endif
#endif /* SNAPMI_TEST_H */
