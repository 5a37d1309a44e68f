/*
 * snapmi.h -- C ABI of libsnapmi.so, the MI355X (gfx950) Snappy raw block codec.
 *
 * This is the drop-in boundary for the hot path of BurntSushi/rust-snappy:
 *   snap::raw::Encoder::compress   (reference src/compress.rs:99-154)
 *   snap::raw::Decoder::decompress (reference src/decompress.rs:75-95)
 * and the functions beside them.  Groups of entry points:
 *
 *  1. The libsnappy C API (snappy-c.h) -- exactly the symbols the reference's
 *     own native seam binds (snappy-cpp/src/lib.rs:66-88, linked by
 *     snappy-cpp/build.rs:2 as dylib=snappy).  Pointing that link line at
 *     libsnapmi.so makes the reference's `--features cpp` tests and benches
 *     run against the GPU codec unchanged.
 *  2. Scalar mirrors of snap::raw::* that carry the full snap::Error
 *     (variant + fields, reference src/error.rs:72-180) across the ABI.
 *  3. The batched, device-resident API a GPU pipeline calls: arrays of
 *     independent raw streams in HBM in, arrays of compressed streams in HBM
 *     out.  This is the form that is benchmarked.
 *  4. The Snappy frame format (reference src/frame.rs, src/crc32.rs,
 *     src/write.rs, src/read.rs): on device buffers (asynchronous), and on
 *     host buffers one batch of chunks per call - what a host-language
 *     FrameEncoder / FrameDecoder (shim/, rust-snappy_amd/frame.py,
 *     tools/szip.cpp) makes per batch.
 *  5. The gather of framed parts across the GPUs of a node (RCCL).
 *
 * Plain pointers and sizes only; no C++ or torch types.  All functions are
 * blocking unless stated otherwise.  Every compute entry point runs HIP
 * kernels on the GPU; there is no CPU fallback -- without a usable device
 * they fail with SNAPMI_E_DEVICE.
 */
#ifndef SNAPMI_H
#define SNAPMI_H

#include <stddef.h>
#include <stdint.h>

/* Every function declared here (and nothing else) is exported by
 * libsnapmi.so: the library is built with -fvisibility=hidden and the export
 * list rust-snappy_amd/csrc/snapmi.map, which csrc/gen_exports.py writes
 * from the SNAPMI_API lines of this header (tests/test_abi_cpu.py compares
 * `nm -D` of the built library with it, name for name). */
#if defined(__GNUC__)
#define SNAPMI_API __attribute__((visibility("default")))
#else
#define SNAPMI_API
#endif

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------ */
/* 1. libsnappy C API (snappy-c.h:46-122; bound by the reference at     */
/*    snappy-cpp/src/lib.rs:66-88).  Host pointers.                     */
/* ------------------------------------------------------------------ */
typedef enum {
    SNAPPY_OK = 0,
    SNAPPY_INVALID_INPUT = 1,
    SNAPPY_BUFFER_TOO_SMALL = 2
} snappy_status;

/* replaces snappy_compress (snappy-cpp/src/lib.rs:67-72).
 * *compressed_length: in = capacity, out = bytes written. */
SNAPMI_API snappy_status snappy_compress(const char *input, size_t input_length,
                              char *compressed, size_t *compressed_length);
/* replaces snappy_uncompress (snappy-cpp/src/lib.rs:74-79) */
SNAPMI_API snappy_status snappy_uncompress(const char *compressed,
                                size_t compressed_length, char *uncompressed,
                                size_t *uncompressed_length);
/* replaces snappy_max_compressed_length (snappy-cpp/src/lib.rs:81) */
SNAPMI_API size_t snappy_max_compressed_length(size_t source_length);
/* replaces snappy_uncompressed_length (snappy-cpp/src/lib.rs:83-87) */
SNAPMI_API snappy_status snappy_uncompressed_length(const char *compressed,
                                         size_t compressed_length,
                                         size_t *result);
/* snappy-c.h:120-122; not bound by the reference, kept for completeness */
SNAPMI_API snappy_status snappy_validate_compressed_buffer(const char *compressed,
                                                size_t compressed_length);

/* ------------------------------------------------------------------ */
/* Errors: snap::Error (reference src/error.rs:72-180), same order.     */
/* ------------------------------------------------------------------ */
enum snapmi_kind {
    SNAPMI_OK = 0,
    SNAPMI_TOO_BIG = 1,                  /* a=given        b=max            */
    SNAPMI_BUFFER_TOO_SMALL = 2,         /* a=given        b=min            */
    SNAPMI_EMPTY = 3,
    SNAPMI_HEADER = 4,
    SNAPMI_HEADER_MISMATCH = 5,          /* a=expected_len b=got_len        */
    SNAPMI_LITERAL = 6,                  /* a=len  b=src_len  c=dst_len     */
    SNAPMI_COPY_READ = 7,                /* a=len  b=src_len                */
    SNAPMI_COPY_WRITE = 8,               /* a=len  b=dst_len                */
    SNAPMI_OFFSET = 9,                   /* a=offset  b=dst_pos             */
    SNAPMI_STREAM_HEADER = 10,           /* a=byte                          */
    SNAPMI_STREAM_HEADER_MISMATCH = 11,  /* a=first 6 body bytes, LE packed */
    SNAPMI_UNSUPPORTED_CHUNK_TYPE = 12,  /* a=byte                          */
    SNAPMI_UNSUPPORTED_CHUNK_LENGTH = 13,/* a=len  b=header (0/1)           */
    SNAPMI_CHECKSUM = 14,                /* a=expected  b=got               */
    /* not snap::Error variants: */
    SNAPMI_E_UNEXPECTED_EOF = 64, /* io::ErrorKind::UnexpectedEof (frame)   */
    SNAPMI_E_DEVICE = 100,  /* no GPU / HIP call failed; see last_error     */
    SNAPMI_E_ARGUMENT = 101 /* NULL pointer, bad context                    */
};

typedef struct snapmi_error {
    int32_t kind; /* enum snapmi_kind */
    uint32_t reserved;
    uint64_t a, b, c;
} snapmi_error;

/* impl fmt::Display for snap::Error (reference src/error.rs:249-335): the
 * text the reference prints for this error - "snappy: corrupt input (expected
 * copy write of length 11; remaining dst: 4)" - into buf (NUL-terminated,
 * truncated to cap).  Returns the length the whole text has.  Host code. */
SNAPMI_API size_t snapmi_error_string(const snapmi_error *err, char *buf, size_t cap);

/* ------------------------------------------------------------------ */
/* Context: one HIP device + stream + device scratch.  Maps to          */
/* snap::raw::Encoder (exclusive &mut self, owns its scratch table --   */
/* reference src/compress.rs:67-70): one context per thread.            */
/* ------------------------------------------------------------------ */
typedef struct snapmi_ctx snapmi_ctx;

/* device: HIP ordinal.  hip_stream: a hipStream_t the kernels are
 * launched on, or NULL for a stream owned by the context. */
SNAPMI_API int snapmi_ctx_create(int device, void *hip_stream, snapmi_ctx **out);
SNAPMI_API void snapmi_ctx_destroy(snapmi_ctx *ctx);
/* Message for the last SNAPMI_E_DEVICE / SNAPMI_E_ARGUMENT on this ctx. */
SNAPMI_API const char *snapmi_last_error(const snapmi_ctx *ctx);
/* Page-locked host memory for the host-buffer entry points (their H2D / D2H
 * copies run at PCIe speed from such buffers, at about a third of it from
 * pageable memory).  NULL when it cannot be had. */
SNAPMI_API void *snapmi_host_alloc(size_t bytes);
SNAPMI_API void snapmi_host_free(void *p);
/* "ms(stride) ms(stride) ... | held at most B of budget B | kept S KiB apart,
 * L lanes, B bytes | placement T ms | free B -> B": the placement probe's
 * time for every candidate region of the last lane-table allocation (none
 * when lane_table_tries is 1), the most device memory it held at once, what
 * it kept, how long it took and hipMemGetInfo's free bytes around it. */
SNAPMI_API const char *snapmi_table_probe_log(const snapmi_ctx *ctx);
/* Name of the dominant kernel of the last batch call - the one
 * snapmi_timing.dominant_ms times: "k_match_both", "k_match_blocks",
 * "k_match_spans", "k_compress_spans", "k_decompress_streams3" ... ("" before
 * the first call).  For profiles: bench.py names its roofline by it. */
SNAPMI_API const char *snapmi_last_kernel(const snapmi_ctx *ctx);
/* hipStream_t the context launches on (for event timing by the caller). */
SNAPMI_API void *snapmi_ctx_stream(const snapmi_ctx *ctx);
/* "snapmi <version> gfx950" */
SNAPMI_API const char *snapmi_version(void);
/*
 * Options (results never depend on them, only speed and memory):
 *   "compress_mode"        0 wavefront-per-block kernel only (k_compress_spans:
 *                          no scratch beyond the caller's buffers), 1
 *                          lane-per-block kernel on large batches (default)
 *                          [2, both at once, is a cross-check of the test
 *                          build: snapmi_test.h]
 *   "span_kernel"          1 (default, and the only value here): the window
 *                          kernels take a window of 63 positions per step
 *                          [0, one copy per step, is a cross-check of the
 *                          test build: snapmi_test.h]
 *   "both_wave_cus"        compress_mode 2 only: CUs the window kernel's
 *                          persistent workgroups take beside the lane kernel
 *                          (0 .. 4096; default 0 = half of the CUs)
 *   "small_table_kernel"   1 (default): blocks of at most 8 KiB - pages,
 *                          short frame chunks, tails - are matched by a
 *                          window kernel with the 16 KiB table the reference
 *                          gives them (src/compress.rs:491-518), ten
 *                          wavefronts per CU instead of five, when a batch
 *                          has "small_table_min_blocks" (default 256) of
 *                          them; 0: they are blocks like any other
 *   "small_batch_kernel"   1 (default): batches of at most two blocks per
 *                          CU run one block per CU with table AND input block
 *                          in LDS; 0 never; 2 whenever the wavefront kernel
 *                          would run
 *   "tiny_stream_kernel"   1 (default): streams of fewer than 256 bytes are
 *                          compressed one per LANE, input, table and output
 *                          in LDS (k_compress_tiny); 0: they are one-block
 *                          streams of the block kernels (and so are the
 *                          streams of the next option)
 *   "small_stream_kernel"  1 (default): streams of 256 .. 1023 bytes are
 *                          compressed a few per wavefront, one per lane, with
 *                          input and table in LDS (k_compress_small); 2: up
 *                          to 2047 bytes (slower than the block kernels from
 *                          1 KiB on); 0: they are one-block streams of the
 *                          block kernels
 *   "span_schedule"        1 (default): a window-kernel launch of more blocks
 *                          than it has wavefronts (1 280) chooses the order
 *                          of its blocks as it goes - the first block of
 *                          every stream first, then the blocks of streams
 *                          that proved heavy, the light ones last - so that
 *                          it ends with small jobs (256 MiB of mixed files:
 *                          a quarter less time); 0: ticket order; 2: also
 *                          for fewer blocks
 *   "lane_min_blocks"      batches with at least this many 64 KiB blocks use
 *                          the lane-per-block kernel (default 20480 = 1.25 GiB)
 *   "lane_coresident"      1 (default): large lane-kernel launches run
 *                          k_match_both - lane wavefronts and two window
 *                          wavefronts on every CU, one two-ended ticket (cfg2:
 *                          115.6 -> 108.4 ms for the match finder; at 4 GiB a
 *                          draw); 0: the lane kernel alone
 *   "lane_coresident_min_blocks"  launches of at least this many blocks are
 *                          "large" for lane_coresident (default 98304 = 6 GiB)
 *   "match_kernel"         the match finder of a large batch: 0 k_match_blocks
 *                          (a lane per block, hash tables in HBM), 1
 *                          k_match_spans (a wavefront per block, table in LDS,
 *                          no tables in HBM), 2 (default) k_match_spans when
 *                          the context's last batch did not compress, else
 *                          k_match_blocks
 *   "match_spans_ratio_pct"  for match_kernel 2, "did not compress": the
 *                          output was at least this per cent of the input
 *                          (1 .. 200; default 90) - such data costs a lane
 *                          three HBM transactions per probe for nothing
 *   "lane_speculate"       1 (default): a lane-kernel launch of at most 24 576
 *                          blocks (1.5 GiB) also fetches, in a probe's round,
 *                          the table entry of the probe that follows a miss -
 *                          fewer dependent rounds per block where a block's
 *                          latency is what is waited for; 0: never
 *   "lane_tail_probes"     2..4: in the tail of a lane-kernel launch - the
 *                          blocks have all been handed out, lanes only finish
 *                          and a round costs its latency - a wavefront
 *                          resolves up to this many probes a round (it
 *                          fetches the entries of the probes that follow a
 *                          miss; default 2); 0 or 1: never
 *   "lane_tail_idle_pct"   ... from the moment this share of the launch's
 *                          lanes is out of work (default 40; 0: from the
 *                          first round)
 *   "lane_segment_blocks"  most blocks per lane-kernel launch (default
 *                          262144 = 16 GiB of input).  A larger batch is
 *                          matched and encoded in equal launches of at most
 *                          this many blocks, and the token scratch - 72 KiB a
 *                          block, 1.13x the input - is one launch's: at cfg2
 *                          (146 700 blocks) 73 350 makes the context hold
 *                          23.3 GB instead of 29.1 and costs 8 % of the
 *                          compress rate, 48 900 21.2 GB (tokens 0.42x the
 *                          input) and 25 % (profiles/r6_token_segments.txt)
 *   "token_pool_pct"       39 (default): the token pool - where the match
 *                          finders of a large batch leave their tokens for
 *                          the encoder, in pages of 2 KiB taken as a block
 *                          needs them - is this share of what the worst case
 *                          of every block would take (1.16x the input: a
 *                          token of 4 bytes per 4 bytes of input, rounded to
 *                          pages), + a page and a half per lane in flight:
 *                          0.49x the input at cfg2 with everything, of which
 *                          cfg2 uses 0.46x; English text needs 0.73x.  A block
 *                          that finds no page is compressed a second time by
 *                          the window kernel (same bytes; costs that block
 *                          twice), and the context's next batch gets a pool
 *                          half as large again when more than 1 % of a batch
 *                          did (a sixth larger when it was under 10 %).
 *                          100: no block ever spills.  Never under
 *   "token_pool_min_pages" 32768 (default; 64 MiB): batches of up to 750
 *                          blocks never spill
 *   "lane_table_spread"    1 (default): the lane kernel's hash tables are
 *                          spread over up to 4x their size, as far as the
 *                          budget below allows (HBM sustains up to 30 % more
 *                          random accesses on tables that are not packed
 *                          into the memory a process is handed first,
 *                          DESIGN 4.1); 0: packed (17-25 GB)
 *   "lane_table_budget_pct"  percent of the device memory that is free when
 *                          a context first needs its lane tables that the
 *                          tables - and, while a placement is being chosen,
 *                          its candidates together - may hold (default 33,
 *                          1..90).  No call holds more at any moment, except
 *                          snapmi_ctx_prepare with SNAPMI_PREPARE_TOP_OF_MEMORY
 *   "lane_table_tries"     placements of the lane tables that are timed
 *                          (k_probe_tables, 3 ms each) before the fastest is
 *                          kept - at most this many (default 2: spread, then
 *                          packed behind that), fewer when one probes at the
 *                          fast rate or the budget has no room for another.
 *                          1: no probing, one region
 *   "release_scratch"      1: the compressor's per-batch scratch (token
 *                          arrays of the lane kernel: 128 KiB per block of a
 *                          launch, up to 34 GB) is freed by
 *                          snapmi_ctx_synchronize instead of being kept for
 *                          the next batch (default 0)
 *   "batch_long_streams"   1 (default): snapmi_decompress_batch looks at a
 *                          batch of at most 16 384 streams first (one small
 *                          kernel, one synchronisation of the context's
 *                          stream, ~30 us) and decodes up to 4 096 long
 *                          streams in it - 32 KiB compressed or more that
 *                          expand by half, 256 KiB or more of anything -
 *                          through their 64 KiB pieces, like
 *                          snapmi_decompress_stream, instead of one wavefront
 *                          each (a batch otherwise waits 3-5 ms for a 700 KB
 *                          stream); 0: never, the call only enqueues
 *   "decode_kernel"        3 (default) k_decompress_streams3; 0 one element
 *                          at a time [2, the second generation alone, is a
 *                          cross-check of the test build]
 *   "frame_parallel_walk_min"  framed streams of at least this many bytes
 *                          decoded without a side index get their chunk
 *                          headers found in parallel (default 4 MiB); the
 *                          chained fronts of a SNAPMI_FRAME_NO_WAIT decode
 *                          follow it too
 *   "host_encode_slice"    input bytes per slice of snapmi_frame_encode_host
 *                          (default 2 GiB: the match finder wants few, large
 *                          launches)
 *   "host_decode_slice_chunks"  data chunks per slice of
 *                          snapmi_frame_decode_host (default 8192)
 *   "host_copy_kernel"     bit 0 / bit 1: decoded / encoded results go home
 *                          by a copy kernel instead of hipMemcpyAsync when
 *                          the caller's buffer is pinned (default 1)
 *   "host_batch_slice"     input bytes per slice of snapmi_compress_batch_host
 *                          / snapmi_decompress_batch_host (default 16 MiB, at
 *                          least 64 KiB): what bounds their device and pinned
 *                          staging, three slices of it being in flight
 *   "range_scratch_bytes"  bytes of 64 KiB rooms snapmi_decompress_ranges_indexed
 *                          may hold for the edge blocks of its ranges at once
 *                          (default 1 GiB, at least 128 KiB; a bound on
 *                          memory, not a tuned number)
 *   "write_scratch_bytes"  bytes of compress slots (76 496 a touched block) and
 *                          64 KiB rooms (one an edge block)
 *                          snapmi_write_ranges_indexed may hold at once
 *                          (default 1 GiB, at least 142 032: one block's slot
 *                          and room; a bound on memory, not a tuned number);
 *                          snapmi_append_indexed holds the same scratch under
 *                          the same cap: a slot a new block, a room a tail
 * The knobs of the test suite and of the experiment drivers are declared in
 * snapmi_test.h (snapmi_ctx_set_test_option).
 * Returns SNAPMI_E_ARGUMENT for an unknown name.
 */
SNAPMI_API int snapmi_ctx_set_option(snapmi_ctx *ctx, const char *name, int64_t value);

/* Allocates and places, NOW, the device memory a batch of `blocks` 64 KiB
 * blocks (input bytes / 65 536, rounded up per stream) would make the first
 * snapmi_compress_batch allocate: the lane kernel's hash tables (256 KiB per
 * lane in flight, 17-26 GB for a batch that fills the chip; nothing for a
 * batch of fewer than lane_min_blocks blocks).  Optional - a compress call
 * does the same on demand, within lane_table_budget_pct.
 * flags:
 *   SNAPMI_PREPARE_TOP_OF_MEMORY  place the tables at the far end of the
 *     device's memory, where HBM sustains 30 % more random accesses than in
 *     the part a process is handed first (cfg2: 72 instead of 57-66 GiB/s,
 *     DESIGN 4.1).  The only way there is through everything in front of it:
 *     for the duration of two hipMalloc calls this call holds ALL free device
 *     memory (any other allocation on the device fails meanwhile - other
 *     processes, torch in this process, other contexts), and the driver then
 *     wipes what was given back, in the background, for a few seconds.  For a
 *     process that owns the GPU, once, at start-up; never taken by default.
 * Like the reference's Encoder::new (src/compress.rs:80-82: an encoder's
 * scratch is its own and allocated once), made explicit because here it is
 * gigabytes. */
#define SNAPMI_PREPARE_TOP_OF_MEMORY 1u
SNAPMI_API int snapmi_ctx_prepare(snapmi_ctx *ctx, uint64_t blocks,
                                  uint32_t flags);

/* What a context holds and what its last batch did, by name:
 *   "scratch_bytes"         device memory the context's grow-only buffers
 *                           hold now (lane tables, token pool, plans, ...)
 *   "token_scratch_bytes"   ... the token pool, its page tables, the counts
 *   "token_pool_pages"      pages (2 KiB) of the last token-path launch's pool
 *   "token_pool_pct_now"    what token_pool_pct has grown to on this context
 *   "token_pages_asked"     pages the last token-path launch asked for, and
 *   "token_blocks_spilled"  blocks of it that found none and were compressed
 *                           a second time (both wait for the launch)
 *   "host_batch_slices"     slices the last host batch call (sections 2b, 4b)
 *                           made
 *   "host_batch_h2d_bytes"  bytes it copied to the device (descriptors, inputs
 *                           and their alignment padding) and
 *   "host_batch_d2h_bytes"  back: one length and one error record per stream
 *                           and the outputs, packed (compress: what was
 *                           written, each stream rounded to 16 bytes)
 *   "host_batch_listed_slices"  slices of it that were decoded from the host's
 *                           chunk list (snapmi_frame_decompress_batch_host)
 *   "index_streams_pieced"  streams of the last
 *                           snapmi_decompress_batch_indexed whose index passed
 *                           and that were delivered by their pieces, and
 *   "index_streams_fallback"  streams of it whose index passed, whose pieces
 *                           did not come out whole and that the batch's own
 *                           launch decoded instead (both wait for the call)
 *   "range_pieces"          pieces the ranges of the last
 *                           snapmi_decompress_ranges_indexed took
 *                           (snapmi_range_pieces of the host's copies), and
 *   "range_ranges_ok" / "range_ranges_failed"  ranges of it that succeeded /
 *                           failed (these two wait for the call)
 *   "write_blocks"          blocks the writes of the last
 *                           snapmi_write_ranges_indexed touched
 *                           (snapmi_write_blocks of its lists),
 *   "write_blocks_decoded"  the edge blocks among them, which were decoded, and
 *   "write_streams_ok" / "write_streams_failed"  touched streams of it that
 *                           succeeded / failed (these two wait for the call)
 *   "append_blocks"         new blocks the last snapmi_append_indexed
 *                           compressed, from the host's copies,
 *   "append_blocks_decoded" the tails it decoded (named streams whose old
 *                           length is no multiple of 65536), and
 *   "append_streams_ok" / "append_streams_failed"  named streams of it that
 *                           succeeded / failed (these two wait for the call)
 *   "index_build_built" / "index_build_unaligned" / "index_build_corrupt" /
 *   "index_build_missized"  streams of the last snapmi_build_block_index by
 *                           verdict, and
 *   "index_build_walked"    streams of it the sequential walker handled (all
 *                           five wait for the call)
 *   "frame_nowait_front"    the front that decided the last
 *                           SNAPMI_FRAME_NO_WAIT decode: 1 the side index, 2
 *                           the parallel walk, 3 the sequential walk, 4 the
 *                           bound was exceeded; -1 before the first (waits
 *                           for the call)
 * SNAPMI_E_ARGUMENT for a name that is not in this list. */
SNAPMI_API int snapmi_ctx_get_info(snapmi_ctx *ctx, const char *name,
                                   int64_t *value);

/* ------------------------------------------------------------------ */
/* 2. Scalar mirrors of snap::raw (host buffers; H2D + kernels + D2H).  */
/*    Return enum snapmi_kind; *err (may be NULL) gets the fields.      */
/* ------------------------------------------------------------------ */
/* snap::raw::max_compress_len, reference src/compress.rs:42-53
 * (0 when the input or the bound exceeds 2^32-1). */
SNAPMI_API size_t snapmi_max_compress_len(size_t input_len);
/* snap::raw::decompress_len, reference src/decompress.rs:30-35.
 * Pure header parse on the host. */
SNAPMI_API int snapmi_decompress_len(const uint8_t *input, size_t input_len,
                          size_t *result, snapmi_error *err);
/* snap::raw::Encoder::compress, reference src/compress.rs:99-154 */
SNAPMI_API int snapmi_raw_compress(snapmi_ctx *ctx, const uint8_t *input,
                        size_t input_len, uint8_t *output, size_t output_cap,
                        size_t *written, snapmi_error *err);
/* snap::raw::Decoder::decompress, reference src/decompress.rs:75-95 */
SNAPMI_API int snapmi_raw_decompress(snapmi_ctx *ctx, const uint8_t *input,
                          size_t input_len, uint8_t *output,
                          size_t output_cap, size_t *written,
                          snapmi_error *err);

/* ------------------------------------------------------------------ */
/* 2b. Many independent raw streams in HOST memory per call.            */
/* ------------------------------------------------------------------ */
/*
 * What a loop of snapmi_raw_compress / snapmi_raw_decompress over n buffers
 * gives, in one blocking call: for every i, h_out_lens[i], h_errs[i] (variant
 * and fields a, b, c) and the bytes h_out_ptrs[i][0, h_out_lens[i]) are
 * exactly those of the scalar call on stream i alone with capacity
 * h_out_caps[i] - one Encoder::compress / Decoder::decompress of the
 * reference each (src/compress.rs:99-154, src/decompress.rs:75-95).  No
 * stream affects another.
 *   a stream that fails   h_out_lens[i] = 0, h_errs[i] says why, and not one
 *                         byte of h_out_ptrs[i] is written
 *   a stream that succeeds  exactly [0, h_out_lens[i]) is written, nothing
 *                         behind it
 *   return value          failures of the call itself only (SNAPMI_E_DEVICE,
 *                         SNAPMI_E_ARGUMENT); SNAPMI_OK when the call ran,
 *                         whatever the streams did
 *   h_errs                may be NULL
 *   h_out_caps            may not be NULL (these are host buffers: there is
 *                         no unchecked mode); compress: cap_i <
 *                         snapmi_max_compress_len(len_i) is BufferTooSmall
 *                         {given, min} for stream i; decompress: cap_i <
 *                         the header's length is BufferTooSmall {cap, n}
 *   n                     below 2^31; n == 0 does nothing and returns OK
 * The buffers may be pageable or pinned (snapmi_host_alloc): same results,
 * other speed.  One context per thread, as everywhere.
 *
 * The batch is cut into slices of whole streams (option "host_batch_slice";
 * a stream larger than a slice is a slice of its own) that overlap: slice
 * i+1 is packed into pinned staging and sent - descriptors and inputs in one
 * copy - while the kernels of snapmi_compress_batch / snapmi_decompress_batch
 * run on slice i and slice i-1 comes home.  Only what was written crosses the
 * link on the way back: compressed streams are gathered on the device
 * (k_hb_pack) to 16-byte-aligned packed offsets first.  Info
 * "host_batch_slices", "host_batch_h2d_bytes", "host_batch_d2h_bytes"
 * describe the last call.
 * Measured (profiles/host_batch.json, one MI355X): 4 096 streams of 16 KiB of
 * text from pageable / pinned buffers 12.1 / 8.1 ms to compress (5.2 / 7.8
 * GiB/s) and 8.0 / 8.8 ms to decompress, where a loop of scalar calls takes
 * 1 752 / 805 ms (145x / 100x); 65 536 streams of 4 KiB 44.5 / 41.5 ms
 * (214x / 138x); 512 streams of 100 B .. 1 MiB 12.1 / 8.3 ms (26x / 22x).
 * The device-resident batch calls take 1.7 / 0.3 ms on the first set and the
 * link moved 17.8 / 27.8 GiB/s host to host on that box: one host thread
 * copies every byte into staging and out of it.
 */
SNAPMI_API int snapmi_compress_batch_host(snapmi_ctx *ctx,
                               const void *const *h_in_ptrs,
                               const size_t *h_in_lens,
                               void *const *h_out_ptrs,
                               const size_t *h_out_caps, size_t *h_out_lens,
                               snapmi_error *h_errs, size_t n);
SNAPMI_API int snapmi_decompress_batch_host(snapmi_ctx *ctx,
                                 const void *const *h_in_ptrs,
                                 const size_t *h_in_lens,
                                 void *const *h_out_ptrs,
                                 const size_t *h_out_caps, size_t *h_out_lens,
                                 snapmi_error *h_errs, size_t n);

/* ------------------------------------------------------------------ */
/* 3. Batched device-resident API.  Every d_* pointer is device memory  */
/*    on the context's device; stream i is an independent raw stream    */
/*    (its own varint header), exactly one Encoder::compress /          */
/*    Decoder::decompress call of the reference.                        */
/*    Asynchronous: work is enqueued on the context's stream; results   */
/*    are valid after snapmi_ctx_synchronize (or a caller-side wait on  */
/*    that stream).  Return value reports enqueue-time failures only;   */
/*    per-stream results land in d_out_lens / d_errs.                   */
/* ------------------------------------------------------------------ */

/*
 * Compress n streams.
 *   d_in_ptrs[i], d_in_lens[i] : input bytes of stream i
 *   h_in_lens                  : host copy of d_in_lens (needed to size the
 *                                launch); NULL = fetched with a blocking D2H
 *   d_out_ptrs[i], d_out_caps[i]: output buffer; capacity must be >=
 *                                snapmi_max_compress_len(len) or stream i
 *                                fails with BufferTooSmall (reference
 *                                src/compress.rs:111-116); d_out_caps NULL =
 *                                capacities are not checked
 *   d_out_lens[i]              : bytes written (0 on error)
 *   d_errs[i]                  : per-stream snapmi_error (may be NULL)
 */
SNAPMI_API int snapmi_compress_batch(snapmi_ctx *ctx, const void *const *d_in_ptrs,
                          const uint64_t *d_in_lens,
                          const uint64_t *h_in_lens, void *const *d_out_ptrs,
                          const uint64_t *d_out_caps, uint64_t *d_out_lens,
                          snapmi_error *d_errs, size_t n);

/*
 * Decompress n streams.  d_out_caps[i] is the capacity of d_out_ptrs[i]
 * (reference: output.len(), src/decompress.rs:84-89); d_out_lens[i] gets the
 * decompressed length on success, 0 on error.
 * A stream is decoded by one wavefront - except the long streams of a batch
 * of at most 16 384 streams, which are cut into pieces like the one stream of
 * snapmi_decompress_stream (option "batch_long_streams": that look at the
 * batch waits once for the context's stream, so with it the call is NOT
 * enqueue-only.  A host that pipelines many small batches from one thread
 * sets the option to 0; while the context's stream is being captured into a
 * hipGraph the look is skipped by itself and the call only enqueues).
 */
SNAPMI_API int snapmi_decompress_batch(snapmi_ctx *ctx, const void *const *d_in_ptrs,
                            const uint64_t *d_in_lens,
                            void *const *d_out_ptrs,
                            const uint64_t *d_out_caps, uint64_t *d_out_lens,
                            snapmi_error *d_errs, size_t n);

/*
 * The block index of raw streams: where, inside a compressed stream, the
 * elements of every 64 KiB block of its input begin.  The compressor knows
 * it for free and the decoder, given it, decodes a long stream on as many
 * wavefronts as it has blocks without looking for the boundaries first.
 *
 * Layout.  Stream i owns d_index[d_index_first[i], d_index_first[i + 1]):
 * blocks_i + 1 entries, blocks_i = ceil(len_i / 65536).  Entry j is the byte
 * offset, inside stream i's compressed bytes, of the first element of block
 * j: entry 0 is the length of the varint header, the last entry equals
 * d_out_lens[i].  An empty input has the one entry {1}; a stream that fails
 * (BufferTooSmall) has all its entries 0.
 *
 * snapmi_block_index_entries: entries the index of n streams takes, the sum
 * of ceil(len_i / 65536) + 1.  Host code.
 *
 * snapmi_compress_batch_indexed: snapmi_compress_batch - the same bytes,
 * lengths and errors, enqueue-only with the same h_in_lens == NULL exception -
 * that also writes d_index_first [n + 1] and d_index.  index_cap: entries
 * d_index has room for; fewer than snapmi_block_index_entries(h_in_lens, n)
 * is SNAPMI_E_ARGUMENT, and nothing is enqueued.
 *
 * snapmi_decompress_batch_indexed: for every i, d_out_lens[i], d_errs[i]
 * (variant and fields) and the bytes d_out_ptrs[i][0, d_out_lens[i]) are
 * those of snapmi_decompress_batch WHATEVER the index holds: it is a hint and
 * decides only how fast the result comes.  index_entries is the host's copy
 * of d_index_first[n] (what snapmi_block_index_entries gave) and sizes every
 * launch; entries at or behind it are never read.  A stream is indexed when
 * it owns at least three entries (two blocks) inside the index, entry 0 is
 * the length of its varint header, the entries strictly increase, the last
 * one is its compressed length, their count is ceil(dlen / 65536) + 1 for the
 * length dlen its header announces, and dlen <= d_out_caps[i].  Piece k of
 * such a stream - input [entry k, entry k + 1) into output [k * 65536,
 * min((k + 1) * 65536, dlen)) - is decoded like an independent stream that
 * must fill exactly its room: no piece writes outside it, so nothing is
 * written outside [d_out_ptrs[i], + d_out_caps[i]) however hostile the index.
 * A stream all of whose pieces report OK and filled their room is done; any
 * other indexed stream (a copy that reaches across a boundary, an entry in
 * the middle of an element, a corrupt byte) and every stream that is not
 * indexed is decoded whole by the batch's ordinary launch behind the pieces,
 * which names the reference's error with whole-stream fields.
 * The streams that are not indexed are decoded beside the pieces, in the
 * same launch.  The call only enqueues - no look at the batch on the host
 * ("batch_long_streams" is not consulted), no wait, so it can be captured
 * into a hipGraph once the context's scratch has grown to the batch's size
 * (a buffer that grows waits for the stream, as in every call of this
 * section; all of them are reserved before the first launch) - and has no
 * limit of 16 384 streams or 4 096 long ones; n + index_entries stays below
 * 2^31 (SNAPMI_E_ARGUMENT).  n == 0 enqueues nothing; index_entries < 3 is
 * snapmi_decompress_batch's plain launch.
 * Info "index_streams_pieced" / "index_streams_fallback" describe the last
 * call.
 */
SNAPMI_API uint64_t snapmi_block_index_entries(const uint64_t *h_in_lens,
                                               size_t n);
SNAPMI_API int snapmi_compress_batch_indexed(
    snapmi_ctx *ctx, const void *const *d_in_ptrs, const uint64_t *d_in_lens,
    const uint64_t *h_in_lens, void *const *d_out_ptrs,
    const uint64_t *d_out_caps, uint64_t *d_out_lens, snapmi_error *d_errs,
    size_t n, uint64_t *d_index_first /* out, [n+1] */,
    uint64_t *d_index /* out */, uint64_t index_cap);
SNAPMI_API int snapmi_decompress_batch_indexed(
    snapmi_ctx *ctx, const void *const *d_in_ptrs, const uint64_t *d_in_lens,
    void *const *d_out_ptrs, const uint64_t *d_out_caps, uint64_t *d_out_lens,
    snapmi_error *d_errs, size_t n, const uint64_t *d_index_first /* [n+1] */,
    const uint64_t *d_index, uint64_t index_entries);

/*
 * Range reads through the block index: bytes [off, off + len) of a stream's
 * OUTPUT, decoding only the 64 KiB blocks the range touches.
 *
 * snapmi_range_pieces: pieces the ranges take, the sum over r of the 64 KiB
 * blocks that [off_r, off_r + len_r) touches (0 for len_r == 0 and for a
 * range whose end passes 2^64; the sum saturates at 2^64 - 1).  Host code.
 *
 * snapmi_decompress_ranges_indexed: range r asks for output bytes
 * [off, off + len) of stream s = d_range_stream[r] of the n streams
 * (d_in_ptrs, d_in_lens) with the index (d_index_first, d_index,
 * index_entries) snapmi_compress_batch_indexed wrote; they go to
 * d_range_out[r][0, len).  h_range_off / h_range_len are the host's copies of
 * d_range_off / d_range_len and size every launch and every buffer, as
 * h_in_lens does for compress; both are required (NULL: SNAPMI_E_ARGUMENT,
 * nothing is enqueued).  The device reads the d_* arrays only and never
 * trusts that they equal the host's copies.
 *   Piece.  Block k of a stream whose header announces dlen is input
 *     [entry k, entry k + 1) into output [k * 65536, min((k + 1) * 65536,
 *     dlen)), decoded like an independent stream that must fill exactly its
 *     room - the piece of snapmi_decompress_batch_indexed.
 *   A range succeeds when every block it touches is such a piece, reports OK
 *     and filled its room: d_range_got[r] = len, the error kind is 0 and the
 *     bytes are [off, off + len) of what snapmi_decompress_batch gives for the
 *     whole stream.  That holds for every stream whose 64 KiB blocks are
 *     self-contained: this encoder's, the reference's, libsnappy's.
 *   Blocks the range does not touch are neither read nor judged: a stream
 *     that is corrupt elsewhere still serves the range.
 *   A range fails with d_range_got[r] = 0; d_range_out[r][0, len) is then
 *     unspecified.  Nothing outside it is ever written, whatever the index,
 *     d_index_first and the range arrays hold, and a failure never touches
 *     another range (with the one exception named under "slots").  Why:
 *       s >= n                         SNAPMI_E_ARGUMENT {s, n}
 *       the header does not parse      the error snapmi_decompress_len_batch
 *                                      gives the stream
 *       off + len wraps or > dlen      SNAPMI_E_ARGUMENT {off, len, dlen}
 *       slots                          the device arrays ask for more pieces
 *         (or edge rooms) than the host's copies sized: SNAPMI_E_ARGUMENT
 *         {first slot, pieces asked, pieces sized}.  Slots are handed out in
 *         range order from what the DEVICE arrays ask for, so the ranges that
 *         no longer fit are the last ones of the group the liar is in; every
 *         range whose slots fit is exact.
 *       no usable index                SNAPMI_E_ARGUMENT {s, block}: the
 *         stream's entries must lie inside [0, index_entries), number
 *         ceil(dlen / 65536) + 1, begin with the varint's length and end
 *         with the compressed length (block: the first block the range
 *         touches), and entry k < entry k + 1 <= compressed length for every
 *         touched block k (block: the first that fails).  A one-block stream
 *         with its 2 entries is usable here, unlike under the batch rule.
 *       a piece fails or is not full   (a copy that reaches across the block
 *         boundary, an entry in the middle of an element, a corrupt byte) the
 *         error of the first such piece in block order, kind and fields a, b,
 *         c those of snapmi_decompress_batch on the stream
 *         varint(room) || piece bytes with capacity room (a piece whose
 *         elements end short of its room is SNAPMI_HEADER_MISMATCH {room,
 *         produced}: no piece reports OK without having filled its room).
 *         The remedy is to decode the stream whole.
 *   len == 0 with off <= dlen is OK: got 0, no piece.  m == 0 enqueues
 *   nothing.  m, and n + index_entries + pieces, stay below 2^31
 *   (SNAPMI_E_ARGUMENT).
 * A touched block that lies wholly inside the range is decoded straight into
 * d_range_out[r]; an EDGE block - cut by the range; told from the range alone,
 * so a stream's short last block counts unless the range ends on a multiple
 * of 65536 - is decoded into a 64 KiB room of context scratch, from where
 * k_range_finish copies the wanted span.  Option "range_scratch_bytes"
 * (default 1 GiB, at least 128 KiB) caps the rooms alive at once: the host
 * cuts the ranges into consecutive groups whose edge blocks fit, the groups
 * run back to back on the stream and reuse the rooms.  The default is a bound
 * on memory, not a tuned number.
 * The call only enqueues - no look at the batch, no wait - and can be
 * captured into a hipGraph once the context's scratch has grown to the call's
 * size (a buffer that grows waits for the stream; all are reserved before the
 * first launch).  Info "range_pieces" (= snapmi_range_pieces of the host's
 * copies), "range_ranges_ok" and "range_ranges_failed" describe the last
 * call; reading the last two waits for it.
 */
SNAPMI_API uint64_t snapmi_range_pieces(const uint64_t *h_range_off,
                                        const uint64_t *h_range_len, size_t m);
SNAPMI_API int snapmi_decompress_ranges_indexed(
    snapmi_ctx *ctx, const void *const *d_in_ptrs, const uint64_t *d_in_lens,
    size_t n, const uint64_t *d_index_first /* [n+1] */,
    const uint64_t *d_index, uint64_t index_entries,
    const uint32_t *d_range_stream, const uint64_t *d_range_off,
    const uint64_t *d_range_len, const uint64_t *h_range_off,
    const uint64_t *h_range_len /* host copies */, void *const *d_range_out,
    uint64_t *d_range_got, snapmi_error *d_range_errs /* may be NULL */,
    size_t m);

/*
 * Range WRITES through the block index: bytes [off, off + len) of a stream's
 * OUTPUT are replaced, and only the 64 KiB blocks the writes touch go through
 * the codec.  Every encoder the index serves compresses each block on its
 * own, so the compressed bytes of a block no write touches stay valid byte
 * for byte: they are copied.
 *
 * snapmi_write_blocks: blocks the writes touch - a block that two
 * neighbouring writes of a stream share counts once; a write of len == 0, or
 * whose end passes 2^64, touches none; the sum saturates at 2^64 - 1.  Host
 * code.
 *
 * snapmi_write_ranges_indexed: write w puts h_write_src[w][0, len) (DEVICE
 * memory) at output bytes [off, off + len) of stream s = h_write_stream[w] of
 * the n streams (d_in_ptrs, d_in_lens) with the index (d_index_first, d_index,
 * index_entries).  A stream's length does not change, so neither does the
 * number of its entries: d_new_index is laid out by d_index_first.
 * The write lists are HOST arrays, read before the call returns; the device
 * gets the host's own copy of them.  What the device distrusts is the
 * streams, d_in_lens, d_index_first and the index.
 *   Host checks (SNAPMI_E_ARGUMENT with snapmi_last_error; nothing is
 *     enqueued, nothing written): a NULL pointer other than d_errs; writes not
 *     sorted by (stream, off), or overlapping; stream >= n; off + len wraps;
 *     m, or n + index_entries + snapmi_write_blocks(...), not below 2^31.  A
 *     write of len == 0 is ignored altogether; m == 0, or every write empty,
 *     enqueues nothing.
 *   Touched blocks.  A block one write covers entirely - [k * 65536,
 *     (k + 1) * 65536) lies inside it - is COVERED and compressed straight
 *     from the write's bytes.  Any other touched block is an EDGE block: its
 *     piece (see the range reads) is decoded into a 64 KiB room of scratch,
 *     the writes' bytes are laid over it, and it is compressed from there.
 *     Told from the writes alone: a stream's short last block is an edge
 *     block unless the write ends on a multiple of 65536.
 *   A stream no write names: nothing of d_out_ptrs[i] is written,
 *     d_out_lens[i] = 0 and the error kind is 0 - no valid stream has 0
 *     bytes, so 0 with OK means "keep the old one".  Its entries are copied.
 *   A stream that succeeds: d_out_ptrs[i][0, d_out_lens[i]) is varint(dlen)
 *     followed, for every block k, by what the compressor gives the patched
 *     block (without a varint) when k is touched and by the old bytes
 *     [entry k, entry k + 1) when it is not; the new entries are the varint's
 *     length and the running sums.  Exactly [0, d_out_lens[i]) is written.
 *     For a stream whose blocks are self-contained this is, bit for bit,
 *     snapmi_compress_batch_indexed of the patched data.  Untouched blocks
 *     are neither read as elements nor judged: for a foreign stream whose
 *     untouched block copies from across its boundary, the result decodes to
 *     whatever those bytes now decode to.
 *   A stream that fails: d_out_lens[i] = 0, NOT ONE BYTE of its buffer is
 *     written, and its old entries are copied to d_new_index - the new index
 *     stays right for the stream the caller keeps.  Why, in this order:
 *       the header does not parse      the error snapmi_decompress_len_batch
 *                                      gives the stream
 *       off + len > dlen               SNAPMI_E_ARGUMENT {off, len, dlen} of
 *                                      the first such write
 *       no usable index                the stream's rule of the range reads
 *         (SNAPMI_E_ARGUMENT {s, 0}), and entry k < entry k + 1 <= compressed
 *         length for EVERY block - each one is copied or replaced -
 *         (SNAPMI_E_ARGUMENT {s, first bad block})
 *       an edge block's piece fails or is not full   that piece's error as
 *         snapmi_decompress_ranges_indexed reports it, for the first such
 *         piece in block order
 *       cap < new length               SNAPMI_BUFFER_TOO_SMALL {cap, new
 *                                      length}; an exact cap passes
 *   Whatever the streams, d_in_lens, d_index_first and the index hold,
 *   nothing is written outside d_out_ptrs[i][0, cap_i), d_out_lens[0, n),
 *   d_errs[0, n) and d_new_index[0, index_entries), no input byte at or
 *   behind d_in_lens[i] and no entry at or behind index_entries is read.  If
 *   d_index_first is not a prefix sum the entries of d_new_index are
 *   unspecified, and each stream's own result still stands by its own rule.
 * Outputs (the buffers, d_out_lens, d_errs, d_new_index) must not overlap the
 * inputs, the old index or the writes' sources.
 * Everything runs on the context's stream.  The host waits only for scratch
 * that must grow, or for the event of its own earlier staging copy; capture
 * into a hipGraph is not promised.  Scratch per touched block: a compress
 * slot, and a room for an edge block; option "write_scratch_bytes" caps what
 * is alive at once - the host cuts the touched streams into consecutive
 * groups of whole streams that fit (a stream that exceeds it alone is a group
 * of its own), the groups run back to back and reuse the scratch.  Info
 * "write_blocks", "write_blocks_decoded", "write_streams_ok" and
 * "write_streams_failed" describe the last call; reading the last two waits
 * for it.
 */
SNAPMI_API uint64_t snapmi_write_blocks(const uint32_t *h_write_stream,
                                        const uint64_t *h_write_off,
                                        const uint64_t *h_write_len, size_t m);
SNAPMI_API int snapmi_write_ranges_indexed(
    snapmi_ctx *ctx, const void *const *d_in_ptrs, const uint64_t *d_in_lens,
    size_t n, const uint64_t *d_index_first /* [n+1] */,
    const uint64_t *d_index, uint64_t index_entries,
    const uint32_t *h_write_stream, const uint64_t *h_write_off,
    const uint64_t *h_write_len,
    const void *const *h_write_src /* HOST array of DEVICE pointers */,
    size_t m, void *const *d_out_ptrs, const uint64_t *d_out_caps,
    uint64_t *d_out_lens, snapmi_error *d_errs /* may be NULL */,
    uint64_t *d_new_index /* out, [index_entries] */);

/*
 * APPENDS through the block index: stream i gets the h_app_len[i] bytes at
 * h_app_src[i] (DEVICE memory) appended to its OUTPUT, and only the stream's
 * short last block and the new bytes go through the codec - every full old
 * block keeps its compressed bytes, which are copied.  h_app_len[i] == 0
 * means "not named".
 *
 * Host copies.  h_out_lens[i] is the length stream i's header announces, as
 * for snapmi_build_block_index; h_out_lens and h_app_len are required and
 * size the new index, the scratch and every launch.  The device never trusts
 * h_out_lens.  The append lists (h_app_src, h_app_len) are HOST arrays, read
 * before the call returns; the device gets the host's own copy of them.
 * New index.  Stream i owns ceil((h_out_lens[i] + h_app_len[i]) / 65536) + 1
 * entries, whatever becomes of it; d_new_index_first [n + 1] is the prefix sum
 * of those counts, written by the call, and their total is
 * snapmi_block_index_entries of the summed lengths.  new_index_cap below the
 * total is SNAPMI_E_ARGUMENT, and nothing is enqueued or written; entries at
 * or behind the total are never written.
 *   Host checks (SNAPMI_E_ARGUMENT with snapmi_last_error; nothing is
 *     enqueued, nothing written): a NULL pointer other than d_errs; a named
 *     stream with a NULL source; h_out_lens[i] + h_app_len[i] wraps;
 *     n + index_entries + new entries + new blocks not below 2^31.  n == 0
 *     enqueues nothing.  If every h_app_len is 0 the call still runs, and
 *     every stream is one nobody names.
 *   Blocks.  With dlen the old length and kf = dlen / 65536, blocks [0, kf)
 *     are the old FULL blocks: their compressed bytes [entry 0, entry kf) are
 *     copied, neither read as elements nor judged.  If dlen % 65536 != 0,
 *     block kf is the TAIL: its piece (see the range reads) is decoded into a
 *     64 KiB room of scratch, the first 65536 - dlen % 65536 appended bytes
 *     are laid behind it, and the room is compressed as the first new block.
 *     Every further new block is compressed straight from the source, 65536
 *     bytes each, the last one maybe shorter.  A stream whose old length is a
 *     multiple of 65536 - 0, the stream whose one entry is {1}, included -
 *     decodes nothing.
 *   A stream that succeeds: d_out_ptrs[i][0, d_out_lens[i]) is
 *     varint(dlen + add), the copied old bytes and, for every new block, what
 *     the compressor gives that block (without its varint); the new entries
 *     are the new varint's length and the running sums, the last one
 *     d_out_lens[i].  Exactly [0, d_out_lens[i]) is written.  For a stream
 *     whose blocks are self-contained this is, bit for bit,
 *     snapmi_compress_batch_indexed of the old data followed by the appended
 *     data (the varint may grow a byte: every entry then shifts).
 *   A stream nobody names: nothing of its buffer is written, d_out_lens[i] =
 *     0 and the error kind is 0 ("keep the old one", as for the writes).  Its
 *     old entries are copied to its place in the new index when d_index_first
 *     gives it exactly its count of entries inside [0, index_entries);
 *     otherwise its new entries are all 0.
 *   A stream that fails: d_out_lens[i] = 0, NOT ONE BYTE of its buffer is
 *     written, and all its new entries are 0 - the caller keeps the old
 *     stream and the old index.  Why, in this order:
 *       the header does not parse      the error snapmi_decompress_len_batch
 *                                      gives the stream
 *       it announces another length    SNAPMI_E_ARGUMENT {i, announced,
 *                                      h_out_lens[i]}
 *       dlen + add > 2^32 - 1          SNAPMI_TOO_BIG {dlen + add, 4294967295}
 *                                      (reference src/compress.rs,
 *                                      Encoder::compress)
 *       no usable index                the stream's rule of the range reads
 *         (SNAPMI_E_ARGUMENT {i, 0}), and entry k < entry k + 1 <= compressed
 *         length for every old block (SNAPMI_E_ARGUMENT {i, first bad block})
 *       the tail's piece fails or is not full   that piece's error as
 *         snapmi_decompress_ranges_indexed reports it
 *       cap < new length               SNAPMI_BUFFER_TOO_SMALL {cap, new
 *                                      length}; an exact cap passes
 *   Whatever the streams, d_in_lens, d_index_first and the index hold,
 *   nothing is written outside d_out_ptrs[i][0, cap_i), d_out_lens[0, n),
 *   d_errs[0, n), d_new_index_first[0, n] and d_new_index[0, total), no input
 *   byte at or behind d_in_lens[i] and no entry at or behind index_entries is
 *   read.
 * Outputs must not overlap the inputs, the old index or the sources.
 * Everything runs on the context's stream.  The host waits only for scratch
 * that must grow, or for the event of its own earlier staging copy; capture
 * into a hipGraph is not promised.  Scratch: a compress slot per new block and
 * a 64 KiB room per tail; option "write_scratch_bytes" caps what is alive at
 * once - the host cuts the named streams into consecutive groups of whole
 * streams that fit (a stream that exceeds it alone is a group of its own),
 * the groups run back to back and reuse the scratch.  Info "append_blocks",
 * "append_blocks_decoded", "append_streams_ok" and "append_streams_failed"
 * describe the last call; reading the last two waits for it.
 */
SNAPMI_API int snapmi_append_indexed(
    snapmi_ctx *ctx, const void *const *d_in_ptrs, const uint64_t *d_in_lens,
    const uint64_t *h_out_lens /* host copy: the length each header announces */,
    size_t n, const uint64_t *d_index_first /* [n+1] */,
    const uint64_t *d_index, uint64_t index_entries,
    const void *const *h_app_src /* HOST array of DEVICE pointers */,
    const uint64_t *h_app_len /* HOST */,
    void *const *d_out_ptrs, const uint64_t *d_out_caps,
    uint64_t *d_out_lens, snapmi_error *d_errs /* may be NULL */,
    uint64_t *d_new_index_first /* out, [n+1] */,
    uint64_t *d_new_index /* out */, uint64_t new_index_cap);

/*
 * The block index of streams that came WITHOUT one - written by the
 * reference, by libsnappy, by snapmi_compress_batch, read from a file - built
 * on the device from the streams alone, so that
 * snapmi_decompress_batch_indexed and snapmi_decompress_ranges_indexed serve
 * data that exists.  Nothing is decoded and no output buffer is needed.
 *
 * The rule (bi_build in csrc/snapmi_blockindex.hpp is its one definition).
 * A stream of at most one block (its header announces dlen <= 65536) is not
 * walked: a header that parses gives the entries {header bytes, compressed
 * length} - which the range call accepts - and SNAPMI_INDEX_BUILT; dlen == 0
 * has the one entry {header bytes}, and only when the stream is nothing but
 * its header (else SNAPMI_INDEX_CORRUPT).  A longer stream is walked from
 * element to element behind the varint, reading tag bytes and literal length
 * bytes only.  Copy offsets are NOT looked at: the builder finds boundaries
 * and gives no verdict on whether the stream decodes - the decoders distrust
 * every index, and a stream that fails there is found there, as today.
 *   SNAPMI_INDEX_BUILT (1)      every element fits inside the stream, the
 *     chain ends exactly at its end having produced exactly dlen, and for
 *     every k in 1 .. blocks - 1 an element starts where exactly k * 65536
 *     bytes have been produced.  Entries: the layout
 *     snapmi_compress_batch_indexed writes - the varint's length, those
 *     elements' offsets, the compressed length.
 *   SNAPMI_INDEX_UNALIGNED (2)  the chain is whole as above, but an element
 *     straddles a multiple of 65536.  All the stream's entries are 0.
 *   SNAPMI_INDEX_CORRUPT (3)    the header does not parse, an element does
 *     not fit, or the chain ends anywhere but at (compressed length, dlen).
 *     All entries 0.
 *   SNAPMI_INDEX_MISSIZED (4)   d_in_lens[i], or the length the header
 *     announces, is not what the host's copy said.  All entries 0.
 * Entries that are all 0 pass neither call's rule: such a stream is decoded
 * whole by snapmi_decompress_batch_indexed, and a range on it fails with "no
 * usable index".
 *
 * Host copies.  h_in_lens is the host's copy of d_in_lens, h_out_lens[i] the
 * length stream i's header announces (from snapmi_decompress_len_batch, or
 * the caller's metadata).  Both are required (NULL: SNAPMI_E_ARGUMENT,
 * nothing is enqueued).  They size the index, the scratch and every launch, as
 * h_range_off / h_range_len do for the range call; the device never trusts
 * them, and a stream they are wrong about is MISSIZED and keeps the
 * ceil(h_out_lens[i] / 65536) + 1 entries the host gave it, all 0.
 * Layout.  d_index_first [n + 1] is the prefix sum of those counts;
 * snapmi_block_index_entries(h_out_lens, n) is their total, the index_entries
 * the decode calls want.  index_cap below it is SNAPMI_E_ARGUMENT, and
 * nothing is enqueued or written.  d_status [n] (may be NULL) gets the
 * verdicts.
 * Bounds.  Entries at or behind d_index_first[n] are never written; nothing
 * outside d_index_first[0, n], d_index[0, entries) and d_status[0, n) is
 * written whatever the streams hold; no input byte at or behind h_in_lens[i]
 * is read; n + entries stays below 2^31 (SNAPMI_E_ARGUMENT); n == 0 writes
 * d_index_first[0] = 0 only.
 * Ordering.  Everything runs on the context's stream.  The call waits on the
 * host in two cases only: a scratch buffer has to grow (before the first
 * launch, as in every call of this section), or its own pinned staging is
 * still being read by a copy of an earlier call - it then waits for the event
 * of that copy, not for the stream.  Capture into a hipGraph is not promised.
 * There is no limit of 16 384 streams or 4 096 long ones: the streams of two
 * blocks and more are cut into groups whose descriptors and scan tables are
 * bounded whatever n is; the groups follow each other on the stream.
 * Info "index_build_built", "index_build_unaligned", "index_build_corrupt",
 * "index_build_missized" count the last call's verdicts and
 * "index_build_walked" the streams its sequential walker handled (those the
 * parallel scan gave up on); reading them waits for the call.
 */
enum snapmi_index_status {
    SNAPMI_INDEX_BUILT = 1,
    SNAPMI_INDEX_UNALIGNED = 2,
    SNAPMI_INDEX_CORRUPT = 3,
    SNAPMI_INDEX_MISSIZED = 4
};
SNAPMI_API int snapmi_build_block_index(
    snapmi_ctx *ctx, const void *const *d_in_ptrs, const uint64_t *d_in_lens,
    const uint64_t *h_in_lens, const uint64_t *h_out_lens /* host copies */,
    size_t n, uint64_t *d_index_first /* out, [n+1] */,
    uint64_t *d_index /* out */, uint64_t index_cap,
    uint8_t *d_status /* out, [n]; may be NULL */);

/*
 * ONE long raw stream, device resident, decoded by many wavefronts.
 * A raw stream has no index (reference src/decompress.rs:130-148 walks it
 * element by element) and snapmi_decompress_batch gives a stream to a single
 * wavefront; here the element chain is first resolved by a hierarchical scan
 * (4 KiB segments, 256 KiB super-segments, one short sequential pass), the
 * stream is cut at the element boundaries next to every 64 KiB of output,
 * and the pieces are decoded like independent streams.  Streams of this
 * encoder, the reference and libsnappy (64 KiB blocks) always take that
 * path; a stream whose pieces depend on each other (a copy reaching across a
 * cut), or with any error, is decoded by the sequential path, so results and
 * errors are those of snapmi_decompress_batch with n = 1.  Asynchronous on
 * the context's stream; d_out_len[0] / d_err[0] as in the batch call.
 * The scalar entry points use it for inputs of 32 KiB and more that announce
 * half as much output again (and 96 KiB or more), and from 256 KiB on for
 * any input - the rule snapmi_decompress_batch applies to the long streams
 * of a batch.
 */
SNAPMI_API int snapmi_decompress_stream(snapmi_ctx *ctx, const void *d_in,
                             uint64_t in_len, void *d_out, uint64_t out_cap,
                             uint64_t *d_out_len, snapmi_error *d_err);
/* Which way the last snapmi_decompress_stream on this context went (waits
 * for it): 0 = pieces on many wavefronts, 1 = the sequential path, -1 = no
 * such call yet.  For tests and benchmarks. */
SNAPMI_API int snapmi_stream_decode_path(snapmi_ctx *ctx);

/* decompress_len for n streams on the device (reference
 * src/decompress.rs:30-35): d_out_lens[i] = header value, d_errs[i] as the
 * reference would return. */
SNAPMI_API int snapmi_decompress_len_batch(snapmi_ctx *ctx,
                                const void *const *d_in_ptrs,
                                const uint64_t *d_in_lens,
                                uint64_t *d_out_lens, snapmi_error *d_errs,
                                size_t n);

/* Wait for everything enqueued on the context's stream. */
SNAPMI_API int snapmi_ctx_synchronize(snapmi_ctx *ctx);

/*
 * Timing of the last batch call, measured with HIP events recorded on the
 * context's stream around each kernel group.  Valid after synchronize.
 * Times in milliseconds; a group that did not run reports 0.
 */
typedef struct snapmi_timing {
    float plan_ms;     /* descriptor scan / block table kernels            */
    float codec_ms;    /* the dominant kernel: compress or decompress      */
    float compact_ms;  /* compress only: gather of blocks 1.. into place   */
    float total_ms;    /* first event to last event                        */
    uint64_t codec_launches; /* launches of the dominant kernel            */
    float dominant_ms; /* the single dominant kernel alone: k_match_blocks,
                          k_compress_blocks or k_decompress_streams         */
    float reserved;
} snapmi_timing;
SNAPMI_API int snapmi_last_timing(snapmi_ctx *ctx, snapmi_timing *out);

/* ------------------------------------------------------------------ */
/* 4. Snappy frame format on the device (reference src/frame.rs,        */
/*    src/crc32.rs, src/write.rs, src/read.rs).  One framed stream per  */
/*    call, or many independent ones per call (the *_batch calls);      */
/*    every <=64 KiB chunk is an independent raw stream, so the chunk   */
/*    is the parallel unit.  All d_* pointers are device memory.        */
/*    Asynchronous like the batch calls.                                */
/* ------------------------------------------------------------------ */

/* Upper bound of snapmi_frame_compress output for n input bytes:
 * stream identifier + per chunk (8-byte header + at most the chunk itself,
 * because of the uncompressed fallback of reference src/frame.rs:85). */
SNAPMI_API size_t snapmi_frame_max_len(size_t n);

/*
 * What write::FrameEncoder::write_all(input) followed by into_inner()
 * produces (reference src/write.rs:123-192 chunking, src/frame.rs:62-104
 * compress_frame, src/crc32.rs:35-38 masked CRC32C of the uncompressed chunk):
 *   d_out_len[0]        : framed length (0 for empty input, as the reference)
 *   d_chunk_offsets     : optional [chunks+1] offsets of every chunk header
 *                         in d_out (a side index; not part of the stream)
 */
SNAPMI_API int snapmi_frame_compress(snapmi_ctx *ctx, const void *d_in, uint64_t in_len,
                          void *d_out, uint64_t out_cap, uint64_t *d_out_len,
                          uint64_t *d_chunk_offsets);

/*
 * read::FrameDecoder over the whole stream (reference src/read.rs:105-238):
 * stream identifier, chunk types, length limits, raw decode, CRC check.
 *   d_chunk_offsets/n_chunks : optional side index of the chunk headers
 *                         (as written by snapmi_frame_compress); without it
 *                         the headers are walked on the device, one after
 *                         the other (the format has no index)
 *   d_out == NULL       : only compute the decompressed length
 *   d_out_len[0]        : decompressed length; on an error the bytes in
 *                         front of the failing chunk (see _ex below)
 *   d_err[0]            : first error in stream order (kind 0 = ok);
 *                         an io::ErrorKind::UnexpectedEof is reported as
 *                         SNAPMI_E_UNEXPECTED_EOF
 */
SNAPMI_API int snapmi_frame_decompress(snapmi_ctx *ctx, const void *d_in,
                            uint64_t in_len, void *d_out, uint64_t out_cap,
                            uint64_t *d_out_len, snapmi_error *d_err,
                            const uint64_t *d_chunk_offsets,
                            uint64_t n_chunks);

/*
 * n independent framed streams per call, in the shape of the raw batch calls
 * of section 3.  Stream i's result is exactly what the one-stream call gives
 * for stream i alone; the batch adds nothing and no stream affects another.
 * The chunks of all streams are compressed / decoded as one list.
 *
 * snapmi_frame_compress_batch: stream i == snapmi_frame_compress(
 * d_in_ptrs[i], d_in_lens[i]), i.e. one write::FrameEncoder::write_all(input)
 * followed by into_inner() (reference src/write.rs:123-192, src/frame.rs:62-104).
 *   h_in_lens      host copy of d_in_lens (sizes the launches); NULL = fetched
 *                  with a blocking D2H
 *   d_out_caps     NULL = not checked; else cap_i < snapmi_frame_max_len(len_i)
 *                  (len_i > 0) makes stream i fail with SNAPMI_BUFFER_TOO_SMALL
 *                  {a = cap_i, b = snapmi_frame_max_len(len_i)}, d_out_lens[i]
 *                  = 0 and nothing written to d_out_ptrs[i]
 *   d_out_lens[i]  framed length (0 for an empty input: the identifier is
 *                  written lazily, src/write.rs:154-170)
 *   d_errs         per-stream snapmi_error; may be NULL
 * Asynchronous (enqueue-only) like snapmi_compress_batch, except for the
 * blocking D2H of a NULL h_in_lens.
 *
 * snapmi_frame_decompress_batch: for every i, d_out_lens[i], d_errs[i] and
 * the bytes d_out_ptrs[i][0, d_out_lens[i]) equal what
 * snapmi_frame_decompress(stream i, d_out_ptrs[i], d_out_caps[i], no index)
 * gives, i.e. one read::FrameDecoder over the stream (reference
 * src/read.rs:105-238): the first error in stream order, the bytes in front
 * of the failing chunk, BufferTooSmall {cap, total} when the output does not
 * fit (then nothing is decoded).  Every stream starts a fresh reader.
 *   d_out_ptrs     NULL = lengths only (d_out == NULL of the one-stream
 *                  call); d_out_caps may then be NULL
 *   d_errs         may be NULL
 * Waits once for the context's stream (the count of data chunks sizes the
 * decode), so it is not enqueue-only and cannot be captured into a hipGraph.
 * The chunk headers of a stream are walked by one thread (~0.7 us per
 * chunk): a stream of many thousands of chunks is better decoded on its own
 * with snapmi_frame_decompress, whose walk is parallel.
 *
 * Both: n and the total number of chunks below 2^31 (else SNAPMI_E_ARGUMENT
 * and snapmi_last_error); n == 0 enqueues nothing.  snapmi_last_kernel and
 * snapmi_last_timing describe the raw codec launch over the chunk list, as
 * for the one-stream frame calls.
 */
SNAPMI_API int snapmi_frame_compress_batch(snapmi_ctx *ctx,
                                const void *const *d_in_ptrs,
                                const uint64_t *d_in_lens,
                                const uint64_t *h_in_lens,
                                void *const *d_out_ptrs,
                                const uint64_t *d_out_caps,
                                uint64_t *d_out_lens, snapmi_error *d_errs,
                                size_t n);
SNAPMI_API int snapmi_frame_decompress_batch(snapmi_ctx *ctx,
                                  const void *const *d_in_ptrs,
                                  const uint64_t *d_in_lens,
                                  void *const *d_out_ptrs,
                                  const uint64_t *d_out_caps,
                                  uint64_t *d_out_lens, snapmi_error *d_errs,
                                  size_t n);

/* ------------------------------------------------------------------ */
/* 4b. Many independent framed streams in HOST memory per call.         */
/* ------------------------------------------------------------------ */
/*
 * The two batch calls above on host buffers, in one blocking call each - how
 * a directory of .sz files is packed and unpacked.  For every i,
 * h_out_lens[i], h_errs[i] (variant and fields a, b, c) and the bytes
 * h_out_ptrs[i][0, h_out_lens[i]) are exactly what snapmi_frame_compress_batch
 * / snapmi_frame_decompress_batch give for stream i alone with capacity
 * h_out_caps[i]: one write::FrameEncoder::write_all + into_inner, or one
 * read::FrameDecoder read to its end.  No stream affects another, and nothing
 * is ever written behind h_out_lens[i].
 *   compress     cap_i < snapmi_frame_max_len(len_i) with len_i > 0: stream i
 *                fails with SNAPMI_BUFFER_TOO_SMALL {cap_i, max_len}, its
 *                length is 0 and its buffer is untouched; an empty input
 *                gives length 0 and OK (no identifier)
 *   decompress   on an error h_out_lens[i] is the number of bytes in front of
 *                the failing chunk, and those bytes are delivered, as in the
 *                device call; an output that does not fit is BufferTooSmall
 *                {cap, total} and nothing is written
 *   h_out_ptrs   decompress: NULL = lengths only - h_out_lens[i] gets the
 *                decoded length of stream i; h_out_caps may then be NULL
 *   return value failures of the call itself only (SNAPMI_E_DEVICE,
 *                SNAPMI_E_ARGUMENT)
 *   h_errs       may be NULL
 *   n            below 2^31, and so is the number of chunks of a slice;
 *                n == 0 does nothing
 * The buffers may be pageable or pinned (snapmi_host_alloc).
 *
 * The pipeline is that of section 2b (slices cut by "host_batch_slice", one
 * copy in, packed output home; info "host_batch_slices",
 * "host_batch_h2d_bytes", "host_batch_d2h_bytes" describe the last call of any
 * of the four).  Decompress: the host walks the chunk headers of every stream
 * before it sends it (the walk of snapmi_frame_decompress_batch, compiled for
 * the host), which gives the room of every stream in the output slab - only
 * decoded bytes come home - and, for a slice whose streams are all
 * well-formed, the chunk list: it travels with the inputs, one thread per
 * chunk checks it against the bytes on the device (k_fbd_from_list), and the
 * device neither walks the streams (0.7 us per chunk on one thread) nor makes
 * the host wait for a chunk count.  A slice that holds a malformed stream is
 * decoded by snapmi_frame_decompress_batch as it is.  Verdicts, lengths and
 * error fields come from the device either way; a list that disagrees with
 * the bytes fails the call (SNAPMI_E_DEVICE).  Info "host_batch_listed_slices":
 * slices of the last call decoded from the list.
 */
SNAPMI_API int snapmi_frame_compress_batch_host(snapmi_ctx *ctx,
                                     const void *const *h_in_ptrs,
                                     const size_t *h_in_lens,
                                     void *const *h_out_ptrs,
                                     const size_t *h_out_caps,
                                     size_t *h_out_lens, snapmi_error *h_errs,
                                     size_t n);
SNAPMI_API int snapmi_frame_decompress_batch_host(snapmi_ctx *ctx,
                                       const void *const *h_in_ptrs,
                                       const size_t *h_in_lens,
                                       void *const *h_out_ptrs,
                                       const size_t *h_out_caps,
                                       size_t *h_out_lens,
                                       snapmi_error *h_errs, size_t n);

/* flags of the frame entry points below */
#define SNAPMI_FRAME_NO_IDENT 1u     /* compress: do not emit the identifier */
#define SNAPMI_FRAME_CONTINUATION 1u /* decode: identifier already seen      */

/*
 * write::FrameEncoder with the chunk boundaries chosen by the caller: the
 * reference cuts a chunk wherever a flush, a direct write larger than its
 * 64 KiB buffer, or a short read of read::FrameEncoder ends it
 * (src/write.rs:123-192, src/read.rs:365-409), so chunks of a stream are not
 * always 65536 bytes.  Chunk i is the next h_chunk_lens[i] (1..65536) bytes
 * of d_in; each goes through compress_frame (src/frame.rs:62-104).  With
 * SNAPMI_FRAME_NO_IDENT the 10-byte stream identifier is not written (a
 * later batch of the same stream, src/write.rs:167-170).  out_cap >=
 * 10 + sum(lens) + 8 n.  h_chunk_lens is host memory, read before the call
 * returns; the rest is asynchronous like snapmi_frame_compress.
 */
SNAPMI_API int snapmi_frame_compress_chunks(snapmi_ctx *ctx, const void *d_in,
                                 const uint32_t *h_chunk_lens, size_t n,
                                 uint32_t flags, void *d_out, uint64_t out_cap,
                                 uint64_t *d_out_len,
                                 uint64_t *d_chunk_offsets);

/*
 * snapmi_frame_decompress for one BATCH of a stream a host reader delivers
 * piecewise (read::FrameDecoder decodes chunk by chunk, src/read.rs:105-238):
 *   flags    SNAPMI_FRAME_CONTINUATION: the stream identifier was seen in an
 *            earlier batch (read.rs:123-128)
 *   stale10  NULL, or the first 10 bytes of the reference reader's scratch
 *            buffer as earlier batches left them (snapmi_frame_scan_host
 *            maintains them): the reference parses a compressed chunk's
 *            length header from that whole buffer (read.rs:216), so a payload
 *            of fewer than 10 bytes without a varint terminator is judged
 *            together with those bytes.  NULL = a fresh reader (zeros).
 * On an error d_out_len[0] is the number of output bytes IN FRONT of the
 * failing chunk: they are decoded and CRC-checked, and the reference's
 * reader has returned them before it reports the error.  The side index is
 * a hint: if it does not tile [identifier, in_len) with plain data chunks,
 * or a chunk needs the stale-buffer rule, the headers are walked instead.
 *
 * Without SNAPMI_FRAME_NO_WAIT the call waits for the context's stream once
 * or more: the host sizes the chunk table and the launches from a chunk count
 * that only the device knows.  With it the caller bounds that count and the
 * call only enqueues:
 *   n_chunks  a promise: the stream holds at most n_chunks data chunks (types
 *             0x00 and 0x01) in front of its first structural error - from
 *             the index snapmi_frame_compress wrote, snapmi_frame_index_host,
 *             snapmi_frame_scan_host, or ceil(decoded length / 65536).  At
 *             most 2^31 - 1 (else SNAPMI_E_ARGUMENT, nothing is enqueued).
 *   d_chunk_offsets  may be NULL (n_chunks is then only the bound); if given
 *             it has n_chunks + 1 entries and is the hint it always is,
 *             checked and never trusted.  No entry behind n_chunks is read.
 * While the promise holds, d_out_len[0], d_err[0] and the bytes d_out[0,
 * d_out_len[0]) are those of the same call without the flag - whatever the
 * index contains and however generous the bound: the bytes in front of a
 * failing chunk, BufferTooSmall {cap, total}, SNAPMI_FRAME_CONTINUATION,
 * stale10 and d_out == NULL (lengths only) included.  When it is broken -
 * more data chunks than n_chunks - d_err[0] = {SNAPMI_E_ARGUMENT, a = the
 * data chunks counted, b = n_chunks}, d_out_len[0] = 0 and d_out[0, out_cap)
 * is unspecified; this verdict wins over every other.  Nothing outside
 * d_out[0, out_cap), d_out_len[0] and d_err[0] is written and no input byte
 * at or behind in_len is read, either way.
 * The fronts that find the chunks are enqueued back to back and the order on
 * the stream alone lets the first that decides win: the side index if one is
 * given, else the parallel walk for in_len >= "frame_parallel_walk_min",
 * then the sequential walk (behind an index that fails its check it is the
 * sequential walk alone that decides, whatever in_len).  Info
 * "frame_nowait_front" tells which it was.  The host waits only for scratch
 * that must grow and, in a context's first frame call, for the CRC tables; a
 * call that has run once eagerly can be captured into a hipGraph, and a
 * replay decodes whatever bytes and index values then lie in the same buffers
 * at that in_len.  A generous bound costs scratch and empty threads: 153
 * bytes of chunk table and 4 of the raw decoder's plan per chunk of the bound,
 * used or not - 177 measured, with the eighth the grow-only buffers add (a
 * 1 GiB stream of 16 384 chunks under a bound of 65 536: 11.9 MB of scratch
 * instead of 3.2 MB, and 3.96 ms instead of 3.86 ms).
 */
#define SNAPMI_FRAME_NO_WAIT 4u   /* decode: n_chunks bounds the data chunks; the call only enqueues */
SNAPMI_API int snapmi_frame_decompress_ex(snapmi_ctx *ctx, const void *d_in,
                               uint64_t in_len, void *d_out, uint64_t out_cap,
                               uint64_t *d_out_len, snapmi_error *d_err,
                               const uint64_t *d_chunk_offsets,
                               uint64_t n_chunks, uint32_t flags,
                               const uint8_t *stale10);

/*
 * Host-side scan for a reader that delivers the stream piecewise: walks the
 * chunk headers of h_in[0, in_len) as far as chunks are complete and
 * well-formed.  *consumed = end of the last such chunk, *n_chunks = data
 * chunks in front of it, h_offsets (optional, cap >= n + 1) = their header
 * offsets followed by *consumed, stale10 (optional, 10 bytes, in/out) = the
 * reference reader's src[0..10) after those chunks.  Returns 0 when
 * consumed == in_len, 2 when the next chunk is cut off by in_len (read more,
 * or at end of input hand the rest to the device: UnexpectedEof), 1 when the
 * next chunk's header is one the decoder rejects (hand [consumed, ...) to
 * the device without an index: it reports the reference's error), or
 * SNAPMI_E_ARGUMENT.  No GPU work.
 */
SNAPMI_API int snapmi_frame_scan_host(const void *h_in, uint64_t in_len, uint32_t flags,
                           uint8_t *stale10, uint64_t *h_offsets,
                           uint64_t cap, uint64_t *n_chunks,
                           uint64_t *consumed);

/*
 * Host-buffer forms of the two calls above (blocking: H2D, kernels, D2H
 * through the context's staging buffers) - what a host-language
 * FrameEncoder / FrameDecoder calls once per batch of chunks (shim/src/
 * write.rs, read.rs; rust-snappy_amd/frame.py; tools/szip.cpp).
 *
 * snapmi_frame_encode_host: chunks as in snapmi_frame_compress_chunks, from
 * h_in back to back; out_cap >= snapmi_frame_encode_bound(sum, n).
 *
 * snapmi_frame_decode_host: decodes the complete, well-formed chunks at the
 * start of h_in[0, in_len) - as many as out_cap / 65536 allows - and reports
 * how far it got: *consumed input bytes, *written output bytes.  Call it again
 * with the rest (plus more input) and SNAPMI_FRAME_CONTINUATION.
 *   consumed == 0 and kind OK : not one whole chunk yet, supply more input
 *   SNAPMI_FRAME_FINAL        : no more input will follow: a cut-off chunk is
 *                               UnexpectedEof instead of "supply more"
 *   on an error (return value = *err's kind) *written bytes in front of the
 *   failing chunk are valid output and must be delivered first
 *   (src/read.rs:111-118); *consumed stays 0.
 *   stale10: 10 bytes of decoder state kept by the caller between calls
 *   (zeros for a new stream), see snapmi_frame_decompress_ex.
 */
#define SNAPMI_FRAME_FINAL 2u
SNAPMI_API size_t snapmi_frame_encode_bound(size_t total_bytes, size_t n_chunks);
SNAPMI_API int snapmi_frame_encode_host(snapmi_ctx *ctx, const uint8_t *h_in,
                             const uint32_t *h_chunk_lens, size_t n,
                             uint32_t flags, uint8_t *h_out, size_t out_cap,
                             size_t *written);
SNAPMI_API int snapmi_frame_decode_host(snapmi_ctx *ctx, const uint8_t *h_in,
                             size_t in_len, uint32_t flags, uint8_t *stale10,
                             uint8_t *h_out, size_t out_cap, size_t *written,
                             size_t *consumed, snapmi_error *err);

/* Host-side chunk scan of a framed stream that is still in HOST memory: the
 * hops FrameDecoder::read makes while it reads (src/read.rs:105-172).  The
 * format is a linked list of chunk headers; on the device every hop is a
 * dependent HBM access (~0.7 us), on the host it is free while the bytes are
 * being staged.  Writes the offsets of the DATA chunk headers (types 0x00 and
 * 0x01) and, last, in_len: n + 1 values; copy them to the device and pass
 * them as d_chunk_offsets.  h_offsets may be NULL to count only.
 * Returns 0 and *n_chunks for a structurally regular stream (identifier
 * first; data, skippable, padding and repeated identifier chunks; ends on a
 * chunk boundary; every length within the format's limits), 1 otherwise or
 * when `cap` < n + 1: decode such a stream WITHOUT an index and the device
 * walk reports the reference's error.  No GPU work. */
SNAPMI_API int snapmi_frame_index_host(const void *h_in, uint64_t in_len,
                            uint64_t *h_offsets, uint64_t cap,
                            uint64_t *n_chunks);

/* Masked CRC32C (reference CheckSummer::crc32c_masked, src/crc32.rs:35-38)
 * of n buffers of any length: d_out[i] is the masked CRC32C of
 * d_ptrs[i][0, d_lens[i]) for any d_lens[i] below 2^64 that the memory really
 * holds.  The pointer may have any alignment; length 0 is valid (the pointer
 * is then not used).
 *   Buffers of at most 65536 bytes are computed by the kernel of the frame
 * codec's chunks, one wavefront a buffer.  A longer buffer is cut into
 * segments of 128 KiB that the whole device shares, one wavefront a segment
 * at a time: 1 GiB in one buffer runs as wide as 1 GiB in 16 384.
 *   Host: the call only enqueues on the context's stream.  d_ptrs, d_lens and
 * d_out are device memory and the host never reads them: no copy to the host,
 * no wait, no look at the batch.  Every launch and the call's scratch (12
 * bytes a buffer) are sized from n and the device's CU count alone; the host
 * waits only when that scratch must grow (and, in a context's first frame or
 * CRC call, for the CRC tables), before the first launch, as in every call of
 * this section.
 *   Graphs: once a call with this n or more has run, the call can be captured
 * into a hipGraph; a replay over other lengths (and pointers, and bytes) in
 * the same arrays gives the CRCs of those.  The launches form one serial
 * chain on the context's stream; there is no side stream.
 *   No byte outside [d_ptrs[i], d_ptrs[i] + d_lens[i]) is read and nothing
 * outside d_out[0, n) is written.  n < 2^31; n == 0 enqueues nothing. */
SNAPMI_API int snapmi_crc32c_masked_batch(snapmi_ctx *ctx, const void *const *d_ptrs,
                               const uint64_t *d_lens, uint32_t *d_out,
                               size_t n);

/* ------------------------------------------------------------------ */
/* 5. Multi-GPU: the one exchange step of the path.         */
/*                                                                      */
/* Raw streams and frame chunks are independent, so N GPUs shard a job  */
/* with no exchange during compute: rank r frames a contiguous range of */
/* chunks with snapmi_frame_compress[_chunks] (ranks behind the first   */
/* pass SNAPMI_FRAME_NO_IDENT, or drop the 10-byte identifier), and the */
/* concatenation of the parts in rank order is the single-stream        */
/* framing the reference's writer produces (src/write.rs:165-192).      */
/* snapmi_gatherv assembles it on one rank over RCCL (xGMI inside a     */
/* node): sizes first, then ONE group of point-to-point transfers       */
/* straight into the root's buffer at every rank's prefix offset, so    */
/* the root's links receive in parallel.  librccl is opened at run time */
/* (dlopen); a process that already holds one (PyTorch) shares it.      */
/* ------------------------------------------------------------------ */
#define SNAPMI_COMM_ID_BYTES 128
typedef struct snapmi_comm snapmi_comm;

/* A fresh rendezvous id (ncclGetUniqueId): call on ONE rank, hand the 128
 * bytes to the others by any means (file, socket, MPI, torch store). */
SNAPMI_API int snapmi_comm_unique_id(uint8_t id_out[SNAPMI_COMM_ID_BYTES]);
/* Collective: every rank calls it with the same id and world, its own rank,
 * and a context on the GPU it drives (one process per GPU). */
SNAPMI_API int snapmi_comm_init(snapmi_ctx *ctx, const uint8_t id[SNAPMI_COMM_ID_BYTES],
                     int rank, int world, snapmi_comm **out);
/* Or use a communicator the host already has (an ncclComm_t, as void *);
 * it is not destroyed by snapmi_comm_destroy. */
SNAPMI_API int snapmi_comm_wrap(snapmi_ctx *ctx, void *nccl_comm, int rank, int world,
                     snapmi_comm **out);
SNAPMI_API void snapmi_comm_destroy(snapmi_comm *comm);
/* Collective, blocking.  Every rank contributes d_send[0, send_bytes) (device
 * memory, may be empty); on `root`, d_recv[0, *total) receives the parts in
 * rank order.  h_sizes (host, [world], may be NULL) and *total are filled on
 * EVERY rank.  recv_cap matters on the root only; if the parts do not fit,
 * every rank returns SNAPMI_E_ARGUMENT and nothing is exchanged. */
SNAPMI_API int snapmi_gatherv(snapmi_ctx *ctx, snapmi_comm *comm, int root,
                   const void *d_send, uint64_t send_bytes, void *d_recv,
                   uint64_t recv_cap, uint64_t *h_sizes, uint64_t *total);

#ifdef __cplusplus
}
#endif
#endif /* SNAPMI_H */
