// snapmi_api.hip -- host side of the C ABI declared in include/snapmi.h: the
// context (create, destroy, options, info, errors) and the scalar calls.  The
// launchers are in snapmi_launch.hip, the lane tables in
// snapmi_lanetables.hip, long streams in snapmi_longstream.hip, the block
// index in snapmi_index.hip, writes and appends through it in
// snapmi_update.hip, the libsnappy seam in snapmi_seam.hip.
//
// Nothing here computes Snappy on the CPU: the only host-side arithmetic is
// the header varint parse (decompress_len) and max_compress_len, which the
// reference also treats as free-standing helpers (src/compress.rs:42-53,
// src/decompress.rs:30-35).  Every compress/decompress entry point launches
// the HIP kernels and fails with SNAPMI_E_DEVICE when there is no GPU.
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <string_view>
#include <vector>

#include "snapmi.h"
#include "snapmi_test.h"
#include "snapmi_ctx.hpp"
#include "snapmi_launch.hpp"
#ifdef SNAPMI_TESTING
#include "snapmi_hostpipe.hpp" // "scratch_fill" reaches the pipe's slots
#endif
#include "snapmi_device.hpp"
#include "snapmi_kernels.hpp"

using namespace snapmi;

namespace {

void set_err(snapmi_error *e, int kind, uint64_t a = 0, uint64_t b = 0,
             uint64_t c = 0)
{
    if (e) {
        e->kind = kind;
        e->reserved = 0;
        e->a = a;
        e->b = b;
        e->c = c;
    }
}

} // namespace

namespace snapmi {
// reference bytes::read_varu64, src/bytes.rs:73-90
size_t host_varint(const uint8_t *p, size_t n, uint64_t *value)
{
    uint64_t acc = 0;
    unsigned shift = 0;
    for (size_t i = 0; i < n; i++) {
        uint8_t b = p[i];
        if (shift >= 64)
            return 0;
        if (b < 0x80) {
            *value = acc | ((uint64_t)b << shift);
            return i + 1;
        }
        acc |= (uint64_t)(b & 0x7F) << shift;
        shift += 7;
    }
    return 0;
}

// option release_scratch: the compressor's per-batch scratch goes back to
// the allocator.  Only behind a synchronisation of ctx->stream (nothing of a
// batch is in flight): snapmi_ctx_synchronize and the scalar / libsnappy
// entry points, which wait for their result anyway.  (The buffers stay
// listed in the context: reserve gives them memory again.)
int release_batch_scratch(snapmi_ctx *ctx)
{
    if (!ctx->release_scratch)
        return SNAPMI_OK;
    for (DevBuf *b : {&ctx->tokens, &ctx->tok_pages, &ctx->tok_stage,
                      &ctx->ntok, &ctx->sched, &ctx->slots}) {
        if (b->p) {
            HIP_TRY(ctx, hipFree(b->p));
            b->p = nullptr;
            b->cap = 0;
        }
    }
    return SNAPMI_OK;
}
} // namespace snapmi

extern "C" {

const char *snapmi_version(void) { return "snapmi 0.1.0 gfx950"; }

int snapmi_ctx_create(int device, void *hip_stream, snapmi_ctx **out)
{
    if (!out)
        return SNAPMI_E_ARGUMENT;
    *out = nullptr;
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count <= 0 || device < 0 || device >= count) {
        fprintf(stderr,
                "snapmi: no usable HIP device (requested %d, %d visible: "
                "%s); the codec has no CPU fallback\n",
                device, count, hipGetErrorString(e));
        return SNAPMI_E_DEVICE;
    }
    if (hipSetDevice(device) != hipSuccess)
        return SNAPMI_E_DEVICE;
    snapmi_ctx *ctx = new (std::nothrow) snapmi_ctx();
    if (!ctx)
        return SNAPMI_E_DEVICE;
    ctx->device = device;
    {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, device) != hipSuccess) {
            delete ctx;
            return SNAPMI_E_DEVICE;
        }
        ctx->num_cus = prop.multiProcessorCount;
    }
    // experiment knobs from the environment (tests/hw drivers): only for a
    // process that says SNAPMI_TESTING=1 - a production host sets what it
    // needs through snapmi_ctx_set_option
#ifdef SNAPMI_TESTING // (the test build, libsnapmi_test.so: Makefile)
    if (getenv("SNAPMI_TESTING")) {
        if (const char *e = getenv("SNAPMI_LANE_WAVES")) {
            const int v = atoi(e);
            ctx->lane_waves_per_cu = (uint32_t)(v < 1 ? 1 : (v > 32 ? 32 : v));
        }
        if (const char *e = getenv("SNAPMI_LANE_SEGMENT_BLOCKS")) {
            const long v = atol(e);
            ctx->lane_segment_blocks = (uint32_t)(v < 64 ? 64 : v);
        }
        if (const char *e = getenv("SNAPMI_LANE_TABLE_SPREAD"))
            ctx->lane_table_spread = atoi(e) != 0;
        if (const char *e = getenv("SNAPMI_LANE_MIN_BLOCKS")) {
            const long v = atol(e);
            ctx->lane_min_blocks = (uint32_t)(v < 1 ? 1 : v);
        }
        if (const char *e = getenv("SNAPMI_FRAME_CRC_SIDE"))
            ctx->frame_crc_side_stream = atoi(e) != 0;
        if (const char *e = getenv("SNAPMI_LANE_UNCACHED"))
            ctx->lane_tables_uncached = atoi(e) != 0;
        if (const char *e = getenv("SNAPMI_HOST_COPY_KERNEL"))
            ctx->host_copy_kernel = atoi(e) & 3;
        if (const char *e = getenv("SNAPMI_HOST_ENCODE_SLICE"))
            ctx->host_encode_slice = (uint64_t)atoll(e) < 65536
                                         ? 65536
                                         : (uint64_t)atoll(e);
        if (const char *e = getenv("SNAPMI_HOST_DECODE_CHUNKS"))
            ctx->host_decode_slice_chunks =
                atoll(e) < 1 ? 1 : (uint64_t)atoll(e);
        if (const char *e = getenv("SNAPMI_DECODE_KERNEL"))
            ctx->decode_kernel = atoi(e) == 0 ? 0 : (atoi(e) == 2 ? 2 : 3);
        if (const char *e = getenv("SNAPMI_SPAN_KERNEL"))
            ctx->span_kernel = atoi(e) != 0;
        if (const char *m = getenv("SNAPMI_COMPRESS"))
            ctx->compress_mode = strcmp(m, "waves") == 0
                                     ? 0
                                     : (strcmp(m, "lanes") == 0 ? 1 : 2);
    }
#endif
    if (hip_stream) {
        ctx->stream = (hipStream_t)hip_stream;
    } else {
        if (hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) !=
            hipSuccess) {
            delete ctx;
            return SNAPMI_E_DEVICE;
        }
        ctx->owns_stream = true;
    }
    for (auto &ev : ctx->ev) {
        if (hipEventCreate(&ev) != hipSuccess) {
            snapmi_ctx_destroy(ctx);
            return SNAPMI_E_DEVICE;
        }
    }
    if (hipStreamCreateWithFlags(&ctx->stream2, hipStreamNonBlocking) !=
            hipSuccess ||
        hipEventCreateWithFlags(&ctx->ev_fork, hipEventDisableTiming) !=
            hipSuccess ||
        hipEventCreateWithFlags(&ctx->ev_join, hipEventDisableTiming) !=
            hipSuccess ||
        hipEventCreateWithFlags(&ctx->ev_crc[0], hipEventDisableTiming) !=
            hipSuccess ||
        hipEventCreateWithFlags(&ctx->ev_crc[1], hipEventDisableTiming) !=
            hipSuccess) {
        snapmi_ctx_destroy(ctx);
        return SNAPMI_E_DEVICE;
    }
    // Hardware self-check the wavefront-per-block compressor rests on (one
    // tiny kernel): without the ascending-lane order of DS atomics that
    // kernel would silently emit non-reference streams, so a context on such
    // a device compresses with the lane-per-block kernel only.
    {
        uint32_t bad = 1;
        if (reserve(ctx, ctx->ticket, 64) != SNAPMI_OK ||
            hipMemsetAsync(ctx->ticket.p, 0, 64, ctx->stream) != hipSuccess) {
            snapmi_ctx_destroy(ctx);
            return SNAPMI_E_DEVICE;
        }
        // (a launch that fills the chip: the properties are checked under
        // the LDS contention of the real kernels)
        hipLaunchKernelGGL(k_probe_lds_order,
                           dim3((uint32_t)(ctx->num_cus > 0 ? ctx->num_cus * 32
                                                             : 32)),
                           dim3(64), 0, ctx->stream,
                           (uint32_t *)ctx->ticket.p);
        if (hipMemcpyAsync(&bad, ctx->ticket.p, 4, hipMemcpyDeviceToHost,
                           ctx->stream) != hipSuccess ||
            hipStreamSynchronize(ctx->stream) != hipSuccess) {
            fprintf(stderr, "snapmi: LDS order self-check did not run: %s\n",
                    hipGetErrorString(hipGetLastError()));
            snapmi_ctx_destroy(ctx);
            return SNAPMI_E_DEVICE;
        }
        ctx->lds_order_ok = ctx->lds_order_hw = (bad & 1) == 0;
        if (bad & 2) { // the element-major decoder needs ordered DS stores
            ctx->lds_store_order_ok = false;
            ctx->decode_kernel = 0;
            fprintf(stderr,
                    "snapmi: this device does not apply overlapping lanes of "
                    "one DS store in ascending lane order; streams are "
                    "decoded one element at a time\n");
        }
        if (!ctx->lds_order_ok)
            fprintf(stderr,
                    "snapmi: this device does not apply the lanes of one DS "
                    "atomic in ascending lane order; the wavefront-per-block "
                    "compressor is disabled (lane-per-block kernel only)\n");
    }
    *out = ctx;
    return SNAPMI_OK;
}

void snapmi_ctx_destroy(snapmi_ctx *ctx)
{
    if (!ctx)
        return;
    (void)hipSetDevice(ctx->device);
    if (ctx->stream)
        (void)hipStreamSynchronize(ctx->stream);
    host_pipe_destroy(ctx);
    for (PinBuf *b : ctx->pin_bufs)
        if (b->p)
            (void)hipHostFree(b->p);
    if (ctx->h_mail)
        (void)hipHostFree((void *)ctx->h_mail);
    if (ctx->h_ratio)
        (void)hipHostFree((void *)ctx->h_ratio);
    if (ctx->h_tokstat)
        (void)hipHostFree((void *)ctx->h_tokstat);
    snapmi::free_lane_tables(ctx);
    for (DevBuf *b : ctx->dev_bufs)
        if (b->p)
            (void)hipFree(b->p);
    for (hipEvent_t ev :
         {ctx->ev_ib, ctx->ev_ibg[0], ctx->ev_ibg[1], ctx->wr.ev, ctx->ap.ev})
        if (ev)
            (void)hipEventDestroy(ev);
    for (auto &ev : ctx->ev)
        if (ev)
            (void)hipEventDestroy(ev);
    if (ctx->stream2) {
        (void)hipStreamSynchronize(ctx->stream2);
        (void)hipStreamDestroy(ctx->stream2);
    }
    if (ctx->ev_fork)
        (void)hipEventDestroy(ctx->ev_fork);
    if (ctx->ev_join)
        (void)hipEventDestroy(ctx->ev_join);
    for (auto &ev : ctx->ev_crc)
        if (ev)
            (void)hipEventDestroy(ev);
    if (ctx->owns_stream && ctx->stream)
        (void)hipStreamDestroy(ctx->stream);
    delete ctx;
}

#ifdef SNAPMI_TESTING // (the test build, libsnapmi_test.so: Makefile)
constexpr bool kTestBuild = true;
#else
constexpr bool kTestBuild = false;
#endif
static_assert(kOptWriteScratchMin == (int64_t)(kSlotBytes + kMaxBlock),
              "snapmi_options.hpp and snapmi_kernels.hpp disagree");

// The names, the values each takes in this build and the fields they are
// stored in: snapmi_options.hpp.  Here only what does more than store.
int snapmi_ctx_set_option(snapmi_ctx *ctx, const char *name, int64_t value)
{
    if (!ctx || !name)
        return SNAPMI_E_ARGUMENT;
    if (option_set(*ctx, name, value, false, kTestBuild) !=
        OptionSet::accepted)
        return fail_ctx(ctx, SNAPMI_E_ARGUMENT, "unknown option %s", name);
    if (strcmp(name, "token_pool_pct") == 0)
        ctx->token_pool_now = 0; // (what it had grown to is forgotten)
    else if (strcmp(name, "decode_kernel") == 0 && !ctx->lds_store_order_ok)
        ctx->decode_kernel = 0;
    return SNAPMI_OK;
}

#ifdef SNAPMI_TESTING
// Test option "scratch_fill" 0..255: with every stream of the context idle,
// the whole capacity of every scratch buffer (ScratchDev / ScratchPin of the
// context, of its UpdateScratch and of the host pipe's slots) is set to the
// byte; kept buffers are left alone.  Counters a call left in such a buffer
// for snapmi_ctx_get_info are gone with it: they read as "no call yet".
static int scratch_fill_now(snapmi_ctx *ctx, int byte)
{
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream2));
    if (ctx->pipe) {
        HIP_TRY(ctx, hipStreamSynchronize(ctx->pipe->s_in));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->pipe->s_out));
    }
    std::vector<DevBuf *> dev;
    std::vector<PinBuf *> pin;
    for (DevBuf *b : ctx->dev_bufs)
        dev.push_back(b);
    for (PinBuf *b : ctx->pin_bufs)
        pin.push_back(b);
    if (ctx->pipe)
        for (PipeSlot &sl : ctx->pipe->slot) {
            for (DevBuf *b : {&sl.in, &sl.out, &sl.desc, &sl.home})
                dev.push_back(b);
            for (PinBuf *b : {&sl.hb_in, &sl.hb_home})
                pin.push_back(b);
        }
    ctx->fill_buffers = ctx->fill_bytes = ctx->fill_seen = 0;
    for (DevBuf *b : dev)
        if (!b->kept && b->p)
            HIP_TRY(ctx, hipMemsetAsync(b->p, byte, b->cap, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    for (PinBuf *b : pin)
        if (!b->kept && b->p)
            memset(b->p, byte, b->cap);
    ctx->rg_stats_live = ctx->ib_stats_live = false;
    ctx->wr.stats_live = ctx->ap.stats_live = false;
    ctx->fr_nowait_live = false;
    // what was filled, and what of it reads back as filled: first, middle
    // and last byte of every buffer
    const uint8_t want = (uint8_t)byte;
    for (DevBuf *b : dev) {
        if (b->kept || !b->p)
            continue;
        ctx->fill_buffers++;
        ctx->fill_bytes += b->cap;
        bool ok = true;
        for (size_t off : {(size_t)0, b->cap / 2, b->cap - 1}) {
            uint8_t got = (uint8_t)~want;
            HIP_TRY(ctx, hipMemcpy(&got, (const uint8_t *)b->p + off, 1,
                                   hipMemcpyDeviceToHost));
            ok = ok && got == want;
        }
        ctx->fill_seen += ok;
    }
    for (PinBuf *b : pin) {
        if (b->kept || !b->p)
            continue;
        ctx->fill_buffers++;
        ctx->fill_bytes += b->cap;
        const volatile uint8_t *p = (const volatile uint8_t *)b->p;
        ctx->fill_seen +=
            p[0] == want && p[b->cap / 2] == want && p[b->cap - 1] == want;
    }
    return SNAPMI_OK;
}

// include/snapmi_test.h: knobs of the test suite and the experiment drivers
// (libsnapmi_test.so only: the product library does not export it)
int snapmi_ctx_set_test_option(snapmi_ctx *ctx, const char *name,
                               int64_t value)
{
    if (!ctx || !name)
        return SNAPMI_E_ARGUMENT;
    if (option_set(*ctx, name, value, true, kTestBuild) != OptionSet::accepted)
        return fail_ctx(ctx, SNAPMI_E_ARGUMENT, "unknown test option %s",
                        name);
    if (strcmp(name, "lds_order_ok") == 0)
        ctx->lds_order_ok = ctx->lds_order_hw && value != 0; // can only lower
    else if (strcmp(name, "lane_tables_renew") == 0) {
        // drop the tables so the next launch places new ones
        if (ctx->lane_tables.p) {
            HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
            snapmi::free_lane_tables(ctx);
        }
    } else if (strcmp(name, "scratch_fill") == 0 && value >= 0)
        return scratch_fill_now(ctx, (int)value);
    return SNAPMI_OK;
}
#endif // SNAPMI_TESTING

void *snapmi_host_alloc(size_t bytes)
{
    void *p = nullptr;
    if (hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocDefault) != hipSuccess) {
        (void)hipGetLastError();
        return nullptr;
    }
    return p;
}

void snapmi_host_free(void *p)
{
    if (p)
        (void)hipHostFree(p);
}

const char *snapmi_table_probe_log(const snapmi_ctx *ctx)
{
    return ctx ? ctx->probe_log.c_str() : "";
}

size_t snapmi_error_string(const snapmi_error *e, char *buf, size_t cap)
{
    // reference src/error.rs:249-335, variant by variant
    char tmp[256];
    const unsigned long long a = e ? e->a : 0, b = e ? e->b : 0,
                             c = e ? e->c : 0;
    int n = 0;
    switch (e ? e->kind : -1) {
    case SNAPMI_TOO_BIG:
        n = snprintf(tmp, sizeof tmp,
                     "snappy: input buffer (size = %llu) is larger than "
                     "allowed (size = %llu)", a, b);
        break;
    case SNAPMI_BUFFER_TOO_SMALL:
        n = snprintf(tmp, sizeof tmp,
                     "snappy: output buffer (size = %llu) is smaller than "
                     "required (size = %llu)", a, b);
        break;
    case SNAPMI_EMPTY:
        n = snprintf(tmp, sizeof tmp, "snappy: corrupt input (empty)");
        break;
    case SNAPMI_HEADER:
        n = snprintf(tmp, sizeof tmp,
                     "snappy: corrupt input (invalid header)");
        break;
    case SNAPMI_HEADER_MISMATCH:
        n = snprintf(tmp, sizeof tmp,
                     "snappy: corrupt input (header mismatch; expected %llu "
                     "decompressed bytes but got %llu)", a, b);
        break;
    case SNAPMI_LITERAL:
        n = snprintf(tmp, sizeof tmp,
                     "snappy: corrupt input (expected literal read of length "
                     "%llu; remaining src: %llu; remaining dst: %llu)", a, b,
                     c);
        break;
    case SNAPMI_COPY_READ:
        n = snprintf(tmp, sizeof tmp,
                     "snappy: corrupt input (expected copy read of length "
                     "%llu; remaining src: %llu)", a, b);
        break;
    case SNAPMI_COPY_WRITE:
        n = snprintf(tmp, sizeof tmp,
                     "snappy: corrupt input (expected copy write of length "
                     "%llu; remaining dst: %llu)", a, b);
        break;
    case SNAPMI_OFFSET:
        n = snprintf(tmp, sizeof tmp,
                     "snappy: corrupt input (expected valid offset but got "
                     "offset %llu; dst position: %llu)", a, b);
        break;
    case SNAPMI_STREAM_HEADER:
        n = snprintf(tmp, sizeof tmp,
                     "snappy: corrupt input (expected stream header but got "
                     "unexpected chunk type byte %llu)", a);
        break;
    case SNAPMI_STREAM_HEADER_MISMATCH: {
        // (six bytes, little-endian in `a`; std::ascii::escape_default)
        char esc[6 * 4 + 1];
        int k = 0;
        for (int i = 0; i < 6; i++) {
            const unsigned ch = (unsigned)(a >> (8 * i)) & 0xFF;
            if (ch == 9 || ch == 10 || ch == 13) {
                esc[k++] = '\\';
                esc[k++] = ch == 9 ? 't' : (ch == 10 ? 'n' : 'r');
            } else if (ch == 39 || ch == 34 || ch == 92) {
                esc[k++] = '\\';
                esc[k++] = (char)ch;
            } else if (ch >= 0x20 && ch <= 0x7E) {
                esc[k++] = (char)ch;
            } else {
                k += snprintf(esc + k, 5, "\\x%02x", ch);
            }
        }
        esc[k] = 0;
        n = snprintf(tmp, sizeof tmp,
                     "snappy: corrupt input (expected sNaPpY stream header "
                     "but got %s)", esc);
        break;
    }
    case SNAPMI_UNSUPPORTED_CHUNK_TYPE:
        n = snprintf(tmp, sizeof tmp,
                     "snappy: corrupt input (unsupported chunk type: %llu)",
                     a);
        break;
    case SNAPMI_UNSUPPORTED_CHUNK_LENGTH:
        n = snprintf(tmp, sizeof tmp,
                     b ? "snappy: corrupt input (invalid stream header "
                         "length: %llu)"
                       : "snappy: corrupt input (unsupported chunk length: "
                         "%llu)", a);
        break;
    case SNAPMI_CHECKSUM:
        n = snprintf(tmp, sizeof tmp,
                     "snappy: corrupt input (bad checksum; expected: %llu, "
                     "got: %llu)", a, b);
        break;
    case SNAPMI_E_UNEXPECTED_EOF:
        // (not a snap::Error: the io::Error of read_exact that the
        // reference's reader passes on, src/read.rs:105-172 - std's text)
        n = snprintf(tmp, sizeof tmp, "failed to fill whole buffer");
        break;
    case SNAPMI_OK:
        n = snprintf(tmp, sizeof tmp, "ok");
        break;
    default:
        n = snprintf(tmp, sizeof tmp, "snapmi: device or argument error %d",
                     e ? e->kind : -1);
    }
    if (buf && cap) {
        const size_t m = (size_t)n < cap - 1 ? (size_t)n : cap - 1;
        memcpy(buf, tmp, m);
        buf[m] = 0;
    }
    return (size_t)n;
}

const char *snapmi_last_kernel(const snapmi_ctx *ctx)
{
    return ctx ? ctx->last_kernel : "";
}

const char *snapmi_last_error(const snapmi_ctx *ctx)
{
    return ctx ? ctx->last_error.c_str() : "null context";
}

void *snapmi_ctx_stream(const snapmi_ctx *ctx)
{
    return ctx ? (void *)ctx->stream : nullptr;
}

int snapmi_ctx_synchronize(snapmi_ctx *ctx)
{
    if (!ctx)
        return SNAPMI_E_ARGUMENT;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return snapmi::release_batch_scratch(ctx);
}

size_t snapmi_max_compress_len(size_t input_len)
{
    return (size_t)max_compress_len_u64(input_len);
}

int snapmi_decompress_len(const uint8_t *input, size_t input_len,
                          size_t *result, snapmi_error *err)
{
    if (!result || (!input && input_len))
        return SNAPMI_E_ARGUMENT;
    *result = 0;
    set_err(err, SNAPMI_OK);
    if (input_len == 0)
        return SNAPMI_OK;
    uint64_t v = 0;
    if (host_varint(input, input_len, &v) == 0) {
        set_err(err, SNAPMI_HEADER);
        return SNAPMI_HEADER;
    }
    if (v > kMaxInput) {
        set_err(err, SNAPMI_TOO_BIG, v, kMaxInput);
        return SNAPMI_TOO_BIG;
    }
    *result = (size_t)v;
    return SNAPMI_OK;
}

// The k counters the kernels of a call keep in `stat`: waits for the call and
// fetches them; all 0 when the last call ran none of its kernels.
static int fetch_counters(snapmi_ctx *ctx, bool live, const DevBuf &stat,
                          unsigned long long *w, size_t k)
{
    memset(w, 0, k * sizeof *w);
    if (live && stat.p) {
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        HIP_TRY(ctx, hipMemcpy(w, stat.p, k * sizeof *w,
                               hipMemcpyDeviceToHost));
    }
    return SNAPMI_OK;
}

// What snapmi_ctx_get_info answers: a name reads a field of the context, or
// word `word` of the counters the kernels of a call keep on the device
// (fetch_counters: waits for the call), or is written out below.  The names,
// and which of them only the test build answers: snapmi_options.hpp.
namespace {

struct InfoDesc {
    const char *name;
    int64_t (*field)(const snapmi_ctx *);
    int (*counters)(snapmi_ctx *, unsigned long long *w);
    size_t word; // (neither: written out in snapmi_ctx_get_info)
};

#define FIELD(name, expr)                                                     \
    {name, [](const snapmi_ctx *c) { return (int64_t)(c->expr); }, nullptr, 0}
#define COUNTER(name, live, stat, k, word)                                    \
    {name, nullptr, [](snapmi_ctx *c, unsigned long long *w) {                \
         return fetch_counters(c, c->live, c->stat, w, k);                    \
     }, word}
constexpr InfoDesc kInfo[] = {
    {"scratch_bytes"},
    {"token_scratch_bytes"},
    FIELD("token_pool_pages", tok_pool_pages_last),
    FIELD("token_pool_pct_now", token_pool_now),
    {"token_pages_asked"},
    {"token_blocks_spilled"},
    FIELD("host_batch_slices", hb_slices),
    FIELD("host_batch_h2d_bytes", hb_h2d_bytes),
    FIELD("host_batch_d2h_bytes", hb_d2h_bytes),
    FIELD("host_batch_listed_slices", hb_listed_slices),
    // (snapmi_decompress_batch_indexed: words 1 and 2 of its gate)
    COUNTER("index_streams_pieced", ix_stats_live, ix_gate, 3, 1),
    COUNTER("index_streams_fallback", ix_stats_live, ix_gate, 3, 2),
    FIELD("range_pieces", rg_pieces),
    COUNTER("range_ranges_ok", rg_stats_live, rg_stat, 2, 0),
    COUNTER("range_ranges_failed", rg_stats_live, rg_stat, 2, 1),
    FIELD("write_blocks", wr.blocks),
    FIELD("write_blocks_decoded", wr.decoded),
    COUNTER("write_streams_ok", wr.stats_live, wr.stat, 2, 0),
    COUNTER("write_streams_failed", wr.stats_live, wr.stat, 2, 1),
    FIELD("append_blocks", ap.blocks),
    FIELD("append_blocks_decoded", ap.decoded),
    COUNTER("append_streams_ok", ap.stats_live, ap.stat, 2, 0),
    COUNTER("append_streams_failed", ap.stats_live, ap.stat, 2, 1),
    COUNTER("index_build_built", ib_stats_live, ib_stat, 5, 0),
    COUNTER("index_build_unaligned", ib_stats_live, ib_stat, 5, 1),
    COUNTER("index_build_corrupt", ib_stats_live, ib_stat, 5, 2),
    COUNTER("index_build_missized", ib_stats_live, ib_stat, 5, 3),
    COUNTER("index_build_walked", ib_stats_live, ib_stat, 5, 4),
    {"frame_nowait_front"},
    {"lane_multi_rounds"},
    FIELD("scratch_fill_buffers", fill_buffers),
    FIELD("scratch_fill_bytes", fill_bytes),
    FIELD("scratch_fill_seen", fill_seen),
};
#undef FIELD
#undef COUNTER
constexpr bool info_names_agree() // kInfo has kInfoNames' names, in order
{
    for (size_t i = 0; i < std::size(kInfo); i++)
        if (std::string_view(kInfoNames[i].name) != kInfo[i].name)
            return false;
    return true;
}
static_assert(std::size(kInfo) == std::size(kInfoNames) && info_names_agree(),
              "kInfo and snapmi_options.hpp's kInfoNames disagree");

} // namespace

int snapmi_ctx_get_info(snapmi_ctx *ctx, const char *name, int64_t *value)
{
    if (!ctx || !name || !value)
        return SNAPMI_E_ARGUMENT;
    const InfoDesc *d = find_named(kInfo, name);
    if (!d || (kInfoNames[d - kInfo].test_only && !kTestBuild)) {
        ctx->last_error = std::string("unknown info: ") + name;
        return SNAPMI_E_ARGUMENT;
    }
    if (d->field) {
        *value = d->field(ctx);
    } else if (d->counters) {
        unsigned long long w[5];
        if (int rc = d->counters(ctx, w))
            return rc;
        *value = (int64_t)w[d->word];
    } else if (strcmp(name, "scratch_bytes") == 0) {
        uint64_t sum = ctx->lane_tables.cap;
        for (const DevBuf *b : ctx->dev_bufs)
            sum += b->cap;
        *value = (int64_t)sum;
    } else if (strcmp(name, "token_scratch_bytes") == 0) {
        *value = (int64_t)(ctx->tokens.cap + ctx->tok_pages.cap +
                           ctx->tok_stage.cap + ctx->ntok.cap);
    } else if (strcmp(name, "token_pages_asked") == 0 ||
               strcmp(name, "token_blocks_spilled") == 0) {
        // of the last token-path launch: wait for it
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        const volatile uint32_t *t = ctx->h_tokstat;
        const bool asked = strcmp(name, "token_pages_asked") == 0;
        *value = !t ? 0 : asked ? t[0] : t[1];
    } else if (strcmp(name, "frame_nowait_front") == 0) {
        // of the last SNAPMI_FRAME_NO_WAIT decode: wait for it
        uint32_t w = 0;
        if (ctx->fr_nowait_live) {
            HIP_TRY(ctx, hipSetDevice(ctx->device));
            HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
            HIP_TRY(ctx, hipMemcpy(&w, ctx->fr_nowait.p, sizeof w,
                                   hipMemcpyDeviceToHost));
        }
        *value = ctx->fr_nowait_live ? (int64_t)w : -1;
#ifdef SNAPMI_TESTING
    } else if (strcmp(name, "lane_multi_rounds") == 0) {
        // of the last token-path segment's lane wavefronts (test build: the
        // kernel counts them): rounds above the launch's own depth; wait
        uint32_t w = 0;
        if (ctx->tok_pages.p) {
            HIP_TRY(ctx, hipSetDevice(ctx->device));
            HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
            HIP_TRY(ctx, hipMemcpy(&w,
                                   (const uint32_t *)ctx->tok_pages.p +
                                       snapmi::kTokCtlMultiRounds,
                                   sizeof w, hipMemcpyDeviceToHost));
        }
        *value = w;
#endif
    }
    return SNAPMI_OK;
}

int snapmi_decompress_len_batch(snapmi_ctx *ctx,
                                const void *const *d_in_ptrs,
                                const uint64_t *d_in_lens,
                                uint64_t *d_out_lens, snapmi_error *d_errs,
                                size_t n)
{
    if (!ctx)
        return SNAPMI_E_ARGUMENT;
    if (n == 0)
        return SNAPMI_OK;
    if (!d_in_ptrs || !d_in_lens || !d_out_lens || n > 0x7FFFFFFFu)
        return fail_ctx(ctx, SNAPMI_E_ARGUMENT,
                        "decompress_len_batch: bad args");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    DecompressArgs a;
    a.in_ptrs = d_in_ptrs;
    a.in_lens = d_in_lens;
    a.out_ptrs = nullptr;
    a.out_caps = nullptr;
    a.out_lens = d_out_lens;
    a.errs = d_errs;
    a.modes = nullptr;
    a.n_streams = (uint32_t)n;
    a.order = nullptr;
    a.bucket_pos = nullptr;
    a.prof = nullptr;
    a.gate = nullptr;
    a.gate_value = 0;
    hipLaunchKernelGGL(k_decompress_len, dim3((uint32_t)((n + 255) / 256)),
                       dim3(256), 0, ctx->stream, a);
    HIP_TRY(ctx, hipGetLastError());
    return SNAPMI_OK;
}

PROF(
// experiment builds only: copy out the 16 cycle counters of the last
// compress batch (not part of include/snapmi.h)
SNAPMI_API int snapmi_debug_profile(snapmi_ctx *ctx, uint64_t *out16)
{
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    HIP_TRY(ctx, hipMemcpy(out16, ctx->st_prof.p, 16 * sizeof(uint64_t),
                           hipMemcpyDeviceToHost));
    return SNAPMI_OK;
}
)
PROF_TAIL(
// experiment build SNAPMI_PROFILE=3: the tail records of the last compress
// call's lane launch (CompressArgs::prof): out[0..2] = start, end and "the
// ticket was first found empty", out[3 + g] = when lane g went out of work,
// all on the device's 100 MHz clock; returns the number of lanes, or < 0
SNAPMI_API int64_t snapmi_debug_lane_tail(snapmi_ctx *ctx, uint64_t *out,
                                          uint64_t cap)
{
    const uint64_t lanes = ctx->prof_tail_lanes;
    if (!ctx->st_prof.p || cap < 3 + lanes)
        return -1;
    if (hipStreamSynchronize(ctx->stream) != hipSuccess)
        return -1;
    uint64_t head[3];
    if (hipMemcpy(head, (const uint64_t *)ctx->st_prof.p + snapmi::kProfTail,
                  sizeof head, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(out + 3,
                  (const uint64_t *)ctx->st_prof.p + snapmi::kProfTailLanes,
                  lanes * sizeof(uint64_t), hipMemcpyDeviceToHost) != hipSuccess)
        return -1;
    out[0] = ~head[0];
    out[1] = head[1];
    out[2] = ~head[2];
    return (int64_t)lanes;
}
)

int snapmi_last_timing(snapmi_ctx *ctx, snapmi_timing *out)
{
    if (!ctx || !out)
        return SNAPMI_E_ARGUMENT;
    memset(out, 0, sizeof *out);
    if (!ctx->timing_valid)
        return fail_ctx(ctx, SNAPMI_E_ARGUMENT, "no batch has been timed");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipEventSynchronize(ctx->ev[3]));
    HIP_TRY(ctx, hipEventElapsedTime(&out->plan_ms, ctx->ev[0], ctx->ev[1]));
    HIP_TRY(ctx, hipEventElapsedTime(&out->codec_ms, ctx->ev[1], ctx->ev[2]));
    HIP_TRY(ctx,
            hipEventElapsedTime(&out->compact_ms, ctx->ev[2], ctx->ev[3]));
    HIP_TRY(ctx, hipEventElapsedTime(&out->total_ms, ctx->ev[0], ctx->ev[3]));
    out->codec_launches = ctx->codec_launches;
    out->dominant_ms = out->codec_ms;
    if (ctx->dominant_split)
        HIP_TRY(ctx, hipEventElapsedTime(&out->dominant_ms, ctx->ev[4],
                                         ctx->ev[5]));
    return SNAPMI_OK;
}

// ----------------------------------------------------------------------
// scalar mirrors (host buffers): stage through device memory, batch of 1
// ----------------------------------------------------------------------
namespace {

struct OneDesc {
    const void *in_ptr;
    uint64_t in_len;
    void *out_ptr;
    uint64_t out_cap;
    uint64_t out_len;
    uint64_t pad;
    snapmi_error err;
};

} // namespace

} // extern "C"

int snapmi::run_one(snapmi_ctx *ctx, bool compress, const uint8_t *input,
            size_t input_len, uint8_t *output, size_t output_cap,
            size_t *written, snapmi_error *err)
{
    if (!ctx || !written || (!input && input_len) || (!output && output_cap))
        return SNAPMI_E_ARGUMENT;
    *written = 0;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    int rc;
    // Device output buffer: what the kernels may write.  For compression the
    // reference demands max_compress_len (checked on the device as well).
    size_t dev_out = output_cap;
    size_t dl = 0; // decompress: the length the header announces
    if (!compress) {
        snapmi_error he;
        if (input_len && snapmi_decompress_len(input, input_len, &dl, &he) ==
                             SNAPMI_OK &&
            dl < dev_out)
            dev_out = dl;
    } else {
        size_t need = snapmi_max_compress_len(input_len);
        if (need && need < dev_out)
            dev_out = need;
    }
    // (inputs up to a few MiB are staged through pinned memory of the
    // context; larger ones are copied from where they lie)
    const bool staged = input_len <= kPinStage && dev_out <= kPinStage;
    if ((rc = reserve(ctx, ctx->st_in, input_len + 16)) ||
        (rc = reserve(ctx, ctx->st_out, dev_out + 64)) ||
        (rc = reserve(ctx, ctx->st_desc, sizeof(OneDesc))) ||
        (rc = pin_reserve(ctx, ctx->pin_desc, 2 * sizeof(OneDesc))) ||
        (staged && ((rc = pin_reserve(ctx, ctx->pin_in, input_len + 16)) ||
                    (rc = pin_reserve(ctx, ctx->pin_out, dev_out + 64)))))
        return rc;
    OneDesc *hd = (OneDesc *)ctx->pin_desc.p; // [0] in, [1] back
    memset(&hd[0], 0, sizeof hd[0]);
    hd[0].in_ptr = ctx->st_in.p;
    hd[0].in_len = input_len;
    hd[0].out_ptr = ctx->st_out.p;
    hd[0].out_cap = output_cap; // the caller's capacity is what is validated
    hipStream_t s = ctx->stream;
    if (input_len) {
        const void *from = input;
        if (staged) {
            memcpy(ctx->pin_in.p, input, input_len);
            from = ctx->pin_in.p;
        }
        HIP_TRY(ctx, hipMemcpyAsync(ctx->st_in.p, from, input_len,
                                    hipMemcpyHostToDevice, s));
    }
    HIP_TRY(ctx, hipMemcpyAsync(ctx->st_desc.p, &hd[0], sizeof hd[0],
                                hipMemcpyHostToDevice, s));
    OneDesc *d = (OneDesc *)ctx->st_desc.p;
    if (compress) {
        uint64_t hl = input_len;
        rc = snapmi_compress_batch(ctx, &d->in_ptr, &d->in_len, &hl,
                                   &d->out_ptr, &d->out_cap, &d->out_len,
                                   &d->err, 1);
    } else if (long_stream_rule(input_len, dl, long_stream_min())) {
        // one wavefront decodes ~140 MB/s: long streams go through the
        // parallel single-stream path
        rc = snapmi_decompress_stream(ctx, ctx->st_in.p, input_len,
                                      ctx->st_out.p, output_cap, &d->out_len,
                                      &d->err);
    } else {
        // (straight to the wavefront decoder: the host has just made the
        // decision snapmi_decompress_batch would wait for the device to make)
        rc = launch_decompress(ctx, &d->in_ptr, &d->in_len, &d->out_ptr,
                               &d->out_cap, &d->out_len, &d->err, nullptr, 1);
    }
    if (rc)
        return rc;
    HIP_TRY(ctx, hipMemcpyAsync(&hd[1], ctx->st_desc.p, sizeof hd[1],
                                hipMemcpyDeviceToHost, s));
    if (staged) {
        // the result comes along in the same round trip: as much as the
        // kernels can have written (the length is not known to the host yet)
        HIP_TRY(ctx, hipMemcpyAsync(ctx->pin_out.p, ctx->st_out.p,
                                    dev_out, hipMemcpyDeviceToHost, s));
    }
    HIP_TRY(ctx, hipStreamSynchronize(s));
    if (compress && (rc = release_batch_scratch(ctx)))
        return rc;
    const OneDesc &h = hd[1];
    if (err)
        *err = h.err;
    if (h.err.kind != SNAPMI_OK)
        return h.err.kind;
    if (h.out_len > output_cap)
        return fail_ctx(ctx, SNAPMI_E_DEVICE, "device wrote %llu > cap %zu",
                        (unsigned long long)h.out_len, output_cap);
    if (h.out_len) {
        if (staged)
            memcpy(output, ctx->pin_out.p, h.out_len);
        else
            HIP_TRY(ctx, hipMemcpy(output, ctx->st_out.p, h.out_len,
                                   hipMemcpyDeviceToHost));
    }
    *written = (size_t)h.out_len;
    return SNAPMI_OK;
}

extern "C" {

int snapmi_raw_compress(snapmi_ctx *ctx, const uint8_t *input,
                        size_t input_len, uint8_t *output, size_t output_cap,
                        size_t *written, snapmi_error *err)
{
    return run_one(ctx, true, input, input_len, output, output_cap, written,
                   err);
}

int snapmi_raw_decompress(snapmi_ctx *ctx, const uint8_t *input,
                          size_t input_len, uint8_t *output,
                          size_t output_cap, size_t *written,
                          snapmi_error *err)
{
    return run_one(ctx, false, input, input_len, output, output_cap, written,
                   err);
}

} // extern "C"
