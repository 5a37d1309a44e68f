// snapmi_hostbatch.hip -- many independent streams in HOST memory per call,
// raw (snapmi_compress_batch_host / snapmi_decompress_batch_host) or framed
// (snapmi_frame_compress_batch_host / snapmi_frame_decompress_batch_host): one
// pipeline, the codec is a parameter.
//
// The batch is cut into slices of whole streams (snapmi_hostbatch.hpp) and
// the slices go through the three slots of the host pipe
// (snapmi_hostpipe.hpp): while the calling thread packs slice t into pinned
// staging and sends it off, the codec runs on slice t-1 and slice t-2 comes
// home and is handed out.  Per slice:
//
//   in    the four descriptor arrays and the inputs - every stream on a
//         16-byte boundary, 16 bytes of slack behind it - are packed into
//         the slot's pinned staging and go to the device as ONE copy; a
//         stream of host_batch_direct_min bytes or more is copied from where
//         it lies instead (the staging copy would cost what the H2D costs)
//   codec snapmi_compress_batch / snapmi_decompress_batch or their frame_
//         forms, unchanged, on the context's stream; lengths and errors land
//         in the head of the slice's "home image".  Framed decode: the host
//         has walked every stream's chunk headers (snapmi_framewalk.hpp) for
//         the rooms below, so a slice whose streams are all well-formed sends
//         its chunk list behind the inputs, in the same copy, and the device
//         neither walks nor makes the host wait for a chunk count
//         (frame_decompress_batch_listed)
//   out   compress: the kernels leave every stream in a slot of
//         max_compress_len bytes and only the device knows what was written:
//         k_hb_sizes + k_scan_u64 give packed offsets and k_hb_pack gathers
//         the streams that succeeded behind the image's head - straight into
//         pinned host memory (16-byte stores over the link), or into device
//         memory followed by one D2H of exactly head + packed total.
//         decompress: the host has read every header, the output slab is
//         tight already: one D2H of head + slab.
//   home  the host hands every successful stream from staging to its
//         caller's buffer; a failed stream's buffer is not touched - except
//         that a framed stream that fails to decode delivers the chunks in
//         front of the failure, as the reader it mirrors has by then.
//
// Verdicts, lengths and error fields always come from the device.
#include <hip/hip_runtime.h>

#include <string.h>
#include <vector>

#include "snapmi.h"
#include "snapmi_ctx.hpp"
#include "snapmi_hostpipe.hpp"
#include "snapmi_frame.hpp"
#include "snapmi_hostbatch.hpp"
#include "snapmi_framewalk.hpp"
#include "snapmi_device.hpp"

using namespace snapmi;

namespace snapmi {
int release_batch_scratch(snapmi_ctx *ctx); // snapmi_api.hip

// packed size of every stream of a compress slice: what it wrote, rounded
// to 16, or nothing if it failed
__global__ __launch_bounds__(256) void k_hb_sizes(const uint64_t *out_lens,
                                                  const snapmi_error *errs,
                                                  uint64_t *sizes, uint32_t n)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n)
        sizes[i] = errs[i].kind == SNAPMI_OK ? hb_align(out_lens[i]) : 0;
}

// Gathers the streams of a compress slice from their slots to their packed
// offsets (offs: exclusive scan of k_hb_sizes, offs[n] = total).  A workgroup
// takes tiles of kHbTile packed bytes, a thread one 16-byte unit of the tile:
// the tile's first and last stream by binary search (wave-uniform), the
// unit's own stream by a search between the two - so five million streams of
// 200 bytes and one stream of 4 GiB are both 4 KiB of copying per workgroup
// and trip.  Sources (slots) and destinations are 16-byte aligned by
// construction; the last unit of a stream is copied bytewise.  dst may be
// pinned host memory.  *total_out (pinned) gets the packed total.
__global__ __launch_bounds__(256) void k_hb_pack(const void *const *src_ptrs,
                                                 const uint64_t *lens,
                                                 const uint64_t *offs,
                                                 uint32_t n, uint8_t *dst,
                                                 uint64_t *total_out)
{
    const uint64_t total = offs[n];
    if (blockIdx.x == 0 && threadIdx.x == 0)
        *total_out = total;
    const uint64_t tiles = (total + kHbTile - 1) / kHbTile;
    typedef __attribute__((address_space(1))) u32x4 g_u32x4;
    for (uint64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const HbTile x = hb_tile(offs, n, total, t);
        const uint64_t p = x.start + (uint64_t)kHbUnit * threadIdx.x;
        if (p > x.last)
            continue;
        const HbUnit u = hb_unit(offs, lens, x.s_lo, x.s_hi, p);
        gcptr from = (gcptr)src_ptrs[u.stream] + u.src_off;
        gptr to = (gptr)dst + p;
        if (u.bytes == kHbUnit) {
            *(g_u32x4 *)to = ld128g(from);
        } else {
            for (uint32_t b = 0; b < u.bytes; b++)
                to[b] = from[b];
        }
    }
}

} // namespace snapmi

namespace {

int pin_buf(snapmi_ctx *ctx, PinBuf &b, size_t bytes)
{
    if (bytes <= b.cap)
        return SNAPMI_OK;
    if (b.p) {
        HIP_TRY(ctx, hipHostFree(b.p));
        b.p = nullptr;
        b.cap = 0;
    }
    const size_t want = bytes + bytes / 8 + 4096;
    HIP_TRY(ctx, hipHostMalloc(&b.p, want, hipHostMallocDefault));
    b.cap = want;
#ifdef SNAPMI_TESTING
    fill_new_pin(ctx, b);
#endif
    return SNAPMI_OK;
}

// what the host keeps of a slice while it is in a slot
struct SliceState {
    HbSlice x{};
    std::vector<uint64_t> in_offs, out_offs;
    size_t m = 0;       // streams
    uint64_t desc = 0;  // bytes of the four descriptor arrays, aligned
    uint64_t head = 0;  // bytes of out_lens + errs in the home image, aligned
    // framed decode from the host's chunk list: its data chunks, and the
    // bytes of first[m + 1] + list[chunks] behind the slice's inputs
    bool listed = false;
    uint64_t chunks = 0, extra = 0;
};

enum Codec { kRaw, kFrame };

int host_batch(snapmi_ctx *ctx, Codec codec, bool compress,
               const void *const *h_in_ptrs, const size_t *h_in_lens,
               void *const *h_out_ptrs, const size_t *h_out_caps,
               size_t *h_out_lens, snapmi_error *h_errs, size_t n)
{
    const bool frame = codec == kFrame;
    const char *what =
        frame ? (compress ? "frame_compress_batch_host"
                          : "frame_decompress_batch_host")
              : (compress ? "compress_batch_host" : "decompress_batch_host");
    // framed decode: a failing stream delivers the chunks in front of the
    // failure; without output buffers it reports lengths only
    const bool prefix = frame && !compress;
    const bool lens_only = prefix && !h_out_ptrs;
    if (!ctx) {
        // (no context can be made without a device: say so)
        int count = 0;
        if (hipGetDeviceCount(&count) != hipSuccess || count == 0) {
            (void)hipGetLastError();
            return SNAPMI_E_DEVICE;
        }
        return SNAPMI_E_ARGUMENT;
    }
    if (n == 0)
        return SNAPMI_OK;
    if (!h_in_ptrs || !h_in_lens || !h_out_lens ||
        (!lens_only && (!h_out_ptrs || !h_out_caps)) || n > 0x7FFFFFFFu)
        return fail_ctx(ctx, SNAPMI_E_ARGUMENT, "%s: bad args", what);
    for (size_t i = 0; i < n; i++)
        if ((h_in_lens[i] && !h_in_ptrs[i]) ||
            (!lens_only && h_out_caps[i] && !h_out_ptrs[i]))
            return fail_ctx(ctx, SNAPMI_E_ARGUMENT,
                            "%s: stream %zu: NULL buffer", what, i);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    ctx->hb_slices = ctx->hb_h2d_bytes = ctx->hb_d2h_bytes = 0;
    ctx->hb_listed_slices = 0;
    // what the codec may write for every stream: the slot the reference
    // demands (src/compress.rs:111-116, src/frame.rs:12) / the length the
    // header announces / the lengths the chunk headers announce, and nothing
    // for a stream the device is going to refuse
    std::vector<uint64_t> rooms(n);
    // framed decode: the data chunks of every stream (stream i owns
    // list[first[i], first[i + 1])) and whether the walk accepted all of it
    const bool want_list = prefix && ctx->host_batch_listed;
    std::vector<FwEntry> list;
    std::vector<uint64_t> first(want_list ? n + 1 : 0);
    std::vector<uint8_t> regular(want_list ? n : 0);
    for (size_t i = 0; i < n; i++) {
        h_out_lens[i] = 0;
        uint64_t room = 0;
        if (frame && compress) {
            const size_t need = snapmi_frame_max_len(h_in_lens[i]);
            if (h_in_lens[i] && need <= h_out_caps[i])
                room = need;
        } else if (frame) {
            if (want_list)
                first[i] = list.size();
            const FwStream w = frame_walk_host(
                (const uint8_t *)h_in_ptrs[i], h_in_lens[i],
                [&](uint64_t off, uint32_t hd) {
                    if (want_list)
                        list.push_back(FwEntry{off, (uint32_t)i, hd});
                });
            if (want_list)
                regular[i] = w.e.kind == SNAPMI_OK;
            if (!lens_only && w.room <= h_out_caps[i])
                room = w.room;
        } else if (compress) {
            const size_t need = snapmi_max_compress_len(h_in_lens[i]);
            if (need && need <= h_out_caps[i])
                room = need;
        } else {
            size_t dl = 0;
            snapmi_error he;
            if (h_in_lens[i] &&
                snapmi_decompress_len((const uint8_t *)h_in_ptrs[i],
                                      h_in_lens[i], &dl, &he) == SNAPMI_OK &&
                dl <= h_out_caps[i])
                room = dl;
        }
        rooms[i] = room;
    }
    if (want_list)
        first[n] = list.size();
    snapmi_host_pipe *P;
    int rc = host_pipe(ctx, &P);
    if (rc)
        return rc;
    hipStream_t sK = ctx->stream;
    PipeDrain drain{ctx, P};
    const uint64_t in_limit = ctx->host_batch_slice;
    // (a decoded slice is bounded too: text expands 2x, zeros 20x)
    const uint64_t out_limit = compress ? ~0ull : 4 * in_limit;
    const uint64_t direct_min = ctx->host_batch_direct_min;
    const bool to_host = compress && ctx->host_batch_pack_to_host;
    const uint32_t cus = ctx->num_cus > 0 ? (uint32_t)ctx->num_cus : 256;
    SliceState state[kSlots];
    size_t cursor = 0, planned = 0;
    for (size_t t = 0;; t++) {
        // ---- slice t: plan, pack, send ----
        if (cursor < n) {
            PipeSlot &s = P->slot[t % kSlots];
            SliceState &st = state[t % kSlots];
            st.x = hb_plan_slice(h_in_lens, rooms.data(), n, cursor, in_limit,
                                 out_limit, nullptr, nullptr);
            st.m = st.x.s1 - st.x.s0;
            if (st.in_offs.size() < st.m) {
                st.in_offs.resize(st.m);
                st.out_offs.resize(st.m);
            }
            st.x = hb_plan_slice(h_in_lens, rooms.data(), n, cursor, in_limit,
                                 out_limit, st.in_offs.data(),
                                 st.out_offs.data());
            const size_t m = st.m;
            st.desc = hb_align(32 * (uint64_t)m);
            // (framed decode: 16 bytes more, the word k_fbd_from_list raises)
            st.head = hb_align((8 + sizeof(snapmi_error)) * (uint64_t)m) +
                      (prefix ? 16 : 0);
            st.listed = want_list;
            for (size_t i = 0; st.listed && i < m; i++)
                st.listed = regular[cursor + i];
            st.chunks = st.listed ? first[st.x.s1] - first[cursor] : 0;
            if (st.chunks > 0x7FFFFFFFu)
                st.listed = false; // (the device call reports it)
            st.extra = st.listed ? hb_align(8 * (uint64_t)(m + 1)) +
                                       sizeof(FwEntry) * st.chunks
                                 : 0;
            uint64_t staged = st.desc;
            for (size_t i = 0; i < m; i++) {
                const uint64_t len = h_in_lens[cursor + i];
                if (len < direct_min)
                    staged += hb_align(len + kHbInSlack);
            }
            if ((rc = slot_reserve(ctx, s.in, st.desc + st.x.in_bytes +
                                                  st.extra + 16)) ||
                (rc = slot_reserve(ctx, s.home,
                                   st.head + (to_host ? 0 : st.x.out_bytes) +
                                       64)) ||
                (compress &&
                 ((rc = slot_reserve(ctx, s.out, st.x.out_bytes + 64)) ||
                  (rc = slot_reserve(ctx, s.desc, (2 * m + 1) * 8 + 64)))) ||
                (rc = pin_buf(ctx, s.hb_in, staged + st.extra + 16)) ||
                (rc = pin_buf(ctx, s.hb_home, st.head + st.x.out_bytes + 64)))
                return rc;
            uint8_t *hs = (uint8_t *)s.hb_in.p;
            uint8_t *d_in = (uint8_t *)s.in.p;
            uint8_t *d_out = compress ? (uint8_t *)s.out.p
                                      : (uint8_t *)s.home.p + st.head;
            uint64_t *a_in_ptrs = (uint64_t *)hs, *a_in_lens = a_in_ptrs + m,
                     *a_out_ptrs = a_in_lens + m, *a_out_caps = a_out_ptrs + m;
            // runs of staging that are contiguous on the device as well: one
            // copy each.  The descriptors are complete only behind the loop:
            // they go last, with the run behind them - the whole slice in one
            // copy unless a stream went from where it lies
            uint64_t run_dev = st.desc, run_stage = st.desc, stage = st.desc;
            bool split = false;
            for (size_t i = 0; i < m; i++) {
                const size_t g = cursor + i;
                const uint64_t len = h_in_lens[g];
                const uint64_t dev_off = st.desc + st.in_offs[i];
                a_in_ptrs[i] = (uint64_t)(uintptr_t)(d_in + dev_off);
                a_in_lens[i] = len;
                a_out_ptrs[i] = (uint64_t)(uintptr_t)(d_out + st.out_offs[i]);
                // (the caller's capacity is what the device validates and
                // reports; it writes no more than the room worked out above)
                a_out_caps[i] = lens_only ? 0 : h_out_caps[g];
                if (len < direct_min) {
                    if (len)
                        memcpy(hs + stage, h_in_ptrs[g], len);
                    stage += hb_align(len + kHbInSlack);
                    continue;
                }
                if (stage > run_stage) {
                    HIP_TRY(ctx, hipMemcpyAsync(d_in + run_dev, hs + run_stage,
                                                stage - run_stage,
                                                hipMemcpyHostToDevice,
                                                P->s_in));
                    ctx->hb_h2d_bytes += stage - run_stage;
                }
                HIP_TRY(ctx, hipMemcpyAsync(d_in + dev_off, h_in_ptrs[g], len,
                                            hipMemcpyHostToDevice, P->s_in));
                ctx->hb_h2d_bytes += len;
                run_stage = stage;
                run_dev = dev_off + hb_align(len + kHbInSlack);
                split = true;
            }
            if (st.listed) {
                // behind the last input, on the device as in staging: part
                // of the slice's last (or only) copy
                uint64_t *l_first = (uint64_t *)(hs + stage);
                FwEntry *l = (FwEntry *)(hs + stage + hb_align(8 * (m + 1)));
                const uint64_t base = first[cursor];
                for (size_t i = 0; i <= m; i++)
                    l_first[i] = first[cursor + i] - base;
                for (uint64_t c = 0; c < st.chunks; c++) {
                    l[c] = list[base + c];
                    l[c].stream -= (uint32_t)cursor;
                }
                stage += st.extra;
            }
            if (split && stage > run_stage) {
                HIP_TRY(ctx, hipMemcpyAsync(d_in + run_dev, hs + run_stage,
                                            stage - run_stage,
                                            hipMemcpyHostToDevice, P->s_in));
                ctx->hb_h2d_bytes += stage - run_stage;
            }
            const uint64_t first = split ? st.desc : stage;
            HIP_TRY(ctx, hipMemcpyAsync(d_in, hs, first, hipMemcpyHostToDevice,
                                        P->s_in));
            ctx->hb_h2d_bytes += first;
            HIP_TRY(ctx, hipEventRecord(s.ev_h2d, P->s_in));
            cursor = st.x.s1;
            planned++;
            ctx->hb_slices++;
        }
        // ---- slice t-1: the codec, and what brings its result home ----
        if (t >= 1 && t - 1 < planned) {
            PipeSlot &s = P->slot[(t - 1) % kSlots];
            const SliceState &st = state[(t - 1) % kSlots];
            const size_t m = st.m;
            uint8_t *dd = (uint8_t *)s.in.p;
            const void *const *d_in_ptrs = (const void *const *)dd;
            const uint64_t *d_in_lens = (const uint64_t *)(dd + 8 * m);
            void *const *d_out_ptrs = (void *const *)(dd + 16 * m);
            const uint64_t *d_out_caps = (const uint64_t *)(dd + 24 * m);
            uint64_t *d_out_lens = (uint64_t *)s.home.p;
            snapmi_error *d_errs = (snapmi_error *)((uint8_t *)s.home.p + 8 * m);
            uint8_t *h_home = (uint8_t *)s.hb_home.p;
            HIP_TRY(ctx, hipStreamWaitEvent(sK, s.ev_h2d, 0));
            HIP_TRY(ctx, hipMemsetAsync(s.home.p, 0, st.head, sK));
            if (compress) {
                const uint64_t *h_lens = (const uint64_t *)s.hb_in.p + m;
                if ((rc = (frame ? snapmi_frame_compress_batch
                                 : snapmi_compress_batch)(
                         ctx, d_in_ptrs, d_in_lens, h_lens, d_out_ptrs,
                         d_out_caps, d_out_lens, d_errs, m)))
                    return rc;
                uint64_t *sizes = (uint64_t *)s.desc.p, *offs = sizes + m;
                hipLaunchKernelGGL(k_hb_sizes,
                                   dim3((uint32_t)((m + 255) / 256)), dim3(256),
                                   0, sK, d_out_lens, d_errs, sizes,
                                   (uint32_t)m);
                HIP_TRY(ctx, hipGetLastError());
                if ((rc = launch_scan_u64(ctx, sK, sizes, offs, (uint32_t)m)))
                    return rc;
                uint64_t tiles = (st.x.out_bytes + kHbTile - 1) / kHbTile;
                if (tiles < 1)
                    tiles = 1;
                if (tiles > 8ull * cus)
                    tiles = 8ull * cus;
                uint8_t *dst = to_host ? h_home + st.head
                                       : (uint8_t *)s.home.p + st.head;
                hipLaunchKernelGGL(k_hb_pack, dim3((uint32_t)tiles), dim3(256),
                                   0, sK, (const void *const *)d_out_ptrs,
                                   d_out_lens, offs, (uint32_t)m, dst,
                                   &s.h_res->len);
                HIP_TRY(ctx, hipGetLastError());
                if (to_host && (rc = pipe_copy_home(ctx, sK, h_home, s.home.p,
                                                    st.head, true)))
                    return rc;
                HIP_TRY(ctx, hipEventRecord(s.ev_k, sK));
            } else {
                void *const *d_outs = lens_only ? nullptr : d_out_ptrs;
                const uint8_t *d_extra = dd + st.desc + st.x.in_bytes;
                if (st.listed) {
                    rc = frame_decompress_batch_listed(
                        ctx, d_in_ptrs, d_in_lens, d_outs, d_out_caps,
                        d_out_lens, d_errs, m, (const uint64_t *)d_extra,
                        d_extra + hb_align(8 * (m + 1)), st.chunks,
                        (uint32_t *)((uint8_t *)s.home.p + st.head - 16));
                    ctx->hb_listed_slices++;
                } else if (frame) {
                    rc = snapmi_frame_decompress_batch(ctx, d_in_ptrs,
                                                       d_in_lens, d_outs,
                                                       d_out_caps, d_out_lens,
                                                       d_errs, m);
                } else {
                    rc = snapmi_decompress_batch(ctx, d_in_ptrs, d_in_lens,
                                                 d_out_ptrs, d_out_caps,
                                                 d_out_lens, d_errs, m);
                }
                if (rc)
                    return rc;
                HIP_TRY(ctx, hipEventRecord(s.ev_k, sK));
                HIP_TRY(ctx, hipStreamWaitEvent(P->s_out, s.ev_k, 0));
                HIP_TRY(ctx, hipMemcpyAsync(h_home, s.home.p,
                                            st.head + st.x.out_bytes,
                                            hipMemcpyDeviceToHost, P->s_out));
                HIP_TRY(ctx, hipEventRecord(s.ev_d2h, P->s_out));
            }
        }
        // ---- slice t-2: wait for it, hand its streams out ----
        if (t >= 2 && t - 2 < planned) {
            PipeSlot &s = P->slot[(t - 2) % kSlots];
            const SliceState &st = state[(t - 2) % kSlots];
            const size_t m = st.m;
            uint8_t *h_home = (uint8_t *)s.hb_home.p;
            uint64_t total = st.x.out_bytes;
            if (compress) {
                HIP_TRY(ctx, hipEventSynchronize(s.ev_k));
                total = s.h_res->len;
                if (total > st.x.out_bytes)
                    return fail_ctx(ctx, SNAPMI_E_DEVICE,
                                    "%s: packed %llu > %llu", what,
                                    (unsigned long long)total,
                                    (unsigned long long)st.x.out_bytes);
                if (!to_host) {
                    HIP_TRY(ctx, hipMemcpyAsync(h_home, s.home.p,
                                                st.head + total,
                                                hipMemcpyDeviceToHost,
                                                P->s_out));
                    HIP_TRY(ctx, hipStreamSynchronize(P->s_out));
                }
            } else {
                HIP_TRY(ctx, hipEventSynchronize(s.ev_d2h));
            }
            ctx->hb_d2h_bytes += st.head + total;
            const uint64_t *lens = (const uint64_t *)h_home;
            const snapmi_error *errs = (const snapmi_error *)(h_home + 8 * m);
            const uint8_t *payload = h_home + st.head;
            if (prefix && *(const uint32_t *)(h_home + st.head - 16))
                return fail_ctx(ctx, SNAPMI_E_DEVICE,
                                "%s: streams %zu..%zu: the chunk list "
                                "disagrees with the bytes on the device",
                                what, st.x.s0, st.x.s1);
            uint64_t off = 0;
            for (size_t i = 0; i < m; i++) {
                const size_t g = st.x.s0 + i;
                if (h_errs)
                    h_errs[g] = errs[i];
                if (errs[i].kind != SNAPMI_OK && !prefix)
                    continue;
                const uint64_t len = lens[i];
                if (lens_only) {
                    h_out_lens[g] = (size_t)len;
                    continue;
                }
                if (len > rooms[g])
                    return fail_ctx(ctx, SNAPMI_E_DEVICE,
                                    "%s: stream %zu: device wrote %llu > %llu",
                                    what, g, (unsigned long long)len,
                                    (unsigned long long)rooms[g]);
                if (len)
                    memcpy(h_out_ptrs[g],
                           payload + (compress ? off : st.out_offs[i]), len);
                h_out_lens[g] = (size_t)len;
                off += hb_align(len);
            }
            if (compress && off != total)
                return fail_ctx(ctx, SNAPMI_E_DEVICE,
                                "%s: packed total %llu, lengths give %llu",
                                what, (unsigned long long)total,
                                (unsigned long long)off);
        }
        if (cursor >= n && t >= planned + 1)
            break;
    }
    if (compress && (rc = release_batch_scratch(ctx)))
        return rc;
    return SNAPMI_OK;
}

} // namespace

extern "C" {

int snapmi_compress_batch_host(snapmi_ctx *ctx, const void *const *h_in_ptrs,
                               const size_t *h_in_lens,
                               void *const *h_out_ptrs,
                               const size_t *h_out_caps, size_t *h_out_lens,
                               snapmi_error *h_errs, size_t n)
{
    return host_batch(ctx, kRaw, true, h_in_ptrs, h_in_lens, h_out_ptrs,
                      h_out_caps, h_out_lens, h_errs, n);
}

int snapmi_decompress_batch_host(snapmi_ctx *ctx,
                                 const void *const *h_in_ptrs,
                                 const size_t *h_in_lens,
                                 void *const *h_out_ptrs,
                                 const size_t *h_out_caps, size_t *h_out_lens,
                                 snapmi_error *h_errs, size_t n)
{
    return host_batch(ctx, kRaw, false, h_in_ptrs, h_in_lens, h_out_ptrs,
                      h_out_caps, h_out_lens, h_errs, n);
}

int snapmi_frame_compress_batch_host(snapmi_ctx *ctx,
                                     const void *const *h_in_ptrs,
                                     const size_t *h_in_lens,
                                     void *const *h_out_ptrs,
                                     const size_t *h_out_caps,
                                     size_t *h_out_lens, snapmi_error *h_errs,
                                     size_t n)
{
    return host_batch(ctx, kFrame, true, h_in_ptrs, h_in_lens, h_out_ptrs,
                      h_out_caps, h_out_lens, h_errs, n);
}

int snapmi_frame_decompress_batch_host(snapmi_ctx *ctx,
                                       const void *const *h_in_ptrs,
                                       const size_t *h_in_lens,
                                       void *const *h_out_ptrs,
                                       const size_t *h_out_caps,
                                       size_t *h_out_lens,
                                       snapmi_error *h_errs, size_t n)
{
    return host_batch(ctx, kFrame, false, h_in_ptrs, h_in_lens, h_out_ptrs,
                      h_out_caps, h_out_lens, h_errs, n);
}

} // extern "C"
