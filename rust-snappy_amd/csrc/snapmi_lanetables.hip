// snapmi_lanetables.hip -- the lane kernel's hash tables in HBM: where they
// are placed (the timed candidates), how they are freed, snapmi_ctx_prepare.
#include <hip/hip_runtime.h>

#include <chrono>
#include <cstdio>
#include <string>
#include <vector>

#include "snapmi.h"
#include "snapmi_ctx.hpp"
#include "snapmi_launch.hpp"
#include "snapmi_route.hpp"
#include "snapmi_device.hpp"
#include "snapmi_kernels.hpp"

using namespace snapmi;

namespace snapmi {
// the lane tables back to the device: a hipMalloc region, or physical chunks
// mapped into one address range (place_lane_tables)
void free_lane_tables(snapmi_ctx *ctx)
{
    if (!ctx->lane_tables.p)
        return;
    if (ctx->lane_va_bytes) {
        (void)hipMemUnmap(ctx->lane_tables.p, ctx->lane_va_bytes);
        for (auto h : ctx->lane_chunks)
            (void)hipMemRelease(h);
        (void)hipMemAddressFree(ctx->lane_tables.p, ctx->lane_va_bytes);
        ctx->lane_chunks.clear();
        ctx->lane_va_bytes = 0;
    } else {
        (void)hipFree(ctx->lane_tables.p);
    }
    ctx->lane_tables.p = nullptr;
    ctx->lane_tables.cap = 0;
    ctx->n_lanes = 0;
}

// ---------------------------------------------------------------------
// Placement probe for the lane tables (place_lane_tables, lane_table_tries):
// the access pattern of k_match_blocks' probe rounds - every lane a chain of
// dependent random 16-byte reads, each followed by a write to the same
// entry, in its own 256 KiB table - without any of the parse.  Its duration
// on a candidate region ranks that region for the real kernel.  The caller
// zeroes the tables afterwards.
// ---------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_probe_tables(unsigned long long *tables,
                                                     unsigned long long stride,
                                                     uint32_t steps,
                                                     uint32_t chunks,
                                                     uint32_t per_chunk)
{
    typedef __attribute__((address_space(1))) u32x4 g_u32x4;
    const uint32_t gid = blockIdx.x * 64 + threadIdx.x;
    // (the lane kernel's own lane -> table map: CompressArgs::lane_chunks)
    const uint32_t slot =
        chunks ? (gid % chunks) * per_chunk + gid / chunks : gid;
    g_u32x4 *t = (g_u32x4 *)tables + (uint64_t)slot * stride;
    uint32_t state = gid * 2654435761u + 12345u;
    for (uint32_t i = 0; i < steps; i++) {
        const uint32_t h = (state * 0x1E35A7BDu) >> 18;
        const u32x4 e = t[h];
        t[h] = (u32x4){state, i, h, gid};
        state = state * 1664525u + (e.x ^ e.y ^ e.z ^ e.w) + 1013904223u;
    }
    if (state == 0x12345678u) // keep the chain alive
        t[0] = (u32x4){state, 0, 0, 0};
}

// n 16-byte entries to zero (the lane tables when they are mapped chunks:
// nothing but a kernel is known to reach every such mapping)
__global__ __launch_bounds__(256) void k_zero16(unsigned long long *p,
                                                unsigned long long n)
{
    typedef __attribute__((address_space(1))) u32x4 g_u32x4;
    g_u32x4 *q = (g_u32x4 *)p;
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256 +
                                threadIdx.x;
         i < n; i += (unsigned long long)gridDim.x * 256)
        q[i] = (u32x4){0, 0, 0, 0};
}

// ---------------------------------------------------------------------
// The lane kernel's hash tables: one 256 KiB table of 16-byte entries per lane
// in flight, allocated when a launch first needs more lanes than the context
// has tables for.
//
// WHERE the tables lie decides 10-25 % of the match finder's duration: HBM
// sustains 2.0e10 dependent random read + write pairs per second on tables
// packed into the memory a fresh process is handed first, and 2.6e10 on
// tables that lie in the last third of the device's memory or are spread
// over enough of it (tests/hw/zone_map.hip, addr_bits.hip, vmm_layouts.hip;
// profiles/r6_table_placement.txt).  The placement cannot be requested, but
// it can be measured - k_probe_tables is the kernel's own access pattern -
// so at most lane_table_tries candidate regions are allocated and timed:
//   0. the tables SPREAD over as much memory as the budget allows (up to a
//      MiB per 256 KiB table);
//   1. the tables PACKED, allocated while candidate 0 is still held (so it
//      lies behind it);
//   2+ spread again, behind what is held.
// The search stops at the first candidate that probes at the fast rate; the
// best one is kept, the others are freed.  At NO moment does the context
// hold more than lane_table_budget_pct of the memory that was free when the
// placement began (tests/test_gpu_parity.py polls hipMemGetInfo from a second
// thread meanwhile).
//
// top_of_memory (snapmi_ctx_prepare with SNAPMI_PREPARE_TOP_OF_MEMORY, never
// taken by a compress call on its own): ONE packed candidate allocated while
// a filler holds everything else that is free, which is given back at once -
// the tables then lie at the far end of the device's memory, the fast part.
// For the duration of two hipMalloc calls the process holds the whole device
// (another allocation on it fails meanwhile), and the driver wipes what the
// filler gives back in the background (seconds for 250 GB, during which large
// allocations wait: round 5 did this once per candidate inside a compress
// call, ten times over - 72 s for a context's first 4 GiB batch,
// profiles/r6_sweep_repro_head.txt).  That is why it is a call of its own.
// ---------------------------------------------------------------------
int place_lane_tables(snapmi_ctx *ctx, uint32_t lanes, bool top_of_memory)
{
    int rc;
    const auto t_begin = std::chrono::steady_clock::now();
    const size_t tbytes = (size_t)kMaxTable * 16;
    if (ctx->lane_tables.p) {
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        free_lane_tables(ctx);
    }
    if ((rc = reserve(ctx, ctx->lane_epochs, (size_t)lanes * sizeof(uint32_t))))
        return rc;
    size_t free_b = 0, total_b = 0;
    HIP_TRY(ctx, hipMemGetInfo(&free_b, &total_b));
    const size_t free_before = free_b;
    // The GPU may be shared: what this context holds while it chooses, and
    // afterwards, stays within lane_table_budget_pct of what is free now (a
    // third by default).
    const size_t budget = free_b / 100 * ctx->lane_table_budget_pct;
    // (a handful of tables has no measurable placement: only a launch that
    // fills the chip is spread or probed)
    const bool full = lanes >= 16384;
    size_t spread = tbytes;
    if (ctx->lane_table_spread && full) {
        spread = budget / lanes / 4096 * 4096;
        if (spread > 4 * tbytes)
            spread = 4 * tbytes;
        if (spread < tbytes)
            spread = tbytes;
    }
    if (ctx->lane_table_stride_kib) // test option
        spread = (size_t)ctx->lane_table_stride_kib << 10;
    uint32_t tries = full && ctx->lane_table_tries ? ctx->lane_table_tries : 1;
    if (spread == tbytes && tries > 1 && !ctx->lane_table_stride_kib)
        tries = 1; // (the budget holds packed tables only: one region)
    if (top_of_memory)
        tries = 1;
    // what the probe takes at the fast rate: 768 dependent read + write
    // pairs per lane at 2.6e10 pairs/s (tests/hw/random_rw16.hip), 3 % on top
    const float fast_ms = (float)((double)lanes * 768 / 2.6e10 * 1e3 * 1.03);
    struct Cand {
        void *p = nullptr;
        size_t stride = 0, bytes = 0;
        float ms = 0;
    };
    // (an error on the way out frees what was allocated here)
    struct Held {
        Cand best, other;
        ~Held()
        {
            for (void *p : {best.p, other.p})
                if (p)
                    (void)hipFree(p);
        }
    } held;
    ctx->probe_log.clear();
    size_t held_peak = 0;
    auto alloc = [&](Cand &c) {
        const bool ok =
            (ctx->lane_tables_uncached
                 ? hipExtMallocWithFlags(&c.p, c.bytes, hipDeviceMallocUncached)
                 : hipMalloc(&c.p, c.bytes)) == hipSuccess;
        if (!ok) {
            (void)hipGetLastError();
            c.p = nullptr;
        }
        return ok;
    };
    // ---- candidate 0 of a chip-filling launch: CHUNKS.  Spreading pays for
    // what lies between the tables with memory; here that memory is given
    // back.  Physical chunks (hipMemCreate) are created one after the other,
    // `pitch` times as many as the tables need; every pitch-th is mapped into
    // one address range and the others are released at once: the tables lie
    // packed in their range and spread over the device's memory, and the
    // context HOLDS what the tables fill (17 GB for 65 536 lanes) - within
    // the budget all the while (pitch x the tables for a moment).  Measured
    // equal to a MiB per table over memory that stays held
    // (tests/hw/vmm_layouts.hip, vmm_spread.hip: chunks of a GiB at every
    // fourth, of 256 MiB at every fourth, against 64 GiB held).  Any call of
    // the virtual-memory API that fails sends the placement to the plain
    // hipMalloc candidates below.
    if (full && ctx->lane_table_spread && !top_of_memory &&
        !ctx->lane_table_stride_kib && !ctx->lane_tables_uncached) {
        const size_t bytes = (size_t)lanes * tbytes;
        const size_t CH = bytes >= ((size_t)8 << 30) ? (size_t)1 << 30
                                                     : (size_t)256 << 20;
        const size_t need = (bytes + CH - 1) / CH;
        size_t pitch = budget / (need * CH);
        if (pitch > 4)
            pitch = 4;
        if (pitch >= 2) {
            hipMemAllocationProp prop = {};
            prop.type = hipMemAllocationTypePinned;
            prop.location.type = hipMemLocationTypeDevice;
            prop.location.id = ctx->device;
            std::vector<hipMemGenericAllocationHandle_t> all;
            all.reserve(need * pitch);
            bool ok = true;
            for (size_t i = 0; ok && i < need * pitch; i++) {
                hipMemGenericAllocationHandle_t h;
                ok = hipMemCreate(&h, CH, &prop, 0) == hipSuccess;
                if (ok)
                    all.push_back(h);
            }
            void *va = nullptr;
            size_t mapped = 0;
            if (ok)
                ok = hipMemAddressReserve(&va, need * CH, 0, nullptr, 0) ==
                     hipSuccess;
            if (ok) {
                // (the last of every group of `pitch`: the farthest in)
                for (size_t i = 0; ok && i < need; i++) {
                    ok = hipMemMap((char *)va + i * CH, CH, 0,
                                   all[i * pitch + pitch - 1], 0) == hipSuccess;
                    if (ok)
                        mapped = i + 1;
                }
            }
            if (ok) {
                hipMemAccessDesc acc = {};
                acc.location = prop.location;
                acc.flags = hipMemAccessFlagsProtReadWrite;
                ok = hipMemSetAccess(va, need * CH, &acc, 1) == hipSuccess;
            }
            held_peak = all.size() * CH;
            // give back what lies between - on failure everything: the
            // mappings first, every chunk once, the address range
            if (!ok) {
                (void)hipGetLastError();
                if (mapped)
                    (void)hipMemUnmap(va, mapped * CH);
            }
            std::vector<hipMemGenericAllocationHandle_t> kept;
            for (size_t i = 0; i < all.size(); i++) {
                if (ok && i % pitch == pitch - 1)
                    kept.push_back(all[i]);
                else
                    (void)hipMemRelease(all[i]);
            }
            if (!ok) {
                if (va)
                    (void)hipMemAddressFree(va, need * CH);
                held_peak = 0;
                ctx->probe_log += "chunks: the virtual-memory calls failed ";
            } else {
                ctx->lane_tables.p = va;
                ctx->lane_tables.cap = need * CH;
                ctx->lane_chunks = kept;
                ctx->lane_chunk_bytes = CH;
                ctx->lane_va_bytes = need * CH;
                ctx->lane_stride = tbytes / 16;
                ctx->lane_chunk_count = (uint32_t)need;
                ctx->lane_per_chunk = (uint32_t)(CH / tbytes);
                float ms = 0;
                const uint32_t per_chunk = (uint32_t)(CH / tbytes);
                hipLaunchKernelGGL(k_probe_tables, dim3(lanes / 64), dim3(64),
                                   0, ctx->stream, (unsigned long long *)va,
                                   (unsigned long long)(tbytes / 16), 64u,
                                   (uint32_t)need, per_chunk);
                HIP_TRY(ctx, hipEventRecord(ctx->ev[4], ctx->stream));
                hipLaunchKernelGGL(k_probe_tables, dim3(lanes / 64), dim3(64),
                                   0, ctx->stream, (unsigned long long *)va,
                                   (unsigned long long)(tbytes / 16), 768u,
                                   (uint32_t)need, per_chunk);
                HIP_TRY(ctx, hipEventRecord(ctx->ev[5], ctx->stream));
                HIP_TRY(ctx, hipEventSynchronize(ctx->ev[5]));
                HIP_TRY(ctx, hipEventElapsedTime(&ms, ctx->ev[4], ctx->ev[5]));
                // tables start as "never used": epoch 0 in every entry
                // (every chunk in full: the lanes' tables are dealt out
                // over all of them)
                hipLaunchKernelGGL(k_zero16, dim3(ctx->num_cus * 8), dim3(256),
                                   0, ctx->stream, (unsigned long long *)va,
                                   (unsigned long long)(need * CH / 16));
                HIP_TRY(ctx, hipMemsetAsync(ctx->lane_epochs.p, 0,
                                            (size_t)lanes * 4, ctx->stream));
                ctx->n_lanes = lanes;
                size_t free_after = 0;
                (void)hipMemGetInfo(&free_after, &total_b);
                const double t_ms =
                    std::chrono::duration<double, std::milli>(
                        std::chrono::steady_clock::now() - t_begin).count();
                char buf[320];
                snprintf(buf, sizeof buf,
                         "%.2f(chunks: %zu of %zu x %zu MiB) | held at most "
                         "%zu of budget %zu | kept %zu KiB apart, %u lanes, "
                         "%zu bytes | placement %.1f ms | free %zu -> %zu",
                         ms, need, need * pitch, CH >> 20, held_peak, budget,
                         tbytes >> 10, lanes, ctx->lane_tables.cap, t_ms,
                         free_before, free_after);
                ctx->probe_log += buf;
                return SNAPMI_OK;
            }
        }
    }
    for (uint32_t t = 0; t < tries; t++) {
        Cand c;
        c.stride = top_of_memory || (t & 1) ? tbytes : spread;
        c.bytes = (size_t)lanes * c.stride;
        // a loser is freed before the next candidate comes unless the budget
        // has room for all three (then the new one cannot be the loser's
        // memory again)
        const size_t alive = held.best.bytes + held.other.bytes;
        if (held.other.p && alive + c.bytes > budget) {
            HIP_TRY(ctx, hipFree(held.other.p));
            held.other = Cand();
        }
        if (t && held.best.bytes + held.other.bytes + c.bytes > budget)
            break; // no room for another candidate within the budget
        void *filler = nullptr;
        if (top_of_memory) {
            // everything that is free but the region itself and a GiB
            // beside it (with less left free the region is pieced together
            // from what is free elsewhere, profiles/r5_table_budget.txt)
            const size_t spare = c.bytes + ((size_t)1 << 30);
            size_t want = free_b > spare ? free_b - spare : 0;
            for (int k = 0; k < 3 && want >= ((size_t)8 << 30); k++) {
                if (hipMalloc(&filler, want) == hipSuccess)
                    break;
                (void)hipGetLastError();
                filler = nullptr;
                want = want / 16 * 15;
            }
        }
        bool got = alloc(c);
        if (filler) {
            (void)hipFree(filler);
            if (!got) // (not behind the filler: the plain way)
                got = alloc(c);
        }
        if (!got)
            break; // keep the best so far
        {
            const size_t now = held.best.bytes + held.other.bytes + c.bytes;
            held_peak = now > held_peak ? now : held_peak;
        }
        // (the probe runs on the memory as it comes: only the region that is
        // kept gets zeroed)
        if (tries > 1 || ctx->lane_table_probe || top_of_memory) {
            hipLaunchKernelGGL(k_probe_tables, dim3(lanes / 64), dim3(64), 0,
                               ctx->stream, (unsigned long long *)c.p,
                               (unsigned long long)(c.stride / 16), 64u, 0u,
                               0u);
            HIP_TRY(ctx, hipEventRecord(ctx->ev[4], ctx->stream));
            hipLaunchKernelGGL(k_probe_tables, dim3(lanes / 64), dim3(64), 0,
                               ctx->stream, (unsigned long long *)c.p,
                               (unsigned long long)(c.stride / 16), 768u, 0u,
                               0u);
            HIP_TRY(ctx, hipEventRecord(ctx->ev[5], ctx->stream));
            HIP_TRY(ctx, hipEventSynchronize(ctx->ev[5]));
            HIP_TRY(ctx, hipEventElapsedTime(&c.ms, ctx->ev[4], ctx->ev[5]));
            char buf[48];
            snprintf(buf, sizeof buf, "%s%.2f(%zuK)", t ? " " : "", c.ms,
                     c.stride >> 10);
            ctx->probe_log += buf;
        }
        if (!held.best.p || c.ms < held.best.ms) {
            if (held.other.p) {
                HIP_TRY(ctx, hipFree(held.other.p));
                held.other = Cand();
            }
            held.other = held.best;
            held.best = c;
        } else {
            if (held.other.p)
                HIP_TRY(ctx, hipFree(held.other.p));
            held.other = c;
        }
        if (tries > 1 && held.best.ms <= fast_ms)
            break;
    }
    if (held.other.p) {
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        HIP_TRY(ctx, hipFree(held.other.p));
        held.other = Cand();
    }
    if (!held.best.p)
        return fail_ctx(ctx, SNAPMI_E_DEVICE,
                        "hipMalloc of %zu bytes of lane tables failed",
                        (size_t)lanes * tbytes);
    // tables start as "never used": epoch 0 in every entry
    HIP_TRY(ctx, hipMemset2DAsync(held.best.p, held.best.stride, 0, tbytes,
                                  lanes, ctx->stream));
    ctx->lane_tables.p = held.best.p;
    ctx->lane_tables.cap = held.best.bytes;
    ctx->lane_chunk_count = 0;
    ctx->lane_per_chunk = 0;
    ctx->lane_stride = held.best.stride / 16;
    held.best = Cand(); // the context owns it now
    HIP_TRY(ctx, hipMemsetAsync(ctx->lane_epochs.p, 0, (size_t)lanes * 4,
                                ctx->stream));
    ctx->n_lanes = lanes;
    {
        size_t free_after = 0;
        (void)hipMemGetInfo(&free_after, &total_b);
        const double ms =
            std::chrono::duration<double, std::milli>(
                std::chrono::steady_clock::now() - t_begin).count();
        char buf[256];
        snprintf(buf, sizeof buf,
                 " | held at most %zu of budget %zu | kept %zu KiB apart, "
                 "%u lanes, %zu bytes%s | placement %.1f ms | free %zu -> %zu",
                 held_peak, budget, (size_t)(ctx->lane_stride * 16) >> 10,
                 lanes, ctx->lane_tables.cap,
                 top_of_memory ? " (top of memory)" : "", ms, free_before,
                 free_after);
        ctx->probe_log += buf;
    }
    return SNAPMI_OK;
}


// snapmi_ctx_prepare: the tables a batch of `blocks` blocks would make the
// first compress call allocate, now (prepare_lanes, snapmi_route.hpp);
// nothing when such a batch does not run the lane kernel or the context
// already has that many tables - unless the far end of the memory is asked
// for and the tables are not there yet.
int prepare_lane_tables(snapmi_ctx *ctx, uint64_t blocks, bool top)
{
    const uint32_t lanes = prepare_lanes(
        *ctx, {ctx->lds_order_ok, (uint32_t)ctx->num_cus}, blocks);
    if (!lanes)
        return SNAPMI_OK;
    if (lanes <= ctx->n_lanes && !(top && !ctx->lane_tables_top))
        return SNAPMI_OK;
    const int rc = place_lane_tables(ctx, lanes > ctx->n_lanes ? lanes
                                                               : ctx->n_lanes,
                                     top);
    if (rc == SNAPMI_OK)
        ctx->lane_tables_top = top;
    return rc;
}

} // namespace snapmi

extern "C" {

int snapmi_ctx_prepare(snapmi_ctx *ctx, uint64_t blocks, uint32_t flags)
{
    if (!ctx || (flags & ~(uint32_t)SNAPMI_PREPARE_TOP_OF_MEMORY))
        return SNAPMI_E_ARGUMENT;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return snapmi::prepare_lane_tables(
        ctx, blocks, (flags & SNAPMI_PREPARE_TOP_OF_MEMORY) != 0);
}

} // extern "C"
