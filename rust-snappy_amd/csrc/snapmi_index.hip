// snapmi_index.hip -- the block index of raw streams on the host side:
// indexed decode, range reads, and the index of streams that came without one
// (range writes and appends: snapmi_update.hip).
#include <hip/hip_runtime.h>

#include <cstring>
#include <vector>

#include "snapmi.h"
#include "snapmi_ctx.hpp"
#include "snapmi_launch.hpp"
#include "snapmi_device.hpp"
#include "snapmi_kernels.hpp"

using namespace snapmi;

static_assert(kBiBuilt == SNAPMI_INDEX_BUILT &&
                  kBiUnaligned == SNAPMI_INDEX_UNALIGNED &&
                  kBiCorrupt == SNAPMI_INDEX_CORRUPT &&
                  kBiMissized == SNAPMI_INDEX_MISSIZED,
              "snapmi_blockindex.hpp restates the verdicts of snapmi.h");

extern "C" {

// The batch with the block index its compressor wrote
// (snapmi_blockindex.hpp; the kernels: k_index_* in snapmi_decompress.hip).
// Enqueue-only: index_entries, the host's copy of first[n], sizes every
// launch, and what the device finds out - whether any stream is indexed,
// which streams' pieces came out whole - reaches the launches behind it
// through device memory (the gate, the modes of the batch's own launch).
int snapmi_decompress_batch_indexed(snapmi_ctx *ctx,
                                    const void *const *d_in_ptrs,
                                    const uint64_t *d_in_lens,
                                    void *const *d_out_ptrs,
                                    const uint64_t *d_out_caps,
                                    uint64_t *d_out_lens,
                                    snapmi_error *d_errs, size_t n,
                                    const uint64_t *d_index_first,
                                    const uint64_t *d_index,
                                    uint64_t index_entries)
{
    if (!ctx)
        return SNAPMI_E_ARGUMENT;
    if (n == 0)
        return SNAPMI_OK;
    if (!d_in_ptrs || !d_in_lens || !d_out_ptrs || !d_out_caps ||
        !d_out_lens || (uint64_t)n + index_entries > 0x7FFFFFFFu ||
        (index_entries && (!d_index_first || !d_index)))
        return fail_ctx(ctx, SNAPMI_E_ARGUMENT,
                        "decompress_batch_indexed: bad args");
    ctx->ix_stats_live = false;
    // (an indexed stream owns three entries or more)
    if (index_entries < 3)
        return launch_decompress(ctx, d_in_ptrs, d_in_lens, d_out_ptrs,
                                 d_out_caps, d_out_lens, d_errs, nullptr, n);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const size_t E = (size_t)index_entries, T = n + E;
    int rc;
    const bool fresh_gate = !ctx->ix_gate.p;
    // the list of T slots, and behind it c_owner [E] (u32)
    const size_t owner_off = (piece_offsets(T).total + 3) & ~(size_t)3;
    // (everything the call's launches need, before the first of them: a
    // buffer that grows waits for the stream)
    if ((rc = reserve(ctx, ctx->ix_modes, n)) ||
        (rc = reserve(ctx, ctx->ix_desc, owner_off + E * 4)) ||
        (rc = reserve(ctx, ctx->ix_gate, 64)) ||
        (rc = reserve(ctx, ctx->order, (T + 72) * sizeof(uint32_t))))
        return rc;
    if (fresh_gate)
        HIP_TRY(ctx, hipMemsetAsync(ctx->ix_gate.p, 0, 64, s));
    const PieceList l = piece_list(ctx->ix_desc.p, T);
    IndexArgs x;
    x.in_ptrs = d_in_ptrs;
    x.in_lens = d_in_lens;
    x.out_ptrs = d_out_ptrs;
    x.out_caps = d_out_caps;
    x.out_lens = d_out_lens;
    x.errs = d_errs;
    x.first = d_index_first;
    x.index = d_index;
    x.entries = index_entries;
    x.n = (uint32_t)n;
    x.modes = (uint8_t *)ctx->ix_modes.p;
    x.c_in = l.c_in;
    x.c_inlen = l.c_inlen;
    x.c_out = l.c_out;
    x.c_cap = l.c_cap;
    x.c_outlen = l.c_outlen;
    x.c_err = l.c_err;
    x.c_mode = l.c_mode;
    x.c_owner = (uint32_t *)((uint8_t *)ctx->ix_desc.p + owner_off);
    x.gate = (unsigned long long *)ctx->ix_gate.p;
    x.seq = ++ctx->ix_seq;
    hipLaunchKernelGGL(k_index_plan, dim3((uint32_t)((n + 255) / 256)),
                       dim3(256), 0, s, x);
    LAUNCH_CHECK(k_index_plan);
    ctx->ix_stats_live = true;
    hipLaunchKernelGGL(k_index_pieces, dim3((uint32_t)((E + 255) / 256)),
                       dim3(256), 0, s, x);
    LAUNCH_CHECK(k_index_pieces);
    // the batch: whole streams and pieces in one launch
    if ((rc = launch_pieces(ctx, l, T)))
        return rc;
    hipLaunchKernelGGL(k_index_finish, dim3((uint32_t)((n + 3) / 4)),
                       dim3(256), 0, s, x);
    LAUNCH_CHECK(k_index_finish);
    // the indexed streams that were handed back, if any (they announce more
    // than a block of output: none is of the lane-per-stream classes)
    return launch_decompress(ctx, d_in_ptrs, d_in_lens, d_out_ptrs, d_out_caps,
                             d_out_lens, d_errs, x.modes, n, x.gate + 3, x.seq,
                             nullptr, nullptr, /*wide_only=*/true);
}

// Range reads through the block index (snapmi_blockindex.hpp; the kernels:
// k_range_* in snapmi_decompress.hip).  Enqueue-only: the host copies of the
// ranges size every launch and every buffer, and cut the ranges into groups
// whose edge rooms fit "range_scratch_bytes"; the groups follow each other on
// the stream and reuse the rooms and the descriptor list.
uint64_t snapmi_range_pieces(const uint64_t *h_range_off,
                             const uint64_t *h_range_len, size_t m)
{
    uint64_t pieces = 0;
    for (size_t r = 0; h_range_off && h_range_len && r < m; r++) {
        uint64_t k0;
        const uint64_t c =
            snapmi::bi_range_blocks(h_range_off[r], h_range_len[r], &k0);
        pieces = pieces + c < pieces ? ~0ull : pieces + c; // (saturates)
    }
    return pieces;
}

int snapmi_decompress_ranges_indexed(
    snapmi_ctx *ctx, const void *const *d_in_ptrs, const uint64_t *d_in_lens,
    size_t n, const uint64_t *d_index_first, const uint64_t *d_index,
    uint64_t index_entries, const uint32_t *d_range_stream,
    const uint64_t *d_range_off, const uint64_t *d_range_len,
    const uint64_t *h_range_off, const uint64_t *h_range_len,
    void *const *d_range_out, uint64_t *d_range_got,
    snapmi_error *d_range_errs, size_t m)
{
    if (!ctx)
        return SNAPMI_E_ARGUMENT;
    if (m == 0)
        return SNAPMI_OK;
    if (!h_range_off || !h_range_len || !d_range_stream || !d_range_off ||
        !d_range_len || !d_range_out || !d_range_got ||
        (n && (!d_in_ptrs || !d_in_lens || !d_index_first)) ||
        (index_entries && !d_index) || m > 0x7FFFFFFFu)
        return fail_ctx(ctx, SNAPMI_E_ARGUMENT,
                        "decompress_ranges_indexed: bad args");
    const uint64_t P = snapmi_range_pieces(h_range_off, h_range_len, m);
    if (P > 0x7FFFFFFFu || (uint64_t)n + index_entries + P > 0x7FFFFFFFu)
        return fail_ctx(ctx, SNAPMI_E_ARGUMENT,
                        "decompress_ranges_indexed: n + index_entries + "
                        "pieces must stay below 2^31");
    // the groups: consecutive ranges whose edge rooms fit the scratch (a
    // range has at most two: the floor of the option holds any one range)
    struct Group {
        uint32_t r0, mg;
        uint64_t pieces, rooms;
    };
    const uint64_t room_cap = ctx->range_scratch_bytes / kBiBlock;
    std::vector<Group> groups;
    Group g{0, 0, 0, 0};
    uint64_t max_pieces = 0, max_rooms = 0;
    for (size_t r = 0; r < m; r++) {
        uint64_t k0;
        const uint64_t c = bi_range_blocks(h_range_off[r], h_range_len[r], &k0);
        const uint32_t e = bi_range_edges(h_range_off[r], h_range_len[r]);
        if (g.mg && g.rooms + e > room_cap) {
            groups.push_back(g);
            g = Group{(uint32_t)r, 0, 0, 0};
        }
        g.mg++;
        g.pieces += c;
        g.rooms += e;
        if (r + 1 == m)
            groups.push_back(g);
    }
    for (const Group &q : groups) {
        max_pieces = q.pieces > max_pieces ? q.pieces : max_pieces;
        max_rooms = q.rooms > max_rooms ? q.rooms : max_rooms;
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    ctx->rg_stats_live = false;
    ctx->rg_pieces = P;
    int rc;
    // (everything the call's launches need, before the first of them: a
    // buffer that grows waits for the stream)
    const size_t parts_max = (m + 1023) / 1024;
    if ((rc = reserve(ctx, ctx->rg_desc,
                      piece_offsets((size_t)max_pieces).total)) ||
        (rc = reserve(ctx, ctx->rg_meta, m * 17 + 64)) ||
        (rc = reserve(ctx, ctx->rg_part, parts_max * 16 + 64)) ||
        (rc = reserve(ctx, ctx->rg_room, max_rooms * kBiBlock + 64)) ||
        (rc = reserve(ctx, ctx->rg_stat, 64)) ||
        (rc = reserve(ctx, ctx->order,
                      (max_pieces + 72) * sizeof(uint32_t))))
        return rc;
    HIP_TRY(ctx, hipMemsetAsync(ctx->rg_stat.p, 0, 64, s));
    ctx->rg_stats_live = true;
    RangeArgs x;
    x.in_ptrs = d_in_ptrs;
    x.in_lens = d_in_lens;
    x.first = d_index_first;
    x.index = d_index;
    x.entries = index_entries;
    x.n = (uint32_t)n;
    x.r_stream = d_range_stream;
    x.r_off = d_range_off;
    x.r_len = d_range_len;
    x.r_out = d_range_out;
    x.r_got = d_range_got;
    x.r_errs = d_range_errs;
    x.slot = (uint64_t *)ctx->rg_meta.p;
    x.eslot = x.slot + m;
    x.state = (uint8_t *)(x.eslot + m);
    x.part = (uint64_t *)ctx->rg_part.p;
    x.room = (uint8_t *)ctx->rg_room.p;
    x.stat = (unsigned long long *)ctx->rg_stat.p;
    for (const Group &q : groups) {
        const size_t T = (size_t)q.pieces;
        const PieceList l = piece_list(ctx->rg_desc.p, T);
        x.r0 = q.r0;
        x.mg = q.mg;
        x.pieces = q.pieces;
        x.rooms = q.rooms;
        x.c_in = l.c_in;
        x.c_inlen = l.c_inlen;
        x.c_out = l.c_out;
        x.c_cap = l.c_cap;
        x.c_outlen = l.c_outlen;
        x.c_err = l.c_err;
        x.c_mode = l.c_mode;
        const uint32_t parts = (q.mg + 1023) / 1024;
        hipLaunchKernelGGL(k_range_scan_a, dim3(parts), dim3(1024), 0, s, x);
        LAUNCH_CHECK(k_range_scan_a);
        hipLaunchKernelGGL(k_range_scan_b, dim3(1), dim3(1024), 0, s, x,
                           parts);
        LAUNCH_CHECK(k_range_scan_b);
        hipLaunchKernelGGL(k_range_scan_c, dim3(parts), dim3(1024), 0, s, x);
        LAUNCH_CHECK(k_range_scan_c);
        hipLaunchKernelGGL(k_range_plan, dim3((q.mg + 255) / 256), dim3(256),
                           0, s, x);
        LAUNCH_CHECK(k_range_plan);
        if (T) {
            hipLaunchKernelGGL(k_range_pieces,
                               dim3((uint32_t)((T + 255) / 256)), dim3(256),
                               0, s, x);
            LAUNCH_CHECK(k_range_pieces);
            if ((rc = launch_pieces(ctx, l, T)))
                return rc;
            hipLaunchKernelGGL(k_range_finish, dim3((q.mg + 3) / 4),
                               dim3(256), 0, s, x);
            LAUNCH_CHECK(k_range_finish);
        }
    }
    return SNAPMI_OK;
}

// The block index of streams that came without one (bi_build of
// snapmi_blockindex.hpp; the kernels: k_index_build_*, k_index_walk in
// snapmi_decompress.hip).  The host's copies of the lengths size the index,
// the scratch and every launch; what the device finds out - which streams are
// missized, which the scan gave up on - reaches the launches behind it
// through device memory (the states, the walk list and its count).
// Pending streams (two blocks and more by the host's copy) are cut into
// groups of at most index_build_group_streams streams and kBuildGroupBytes of
// input - a longer stream is a group of its own - so that the descriptors and
// the scan's tables are bounded whatever n is; the groups run back to back on
// the stream and reuse the tables.
int snapmi_build_block_index(snapmi_ctx *ctx, const void *const *d_in_ptrs,
                             const uint64_t *d_in_lens,
                             const uint64_t *h_in_lens,
                             const uint64_t *h_out_lens, size_t n,
                             uint64_t *d_index_first, uint64_t *d_index,
                             uint64_t index_cap, uint8_t *d_status)
{
    if (!ctx)
        return SNAPMI_E_ARGUMENT;
    if (!d_index_first || n > 0x7FFFFFFFu ||
        (n && (!d_in_ptrs || !d_in_lens || !h_in_lens || !h_out_lens)))
        return fail_ctx(ctx, SNAPMI_E_ARGUMENT, "build_block_index: bad args");
    const uint64_t entries = snapmi_block_index_entries(h_out_lens, n);
    if (entries > index_cap || (entries && !d_index))
        return fail_ctx(ctx, SNAPMI_E_ARGUMENT,
                        "build_block_index: the index takes %llu entries, "
                        "index_cap is %llu",
                        (unsigned long long)entries,
                        (unsigned long long)index_cap);
    if ((uint64_t)n + entries > 0x7FFFFFFFu)
        return fail_ctx(ctx, SNAPMI_E_ARGUMENT,
                        "build_block_index: n + entries must stay below 2^31");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    ctx->ib_stats_live = false;
    if (n == 0) {
        HIP_TRY(ctx, hipMemsetAsync(d_index_first, 0, sizeof(uint64_t), s));
        return SNAPMI_OK;
    }
    // a pending stream longer than this is the walker's: no valid stream is
    // (a length of 2^32 - 1 compresses to less than 2^33 bytes), and the
    // scan's plan (plan_streams: fits) holds everything below it
    constexpr uint64_t kScanMaxLen = 1ull << 36;
    constexpr uint64_t kBuildGroupBytes = 256ull << 20;
    const uint32_t route = ctx->index_build_route;

    // ---- the groups of the scan route, planned on the host ----------------
    struct Group {
        StreamPlan p;
        size_t j0; // its first stream in slots / idx
    };
    std::vector<StreamSlot> slots;
    std::vector<uint32_t> idx;
    std::vector<Group> groups;
    std::vector<std::vector<uint32_t>> pres;
    size_t pending = 0;
    if (route != 1) {
        size_t j0 = 0;
        uint64_t bytes = 0;
        auto flush = [&]() {
            if (slots.size() == j0)
                return;
            const uint32_t mg = (uint32_t)(slots.size() - j0);
            pres.emplace_back((size_t)kPre * (mg + 1));
            Group g;
            g.j0 = j0;
            g.p = plan_streams(slots.data() + j0, mg, false,
                               ctx->stream_seg_log2, ctx->stream_scan_segs,
                               sizeof(StreamArgs), pres.back().data());
            groups.push_back(g);
            j0 = slots.size();
            bytes = 0;
        };
        for (size_t i = 0; i < n; i++) {
            if (h_out_lens[i] <= kBiBlock)
                continue;
            pending++;
            if (h_in_lens[i] > kScanMaxLen)
                continue;
            if (slots.size() - j0 >= ctx->index_build_group_streams ||
                (slots.size() > j0 && bytes + h_in_lens[i] > kBuildGroupBytes))
                flush();
            StreamSlot t = {};
            t.in_len = h_in_lens[i];
            t.bound = h_out_lens[i];
            slots.push_back(t);
            idx.push_back((uint32_t)i);
            bytes += h_in_lens[i];
        }
        flush();
    } else {
        for (size_t i = 0; i < n; i++)
            pending += h_out_lens[i] > kBiBlock;
    }
    size_t t_bytes = 0, g_bytes = 0;
    for (const Group &g : groups) {
        if (!g.p.fits)
            return fail_ctx(ctx, SNAPMI_E_ARGUMENT,
                            "build_block_index: a stream too long to plan");
        t_bytes = g.p.t_bytes > t_bytes ? g.p.t_bytes : t_bytes;
        const size_t b = g.p.desc_bytes + (size_t)g.p.n * sizeof(uint32_t);
        g_bytes = b > g_bytes ? b : g_bytes;
    }

    // ---- everything the launches need, before the first of them -----------
    // device: h_in [n], h_out [n], first [n + 1], walk list [n] (u32),
    // states [n]
    const size_t plan_bytes = (3 * n + 1) * sizeof(uint64_t);
    int rc;
    if ((rc = reserve(ctx, ctx->ib_meta, plan_bytes + n * 5 + 64)) ||
        (rc = reserve(ctx, ctx->ib_stat, 64)) ||
        (groups.size() &&
         ((rc = reserve(ctx, ctx->sd_tables, t_bytes)) ||
          (rc = reserve(ctx, ctx->bl_descs, g_bytes + 64)))))
        return rc;
    for (hipEvent_t *ev : {&ctx->ev_ib, &ctx->ev_ibg[0], &ctx->ev_ibg[1]})
        if (!*ev)
            HIP_TRY(ctx, hipEventCreateWithFlags(ev, hipEventDisableTiming));
    // (the staging of an earlier call may still be read by its copy: wait for
    // that copy's event, not for the stream)
    auto staging = [&](PinBuf &b, size_t bytes, hipEvent_t ev,
                       bool *live) -> int {
        if (*live) {
            HIP_TRY(ctx, hipEventSynchronize(ev));
            *live = false;
        }
        return pin_reserve(ctx, b, bytes);
    };
    if ((rc = staging(ctx->pin_ib, plan_bytes, ctx->ev_ib, &ctx->ev_ib_live)))
        return rc;
    if (groups.size())
        for (int q = 0; q < 2; q++)
            if ((rc = pin_reserve(ctx, ctx->pin_ibg[q], g_bytes)))
                return rc;

    // ---- the host's arrays and the prefix sum, to the device --------------
    uint64_t *const hp = (uint64_t *)ctx->pin_ib.p;
    memcpy(hp, h_in_lens, n * sizeof(uint64_t));
    memcpy(hp + n, h_out_lens, n * sizeof(uint64_t));
    uint64_t *const hfirst = hp + 2 * n;
    hfirst[0] = 0;
    for (size_t i = 0; i < n; i++)
        hfirst[i + 1] = hfirst[i] + bi_entries(h_out_lens[i]);
    uint64_t *const dp = (uint64_t *)ctx->ib_meta.p;
    HIP_TRY(ctx, hipMemcpyAsync(dp, hp, plan_bytes, hipMemcpyHostToDevice, s));
    HIP_TRY(ctx, hipMemcpyAsync(d_index_first, hfirst,
                                (n + 1) * sizeof(uint64_t),
                                hipMemcpyHostToDevice, s));
    HIP_TRY(ctx, hipEventRecord(ctx->ev_ib, s));
    ctx->ev_ib_live = true;
    HIP_TRY(ctx, hipMemsetAsync(ctx->ib_stat.p, 0, 64, s));
    HIP_TRY(ctx, hipMemsetAsync(d_index, 0, entries * sizeof(uint64_t), s));
    ctx->ib_stats_live = true;

    BuildArgs x;
    x.in_ptrs = d_in_ptrs;
    x.in_lens = d_in_lens;
    x.h_in = dp;
    x.h_out = dp + n;
    x.first = dp + 2 * n;
    x.index = d_index;
    x.status = d_status;
    x.n = (uint32_t)n;
    x.walk = (uint32_t *)(dp + 3 * n + 1);
    x.state = (uint8_t *)(x.walk + n);
    x.stat = (unsigned long long *)ctx->ib_stat.p;
    x.route = route;
    x.scan_max_len = kScanMaxLen;
    hipLaunchKernelGGL(k_index_build_plan, dim3((uint32_t)((n + 255) / 256)),
                       dim3(256), 0, s, x);
    LAUNCH_CHECK(k_index_build_plan);

    // ---- the scan route, group by group -----------------------------------
    for (size_t gi = 0; gi < groups.size(); gi++) {
        const Group &g = groups[gi];
        const StreamPlan &p = g.p;
        const uint32_t mg = p.n;
        const int q = (int)(ctx->ib_groups++ & 1);
        if (ctx->ev_ibg_live[q]) {
            HIP_TRY(ctx, hipEventSynchronize(ctx->ev_ibg[q]));
            ctx->ev_ibg_live[q] = false;
        }
        StreamArgs *const descs = (StreamArgs *)ctx->pin_ibg[q].p;
        for (uint32_t j = 0; j < mg; j++) {
            StreamArgs &a = descs[j];
            const StreamSlot &t = slots[g.j0 + j];
            memset(&a, 0, sizeof a);
            a.in = nullptr; // (k_index_build_adopt)
            a.in_len = t.in_len;
            // no output exists: stream_head only asks that dlen fits
            a.out = nullptr;
            a.out_cap = t.bound;
            stream_pointers(ctx, p, t, a);
            a.c_in = nullptr; // no piece descriptors: nothing is decoded
            a.c_inlen = nullptr;
            a.c_out = nullptr;
            a.c_cap = nullptr;
            a.c_outlen = nullptr;
            a.c_err = nullptr;
            a.c_mode = nullptr;
        }
        uint8_t *const blk = (uint8_t *)descs;
        memcpy(blk + p.pre_off, pres[gi].data(),
               pres[gi].size() * sizeof(uint32_t));
        memcpy(blk + p.desc_bytes, idx.data() + g.j0, mg * sizeof(uint32_t));
        const size_t bytes = p.desc_bytes + (size_t)mg * sizeof(uint32_t);
        HIP_TRY(ctx, hipMemcpyAsync(ctx->bl_descs.p, descs, bytes,
                                    hipMemcpyHostToDevice, s));
        HIP_TRY(ctx, hipEventRecord(ctx->ev_ibg[q], s));
        ctx->ev_ibg_live[q] = true;
        HIP_TRY(ctx, hipMemsetAsync((uint8_t *)ctx->sd_tables.p + p.e_off,
                                    0xFF, p.e_bytes, s));
        BuildGroup bg;
        bg.descs = (StreamArgs *)ctx->bl_descs.p;
        bg.idx = (const uint32_t *)((const uint8_t *)ctx->bl_descs.p +
                                    p.desc_bytes);
        bg.mg = mg;
        hipLaunchKernelGGL(k_index_build_adopt, dim3((mg + 255) / 256),
                           dim3(256), 0, s, x, bg);
        LAUNCH_CHECK(k_index_build_adopt);
        if ((rc = launch_stream_cuts(ctx, p, ctx->bl_descs.p)))
            return rc;
        hipLaunchKernelGGL(k_index_build_entries, dim3((mg + 3) / 4),
                           dim3(256), 0, s, x, bg);
        LAUNCH_CHECK(k_index_build_entries);
    }

    // ---- the sequential route: what the list holds by now -----------------
    if (pending && route != 2) {
        const size_t cap = (size_t)(ctx->num_cus > 0 ? ctx->num_cus : 256) * 8;
        hipLaunchKernelGGL(k_index_walk,
                           dim3((uint32_t)(pending < cap ? pending : cap)),
                           dim3(64), 0, s, x);
        LAUNCH_CHECK(k_index_walk);
    }
    return SNAPMI_OK;
}

} // extern "C"
