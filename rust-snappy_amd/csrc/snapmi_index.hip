// snapmi_index.hip -- the block index of raw streams on the host side:
// indexed decode, range reads, and the index of streams that came without one.
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

// Range writes through the block index (bi_write_* of snapmi_blockindex.hpp;
// the kernels: k_write_* in snapmi_decompress.hip).  The write lists are the
// host's: it checks them, lists the touched streams and blocks, cuts the
// touched streams into groups whose compress slots and edge rooms fit
// "write_scratch_bytes", and sends the lists through pinned staging guarded by
// an event.  The groups follow each other on the stream and reuse the slots,
// the rooms and the descriptors.
uint64_t snapmi_write_blocks(const uint32_t *h_write_stream,
                             const uint64_t *h_write_off,
                             const uint64_t *h_write_len, size_t m)
{
    if (!h_write_stream || !h_write_off || !h_write_len)
        return 0;
    BiWriteWalk walk;
    uint64_t blocks = 0;
    for (size_t w = 0; w < m; w++) {
        if (h_write_len[w] == 0)
            continue;
        uint64_t k0;
        const uint64_t c = bi_write_touch(walk, h_write_stream[w],
                                          h_write_off[w], h_write_len[w], &k0);
        blocks = blocks + c < blocks ? ~0ull : blocks + c; // (saturates)
    }
    return blocks;
}

int snapmi_write_ranges_indexed(
    snapmi_ctx *ctx, const void *const *d_in_ptrs, const uint64_t *d_in_lens,
    size_t n, const uint64_t *d_index_first, const uint64_t *d_index,
    uint64_t index_entries, const uint32_t *h_write_stream,
    const uint64_t *h_write_off, const uint64_t *h_write_len,
    const void *const *h_write_src, size_t m, void *const *d_out_ptrs,
    const uint64_t *d_out_caps, uint64_t *d_out_lens, snapmi_error *d_errs,
    uint64_t *d_new_index)
{
    if (!ctx)
        return SNAPMI_E_ARGUMENT;
    if (m == 0)
        return SNAPMI_OK;
    if (!d_in_ptrs || !d_in_lens || !d_index_first || !d_index ||
        !h_write_stream || !h_write_off || !h_write_len || !h_write_src ||
        !d_out_ptrs || !d_out_caps || !d_out_lens || !d_new_index ||
        m > 0x7FFFFFFFu)
        return fail_ctx(ctx, SNAPMI_E_ARGUMENT,
                        "write_ranges_indexed: bad args");
    size_t bad = 0;
    switch (bi_write_check(h_write_stream, h_write_off, h_write_len, m, n,
                           &bad)) {
    case kBiWriteWraps:
        return fail_ctx(ctx, SNAPMI_E_ARGUMENT,
                        "write_ranges_indexed: off + len of write %zu wraps",
                        bad);
    case kBiWriteNoStream:
        return fail_ctx(ctx, SNAPMI_E_ARGUMENT,
                        "write_ranges_indexed: write %zu names stream %u of "
                        "%zu", bad, h_write_stream[bad], n);
    case kBiWriteOrder:
        return fail_ctx(ctx, SNAPMI_E_ARGUMENT,
                        "write_ranges_indexed: write %zu is not behind the "
                        "write in front of it (sorted by stream and offset, "
                        "no overlap)", bad);
    default:
        break;
    }
    for (size_t w = 0; w < m; w++)
        if (h_write_len[w] && !h_write_src[w])
            return fail_ctx(ctx, SNAPMI_E_ARGUMENT,
                            "write_ranges_indexed: write %zu has no source",
                            w);
    const uint64_t TB64 =
        snapmi_write_blocks(h_write_stream, h_write_off, h_write_len, m);
    if (TB64 > 0x7FFFFFFFu ||
        (uint64_t)n + index_entries + TB64 > 0x7FFFFFFFu)
        return fail_ctx(ctx, SNAPMI_E_ARGUMENT,
                        "write_ranges_indexed: n + index_entries + touched "
                        "blocks must stay below 2^31");
    ctx->wr_stats_live = false;
    ctx->wr_blocks = TB64;
    ctx->wr_decoded = 0;
    if (TB64 == 0) // every write is empty
        return SNAPMI_OK;

    // ---- the lists: non-empty writes, touched streams, touched blocks ------
    const size_t TB = (size_t)TB64;
    std::vector<uint64_t> w_off, w_len, w_src, tb_k(TB);
    std::vector<uint32_t> ts_stream, ts_w0, ts_b0, tb_w(TB), tb_room(TB),
        tb_ts(TB);
    std::vector<uint8_t> tb_edge(TB);
    {
        BiWriteWalk walk;
        size_t b = 0;
        for (size_t w = 0; w < m; w++) {
            if (h_write_len[w] == 0)
                continue;
            const uint32_t s = h_write_stream[w];
            if (ts_stream.empty() || ts_stream.back() != s) {
                ts_stream.push_back(s);
                ts_w0.push_back((uint32_t)w_off.size());
                ts_b0.push_back((uint32_t)b);
            }
            uint64_t k0;
            const uint64_t c =
                bi_write_touch(walk, s, h_write_off[w], h_write_len[w], &k0);
            for (uint64_t k = k0; k < k0 + c; k++, b++) {
                tb_k[b] = k;
                tb_w[b] = (uint32_t)w_off.size();
                tb_ts[b] = (uint32_t)(ts_stream.size() - 1);
                tb_edge[b] = bi_write_edge(h_write_off[w], h_write_len[w], k);
            }
            w_off.push_back(h_write_off[w]);
            w_len.push_back(h_write_len[w]);
            w_src.push_back((uint64_t)(uintptr_t)h_write_src[w]);
        }
        ts_w0.push_back((uint32_t)w_off.size());
        ts_b0.push_back((uint32_t)b);
    }
    const size_t W = w_off.size(), TS = ts_stream.size();

    // ---- the groups: whole touched streams whose slots and rooms fit -------
    struct Group {
        uint32_t t0, tg, b0, bg, rooms;
    };
    std::vector<Group> groups;
    size_t max_tg = 0, max_bg = 0, max_rooms = 0;
    {
        Group g{0, 0, 0, 0, 0};
        uint64_t bytes = 0;
        for (size_t t = 0; t < TS; t++) {
            uint32_t rooms = 0;
            for (uint32_t b = ts_b0[t]; b < ts_b0[t + 1]; b++)
                rooms += tb_edge[b];
            const uint32_t nt = ts_b0[t + 1] - ts_b0[t];
            const uint64_t need =
                (uint64_t)nt * kSlotBytes + (uint64_t)rooms * kBiBlock;
            if (g.tg && bytes + need > ctx->write_scratch_bytes) {
                groups.push_back(g);
                g = Group{(uint32_t)t, 0, ts_b0[t], 0, 0};
                bytes = 0;
            }
            // (the rooms of a group are numbered from 0)
            uint32_t r = g.rooms;
            for (uint32_t b = ts_b0[t]; b < ts_b0[t + 1]; b++)
                tb_room[b] = tb_edge[b] ? r++ : 0xFFFFFFFFu;
            g.tg++;
            g.bg += nt;
            g.rooms += rooms;
            bytes += need;
            ctx->wr_decoded += rooms;
        }
        groups.push_back(g);
        for (const Group &q : groups) {
            max_tg = q.tg > max_tg ? q.tg : max_tg;
            max_bg = q.bg > max_bg ? q.bg : max_bg;
            max_rooms = q.rooms > max_rooms ? q.rooms : max_rooms;
        }
    }

    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    // ---- everything the launches need, before the first of them -----------
    // the lists: w_off w_len w_src [W], tb_k [TB] (u64), then ts_stream [TS],
    // ts_w0 ts_b0 [TS + 1], tb_w tb_room tb_ts [TB] (u32)
    const size_t list_bytes =
        (3 * W + TB) * sizeof(uint64_t) +
        (TS + 2 * (TS + 1) + 3 * TB) * sizeof(uint32_t);
    // the states: st_dlen [TS], jobs_first [max_tg + 1], tb_cum [TB + TS]
    // (u64), st_hdr [TS] (u32), st_state [TS]
    const size_t state_bytes =
        (TS + max_tg + 1 + TB + TS) * sizeof(uint64_t) + TS * 5;
    int rc;
    if ((rc = reserve(ctx, ctx->wr_meta, list_bytes + 64)) ||
        (rc = reserve(ctx, ctx->wr_state, state_bytes + 64)) ||
        (rc = reserve(ctx, ctx->wr_z, max_bg * 4 * sizeof(uint64_t) + 64)) ||
        (rc = reserve(ctx, ctx->wr_slot, max_bg * (size_t)kSlotBytes + 64)) ||
        (rc = reserve(ctx, ctx->wr_room, max_rooms * kBiBlock + 64)) ||
        (rc = reserve(ctx, ctx->wr_desc, piece_offsets(max_rooms).total)) ||
        (rc = reserve(ctx, ctx->wr_stat, 64)) ||
        (rc = reserve(ctx, ctx->order, (max_rooms + 72) * sizeof(uint32_t))))
        return rc;
    if (!ctx->ev_wr)
        HIP_TRY(ctx,
                hipEventCreateWithFlags(&ctx->ev_wr, hipEventDisableTiming));
    // (the staging of an earlier call may still be read by its copy: wait for
    // that copy's event, not for the stream)
    if (ctx->ev_wr_live) {
        HIP_TRY(ctx, hipEventSynchronize(ctx->ev_wr));
        ctx->ev_wr_live = false;
    }
    if ((rc = pin_reserve(ctx, ctx->pin_wr, list_bytes)))
        return rc;

    // ---- the lists, to the device ------------------------------------------
    WriteArgs x;
    {
        uint8_t *h = (uint8_t *)ctx->pin_wr.p;
        const uint8_t *const h0 = h;
        uint8_t *const d0 = (uint8_t *)ctx->wr_meta.p;
        // (copies one list to the staging and names its place on the device)
        auto put = [&](const void *src, size_t bytes) {
            memcpy(h, src, bytes);
            const void *d = d0 + (h - h0);
            h += bytes;
            return d;
        };
        x.w_off = (const uint64_t *)put(w_off.data(), W * 8);
        x.w_len = (const uint64_t *)put(w_len.data(), W * 8);
        x.w_src = (const uint64_t *)put(w_src.data(), W * 8);
        x.tb_k = (const uint64_t *)put(tb_k.data(), TB * 8);
        x.ts_stream = (const uint32_t *)put(ts_stream.data(), TS * 4);
        x.ts_w0 = (const uint32_t *)put(ts_w0.data(), (TS + 1) * 4);
        x.ts_b0 = (const uint32_t *)put(ts_b0.data(), (TS + 1) * 4);
        x.tb_w = (const uint32_t *)put(tb_w.data(), TB * 4);
        x.tb_room = (const uint32_t *)put(tb_room.data(), TB * 4);
        x.tb_ts = (const uint32_t *)put(tb_ts.data(), TB * 4);
    }
    HIP_TRY(ctx, hipMemcpyAsync(ctx->wr_meta.p, ctx->pin_wr.p, list_bytes,
                                hipMemcpyHostToDevice, s));
    HIP_TRY(ctx, hipEventRecord(ctx->ev_wr, s));
    ctx->ev_wr_live = true;
    HIP_TRY(ctx, hipMemsetAsync(ctx->wr_stat.p, 0, 64, s));
    ctx->wr_stats_live = true;

    x.in_ptrs = d_in_ptrs;
    x.in_lens = d_in_lens;
    x.first = d_index_first;
    x.index = d_index;
    x.entries = index_entries;
    x.n = (uint32_t)n;
    x.out_ptrs = d_out_ptrs;
    x.out_caps = d_out_caps;
    x.out_lens = d_out_lens;
    x.errs = d_errs;
    x.new_index = d_new_index;
    x.ts = (uint32_t)TS;
    x.st_dlen = (uint64_t *)ctx->wr_state.p;
    x.jobs_first = x.st_dlen + TS;
    x.tb_cum = x.jobs_first + max_tg + 1;
    x.st_hdr = (uint32_t *)(x.tb_cum + TB + TS);
    x.st_state = (uint8_t *)(x.st_hdr + TS);
    x.z_in = (const void **)ctx->wr_z.p;
    x.z_inlen = (uint64_t *)ctx->wr_z.p + max_bg;
    x.z_out = (void **)ctx->wr_z.p + 2 * max_bg;
    x.z_outlen = (uint64_t *)ctx->wr_z.p + 3 * max_bg;
    x.slot = (uint8_t *)ctx->wr_slot.p;
    x.room = (uint8_t *)ctx->wr_room.p;
    x.stat = (unsigned long long *)ctx->wr_stat.p;
    x.t0 = x.tg = x.b0 = x.bg = x.rooms = 0;
    x.c_in = nullptr;
    x.c_inlen = x.c_cap = x.c_outlen = nullptr;
    x.c_out = nullptr;
    x.c_err = nullptr;
    x.c_mode = nullptr;
    hipLaunchKernelGGL(k_write_init, dim3((uint32_t)((n + 255) / 256)),
                       dim3(256), 0, s, x);
    LAUNCH_CHECK(k_write_init);
    // the splice's grid: the host does not know the jobs, only that there is
    // at most one per index entry
    const uint64_t cus = ctx->num_cus > 0 ? ctx->num_cus : 256;
    const uint64_t by_entries = (index_entries + 3) / 4;
    const uint32_t splice_grid = (uint32_t)(
        by_entries < cus * 8 ? (by_entries ? by_entries : 1) : cus * 8);
    for (const Group &q : groups) {
        const PieceList l = piece_list(ctx->wr_desc.p, q.rooms);
        x.t0 = q.t0;
        x.tg = q.tg;
        x.b0 = q.b0;
        x.bg = q.bg;
        x.rooms = q.rooms;
        x.c_in = l.c_in;
        x.c_inlen = l.c_inlen;
        x.c_out = l.c_out;
        x.c_cap = l.c_cap;
        x.c_outlen = l.c_outlen;
        x.c_err = l.c_err;
        x.c_mode = l.c_mode;
        hipLaunchKernelGGL(k_write_plan, dim3((q.tg + 3) / 4), dim3(256), 0,
                           s, x);
        LAUNCH_CHECK(k_write_plan);
        hipLaunchKernelGGL(k_write_blocks, dim3((q.bg + 255) / 256), dim3(256),
                           0, s, x);
        LAUNCH_CHECK(k_write_blocks);
        if (q.rooms) {
            if ((rc = launch_pieces(ctx, l, q.rooms)))
                return rc;
            hipLaunchKernelGGL(k_write_patch, dim3((q.bg + 3) / 4), dim3(256),
                               0, s, x);
            LAUNCH_CHECK(k_write_patch);
        }
        // the touched blocks as one-block raw streams into their slots (as the
        // frame layer compresses its chunks: device lengths, no caps, no
        // errors - a slot holds whatever a block compresses to)
        if ((rc = launch_compress(ctx, x.z_in, x.z_inlen, x.z_out, nullptr,
                                  x.z_outlen, nullptr, q.bg, q.bg, 0)))
            return rc;
        hipLaunchKernelGGL(k_write_sizes, dim3(q.tg), dim3(256), 0, s, x);
        LAUNCH_CHECK(k_write_sizes);
        hipLaunchKernelGGL(k_write_jobs, dim3(1), dim3(1024), 0, s, x);
        LAUNCH_CHECK(k_write_jobs);
        hipLaunchKernelGGL(k_write_splice, dim3(splice_grid), dim3(256), 0, s,
                           x);
        LAUNCH_CHECK(k_write_splice);
    }
    if (index_entries) {
        hipLaunchKernelGGL(k_write_index,
                           dim3((uint32_t)((index_entries + 255) / 256)),
                           dim3(256), 0, s, x);
        LAUNCH_CHECK(k_write_index);
    }
    return SNAPMI_OK;
}

// Appends through the block index (bi_append_* of snapmi_blockindex.hpp; the
// kernels: k_append_* in snapmi_decompress.hip).  The append lists are the
// host's: it checks them, lays out the new index, lists the named streams and
// their new blocks, cuts the named streams into groups whose compress slots
// and tail rooms fit "write_scratch_bytes", and sends the lists through pinned
// staging guarded by an event.  The groups follow each other on the stream
// and reuse the slots, the rooms and the descriptors (those of the writes).
int snapmi_append_indexed(
    snapmi_ctx *ctx, const void *const *d_in_ptrs, const uint64_t *d_in_lens,
    const uint64_t *h_out_lens, size_t n, const uint64_t *d_index_first,
    const uint64_t *d_index, uint64_t index_entries,
    const void *const *h_app_src, const uint64_t *h_app_len,
    void *const *d_out_ptrs, const uint64_t *d_out_caps, uint64_t *d_out_lens,
    snapmi_error *d_errs, uint64_t *d_new_index_first, uint64_t *d_new_index,
    uint64_t new_index_cap)
{
    if (!ctx)
        return SNAPMI_E_ARGUMENT;
    if (n == 0)
        return SNAPMI_OK;
    if (!d_in_ptrs || !d_in_lens || !h_out_lens || !d_index_first ||
        !d_index || !h_app_src || !h_app_len || !d_out_ptrs || !d_out_caps ||
        !d_out_lens || !d_new_index_first || !d_new_index)
        return fail_ctx(ctx, SNAPMI_E_ARGUMENT, "append_indexed: bad args");
    size_t bad = 0;
    uint64_t NE = 0, TB64 = 0;
    switch (bi_append_check(h_out_lens, h_app_len, n, index_entries, &NE,
                            &TB64, &bad)) {
    case kBiAppendWraps:
        return fail_ctx(ctx, SNAPMI_E_ARGUMENT,
                        "append_indexed: the length of stream %zu and what "
                        "is appended to it wrap", bad);
    case kBiAppendTooMany:
        return fail_ctx(ctx, SNAPMI_E_ARGUMENT,
                        "append_indexed: n + index_entries + new entries + "
                        "new blocks must stay below 2^31");
    default:
        break;
    }
    if (NE > new_index_cap)
        return fail_ctx(ctx, SNAPMI_E_ARGUMENT,
                        "append_indexed: the new index takes %llu entries, "
                        "new_index_cap is %llu", (unsigned long long)NE,
                        (unsigned long long)new_index_cap);
    for (size_t i = 0; i < n; i++)
        if (h_app_len[i] && !h_app_src[i])
            return fail_ctx(ctx, SNAPMI_E_ARGUMENT,
                            "append_indexed: stream %zu has no source", i);

    // ---- the lists: named streams and their new blocks ---------------------
    const size_t TB = (size_t)TB64;
    std::vector<uint64_t> nf(n + 1), ns_dlen, ns_add, ns_src;
    std::vector<uint32_t> ns_stream, ns_b0, ns_room, nb_ns(TB);
    nf[0] = 0;
    {
        size_t b = 0;
        for (size_t i = 0; i < n; i++) {
            nf[i + 1] = nf[i] + bi_append_entries(h_out_lens[i], h_app_len[i]);
            if (h_app_len[i] == 0)
                continue;
            ns_stream.push_back((uint32_t)i);
            ns_dlen.push_back(h_out_lens[i]);
            ns_add.push_back(h_app_len[i]);
            ns_src.push_back((uint64_t)(uintptr_t)h_app_src[i]);
            ns_b0.push_back((uint32_t)b);
            const uint64_t c = bi_append_blocks(h_out_lens[i], h_app_len[i]);
            for (uint64_t j = 0; j < c; j++)
                nb_ns[b++] = (uint32_t)(ns_stream.size() - 1);
        }
        ns_b0.push_back((uint32_t)b);
    }
    const size_t NS = ns_stream.size();
    ns_room.assign(NS, 0xFFFFFFFFu);

    // ---- the groups: whole named streams whose slots and rooms fit ---------
    struct Group {
        uint32_t t0, tg, b0, bg, rooms;
    };
    std::vector<Group> groups;
    size_t max_tg = 0, max_bg = 0, max_rooms = 0;
    ctx->ap_stats_live = false;
    ctx->ap_blocks = TB64;
    ctx->ap_decoded = 0;
    if (NS) {
        Group g{0, 0, 0, 0, 0};
        uint64_t bytes = 0;
        for (size_t t = 0; t < NS; t++) {
            const uint32_t nt = ns_b0[t + 1] - ns_b0[t];
            const uint32_t tail = bi_append_tail(ns_dlen[t]) ? 1 : 0;
            const uint64_t need =
                (uint64_t)nt * kSlotBytes + (uint64_t)tail * kBiBlock;
            if (g.tg && bytes + need > ctx->write_scratch_bytes) {
                groups.push_back(g);
                g = Group{(uint32_t)t, 0, ns_b0[t], 0, 0};
                bytes = 0;
            }
            // (the rooms of a group are numbered from 0)
            if (tail)
                ns_room[t] = g.rooms;
            g.tg++;
            g.bg += nt;
            g.rooms += tail;
            bytes += need;
            ctx->ap_decoded += tail;
        }
        groups.push_back(g);
        for (const Group &q : groups) {
            max_tg = q.tg > max_tg ? q.tg : max_tg;
            max_bg = q.bg > max_bg ? q.bg : max_bg;
            max_rooms = q.rooms > max_rooms ? q.rooms : max_rooms;
        }
    }

    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    // ---- everything the launches need, before the first of them -----------
    // the lists: nf [n + 1], ns_dlen ns_add ns_src [NS] (u64), then ns_stream
    // [NS], ns_b0 [NS + 1], ns_room [NS], nb_ns [TB] (u32)
    const size_t list_bytes = (n + 1 + 3 * NS) * sizeof(uint64_t) +
                              (3 * NS + 1 + TB) * sizeof(uint32_t);
    // the states: jobs_first [max_tg + 1], nb_cum [TB + NS] (u64), st_hdr
    // [NS] (u32), st_state [NS]
    const size_t state_bytes =
        (max_tg + 1 + TB + NS) * sizeof(uint64_t) + NS * 5;
    int rc;
    if ((rc = reserve(ctx, ctx->ap_meta, list_bytes + 64)) ||
        (rc = reserve(ctx, ctx->ap_state, state_bytes + 64)) ||
        (rc = reserve(ctx, ctx->ap_stat, 64)) ||
        (NS &&
         ((rc = reserve(ctx, ctx->wr_z, max_bg * 4 * sizeof(uint64_t) + 64)) ||
          (rc = reserve(ctx, ctx->wr_slot,
                        max_bg * (size_t)kSlotBytes + 64)) ||
          (rc = reserve(ctx, ctx->wr_room, max_rooms * kBiBlock + 64)) ||
          (rc = reserve(ctx, ctx->wr_desc, piece_offsets(max_rooms).total)) ||
          (rc = reserve(ctx, ctx->order,
                        (max_rooms + 72) * sizeof(uint32_t))))))
        return rc;
    if (!ctx->ev_ap)
        HIP_TRY(ctx,
                hipEventCreateWithFlags(&ctx->ev_ap, hipEventDisableTiming));
    // (the staging of an earlier call may still be read by its copy: wait for
    // that copy's event, not for the stream)
    if (ctx->ev_ap_live) {
        HIP_TRY(ctx, hipEventSynchronize(ctx->ev_ap));
        ctx->ev_ap_live = false;
    }
    if ((rc = pin_reserve(ctx, ctx->pin_ap, list_bytes)))
        return rc;

    // ---- the lists, to the device ------------------------------------------
    AppendArgs x;
    {
        uint8_t *h = (uint8_t *)ctx->pin_ap.p;
        const uint8_t *const h0 = h;
        uint8_t *const d0 = (uint8_t *)ctx->ap_meta.p;
        // (copies one list to the staging and names its place on the device)
        auto put = [&](const void *src, size_t bytes) {
            if (bytes)
                memcpy(h, src, bytes);
            const void *d = d0 + (h - h0);
            h += bytes;
            return d;
        };
        x.nf = (const uint64_t *)put(nf.data(), (n + 1) * 8);
        x.ns_dlen = (const uint64_t *)put(ns_dlen.data(), NS * 8);
        x.ns_add = (const uint64_t *)put(ns_add.data(), NS * 8);
        x.ns_src = (const uint64_t *)put(ns_src.data(), NS * 8);
        x.ns_stream = (const uint32_t *)put(ns_stream.data(), NS * 4);
        x.ns_b0 = (const uint32_t *)put(ns_b0.data(), (NS + 1) * 4);
        x.ns_room = (const uint32_t *)put(ns_room.data(), NS * 4);
        x.nb_ns = (const uint32_t *)put(nb_ns.data(), TB * 4);
    }
    HIP_TRY(ctx, hipMemcpyAsync(ctx->ap_meta.p, ctx->pin_ap.p, list_bytes,
                                hipMemcpyHostToDevice, s));
    HIP_TRY(ctx, hipEventRecord(ctx->ev_ap, s));
    ctx->ev_ap_live = true;
    HIP_TRY(ctx, hipMemsetAsync(ctx->ap_stat.p, 0, 64, s));
    ctx->ap_stats_live = true;

    x.in_ptrs = d_in_ptrs;
    x.in_lens = d_in_lens;
    x.first = d_index_first;
    x.index = d_index;
    x.entries = index_entries;
    x.n = (uint32_t)n;
    x.out_ptrs = d_out_ptrs;
    x.out_caps = d_out_caps;
    x.out_lens = d_out_lens;
    x.errs = d_errs;
    x.new_first = d_new_index_first;
    x.new_index = d_new_index;
    x.new_entries = NE;
    x.ns = (uint32_t)NS;
    x.jobs_first = (uint64_t *)ctx->ap_state.p;
    x.nb_cum = x.jobs_first + max_tg + 1;
    x.st_hdr = (uint32_t *)(x.nb_cum + TB + NS);
    x.st_state = (uint8_t *)(x.st_hdr + NS);
    x.z_in = (const void **)ctx->wr_z.p;
    x.z_inlen = (uint64_t *)ctx->wr_z.p + max_bg;
    x.z_out = (void **)ctx->wr_z.p + 2 * max_bg;
    x.z_outlen = (uint64_t *)ctx->wr_z.p + 3 * max_bg;
    x.slot = (uint8_t *)ctx->wr_slot.p;
    x.room = (uint8_t *)ctx->wr_room.p;
    x.stat = (unsigned long long *)ctx->ap_stat.p;
    x.t0 = x.tg = x.b0 = x.bg = x.rooms = 0;
    x.c_in = nullptr;
    x.c_inlen = x.c_cap = x.c_outlen = nullptr;
    x.c_out = nullptr;
    x.c_err = nullptr;
    x.c_mode = nullptr;
    hipLaunchKernelGGL(k_append_init, dim3((uint32_t)((n + 255) / 256)),
                       dim3(256), 0, s, x);
    LAUNCH_CHECK(k_append_init);
    // the splice's grid: the host does not know the jobs (the compressed
    // lengths live on the device)
    const uint32_t splice_grid =
        (uint32_t)(ctx->num_cus > 0 ? ctx->num_cus : 256) * 8;
    for (const Group &q : groups) {
        const PieceList l = piece_list(ctx->wr_desc.p, q.rooms);
        x.t0 = q.t0;
        x.tg = q.tg;
        x.b0 = q.b0;
        x.bg = q.bg;
        x.rooms = q.rooms;
        x.c_in = l.c_in;
        x.c_inlen = l.c_inlen;
        x.c_out = l.c_out;
        x.c_cap = l.c_cap;
        x.c_outlen = l.c_outlen;
        x.c_err = l.c_err;
        x.c_mode = l.c_mode;
        hipLaunchKernelGGL(k_append_plan, dim3((q.tg + 3) / 4), dim3(256), 0,
                           s, x);
        LAUNCH_CHECK(k_append_plan);
        hipLaunchKernelGGL(k_append_blocks, dim3((q.bg + 255) / 256),
                           dim3(256), 0, s, x);
        LAUNCH_CHECK(k_append_blocks);
        if (q.rooms) {
            if ((rc = launch_pieces(ctx, l, q.rooms)))
                return rc;
            hipLaunchKernelGGL(k_append_fill, dim3((q.tg + 3) / 4), dim3(256),
                               0, s, x);
            LAUNCH_CHECK(k_append_fill);
        }
        // the new blocks as one-block raw streams into their slots, as the
        // write path compresses its touched blocks
        if ((rc = launch_compress(ctx, x.z_in, x.z_inlen, x.z_out, nullptr,
                                  x.z_outlen, nullptr, q.bg, q.bg, 0)))
            return rc;
        hipLaunchKernelGGL(k_append_sizes, dim3(q.tg), dim3(256), 0, s, x);
        LAUNCH_CHECK(k_append_sizes);
        hipLaunchKernelGGL(k_append_jobs, dim3(1), dim3(1024), 0, s, x);
        LAUNCH_CHECK(k_append_jobs);
        hipLaunchKernelGGL(k_append_splice, dim3(splice_grid), dim3(256), 0,
                           s, x);
        LAUNCH_CHECK(k_append_splice);
    }
    const uint64_t places = NE > n + 1 ? NE : n + 1;
    hipLaunchKernelGGL(k_append_index, dim3((uint32_t)((places + 255) / 256)),
                       dim3(256), 0, s, x);
    LAUNCH_CHECK(k_append_index);
    return SNAPMI_OK;
}

} // extern "C"
