// snapmi_index.hip -- what READS the block index of raw streams, kernels and
// host side: indexed decode (snapmi_decompress_batch_indexed), range reads
// (snapmi_decompress_ranges_indexed) and the index of streams that came
// without one (snapmi_build_block_index); each family of kernels and its
// argument block stand in front of the entry point that launches them.  Last
// in the file, what WRITES the index of a batch as it is compressed
// (snapmi_compress_batch_indexed: launch_block_index, which launch_compress
// calls).  What CHANGES an index - range writes and appends - is
// snapmi_update.hip; the rules of all are snapmi_blockindex.hpp.  The readers
// decode nothing: they cut pieces into a descriptor list (snapmi_piecelist.hpp;
// piece_put, piece_whole of snapmi_device.hpp) which the batch decoder runs over.
#include <hip/hip_runtime.h>

#include <cstring>
#include <vector>

#include "snapmi.h"
#include "snapmi_ctx.hpp"
#include "snapmi_launch.hpp"
#include "snapmi_device.hpp"
#include "snapmi_kernels.hpp"
#include "snapmi_scan.hpp"

using namespace snapmi;

static_assert(kBiBuilt == SNAPMI_INDEX_BUILT &&
                  kBiUnaligned == SNAPMI_INDEX_UNALIGNED &&
                  kBiCorrupt == SNAPMI_INDEX_CORRUPT &&
                  kBiMissized == SNAPMI_INDEX_MISSIZED,
              "snapmi_blockindex.hpp restates the verdicts of snapmi.h");

namespace snapmi {

// ---------------------------------------------------------------------
// snapmi_decompress_batch_indexed: the caller hands the block boundaries in
// (snapmi_blockindex.hpp), so nothing is scanned and the host waits for
// nothing.  ONE descriptor list holds the batch: slot i < n is stream i -
// whole (mode 0) when its entries do not pass the rule, not this launch's
// (mode 3) when they do (k_index_plan) - and slot n + e is index entry e:
// for every entry of an indexed stream but its last a piece in mode 2,
// exactly its room, so a piece writes only its own 64 KiB whatever the
// entries say (k_index_pieces).  One launch of the batch decoder runs over
// all of it, the short streams beside the pieces.  k_index_finish carries
// the results of the whole streams to the caller's arrays and applies
// stream_finish's rule to the indexed ones - every piece is this stream's,
// reports OK and filled its room; a stream that fails it is decoded whole by
// a second, gated launch over the caller's arrays (modes 0 for it, 3 for
// every other stream), which names the error.
// ---------------------------------------------------------------------
// the batch, the caller's index and the one descriptor list
struct IndexArgs {
    const void *const *in_ptrs;
    const uint64_t *in_lens;
    void *const *out_ptrs;
    const uint64_t *out_caps;
    uint64_t *out_lens;
    snapmi_error *errs;    // [n] or nullptr
    const uint64_t *first; // [n + 1]
    const uint64_t *index; // [entries]
    uint64_t entries;
    uint32_t n;
    // [n], of the launch behind the list over the caller's own arrays: 0 =
    // an indexed stream whose pieces did not come out whole, 3 = any other
    uint8_t *modes;
    PieceList c;       // [n + entries]
    uint32_t *c_owner; // [entries] the stream entry e is a piece of
    // [0] = seq once a stream of this call is indexed, [1] streams delivered
    // by pieces, [2] handed back, [3] = seq once one was handed back (what
    // the launch behind waits for)
    unsigned long long *gate;
    unsigned long long seq;
};

__global__ __launch_bounds__(256) void k_index_plan(IndexArgs x)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0) {
        x.gate[1] = 0; // streams delivered by pieces
        x.gate[2] = 0; // ... handed back
    }
    if (i >= x.n)
        return;
    const bool indexed = bi_stream_indexed(
        (const uint8_t *)x.in_ptrs[i], x.in_lens[i], x.out_caps[i], x.index,
        x.first[i], x.first[i + 1], x.entries);
    x.modes[i] = 3; // of the launch behind: k_index_finish says who needs it
    piece_put(x.c, i, x.in_ptrs[i], x.in_lens[i], x.out_ptrs[i],
              x.out_caps[i], indexed ? 3 : 0);
    if (indexed)
        x.gate[0] = x.seq; // (every writer stores the same value)
}

__global__ __launch_bounds__(256) void k_index_pieces(IndexArgs x)
{
    const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= x.entries)
        return;
    // a slot that is no piece: not the launch's (mode 3)
    const void *in = nullptr;
    void *out = nullptr;
    uint64_t in_len = 0, room = 0;
    uint32_t owner = 0xFFFFFFFFu;
    uint8_t mode = 3;
    if (x.gate[0] == x.seq) { // (else no stream is indexed)
        const uint32_t s = bi_find_stream(x.first, x.n, e);
        const uint64_t f0 = x.first[s], f1 = x.first[s + 1];
        // (first[] is the caller's too: the search may land anywhere)
        if (x.c.c_mode[s] == 3 && f0 <= e && e + 1 < f1 && f1 <= x.entries) {
            uint64_t dlen = 0;
            const uint8_t *sin = (const uint8_t *)x.in_ptrs[s];
            if (bi_header(sin, x.in_lens[s], &dlen)) {
                const BiPiece p = bi_piece(x.index + f0, dlen, e - f0);
                in = sin + p.in_off;
                in_len = p.in_len;
                out = (uint8_t *)x.out_ptrs[s] + p.out_off;
                room = p.out_len;
                owner = s;
                mode = 2;
            }
        }
    }
    piece_put(x.c, (uint64_t)x.n + e, in, in_len, out, room, mode);
    x.c_owner[e] = owner;
}

// a wavefront per stream
__global__ __launch_bounds__(256) void k_index_finish(IndexArgs x)
{
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t i = (uint64_t)blockIdx.x * (blockDim.x >> 6) +
                       (threadIdx.x >> 6);
    if (i >= x.n)
        return;
    if (x.c.c_mode[i] != 3) { // decoded whole, as slot i: its results home
        if (lane == 0) {
            x.out_lens[i] = x.c.c_outlen[i];
            if (x.errs)
                x.errs[i] = x.c.c_err[i];
        }
        return;
    }
    const uint64_t f0 = x.first[i], f1 = x.first[i + 1];
    bool bad = false;
    for (uint64_t e = f0 + lane; e + 1 < f1; e += 64)
        if (x.c_owner[e] != (uint32_t)i || !piece_whole(x.c, (uint64_t)x.n + e))
            bad = true;
    const bool any_bad = __ballot(bad) != 0;
    if (lane != 0)
        return;
    if (any_bad) {
        x.modes[i] = 0;    // the launch behind decodes it whole
        x.gate[3] = x.seq; // ... and has something to do
        atomicAdd(&x.gate[2], 1ull);
        return;
    }
    uint64_t dlen = 0;
    bi_header((const uint8_t *)x.in_ptrs[i], x.in_lens[i], &dlen);
    x.out_lens[i] = dlen;
    set_error(x.errs, i, SNAPMI_OK, 0, 0, 0);
    atomicAdd(&x.gate[1], 1ull);
}

} // namespace snapmi

extern "C" {

// The batch with the block index its compressor wrote
// (snapmi_blockindex.hpp; the kernels: k_index_* above).
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
    x.c = piece_list(ctx->ix_desc.p, T);
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
    if ((rc = launch_pieces(ctx, x.c, T)))
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

} // extern "C"

namespace snapmi {

// ---------------------------------------------------------------------
// snapmi_decompress_ranges_indexed: bytes [off, off + len) of a stream's
// output from the pieces of the blocks the range touches, nothing else of the
// stream being read (snapmi_blockindex.hpp has the rules).  The host cuts the
// ranges into consecutive groups whose edge rooms fit the scratch and runs,
// per group: the scan (a) (b) (c) of what the DEVICE arrays ask for - pieces
// and edge rooms per range, so every range knows its slots -, k_range_plan
// (a thread per range: its verdict), k_range_pieces (a thread per piece slot:
// a descriptor in mode 2, straight into the caller's buffer for a block that
// lies wholly inside the range, into a room for an edge block; mode 3 for
// a slot that is nobody's), one launch of the batch decoder over the list,
// and k_range_finish (a wavefront per range: all pieces OK and full, the
// wanted span of the rooms copied out, got and err).  A piece writes exactly
// its room and a room or a block inside the buffer is all it is ever given,
// so nothing outside [r_out[r], + r_len[r]) and the scratch is written
// whatever the index, first[] and the range arrays hold; slots are bounded by
// what the HOST sized (pieces, rooms), which bounds every list and the
// scratch.
// ---------------------------------------------------------------------
// The streams, their index, the ranges, and ONE GROUP (bi_range_groups) of
// consecutive ranges [r0, r0 + mg) whose pieces (host: `pieces`) and edge
// rooms (host: `rooms`) this round of launches runs.  Slot j < pieces of the
// descriptor list is the j-th touched block of the group in range order.
struct RangeArgs {
    const void *const *in_ptrs;
    const uint64_t *in_lens;
    const uint64_t *first; // [n + 1]
    const uint64_t *index; // [entries]
    uint64_t entries;
    uint32_t n;
    const uint32_t *r_stream; // [m], as are the next five
    const uint64_t *r_off;
    const uint64_t *r_len;
    void *const *r_out;
    uint64_t *r_got;
    snapmi_error *r_errs; // or nullptr
    uint32_t r0, mg;
    uint64_t pieces, rooms; // what the host sized for this group
    // [m]: first piece slot and first edge room of the range inside its group
    // (exclusive scans of what the DEVICE arrays ask for), and its verdict:
    // 0 failed or empty (got and err are written), 1 its pieces decide
    uint64_t *slot, *eslot;
    uint8_t *state;
    uint64_t *part; // [2 * parts]: the scans' workgroup totals
    uint8_t *room;  // [rooms * 64 KiB]
    PieceList c;    // [pieces]
    unsigned long long *stat; // [0] ranges that succeeded, [1] that failed
};
// pieces a range may ask for in the scan: more than any call holds
constexpr uint64_t kRangeCountClamp = 1ull << 32;

namespace {
// what range r of the device arrays asks for (the count clamped: the sums of
// m < 2^31 of them cannot wrap)
__device__ __forceinline__ uint64_t range_count(const RangeArgs &x, uint64_t r,
                                                uint64_t *k0, uint32_t *edges)
{
    const uint64_t off = x.r_off[r], len = x.r_len[r];
    const uint64_t cnt = bi_range_blocks(off, len, k0);
    *edges = bi_range_edges(off, len);
    return cnt < kRangeCountClamp ? cnt : kRangeCountClamp;
}

// ... and the slots it is given in the scans: none when it asks for more
// than the whole group was sized for - it fails wherever it stands, and the
// ranges behind it keep their places
__device__ __forceinline__ void range_slots(const RangeArgs &x, uint64_t r,
                                            uint64_t *cnt, uint64_t *edges)
{
    uint64_t k0;
    uint32_t e;
    const uint64_t c = range_count(x, r, &k0, &e);
    const bool fits = c <= x.pieces && e <= x.rooms;
    *cnt = fits ? c : 0;
    *edges = fits ? e : 0;
}

__device__ __forceinline__ void range_fail(const RangeArgs &x, uint64_t r,
                                           int kind, uint64_t a, uint64_t b,
                                           uint64_t c)
{
    x.r_got[r] = 0;
    set_error(x.r_errs, r, kind, a, b, c);
    x.state[r] = 0;
    if (kind != SNAPMI_OK)
        atomicAdd(&x.stat[1], 1ull);
    else
        atomicAdd(&x.stat[0], 1ull);
}
} // namespace

// (the three launches of snapmi_scan.hpp; part: pieces and rooms per
// workgroup, and nobody wants the totals)
__global__ __launch_bounds__(1024) void k_range_scan_a(RangeArgs x)
{
    wg_scan_a<uint64_t, 2>(
        x.mg, x.part,
        [&](uint32_t i, uint64_t (&v)[2]) {
            range_slots(x, (uint64_t)x.r0 + i, &v[0], &v[1]);
        },
        [&](uint32_t i, const uint64_t (&)[2], const uint64_t (&ex)[2]) {
            x.slot[x.r0 + i] = ex[0];
            x.eslot[x.r0 + i] = ex[1];
        });
}

__global__ __launch_bounds__(1024) void k_range_scan_b(RangeArgs x,
                                                       uint32_t nparts)
{
    uint64_t carry[2] = {0, 0};
    wg_scan_b(x.part, nparts, carry);
}

__global__ __launch_bounds__(1024) void k_range_scan_c(RangeArgs x)
{
    wg_scan_c<uint64_t, 2>(x.mg, x.part,
                           [&](uint32_t i, const uint64_t (&off)[2]) {
                               x.slot[x.r0 + i] += off[0];
                               x.eslot[x.r0 + i] += off[1];
                           });
}

// a thread per range: everything that can be said without its pieces
__global__ __launch_bounds__(256) void k_range_plan(RangeArgs x)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= x.mg)
        return;
    const uint64_t r = (uint64_t)x.r0 + i;
    const uint32_t s = x.r_stream[r];
    const uint64_t off = x.r_off[r], len = x.r_len[r];
    if (s >= x.n) {
        range_fail(x, r, SNAPMI_E_ARGUMENT, s, x.n, 0);
        return;
    }
    const uint64_t in_len = x.in_lens[s];
    uint32_t hdr = 0;
    uint64_t dlen = 0;
    // (an empty stream announces nothing, as for snapmi_decompress_len_batch)
    if (in_len != 0) {
        snapmi_error he;
        if (read_header((gcptr)x.in_ptrs[s], in_len, &hdr, &dlen, &he, 0) !=
            SNAPMI_OK) {
            range_fail(x, r, he.kind, he.a, he.b, he.c);
            return;
        }
    }
    if (off + len < off || off + len > dlen) {
        range_fail(x, r, SNAPMI_E_ARGUMENT, off, len, dlen);
        return;
    }
    if (len == 0) {
        range_fail(x, r, SNAPMI_OK, 0, 0, 0); // (nothing to fetch: done)
        return;
    }
    // its slots, inside what the host sized
    uint64_t k0;
    uint32_t edges;
    const uint64_t cnt = range_count(x, r, &k0, &edges);
    if (cnt > x.pieces || edges > x.rooms || x.slot[r] > x.pieces ||
        cnt > x.pieces - x.slot[r] ||
        x.eslot[r] > x.rooms || edges > x.rooms - x.eslot[r]) {
        range_fail(x, r, SNAPMI_E_ARGUMENT, x.slot[r], cnt, x.pieces);
        return;
    }
    if (!bi_range_stream_usable(in_len, hdr, dlen, x.index, x.first[s],
                                x.first[s + 1], x.entries)) {
        range_fail(x, r, SNAPMI_E_ARGUMENT, s, k0, 0);
        return;
    }
    x.state[r] = 1;
}

// a thread per piece slot of the group
__global__ __launch_bounds__(256) void k_range_pieces(RangeArgs x)
{
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= x.pieces)
        return;
    // the range whose slots hold j: the last one of the group that starts at
    // or in front of it (a range without pieces starts where the next does)
    uint32_t lo = 0, hi = x.mg;
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (x.slot[x.r0 + mid] <= j)
            lo = mid;
        else
            hi = mid;
    }
    const uint64_t r = (uint64_t)x.r0 + lo;
    const void *in = nullptr;
    void *out = nullptr;
    uint64_t in_len = 0, room = 0;
    uint8_t mode = 3; // nobody's, or a failed range's: not the launch's
    snapmi_error err;
    err.kind = SNAPMI_OK;
    err.reserved = 0;
    err.a = err.b = err.c = 0;
    if (x.state[r] == 1 && x.slot[r] <= j) {
        const uint64_t off = x.r_off[r], len = x.r_len[r];
        uint64_t k0;
        uint32_t edges;
        const uint64_t cnt = range_count(x, r, &k0, &edges);
        if (j - x.slot[r] < cnt) {
            // (state 1: the stream exists, its header parses, the range lies
            // inside it, its entries inside the index)
            const uint32_t s = x.r_stream[r];
            const uint64_t k = k0 + (j - x.slot[r]);
            const uint8_t *sin = (const uint8_t *)x.in_ptrs[s];
            const uint64_t s_len = x.in_lens[s];
            const uint64_t *e = x.index + x.first[s];
            uint64_t dlen = 0;
            bi_header(sin, s_len, &dlen);
            if (!bi_range_block_usable(e, s_len, k)) {
                err.kind = SNAPMI_E_ARGUMENT;
                err.a = s;
                err.b = k;
            } else {
                const BiPiece p = bi_piece(e, dlen, k);
                in = sin + p.in_off;
                in_len = p.in_len;
                room = p.out_len;
                if (bi_range_edge(off, len, k))
                    out = x.room + (x.eslot[r] +
                                    bi_range_edge_slot(off, len, k)) *
                                       kBiBlock;
                else
                    out = (uint8_t *)x.r_out[r] + (k * kBiBlock - off);
                mode = 2;
            }
        }
    }
    piece_put_err(x.c, j, in, in_len, out, room, mode, err);
}

// a wavefront per range
__global__ __launch_bounds__(256) void k_range_finish(RangeArgs x)
{
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t i = (uint64_t)blockIdx.x * (blockDim.x >> 6) +
                       (threadIdx.x >> 6);
    if (i >= x.mg)
        return;
    const uint64_t r = (uint64_t)x.r0 + i;
    if (x.state[r] != 1) // k_range_plan wrote its got and err
        return;
    const uint64_t off = x.r_off[r], len = x.r_len[r];
    uint64_t k0;
    uint32_t edges;
    const uint64_t cnt = range_count(x, r, &k0, &edges);
    const uint64_t j0 = x.slot[r];
    // the first piece, in block order, that is not OK and full
    uint64_t bad = ~0ull;
    for (uint64_t t = lane; t < cnt && bad == ~0ull; t += 64) {
        const uint64_t j = j0 + t;
        if (!piece_whole(x.c, j))
            bad = j;
    }
    for (uint32_t o = 32; o; o >>= 1) {
        const uint64_t t = __shfl_xor(bad, o);
        bad = t < bad ? t : bad;
    }
    if (bad != ~0ull) {
        if (lane == 0) {
            const snapmi_error e = x.c.c_err[bad];
            x.r_got[r] = 0;
            if (e.kind != SNAPMI_OK)
                set_error(x.r_errs, r, e.kind, e.a, e.b, e.c);
            // not reached, kept as the guard of an invariant: every decoder
            // takes a mode-2 piece's room for the announced length, writes
            // out_lens = room only beside OK and reports HEADER_MISMATCH
            // {room, produced} when the elements end short of it, so a piece
            // that reports OK is full - and a state-1 range's slots are all
            // mode 2 or carry k_range_pieces' own error
            else
                set_error(x.r_errs, r, SNAPMI_E_ARGUMENT,
                          x.r_stream[r], k0 + (bad - j0), 0);
            atomicAdd(&x.stat[1], 1ull);
        }
        return;
    }
    // the wanted span of the edge rooms
    for (uint32_t q = 0; q < 2; q++) {
        const uint64_t k = q == 0 ? k0 : k0 + cnt - 1;
        if ((q == 1 && cnt == 1) || !bi_range_edge(off, len, k))
            continue;
        const BiSpan sp = bi_range_span(off, len, k); // n <= 64 KiB
        wave_copy<false>((gptr)x.r_out[r] + sp.to,
                         (gcptr)x.room +
                             (x.eslot[r] + bi_range_edge_slot(off, len, k)) *
                                 kBiBlock +
                             sp.from,
                         sp.n, lane);
    }
    if (lane == 0) {
        x.r_got[r] = len;
        set_error(x.r_errs, r, SNAPMI_OK, 0, 0, 0);
        atomicAdd(&x.stat[0], 1ull);
    }
}

} // namespace snapmi

extern "C" {

// Range reads through the block index (snapmi_blockindex.hpp; the kernels:
// k_range_* above).  Enqueue-only: the host copies of the ranges size every
// launch and every buffer, and cut the ranges into groups whose edge rooms fit
// "range_scratch_bytes" (bi_range_groups); the groups follow each other on
// the stream and reuse the rooms and the descriptor list.
uint64_t snapmi_range_pieces(const uint64_t *h_range_off,
                             const uint64_t *h_range_len, size_t m)
{
    if (!h_range_off || !h_range_len)
        return 0;
    return bi_range_pieces(h_range_off, h_range_len, m);
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
    std::vector<BiRangeGroup> groups(m);
    BiRangeMax max;
    groups.resize(bi_range_groups(h_range_off, h_range_len, m,
                                  ctx->range_scratch_bytes, groups.data(),
                                  &max));
    const uint64_t max_pieces = max.pieces, max_rooms = max.rooms;
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
    for (const BiRangeGroup &q : groups) {
        const size_t T = (size_t)q.pieces;
        x.r0 = q.r0;
        x.mg = q.mg;
        x.pieces = q.pieces;
        x.rooms = q.rooms;
        x.c = piece_list(ctx->rg_desc.p, T);
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
            if ((rc = launch_pieces(ctx, x.c, T)))
                return rc;
            hipLaunchKernelGGL(k_range_finish, dim3((q.mg + 3) / 4),
                               dim3(256), 0, s, x);
            LAUNCH_CHECK(k_range_finish);
        }
    }
    return SNAPMI_OK;
}

} // extern "C"

namespace snapmi {

// ---------------------------------------------------------------------
// snapmi_build_block_index: bi_build (snapmi_blockindex.hpp) for every stream
// of a batch that came without an index.  The host's copies of the lengths
// size the index, the scratch and every launch; the device checks them and
// trusts them for nothing else.
//   k_index_build_plan     a thread per stream: the caller's length and the
//       header against the host's copies (MISSIZED), the entries of a stream
//       of at most one block; a stream of two blocks and more stays pending
//       (state 0) - or goes straight to the walk list (route 1, or too long
//       for the scan's plan).  The index is all 0 when it runs.
//   per group of pending streams: k_index_build_adopt hands the descriptors
//       the host laid out their input pointers (a stream that is no longer
//       pending gets an empty input: stream_head leaves it alone with
//       meta[2] = 1 and no kernel behind it reads a byte), k_bstream_head ..
//       k_bstream_cuts as for the decoder, and k_index_build_entries (a
//       wavefront per stream) turns cuts[] into entries: BUILT when every
//       interior cut stands exactly on its boundary, UNALIGNED when one
//       stands behind it; a stream the scan gave up on (meta[2] != 0) joins
//       the walk list.
//   k_index_walk           a wavefront per listed stream runs bi_walk.  The
//       list and its count are device memory: the launch reads them, the host
//       never does.
// Every writer of entries writes inside [first[i], first[i + 1]) of its own
// stream, whose count is bi_entries(h_out[i]): what the host sized.
// ---------------------------------------------------------------------
// snapmi_build_block_index (bi_build of snapmi_blockindex.hpp on the device):
// the batch, the device's copies of the host's arrays - which size the index
// and every launch and are trusted for nothing else -, and what the kernels
// hand each other.
struct BuildArgs {
    const void *const *in_ptrs;
    const uint64_t *in_lens; // the caller's
    const uint64_t *h_in;    // [n] copies of h_in_lens, h_out_lens
    const uint64_t *h_out;
    const uint64_t *first;   // [n + 1] the prefix sum the host made
    uint64_t *index;         // [first[n]], all 0 when k_index_build_plan runs
    uint8_t *status;         // [n] or nullptr
    uint32_t n;
    // [n]: 0 = a stream of two blocks and more that awaits its walk (scan or
    // k_index_walk), else its verdict
    uint8_t *state;
    // the streams k_index_walk walks, and the counters: [0..3] streams built,
    // unaligned, corrupt, missized; [4] streams in `walk`
    uint32_t *walk;
    unsigned long long *stat;
    // 0: pending streams are the scan's, those it gives up on the walker's;
    // 1: all pending streams are the walker's; 2: the scan alone, what it
    // gives up on is corrupt (test option "index_build_route")
    uint32_t route;
    // a pending stream longer than this is the walker's under every route
    // (the scan's plan does not hold it)
    uint64_t scan_max_len;
};
// one group of pending streams on the scan route: descriptors [mg] (as
// launch_stream_chain takes them) and the batch's stream of each
struct BuildGroup {
    StreamArgs *descs;
    const uint32_t *idx;
    uint32_t mg;
};

namespace {
__device__ __forceinline__ void build_verdict(const BuildArgs &x, uint32_t i,
                                              int st)
{
    x.state[i] = (uint8_t)st;
    if (x.status)
        x.status[i] = (uint8_t)st;
    atomicAdd(&x.stat[st - 1], 1ull);
}
__device__ __forceinline__ void build_to_walker(const BuildArgs &x, uint32_t i)
{
    // (at most one entry per stream: the list holds n)
    const unsigned long long slot = atomicAdd(&x.stat[4], 1ull);
    x.walk[slot] = i;
}
} // namespace

__global__ __launch_bounds__(256) void k_index_build_plan(BuildArgs x)
{
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= x.n)
        return;
    const uint32_t i = (uint32_t)t;
    const uint64_t in_len = x.h_in[i], dlen = x.h_out[i];
    if (x.in_lens[i] != in_len) {
        build_verdict(x, i, kBiMissized);
        return;
    }
    const uint8_t *in = (const uint8_t *)x.in_ptrs[i];
    uint64_t announced = 0;
    const uint32_t hdr = bi_header(in, in_len, &announced);
    if (hdr && announced != dlen) {
        build_verdict(x, i, kBiMissized);
        return;
    }
    if (dlen > kBiBlock) {
        // (a header that does not parse included: its walk says CORRUPT)
        x.state[i] = 0;
        if (x.route == 2 && in_len > x.scan_max_len)
            build_verdict(x, i, kBiCorrupt); // (no walker under route 2)
        else if (x.route == 1 || in_len > x.scan_max_len)
            build_to_walker(x, i);
        return;
    }
    if (hdr == 0 || (dlen == 0 && in_len != hdr)) {
        build_verdict(x, i, kBiCorrupt);
        return;
    }
    uint64_t *e = x.index + x.first[i];
    e[0] = hdr;
    if (dlen)
        e[1] = in_len;
    build_verdict(x, i, kBiBuilt);
}

__global__ __launch_bounds__(256) void k_index_build_adopt(BuildArgs x,
                                                           BuildGroup g)
{
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= g.mg)
        return;
    const uint32_t i = g.idx[j];
    const bool pending = x.state[i] == 0;
    g.descs[j].in = pending ? (const uint8_t *)x.in_ptrs[i] : nullptr;
    if (!pending)
        g.descs[j].in_len = 0;
}

// a wavefront per stream of the group
__global__ __launch_bounds__(256) void k_index_build_entries(BuildArgs x,
                                                             BuildGroup g)
{
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t j = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (j >= g.mg)
        return;
    const uint32_t i = g.idx[j];
    if (x.state[i] != 0)
        return;
    const StreamArgs &a = g.descs[j];
    if (a.meta[2] != 0) { // the scan gave up
        if (lane == 0) {
            if (x.route == 2)
                build_verdict(x, i, kBiCorrupt);
            else
                build_to_walker(x, i);
        }
        return;
    }
    // (stream_head: meta[1] == h_out[i], meta[3] its blocks)
    const uint64_t K = bi_blocks(x.h_out[i]);
    bool off = false;
    for (uint64_t k = 1 + lane; k < K; k += 64)
        off = off || a.cuts[2 * k + 1] != k * kBiBlock;
    const bool unaligned = __ballot(off) != 0;
    if (!unaligned) {
        uint64_t *e = x.index + x.first[i];
        for (uint64_t k = 1 + lane; k < K; k += 64)
            e[k] = a.cuts[2 * k];
        if (lane == 0) {
            e[0] = a.meta[0];
            e[K] = x.h_in[i];
        }
    }
    if (lane == 0)
        build_verdict(x, i, unaligned ? kBiUnaligned : kBiBuilt);
}

// ---------------------------------------------------------------------
// k_index_walk: bi_walk by one wavefront per listed stream, every lane the
// same walk on wave-uniform values (scalar work; lane 0 stores).  The chain
// is sequential - a hop needs the tag the hop before it led to - so the
// wavefront is as fast as one dependent chain.
// Measured on 256 streams of 1 MiB of text, walker alone (~221 000 hops a
// stream, profiles/raw_index_build_walker.txt): 67.41 ms hopping through
// memory, 67.55 ms with the input staged through 1 KiB windows in LDS (64
// lanes x 16 bytes per refill, ds_read_u8 per hop) - 305 ns a hop either
// way.  What a hop waits for is not its load (neighbouring tags share a cache
// line) but the ~70 dependent scalar instructions and ten branches around it,
// issued by a lone wavefront.  The windows bought nothing and are gone; what
// would is fewer instructions per hop (k_bstream_scan's table of tags) or
// its parallel entries, i.e. the scan route, which takes these streams first.
// ---------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_index_walk(BuildArgs x)
{
    const uint32_t lane = threadIdx.x;
    const uint64_t count = x.stat[4];
    for (uint64_t w = blockIdx.x; w < count; w += gridDim.x) {
        const uint32_t i = x.walk[w];
        const gcptr in = (gcptr)x.in_ptrs[i];
        const uint64_t in_len = x.h_in[i], dlen = x.h_out[i];
        uint64_t *e = x.index + x.first[i];
        const uint64_t cnt = bi_entries(dlen);
        uint64_t announced = 0;
        const uint32_t hdr = uni(
            bi_header((const uint8_t *)x.in_ptrs[i], in_len, &announced));
        int st = kBiCorrupt;
        if (hdr != 0 && announced != dlen)
            st = kBiMissized; // (k_index_build_plan has seen to it)
        else if (hdr != 0)
            st = bi_walk([in](uint64_t pos) { return uni(in[pos]); }, in_len,
                         hdr, dlen, [e, lane](uint64_t k, uint64_t p) {
                             if (lane == 0)
                                 e[k] = p;
                         });
        if (st == kBiBuilt) {
            if (lane == 0) {
                e[0] = hdr;
                e[cnt - 1] = in_len;
            }
        } else {
            // (what the walk put before it knew)
            __syncthreads();
            for (uint64_t k = lane; k < cnt; k += 64)
                e[k] = 0;
        }
        if (lane == 0)
            build_verdict(x, i, st);
    }
}

} // namespace snapmi

extern "C" {

// The block index of streams that came without one (bi_build of
// snapmi_blockindex.hpp; the kernels: k_index_build_*, k_index_walk above).
// The host's copies of the lengths size the index,
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
            // (cuts only: the scan's streams have no ends and no pieces)
            descs[j] = stream_desc(ctx, p, slots[g.j0 + j], nullptr);
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

namespace snapmi {

// ---------------------------------------------------------------------
// The block index of snapmi_compress_batch_indexed (snapmi_blockindex.hpp):
// first[] is the exclusive scan of the streams' entry counts - on one
// workgroup, or as wg_scan_a, _b, _c like the scans above -, and behind
// everything else of the batch one thread per entry reads what the compressor
// already knows: the varint's length, blk_off, the stream's length.
// ---------------------------------------------------------------------
__global__ __launch_bounds__(1024) void k_index_first(const uint64_t *in_lens,
                                                      uint32_t n,
                                                      uint64_t *first)
{
    uint64_t carry[1] = {0};
    wg_scan_strided(
        n, carry,
        [&](uint32_t i, uint64_t (&x)[1]) { x[0] = bi_entries(in_lens[i]); },
        [&](uint32_t i, const uint64_t (&)[1], const uint64_t (&ex)[1]) {
            first[i] = ex[0];
        });
    if (threadIdx.x == 0)
        first[n] = carry[0];
}

__global__ __launch_bounds__(1024) void k_index_first_a(
    const uint64_t *in_lens, uint32_t n, uint64_t *first, uint64_t *part)
{
    wg_scan_a<uint64_t, 1>(
        n, part,
        [&](uint32_t i, uint64_t (&x)[1]) { x[0] = bi_entries(in_lens[i]); },
        [&](uint32_t i, const uint64_t (&)[1], const uint64_t (&ex)[1]) {
            first[i] = ex[0];
        });
}

__global__ __launch_bounds__(1024) void k_index_first_b(uint32_t n,
                                                        uint64_t *first,
                                                        uint64_t *part,
                                                        uint32_t nparts)
{
    uint64_t carry[1] = {0};
    wg_scan_b(part, nparts, carry);
    if (threadIdx.x == 0)
        first[n] = carry[0];
}

__global__ __launch_bounds__(1024) void k_index_first_c(uint32_t n,
                                                        uint64_t *first,
                                                        const uint64_t *part)
{
    wg_scan_c<uint64_t, 1>(
        n, part,
        [&](uint32_t i, const uint64_t (&off)[1]) { first[i] += off[0]; });
}

// Entry j of stream st: the varint's length plus the compressed bytes of the
// stream's blocks in front of block j.  A stream without blocks of its own
// (empty: the one entry {1}; under small_limit: the lane-per-stream kernels')
// has the varint's length and its compressed length; a stream that failed
// (out_lens 0) has zeros.
__global__ __launch_bounds__(256) void k_block_index(CompressArgs a,
                                                     const uint64_t *first,
                                                     uint64_t *index,
                                                     uint64_t entries)
{
    const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= entries || e >= first[a.n_streams])
        return;
    const uint32_t st = bi_find_stream(first, a.n_streams, e);
    const uint64_t j = e - first[st];
    const uint64_t len = a.in_lens[st], out_len = a.out_lens[st];
    const uint64_t last = bi_entries(len) - 1;
    const uint32_t fb = a.blk_first[st];
    const uint32_t nb = a.blk_first[st + 1] - fb;
    uint64_t v = 0;
    if (out_len != 0 && j <= last) {
        const uint32_t vl = varint_len(len);
        if (j == 0)
            v = vl;
        else if (j == last)
            v = out_len;
        // (a middle entry: the stream has last >= 2 blocks, and one that
        // succeeded - out_len != 0 - was given exactly `last` blocks inside
        // the launch by k_plan_compress, which rejects any other; the test
        // is the bound of the read, never the reason for a 0)
        else if (j < nb && (uint64_t)fb + nb <= a.host_blocks)
            v = vl + (a.blk_off[fb + j] - a.blk_off[fb]);
    }
    index[e] = v;
}

// first[], then a thread per entry, behind every scan of the batch: plan_part
// is free again
void launch_block_index(snapmi_ctx *ctx, const CompressArgs &a,
                        uint64_t *d_index_first, uint64_t *d_index,
                        uint64_t index_entries)
{
    hipStream_t s = ctx->stream;
    const uint32_t n = a.n_streams;
    uint64_t *part = (uint64_t *)ctx->plan_part.p;
    launch_scan(
        n,
        [&] {
            hipLaunchKernelGGL(k_index_first, dim3(1), dim3(1024), 0, s,
                               a.in_lens, n, d_index_first);
        },
        [&](uint32_t parts) {
            hipLaunchKernelGGL(k_index_first_a, dim3(parts), dim3(1024), 0, s,
                               a.in_lens, n, d_index_first, part);
            hipLaunchKernelGGL(k_index_first_b, dim3(1), dim3(1024), 0, s, n,
                               d_index_first, part, parts);
            hipLaunchKernelGGL(k_index_first_c, dim3(parts), dim3(1024), 0, s,
                               n, d_index_first, part);
        });
    if (index_entries)
        hipLaunchKernelGGL(k_block_index,
                           dim3((uint32_t)((index_entries + 255) / 256)),
                           dim3(256), 0, s, a, d_index_first, d_index,
                           index_entries);
}

} // namespace snapmi
