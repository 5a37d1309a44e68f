// snapmi_update.hip -- updates of indexed raw streams in place of a full
// recompress: range writes (snapmi_write_ranges_indexed) and appends
// (snapmi_append_indexed), kernels and host side.  Only the blocks an update
// changes go through the codec; every other block keeps its compressed bytes
// (snapmi_blockindex.hpp has the rules: bi_write_*, bi_append_*,
// bi_update_groups; what only reads an index is snapmi_index.hip).
//
// Both calls are one pipeline.  The host checks its own arrays, lists the
// NAMED streams - those a write touches, those bytes are appended to - and
// their blocks, cuts the named streams into groups whose compress slots and
// rooms fit "write_scratch_bytes", and sends the lists through pinned staging
// guarded by an event.  Per group, on the stream:
//   plan      a wavefront per named stream: header, the call's own checks of
//             what the stream announces, the index rule over EVERY old block
//   blocks    a thread per block: the block as a one-block stream of the
//             compress launch - from its room or straight from the source -
//             and the piece that is decoded into the room first
//   (the batch decoder over the pieces)
//   patch / fill   the caller's bytes over / behind what was decoded
//   (the batch compressor over the blocks, into their slots)
//   sizes     a workgroup per named stream: its pieces OK and full, the
//             running sum of its blocks, the cap, out_lens, errs, the varint
//   jobs      one workgroup: the first splice job of every named stream
//   splice    the copies, the wavefronts of a fixed grid taking jobs in turn
// and behind the last group one kernel writes the new index.  What the two
// calls share is written once, over UpdateArgs; k_write_* and k_append_* hold
// what differs.
//
// The output of a stream is written by the sizes kernel (the varint) and the
// splice alone, both only for a stream in state 2: new length <= cap is known
// by then, and the jobs' destinations tile [varint, new length).  The lists
// are the host's own; what the device reads of the caller's - in_lens,
// first[], the index - is checked by the plan kernel before anything is
// addressed with it: a stream in state 1 has its entries inside the index and
// e[k] < e[k + 1] <= in_len for every old block.
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

static_assert(kBiSlot == kSlotBytes,
              "snapmi_blockindex.hpp restates the size of a compress slot");

namespace snapmi {

// The caller's arrays, as both calls take them: the streams and their index,
// which the device distrusts, and where the answers go.
struct UpdateBatch {
    const void *const *in_ptrs;
    const uint64_t *in_lens;
    const uint64_t *first; // [n + 1]
    const uint64_t *index; // [entries]
    uint64_t entries;
    uint32_t n;
    void *const *out_ptrs;
    const uint64_t *out_caps;
    uint64_t *out_lens;
    snapmi_error *errs;  // or nullptr
    uint64_t *new_index; // a write: [entries]; an append: [new_entries]
};

// What the kernels of both calls run over: the batch; the lists of the named
// streams, which the HOST built from its own arrays and which are trusted; the
// states the kernels hand each other; and ONE GROUP of consecutive named
// streams [t0, t0 + tg) whose blocks [b0, b0 + bg) have their compress slots,
// and those among them that are decoded first their rooms, in the scratch.
struct UpdateArgs : UpdateBatch {
    // the named streams, ascending: [ts], and [ts + 1] the first block of each
    const uint32_t *ts_stream, *ts_b0;
    uint32_t ts;
    // [ts]: 0 failed (out_lens and errs are written), 1 planned, 2 passed:
    // its bytes are spliced; the bytes of its old header; [tg + 1], of the
    // group: the first splice job of each
    uint8_t *st_state;
    uint32_t *st_hdr;
    uint64_t *jobs_first;
    // [blocks + ts]: block b of named stream t has its running sum - of what
    // the touched blocks in front of it grew (bi_write_entry's tcum), of the
    // sizes of the new blocks in front of it (bi_append_entry's ncum) - at
    // b + t, the stream's total at ts_b0[t + 1] + t
    uint64_t *cum;
    // the group
    uint32_t t0, tg, b0, bg, rooms;
    // [bg]: the one-block streams of the group's compress launch
    const void **z_in;
    uint64_t *z_inlen;
    void **z_out;
    uint64_t *z_outlen;
    uint8_t *slot; // [bg * kSlotBytes]
    uint8_t *room; // [rooms * 64 KiB]
    PieceList c;   // [rooms]
    unsigned long long *stat; // [0] streams that succeeded, [1] that failed
};

// snapmi_write_ranges_indexed: the named streams are the TOUCHED ones.  The
// write lists are the host's: the non-empty writes and the touched blocks of
// the call.
struct WriteArgs : UpdateArgs {
    // the writes: [writes]
    const uint64_t *w_off, *w_len, *w_src;
    const uint32_t *ts_w0; // [ts + 1] the first write of each touched stream
    // the touched blocks: [tb] the block, its first write, its room inside
    // its group (~0: covered) and its touched stream
    const uint64_t *tb_k;
    const uint32_t *tb_w, *tb_room, *tb_ts;
    uint64_t *st_dlen; // [ts] the length the stream's header announces
};

// snapmi_append_indexed: the named streams are those bytes are appended to,
// their blocks the NEW ones.  The lists are laid out by the host's copy of
// what a stream announces: a stream that announces anything else fails
// before the lists are used for it.
struct AppendArgs : UpdateArgs {
    uint64_t *new_first; // [n + 1], the caller's
    uint64_t new_entries;
    const uint64_t *nf; // [n + 1] the prefix sum the host made
    // [ts]: the host's copy of what the stream announces, the bytes appended
    // and their source; its room inside its group (~0: no tail)
    const uint64_t *ns_dlen, *ns_add, *ns_src;
    const uint32_t *ns_room;
    const uint32_t *nb_ns; // [new blocks] the named stream of each
};

// old bytes a splice job of an append copies at most
constexpr uint64_t kAppendCopyBytes = 16384;

namespace {

// ---------------------------------------------------------------------
// the steps both calls take
// ---------------------------------------------------------------------
__device__ __forceinline__ void update_fail(const UpdateArgs &x, uint32_t t,
                                            uint32_t s, int kind, uint64_t a,
                                            uint64_t b, uint64_t c)
{
    x.out_lens[s] = 0;
    set_error(x.errs, s, kind, a, b, c);
    x.st_state[t] = 0;
    atomicAdd(&x.stat[1], 1ull);
}

__device__ __forceinline__ uint64_t wave_min64(uint64_t v)
{
    for (uint32_t o = 32; o; o >>= 1) {
        const uint64_t t = __shfl_xor(v, o);
        v = t < v ? t : v;
    }
    return v;
}

// The plan of named stream t, by its wavefront: the header; own(s, dlen) -
// the call's checks of what the stream announces, which fails the stream and
// returns false, or returns true -; the stream's part of the index rule; the
// block's part over every old block (bi_write_first_bad_block, the lanes
// taking a block each).  A stream that passes is in state 1 and *dlen is what
// it announces; one that does not has its out_lens and errs.  The order of
// the checks is which error a stream that is bad twice reports.
template <class Own>
__device__ __forceinline__ bool update_plan(const UpdateArgs &x, uint32_t t,
                                            uint32_t lane, uint64_t *dlen_out,
                                            Own own)
{
    const uint32_t s = x.ts_stream[t];
    const uint64_t in_len = x.in_lens[s];
    uint32_t hdr = 0;
    uint64_t dlen = 0;
    // (an empty stream announces nothing, as for snapmi_decompress_len_batch)
    if (in_len != 0) {
        snapmi_error he;
        if (read_header((gcptr)x.in_ptrs[s], in_len, &hdr, &dlen, &he, 0) !=
            SNAPMI_OK) {
            if (lane == 0)
                update_fail(x, t, s, he.kind, he.a, he.b, he.c);
            return false;
        }
    }
    if (!own(s, dlen))
        return false;
    const uint64_t f0 = x.first[s], f1 = x.first[s + 1];
    if (!bi_range_stream_usable(in_len, hdr, dlen, x.index, f0, f1,
                                x.entries)) {
        if (lane == 0)
            update_fail(x, t, s, SNAPMI_E_ARGUMENT, s, 0, 0);
        return false;
    }
    const uint64_t *e = x.index + f0;
    const uint64_t blocks = f1 - f0 - 1;
    uint64_t bad = ~0ull;
    for (uint64_t k = lane; k < blocks && bad == ~0ull; k += 64)
        if (!bi_range_block_usable(e, in_len, k))
            bad = k;
    bad = wave_min64(bad);
    if (bad != ~0ull) {
        if (lane == 0)
            update_fail(x, t, s, SNAPMI_E_ARGUMENT, s, bad, 0);
        return false;
    }
    if (lane == 0) {
        x.st_hdr[t] = hdr;
        x.st_state[t] = 1;
    }
    *dlen_out = dlen;
    return true;
}

// Block j of the group as the compress launch and the batch decoder see it.
// As it stands: the block of a failed stream - an empty stream of the compress
// launch, and a piece that is not the decoder's (mode 3).
struct UpdateBlock {
    const void *z_in;      // what the compressor reads: z_len bytes
    uint64_t z_len = 0;
    const void *p_in = nullptr; // the piece that is decoded first, into p_out
    uint64_t p_inlen = 0;
    void *p_out = nullptr;
    uint64_t p_cap = 0;
    uint8_t mode = 3;
};

// ... stored: the one-block stream j and, if the block has a room, piece r
__device__ __forceinline__ void update_store_block(const UpdateArgs &x,
                                                   uint64_t j, uint32_t r,
                                                   uint8_t *slot,
                                                   const UpdateBlock &b)
{
    x.z_in[j] = b.z_in;
    x.z_inlen[j] = b.z_len;
    x.z_out[j] = slot;
    x.z_outlen[j] = 0;
    if (r != 0xFFFFFFFFu)
        piece_put_err(x.c, r, b.p_in, b.p_inlen, b.p_out, b.p_cap, b.mode,
                      snapmi_error{SNAPMI_OK, 0, 0, 0, 0});
}

// The piece of room r did not come out whole (piece_whole): the stream fails
// with the piece's error (k: its block)
__device__ __forceinline__ void update_piece_fail(const UpdateArgs &x,
                                                  uint32_t t, uint32_t s,
                                                  uint32_t r, uint64_t k)
{
    const snapmi_error e = x.c.c_err[r];
    if (e.kind != SNAPMI_OK)
        update_fail(x, t, s, e.kind, e.a, e.b, e.c);
    // not reached, kept as the guard of an invariant (see k_range_finish of
    // snapmi_index.hip): a
    // mode-2 piece that reports OK is full
    else
        update_fail(x, t, s, SNAPMI_E_ARGUMENT, s, k, 0);
}

// The running sum of named stream t's blocks, by its workgroup, blockDim.x
// blocks a stride: term(i, j) is what block i of the stream - stream j of the
// group's compress launch - adds.  Returns the total, in every thread.
template <class Term>
__device__ __forceinline__ uint64_t update_sum(const UpdateArgs &x, uint32_t t,
                                               Term term)
{
    const uint32_t ba = x.ts_b0[t], nt = x.ts_b0[t + 1] - ba;
    uint64_t *cum = x.cum + ba + t;
    uint64_t carry[1] = {0};
    wg_scan_strided(
        nt, carry,
        [&](uint32_t i, uint64_t (&d)[1]) { d[0] = term(i, ba + i - x.b0); },
        [&](uint32_t i, const uint64_t (&)[1], const uint64_t (&ex)[1]) {
            cum[i] = ex[0];
        });
    if (threadIdx.x == 0)
        cum[nt] = carry[0];
    return carry[0];
}

// The last verdict, by one thread: the new stream of new_len bytes, which
// announces `announced`, fits its buffer - then its varint is written and the
// stream is in state 2 - or it fails.
__device__ __forceinline__ void update_commit(const UpdateArgs &x, uint32_t t,
                                              uint32_t s, uint64_t announced,
                                              uint64_t new_len)
{
    const uint64_t cap = x.out_caps[s];
    if (!bi_write_fits(cap, new_len)) {
        update_fail(x, t, s, SNAPMI_BUFFER_TOO_SMALL, cap, new_len, 0);
        return;
    }
    gptr out = (gptr)x.out_ptrs[s];
    const uint32_t hn = varint_len(announced);
    uint64_t v = announced;
    for (uint32_t q = 0; q < hn; q++) {
        out[q] = (uint8_t)((v & 0x7F) | (q + 1 < hn ? 0x80 : 0));
        v >>= 7;
    }
    x.out_lens[s] = new_len;
    set_error(x.errs, s, SNAPMI_OK, 0, 0, 0);
    x.st_state[t] = 2;
    atomicAdd(&x.stat[0], 1ull);
}

// One workgroup: the first splice job of every named stream of the group -
// jobs(t) of them for a stream that passed, none for the others.
template <class Jobs>
__device__ __forceinline__ void update_jobs(const UpdateArgs &x, Jobs jobs)
{
    uint64_t carry[1] = {0};
    wg_scan_strided(
        x.tg, carry,
        [&](uint32_t i, uint64_t (&c)[1]) {
            if (x.st_state[x.t0 + i] == 2)
                c[0] = jobs(x.t0 + i);
        },
        [&](uint32_t i, const uint64_t (&)[1], const uint64_t (&ex)[1]) {
            x.jobs_first[i] = ex[0];
        });
    if (threadIdx.x == 0)
        x.jobs_first[x.tg] = carry[0];
}

// the last stream of the group whose jobs start at or in front of job id (a
// stream without jobs shares its first job with the stream behind it)
__device__ __forceinline__ uint32_t update_job_owner(const UpdateArgs &x,
                                                     uint64_t id)
{
    uint32_t lo = 0, hi = x.tg;
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (x.jobs_first[mid] <= id)
            lo = mid;
        else
            hi = mid;
    }
    return lo;
}

// the named stream batch stream s is, or ~0: nobody names it
__device__ __forceinline__ uint32_t update_named(const UpdateArgs &x,
                                                 uint32_t s)
{
    uint32_t lo = 0, hi = x.ts;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (x.ts_stream[mid] < s)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo < x.ts && x.ts_stream[lo] == s ? lo : 0xFFFFFFFFu;
}

} // namespace

// a thread per stream: "nobody names it" until a later kernel says more
__global__ __launch_bounds__(256) void k_update_init(UpdateArgs x)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= x.n)
        return;
    x.out_lens[i] = 0;
    set_error(x.errs, i, SNAPMI_OK, 0, 0, 0);
}

// ---------------------------------------------------------------------
// snapmi_write_ranges_indexed: bytes [off, off + len) of a stream's output
// replaced.  An EDGE block - one a write cuts - is decoded into its room and
// patched there; a COVERED block is compressed straight from the write that
// covers it.  A splice job per block of a stream that passed: the block's
// bytes - the old ones, or the slot's behind its varint - to the stream's new
// entry k.
// ---------------------------------------------------------------------
// a wavefront per touched stream of the group
__global__ __launch_bounds__(256) void k_write_plan(WriteArgs x)
{
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t i = (uint64_t)blockIdx.x * (blockDim.x >> 6) +
                       (threadIdx.x >> 6);
    if (i >= x.tg)
        return;
    const uint32_t t = x.t0 + (uint32_t)i;
    uint64_t announced;
    const bool ok =
        update_plan(x, t, lane, &announced, [&](uint32_t s, uint64_t dlen) {
            // the first write that passes the stream's end
            uint64_t bad = ~0ull;
            for (uint32_t w = x.ts_w0[t] + lane;
                 w < x.ts_w0[t + 1] && bad == ~0ull; w += 64)
                if (x.w_off[w] + x.w_len[w] > dlen)
                    bad = w;
            bad = wave_min64(bad);
            if (bad != ~0ull && lane == 0)
                update_fail(x, t, s, SNAPMI_E_ARGUMENT, x.w_off[bad],
                            x.w_len[bad], dlen);
            return bad == ~0ull;
        });
    if (ok && lane == 0)
        x.st_dlen[t] = announced;
}

// a thread per touched block of the group
__global__ __launch_bounds__(256) void k_write_blocks(WriteArgs x)
{
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= x.bg)
        return;
    const uint32_t b = x.b0 + (uint32_t)j;
    const uint32_t t = x.tb_ts[b], r = x.tb_room[b];
    uint8_t *const slot = x.slot + j * kSlotBytes;
    UpdateBlock u;
    u.z_in = slot;
    if (x.st_state[t] == 1) {
        // (state 1: every write lies inside dlen, so k < 65 536; the entries
        // lie inside the index and inside the stream)
        const uint32_t s = x.ts_stream[t];
        const uint64_t k = x.tb_k[b];
        const uint64_t rest = x.st_dlen[t] - k * kBiBlock;
        u.z_len = rest < kBiBlock ? rest : kBiBlock;
        if (r != 0xFFFFFFFFu) {
            const uint64_t *e = x.index + x.first[s];
            u.p_in = (const uint8_t *)x.in_ptrs[s] + e[k];
            u.p_inlen = e[k + 1] - e[k];
            u.p_out = x.room + (uint64_t)r * kBiBlock;
            u.p_cap = u.z_len;
            u.mode = 2;
            u.z_in = u.p_out;
        } else {
            const uint32_t w = x.tb_w[b];
            u.z_in = (const uint8_t *)x.w_src[w] + (k * kBiBlock - x.w_off[w]);
        }
    }
    update_store_block(x, j, r, slot, u);
}

// a wavefront per touched block of the group: every write that touches an
// edge block, over its room.  (A room whose piece failed is patched too: its
// stream fails in k_write_sizes and what the block compresses to is dropped.)
__global__ __launch_bounds__(256) void k_write_patch(WriteArgs x)
{
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t j = (uint64_t)blockIdx.x * (blockDim.x >> 6) +
                       (threadIdx.x >> 6);
    if (j >= x.bg)
        return;
    const uint32_t b = x.b0 + (uint32_t)j;
    const uint32_t t = x.tb_ts[b], r = x.tb_room[b];
    if (r == 0xFFFFFFFFu || x.st_state[t] != 1)
        return;
    const uint64_t k = x.tb_k[b];
    const gptr room = (gptr)(x.room + (uint64_t)r * kBiBlock);
    // its first write, and those behind it that start inside the block
    for (uint32_t w = x.tb_w[b]; w < x.ts_w0[t + 1]; w++) {
        const uint64_t off = x.w_off[w], len = x.w_len[w];
        if (off / kBiBlock > k)
            break;
        const BiSpan sp = bi_write_span(off, len, k);
        wave_copy<false>(room + sp.from, (gcptr)x.w_src[w] + sp.to, sp.n,
                         lane);
    }
}

// a workgroup per touched stream of the group
__global__ __launch_bounds__(256) void k_write_sizes(WriteArgs x)
{
    __shared__ uint64_t wave_bad[4];
    const uint32_t t = x.t0 + blockIdx.x;
    if (x.st_state[t] != 1) // k_write_plan wrote its out_lens and errs
        return;
    const uint32_t s = x.ts_stream[t];
    const uint32_t ba = x.ts_b0[t], nt = x.ts_b0[t + 1] - ba;
    // the first piece, in block order, that is not OK and full
    uint64_t bad = ~0ull;
    for (uint32_t i = threadIdx.x; i < nt && bad == ~0ull; i += blockDim.x) {
        const uint32_t r = x.tb_room[ba + i];
        if (r != 0xFFFFFFFFu && !piece_whole(x.c, r))
            bad = i;
    }
    bad = wave_min64(bad);
    if ((threadIdx.x & 63) == 0)
        wave_bad[threadIdx.x >> 6] = bad;
    __syncthreads();
    for (uint32_t w = 0; w < 4; w++)
        bad = wave_bad[w] < bad ? wave_bad[w] : bad;
    if (bad != ~0ull) {
        if (threadIdx.x == 0)
            update_piece_fail(x, t, s, x.tb_room[ba + bad], x.tb_k[ba + bad]);
        return;
    }
    // what the touched blocks grew: new size - old size, modulo 2^64
    const uint64_t *e = x.index + x.first[s];
    const uint64_t grown = update_sum(x, t, [&](uint32_t i, uint32_t j) {
        const uint64_t k = x.tb_k[ba + i];
        return x.z_outlen[j] - varint_len(x.z_inlen[j]) - (e[k + 1] - e[k]);
    });
    if (threadIdx.x != 0)
        return;
    const uint64_t dlen = x.st_dlen[t];
    // (the last old entry is in_len: bi_range_stream_usable)
    update_commit(x, t, s, dlen,
                  x.in_lens[s] + varint_len(dlen) - x.st_hdr[t] + grown);
}

__global__ __launch_bounds__(1024) void k_write_jobs(WriteArgs x)
{
    update_jobs(x, [&](uint32_t t) { return bi_blocks(x.st_dlen[t]); });
}

// (the host does not know how many jobs there are: dlen lives here)
__global__ __launch_bounds__(256) void k_write_splice(WriteArgs x)
{
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t waves = (uint64_t)gridDim.x * (blockDim.x >> 6);
    const uint64_t total = x.jobs_first[x.tg];
    for (uint64_t id = (uint64_t)blockIdx.x * (blockDim.x >> 6) +
                       (threadIdx.x >> 6);
         id < total; id += waves) {
        const uint32_t lo = update_job_owner(x, id);
        const uint32_t t = x.t0 + lo;
        const uint64_t k = id - x.jobs_first[lo];
        const uint32_t s = x.ts_stream[t];
        const uint32_t ba = x.ts_b0[t], nt = x.ts_b0[t + 1] - ba;
        const uint64_t *tk = x.tb_k + ba;
        const uint64_t *e = x.index + x.first[s];
        const uint64_t below = bi_write_below(tk, nt, k);
        const gptr dst = (gptr)x.out_ptrs[s] + e[k] +
                         varint_len(x.st_dlen[t]) - x.st_hdr[t] +
                         x.cum[ba + t + below];
        gcptr src;
        uint64_t len;
        if (below < nt && tk[below] == k) {
            const uint32_t j = ba + (uint32_t)below - x.b0;
            const uint32_t vl = varint_len(x.z_inlen[j]);
            src = (gcptr)(x.slot + (uint64_t)j * kSlotBytes) + vl;
            len = x.z_outlen[j] - vl;
        } else {
            src = (gcptr)x.in_ptrs[s] + e[k];
            len = e[k + 1] - e[k];
        }
        wave_copy<true>(dst, src, len, lane);
    }
}

// a thread per entry: the old entry, moved where a stream that passed owns it
__global__ __launch_bounds__(256) void k_write_index(WriteArgs x)
{
    const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= x.entries)
        return;
    uint64_t v = x.index[e];
    const uint32_t s = bi_find_stream(x.first, x.n, e);
    const uint64_t f0 = x.first[s], f1 = x.first[s + 1];
    if (f0 <= e && e < f1) {
        const uint32_t t = update_named(x, s);
        // (state 2: [f0, f1) lies inside the index, blocks + 1 entries)
        if (t != 0xFFFFFFFFu && x.st_state[t] == 2) {
            const uint32_t ba = x.ts_b0[t], nt = x.ts_b0[t + 1] - ba;
            v = bi_write_entry(x.index + f0, e - f0, x.tb_k + ba,
                               x.cum + ba + t, nt, x.st_hdr[t],
                               varint_len(x.st_dlen[t]));
        }
    }
    x.new_index[e] = v;
}

// ---------------------------------------------------------------------
// snapmi_append_indexed: bytes appended to a stream's output.  The short last
// block - the TAIL - is decoded into its room, the first source bytes are laid
// behind it and the room is the first new block; every further new block is
// compressed straight from the source.  The splice jobs of a stream that
// passed: its old full blocks' bytes in pieces of kAppendCopyBytes, then a job
// per new block.
// ---------------------------------------------------------------------
// a wavefront per named stream of the group
__global__ __launch_bounds__(256) void k_append_plan(AppendArgs x)
{
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t i = (uint64_t)blockIdx.x * (blockDim.x >> 6) +
                       (threadIdx.x >> 6);
    if (i >= x.tg)
        return;
    const uint32_t t = x.t0 + (uint32_t)i;
    uint64_t announced; // (the host's copy of it lays out the lists)
    update_plan(x, t, lane, &announced, [&](uint32_t s, uint64_t dlen) {
        if (dlen != x.ns_dlen[t]) {
            if (lane == 0)
                update_fail(x, t, s, SNAPMI_E_ARGUMENT, s, dlen, x.ns_dlen[t]);
            return false;
        }
        // (dlen <= 2^32 - 1, and dlen + add does not wrap: the host's check)
        if (dlen + x.ns_add[t] > kMaxInput) {
            if (lane == 0)
                update_fail(x, t, s, SNAPMI_TOO_BIG, dlen + x.ns_add[t],
                            kMaxInput, 0);
            return false;
        }
        return true;
    });
}

// a thread per new block of the group
__global__ __launch_bounds__(256) void k_append_blocks(AppendArgs x)
{
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= x.bg)
        return;
    const uint32_t b = x.b0 + (uint32_t)j;
    const uint32_t t = x.nb_ns[b];
    const uint64_t q = b - x.ts_b0[t]; // the block among its stream's new ones
    const uint32_t r = q == 0 ? x.ns_room[t] : 0xFFFFFFFFu;
    uint8_t *const slot = x.slot + j * kSlotBytes;
    UpdateBlock u;
    u.z_in = slot;
    if (x.st_state[t] == 1) {
        // (state 1: the stream announces ns_dlen[t]; its entries lie inside
        // the index and inside the stream)
        const uint32_t s = x.ts_stream[t];
        const uint64_t dlen = x.ns_dlen[t];
        const BiAppendBlock nb = bi_append_block(dlen, x.ns_add[t], q);
        u.z_len = nb.in_len;
        if (nb.room) {
            const uint64_t *e = x.index + x.first[s];
            const uint64_t kf = bi_append_full(dlen);
            u.p_in = (const uint8_t *)x.in_ptrs[s] + e[kf];
            u.p_inlen = e[kf + 1] - e[kf];
            u.p_out = x.room + (uint64_t)r * kBiBlock;
            u.p_cap = bi_append_tail(dlen);
            u.mode = 2;
            u.z_in = u.p_out;
        } else {
            u.z_in = (const uint8_t *)x.ns_src[t] + nb.off;
        }
    }
    update_store_block(x, j, r, slot, u);
}

// a wavefront per named stream of the group: the source bytes that fill the
// tail's room, behind the decoded piece.  (A room whose piece failed is filled
// too: its stream fails in k_append_sizes and what the block compresses to is
// dropped.)
__global__ __launch_bounds__(256) void k_append_fill(AppendArgs x)
{
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t i = (uint64_t)blockIdx.x * (blockDim.x >> 6) +
                       (threadIdx.x >> 6);
    if (i >= x.tg)
        return;
    const uint32_t t = x.t0 + (uint32_t)i;
    const uint32_t r = x.ns_room[t];
    if (r == 0xFFFFFFFFu || x.st_state[t] != 1)
        return;
    const uint64_t dlen = x.ns_dlen[t];
    wave_copy<false>((gptr)(x.room + (uint64_t)r * kBiBlock) +
                         bi_append_tail(dlen),
                     (gcptr)x.ns_src[t], bi_append_fill(dlen, x.ns_add[t]),
                     lane);
}

// a workgroup per named stream of the group
__global__ __launch_bounds__(256) void k_append_sizes(AppendArgs x)
{
    const uint32_t t = x.t0 + blockIdx.x;
    if (x.st_state[t] != 1) // k_append_plan wrote its out_lens and errs
        return;
    const uint32_t s = x.ts_stream[t];
    const uint32_t r = x.ns_room[t];
    const uint64_t dlen = x.ns_dlen[t];
    // the tail's piece
    if (r != 0xFFFFFFFFu && !piece_whole(x.c, r)) {
        if (threadIdx.x == 0)
            update_piece_fail(x, t, s, r, bi_append_full(dlen));
        return;
    }
    // the sizes of the new blocks
    const uint64_t sizes = update_sum(x, t, [&](uint32_t, uint32_t j) {
        return x.z_outlen[j] - varint_len(x.z_inlen[j]);
    });
    if (threadIdx.x != 0)
        return;
    const uint64_t total = dlen + x.ns_add[t];
    const uint64_t *e = x.index + x.first[s];
    // (the old full blocks' bytes are [e[0], e[kf]), e[0] the old header)
    update_commit(x, t, s, total,
                  e[bi_append_full(dlen)] + varint_len(total) - x.st_hdr[t] +
                      sizes);
}

namespace {
// splice jobs that copy the old full blocks' bytes of named stream t (state 2)
__device__ __forceinline__ uint64_t append_copy_jobs(const AppendArgs &x,
                                                     uint32_t t)
{
    const uint64_t *e = x.index + x.first[x.ts_stream[t]];
    const uint64_t bytes = e[bi_append_full(x.ns_dlen[t])] - e[0];
    return (bytes + kAppendCopyBytes - 1) / kAppendCopyBytes;
}
} // namespace

__global__ __launch_bounds__(1024) void k_append_jobs(AppendArgs x)
{
    update_jobs(x, [&](uint32_t t) {
        return append_copy_jobs(x, t) + (x.ts_b0[t + 1] - x.ts_b0[t]);
    });
}

// (the host does not know how many jobs there are: the compressed lengths
// live here)
__global__ __launch_bounds__(256) void k_append_splice(AppendArgs x)
{
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t waves = (uint64_t)gridDim.x * (blockDim.x >> 6);
    const uint64_t total = x.jobs_first[x.tg];
    for (uint64_t id = (uint64_t)blockIdx.x * (blockDim.x >> 6) +
                       (threadIdx.x >> 6);
         id < total; id += waves) {
        const uint32_t lo = update_job_owner(x, id);
        const uint32_t t = x.t0 + lo;
        const uint64_t q = id - x.jobs_first[lo];
        const uint32_t s = x.ts_stream[t];
        const uint64_t *e = x.index + x.first[s];
        const uint64_t dlen = x.ns_dlen[t];
        const uint64_t old_end = e[bi_append_full(dlen)];
        const uint64_t copies = append_copy_jobs(x, t);
        const uint32_t hn = varint_len(dlen + x.ns_add[t]);
        const gptr out = (gptr)x.out_ptrs[s];
        if (q < copies) {
            const uint64_t from = e[0] + q * kAppendCopyBytes;
            const uint64_t len = old_end - from < kAppendCopyBytes
                                     ? old_end - from
                                     : kAppendCopyBytes;
            wave_copy<true>(out + hn + q * kAppendCopyBytes,
                            (gcptr)x.in_ptrs[s] + from, len, lane);
        } else {
            const uint32_t ba = x.ts_b0[t];
            const uint32_t j = ba + (uint32_t)(q - copies) - x.b0;
            const uint32_t vl = varint_len(x.z_inlen[j]);
            wave_copy<true>(out + hn + (old_end - e[0]) +
                                x.cum[ba + t + (q - copies)],
                            (gcptr)(x.slot + (uint64_t)j * kSlotBytes) + vl,
                            x.z_outlen[j] - vl, lane);
        }
    }
}

// a thread per new entry, and per place of the new first[]: the entries of a
// stream that passed by bi_append_entry; the old ones of a stream nobody
// names when first[] gives it just as many inside the index; else 0
__global__ __launch_bounds__(256) void k_append_index(AppendArgs x)
{
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g <= x.n)
        x.new_first[g] = x.nf[g];
    if (g >= x.new_entries)
        return;
    // (nf is the host's prefix sum, nf[0] = 0: s owns g)
    const uint32_t s = bi_find_stream(x.nf, x.n, g);
    const uint64_t k = g - x.nf[s], cnt = x.nf[s + 1] - x.nf[s];
    const uint32_t t = update_named(x, s);
    uint64_t v = 0;
    if (t != 0xFFFFFFFFu) {
        // (state 2: its old entries lie inside the index)
        if (x.st_state[t] == 2) {
            const uint64_t dlen = x.ns_dlen[t];
            v = bi_append_entry(x.index + x.first[s], k, bi_append_full(dlen),
                                x.cum + x.ts_b0[t] + t, x.st_hdr[t],
                                varint_len(dlen + x.ns_add[t]));
        }
    } else {
        const uint64_t f0 = x.first[s], f1 = x.first[s + 1];
        if (f1 <= x.entries && f0 <= f1 && f1 - f0 == cnt)
            v = x.index[f0 + k];
    }
    x.new_index[g] = v;
}

// ---------------------------------------------------------------------
// the host side of both calls
// ---------------------------------------------------------------------
namespace {

// The groups of a call (bi_update_groups) from the first block and the rooms
// of every named stream; room0[t]: the first room of stream t in its group.
struct UpdateGroups {
    std::vector<BiUpdateGroup> groups;
    std::vector<uint32_t> room0;
    BiUpdateMax max;
};

UpdateGroups update_groups(const snapmi_ctx *ctx,
                           const std::vector<uint32_t> &ts_b0,
                           const std::vector<uint32_t> &ts_rooms)
{
    const size_t TS = ts_rooms.size();
    UpdateGroups g;
    g.groups.resize(TS);
    g.room0.resize(TS);
    g.groups.resize(bi_update_groups(ts_b0.data(), ts_rooms.data(), TS,
                                     ctx->write_scratch_bytes,
                                     g.groups.data(), g.room0.data(), &g.max));
    return g;
}

// Everything from the scratch to the last group's splice, for the call whose
// scratch is `u`: x gets the batch, the shared lists and states and, group by
// group, the scratch.  list_bytes: the call's own lists, which lists(put)
// copies - 8-byte lists first - naming their places in x; own_words: 8-byte
// words of state the call keeps per named stream beside the shared ones
// (*own).  The call's kernels run in plan(q) - ahead of the batch decoder -,
// rooms(q) - behind it, when the group has rooms - and finish(q) - behind the
// batch compressor.
template <class Args, class Lists, class Plan, class Rooms, class Finish>
int update_run(snapmi_ctx *ctx, UpdateScratch &u, Args &x,
               const UpdateBatch &batch, const std::vector<uint32_t> &ts_stream,
               const std::vector<uint32_t> &ts_b0, const UpdateGroups &g,
               size_t list_bytes, size_t own_words, uint64_t **own,
               Lists lists, Plan plan, Rooms rooms, Finish finish)
{
    const size_t TS = ts_stream.size(), TB = ts_b0[TS];
    const size_t max_tg = g.max.tg, max_bg = g.max.bg, max_rooms = g.max.rooms;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    // ---- everything the launches need, before the first of them -----------
    // the lists: the call's, then ts_stream [TS], ts_b0 [TS + 1] (u32)
    list_bytes += (2 * TS + 1) * sizeof(uint32_t);
    // the states: the call's own, jobs_first [max_tg + 1], cum [TB + TS]
    // (u64), st_hdr [TS] (u32), st_state [TS]
    const size_t state_bytes =
        (own_words + max_tg + 1 + TB + TS) * sizeof(uint64_t) + TS * 5;
    int rc;
    if ((rc = reserve(ctx, u.meta, list_bytes + 64)) ||
        (rc = reserve(ctx, u.state, state_bytes + 64)) ||
        (rc = reserve(ctx, u.stat, 64)) ||
        (TS &&
         ((rc = reserve(ctx, ctx->up_z, max_bg * 4 * sizeof(uint64_t) + 64)) ||
          (rc = reserve(ctx, ctx->up_slot,
                        max_bg * (size_t)kSlotBytes + 64)) ||
          (rc = reserve(ctx, ctx->up_room, max_rooms * kBiBlock + 64)) ||
          (rc = reserve(ctx, ctx->up_desc, piece_offsets(max_rooms).total)) ||
          (rc = reserve(ctx, ctx->order,
                        (max_rooms + 72) * sizeof(uint32_t))))))
        return rc;
    if (!u.ev)
        HIP_TRY(ctx, hipEventCreateWithFlags(&u.ev, hipEventDisableTiming));
    // (the staging of an earlier call may still be read by its copy: wait for
    // that copy's event, not for the stream)
    if (u.ev_live) {
        HIP_TRY(ctx, hipEventSynchronize(u.ev));
        u.ev_live = false;
    }
    if ((rc = pin_reserve(ctx, u.pin, list_bytes)))
        return rc;

    // ---- the lists, to the device ------------------------------------------
    {
        uint8_t *h = (uint8_t *)u.pin.p;
        const uint8_t *const h0 = h;
        uint8_t *const d0 = (uint8_t *)u.meta.p;
        // (copies one list to the staging and names its place on the device)
        auto put = [&](const void *src, size_t bytes) {
            if (bytes)
                memcpy(h, src, bytes);
            const void *d = d0 + (h - h0);
            h += bytes;
            return d;
        };
        lists(put);
        x.ts_stream = (const uint32_t *)put(ts_stream.data(), TS * 4);
        x.ts_b0 = (const uint32_t *)put(ts_b0.data(), (TS + 1) * 4);
    }
    HIP_TRY(ctx, hipMemcpyAsync(u.meta.p, u.pin.p, list_bytes,
                                hipMemcpyHostToDevice, s));
    HIP_TRY(ctx, hipEventRecord(u.ev, s));
    u.ev_live = true;
    HIP_TRY(ctx, hipMemsetAsync(u.stat.p, 0, 64, s));
    u.stats_live = true;

    static_cast<UpdateBatch &>(x) = batch;
    x.ts = (uint32_t)TS;
    *own = (uint64_t *)u.state.p;
    x.jobs_first = *own + own_words;
    x.cum = x.jobs_first + max_tg + 1;
    x.st_hdr = (uint32_t *)(x.cum + TB + TS);
    x.st_state = (uint8_t *)(x.st_hdr + TS);
    x.z_in = (const void **)ctx->up_z.p;
    x.z_inlen = (uint64_t *)ctx->up_z.p + max_bg;
    x.z_out = (void **)ctx->up_z.p + 2 * max_bg;
    x.z_outlen = (uint64_t *)ctx->up_z.p + 3 * max_bg;
    x.slot = (uint8_t *)ctx->up_slot.p;
    x.room = (uint8_t *)ctx->up_room.p;
    x.stat = (unsigned long long *)u.stat.p;
    x.t0 = x.tg = x.b0 = x.bg = x.rooms = 0;
    x.c = PieceList{};
    hipLaunchKernelGGL(k_update_init, dim3((uint32_t)((x.n + 255) / 256)),
                       dim3(256), 0, s, static_cast<const UpdateArgs &>(x));
    LAUNCH_CHECK(k_update_init);
    for (const BiUpdateGroup &q : g.groups) {
        x.t0 = q.t0;
        x.tg = q.tg;
        x.b0 = q.b0;
        x.bg = q.bg;
        x.rooms = q.rooms;
        x.c = piece_list(ctx->up_desc.p, q.rooms);
        if ((rc = plan(q)))
            return rc;
        if (q.rooms) {
            if ((rc = launch_pieces(ctx, x.c, q.rooms)) || (rc = rooms(q)))
                return rc;
        }
        // the blocks as one-block raw streams into their slots (as the frame
        // layer compresses its chunks: device lengths, no caps, no errors - a
        // slot holds whatever a block compresses to)
        if ((rc = launch_compress(ctx, x.z_in, x.z_inlen, x.z_out, nullptr,
                                  x.z_outlen, nullptr, q.bg, q.bg, 0)) ||
            (rc = finish(q)))
            return rc;
    }
    return SNAPMI_OK;
}

} // namespace
} // namespace snapmi

extern "C" {

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
    ctx->wr.stats_live = false;
    ctx->wr.blocks = TB64;
    ctx->wr.decoded = 0;
    if (TB64 == 0) // every write is empty
        return SNAPMI_OK;

    // ---- the lists: non-empty writes, touched streams, touched blocks ------
    const size_t TB = (size_t)TB64;
    std::vector<uint64_t> w_off, w_len, w_src, tb_k(TB);
    std::vector<uint32_t> ts_stream, ts_w0, ts_b0, ts_rooms, tb_w(TB),
        tb_room(TB), tb_ts(TB);
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
                ts_rooms.push_back(0);
            }
            uint64_t k0;
            const uint64_t c =
                bi_write_touch(walk, s, h_write_off[w], h_write_len[w], &k0);
            for (uint64_t k = k0; k < k0 + c; k++, b++) {
                tb_k[b] = k;
                tb_w[b] = (uint32_t)w_off.size();
                tb_ts[b] = (uint32_t)(ts_stream.size() - 1);
                tb_edge[b] = bi_write_edge(h_write_off[w], h_write_len[w], k);
                ts_rooms.back() += tb_edge[b];
            }
            w_off.push_back(h_write_off[w]);
            w_len.push_back(h_write_len[w]);
            w_src.push_back((uint64_t)(uintptr_t)h_write_src[w]);
        }
        ts_w0.push_back((uint32_t)w_off.size());
        ts_b0.push_back((uint32_t)b);
    }
    const size_t W = w_off.size(), TS = ts_stream.size();

    // ---- the groups; an edge block's room, in block order ------------------
    const UpdateGroups g = update_groups(ctx, ts_b0, ts_rooms);
    for (size_t t = 0; t < TS; t++) {
        uint32_t r = g.room0[t];
        for (uint32_t b = ts_b0[t]; b < ts_b0[t + 1]; b++)
            tb_room[b] = tb_edge[b] ? r++ : 0xFFFFFFFFu;
        ctx->wr.decoded += ts_rooms[t];
    }

    WriteArgs x;
    // w_off w_len w_src [W], tb_k [TB] (u64), then ts_w0 [TS + 1], tb_w
    // tb_room tb_ts [TB] (u32)
    const size_t list_bytes = (3 * W + TB) * sizeof(uint64_t) +
                              (TS + 1 + 3 * TB) * sizeof(uint32_t);
    hipStream_t s = ctx->stream;
    // the splice's grid: the host does not know the jobs, only that there is
    // at most one per index entry
    const uint64_t cus = ctx->num_cus > 0 ? ctx->num_cus : 256;
    const uint64_t by_entries = (index_entries + 3) / 4;
    const uint32_t splice_grid = (uint32_t)(
        by_entries < cus * 8 ? (by_entries ? by_entries : 1) : cus * 8);
    const int rc = update_run(
        ctx, ctx->wr, x,
        UpdateBatch{d_in_ptrs, d_in_lens, d_index_first, d_index,
                    index_entries, (uint32_t)n, d_out_ptrs, d_out_caps,
                    d_out_lens, d_errs, d_new_index},
        ts_stream, ts_b0, g, list_bytes, TS, &x.st_dlen,
        [&](auto put) {
            x.w_off = (const uint64_t *)put(w_off.data(), W * 8);
            x.w_len = (const uint64_t *)put(w_len.data(), W * 8);
            x.w_src = (const uint64_t *)put(w_src.data(), W * 8);
            x.tb_k = (const uint64_t *)put(tb_k.data(), TB * 8);
            x.ts_w0 = (const uint32_t *)put(ts_w0.data(), (TS + 1) * 4);
            x.tb_w = (const uint32_t *)put(tb_w.data(), TB * 4);
            x.tb_room = (const uint32_t *)put(tb_room.data(), TB * 4);
            x.tb_ts = (const uint32_t *)put(tb_ts.data(), TB * 4);
        },
        [&](const BiUpdateGroup &q) -> int {
            hipLaunchKernelGGL(k_write_plan, dim3((q.tg + 3) / 4), dim3(256),
                               0, s, x);
            LAUNCH_CHECK(k_write_plan);
            hipLaunchKernelGGL(k_write_blocks, dim3((q.bg + 255) / 256),
                               dim3(256), 0, s, x);
            LAUNCH_CHECK(k_write_blocks);
            return SNAPMI_OK;
        },
        [&](const BiUpdateGroup &q) -> int {
            hipLaunchKernelGGL(k_write_patch, dim3((q.bg + 3) / 4), dim3(256),
                               0, s, x);
            LAUNCH_CHECK(k_write_patch);
            return SNAPMI_OK;
        },
        [&](const BiUpdateGroup &q) -> int {
            hipLaunchKernelGGL(k_write_sizes, dim3(q.tg), dim3(256), 0, s, x);
            LAUNCH_CHECK(k_write_sizes);
            hipLaunchKernelGGL(k_write_jobs, dim3(1), dim3(1024), 0, s, x);
            LAUNCH_CHECK(k_write_jobs);
            hipLaunchKernelGGL(k_write_splice, dim3(splice_grid), dim3(256),
                               0, s, x);
            LAUNCH_CHECK(k_write_splice);
            return SNAPMI_OK;
        });
    if (rc)
        return rc;
    if (index_entries) {
        hipLaunchKernelGGL(k_write_index,
                           dim3((uint32_t)((index_entries + 255) / 256)),
                           dim3(256), 0, s, x);
        LAUNCH_CHECK(k_write_index);
    }
    return SNAPMI_OK;
}

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
    std::vector<uint32_t> ts_stream, ts_b0, ts_rooms, nb_ns(TB);
    nf[0] = 0;
    {
        size_t b = 0;
        for (size_t i = 0; i < n; i++) {
            nf[i + 1] = nf[i] + bi_append_entries(h_out_lens[i], h_app_len[i]);
            if (h_app_len[i] == 0)
                continue;
            ts_stream.push_back((uint32_t)i);
            ns_dlen.push_back(h_out_lens[i]);
            ns_add.push_back(h_app_len[i]);
            ns_src.push_back((uint64_t)(uintptr_t)h_app_src[i]);
            ts_b0.push_back((uint32_t)b);
            ts_rooms.push_back(bi_append_tail(h_out_lens[i]) ? 1 : 0);
            const uint64_t c = bi_append_blocks(h_out_lens[i], h_app_len[i]);
            for (uint64_t j = 0; j < c; j++)
                nb_ns[b++] = (uint32_t)(ts_stream.size() - 1);
        }
        ts_b0.push_back((uint32_t)b);
    }
    const size_t NS = ts_stream.size();

    // ---- the groups; the tail's room ---------------------------------------
    ctx->ap.stats_live = false;
    ctx->ap.blocks = TB64;
    ctx->ap.decoded = 0;
    const UpdateGroups g = update_groups(ctx, ts_b0, ts_rooms);
    std::vector<uint32_t> ns_room(NS);
    for (size_t t = 0; t < NS; t++) {
        ns_room[t] = ts_rooms[t] ? g.room0[t] : 0xFFFFFFFFu;
        ctx->ap.decoded += ts_rooms[t];
    }

    AppendArgs x;
    x.new_first = d_new_index_first;
    x.new_entries = NE;
    // nf [n + 1], ns_dlen ns_add ns_src [NS] (u64), then ns_room [NS], nb_ns
    // [TB] (u32)
    const size_t list_bytes = (n + 1 + 3 * NS) * sizeof(uint64_t) +
                              (NS + TB) * sizeof(uint32_t);
    hipStream_t s = ctx->stream;
    // the splice's grid: the host does not know the jobs (the compressed
    // lengths live on the device)
    const uint32_t splice_grid =
        (uint32_t)(ctx->num_cus > 0 ? ctx->num_cus : 256) * 8;
    uint64_t *own;
    const int rc = update_run(
        ctx, ctx->ap, x,
        UpdateBatch{d_in_ptrs, d_in_lens, d_index_first, d_index,
                    index_entries, (uint32_t)n, d_out_ptrs, d_out_caps,
                    d_out_lens, d_errs, d_new_index},
        ts_stream, ts_b0, g, list_bytes, 0, &own,
        [&](auto put) {
            x.nf = (const uint64_t *)put(nf.data(), (n + 1) * 8);
            x.ns_dlen = (const uint64_t *)put(ns_dlen.data(), NS * 8);
            x.ns_add = (const uint64_t *)put(ns_add.data(), NS * 8);
            x.ns_src = (const uint64_t *)put(ns_src.data(), NS * 8);
            x.ns_room = (const uint32_t *)put(ns_room.data(), NS * 4);
            x.nb_ns = (const uint32_t *)put(nb_ns.data(), TB * 4);
        },
        [&](const BiUpdateGroup &q) -> int {
            hipLaunchKernelGGL(k_append_plan, dim3((q.tg + 3) / 4), dim3(256),
                               0, s, x);
            LAUNCH_CHECK(k_append_plan);
            hipLaunchKernelGGL(k_append_blocks, dim3((q.bg + 255) / 256),
                               dim3(256), 0, s, x);
            LAUNCH_CHECK(k_append_blocks);
            return SNAPMI_OK;
        },
        [&](const BiUpdateGroup &q) -> int {
            hipLaunchKernelGGL(k_append_fill, dim3((q.tg + 3) / 4), dim3(256),
                               0, s, x);
            LAUNCH_CHECK(k_append_fill);
            return SNAPMI_OK;
        },
        [&](const BiUpdateGroup &q) -> int {
            hipLaunchKernelGGL(k_append_sizes, dim3(q.tg), dim3(256), 0, s, x);
            LAUNCH_CHECK(k_append_sizes);
            hipLaunchKernelGGL(k_append_jobs, dim3(1), dim3(1024), 0, s, x);
            LAUNCH_CHECK(k_append_jobs);
            hipLaunchKernelGGL(k_append_splice, dim3(splice_grid), dim3(256),
                               0, s, x);
            LAUNCH_CHECK(k_append_splice);
            return SNAPMI_OK;
        });
    if (rc)
        return rc;
    // (with nobody named as well: the new first[], and every stream's old
    // entries or 0)
    const uint64_t places = NE > n + 1 ? NE : n + 1;
    hipLaunchKernelGGL(k_append_index, dim3((uint32_t)((places + 255) / 256)),
                       dim3(256), 0, s, x);
    LAUNCH_CHECK(k_append_index);
    return SNAPMI_OK;
}

} // extern "C"
