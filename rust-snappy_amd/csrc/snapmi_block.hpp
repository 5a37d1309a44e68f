// snapmi_block.hpp -- the block rules of the batch compressor, once: how many
// blocks a launch has, which stream a global block belongs to, where its
// bytes go, when its stream was rejected, how large its hash table is.  Every
// compress kernel asks here.  Plain functions over CompressArgs, no HIP:
// tests/test_block_cpu.py holds them against a linear walk over the streams.
// The layout is k_plan_compress's: stream i owns the global blocks
// blk_first[i] .. blk_first[i + 1] - 1, 64 KiB of its input each, and, for
// its blocks behind the first, the scratch slots from slot_first[i]; a stream
// that does not fit what the host sized (host_blocks, host_slots) is rejected
// (E_ARGUMENT), never overrun.
#ifndef SNAPMI_BLOCK_HPP
#define SNAPMI_BLOCK_HPP

#include <stdint.h>

#include "snapmi_element.hpp"
#include "snapmi_kernels.hpp"
#include "snapmi_tiny.hpp" // SNAPMI_LANE_FN

namespace snapmi {

constexpr uint32_t kMaxBlock = 1u << 16;      // reference src/lib.rs:97
constexpr uint32_t kMaxTable = 1u << 14;      // reference src/compress.rs:11
constexpr uint32_t kInputMargin = 15;         // reference src/compress.rs:20
constexpr uint32_t kMinNonLiteral = 17;       // reference src/compress.rs:24
// (kMaxInput, reference src/lib.rs:93: snapmi_element.hpp)
// max_compress_len(65536) = 76490 (reference src/frame.rs:12), rounded up to
// a multiple of 16 so scratch slots stay 16-byte aligned.
constexpr uint32_t kSlotBytes = 76496;

// max_compress_len, reference src/compress.rs:42-53.
SNAPMI_LANE_FN uint64_t max_compress_len_u64(uint64_t n)
{
    if (n > kMaxInput)
        return 0;
    uint64_t m = 32 + n + n / 6;
    return m > kMaxInput ? 0 : m;
}

SNAPMI_LANE_FN uint32_t varint_len(uint64_t n)
{
    uint32_t k = 1;
    while (n >= 0x80) {
        n >>= 7;
        k++;
    }
    return k;
}

// varint(v) at dst: reference src/compress.rs:128 and src/bytes.rs:61-70
// (P: the caller's kind of byte pointer; varint_len(v) bytes are written)
template <class P> SNAPMI_LANE_FN void put_varint(P dst, uint64_t v)
{
    uint32_t i = 0;
    while (v >= 0x80) {
        dst[i++] = (uint8_t)v | 0x80;
        v >>= 7;
    }
    dst[i] = (uint8_t)v;
}

// blocks of a stream of `total` bytes
SNAPMI_LANE_FN uint64_t stream_blocks(uint64_t total)
{
    return (total + kMaxBlock - 1) / kMaxBlock;
}

// The blocks of a launch: what the plan counted, inside what the host sized
SNAPMI_LANE_FN uint32_t launch_blocks(const CompressArgs &a)
{
    uint32_t nblocks = a.blk_first[a.n_streams];
    if (nblocks > a.host_blocks)
        nblocks = a.host_blocks;
    return nblocks;
}
// ... and inside the segment [blk_lo, blk_hi) of a token-path launch: its end
SNAPMI_LANE_FN uint32_t segment_blocks(const CompressArgs &a)
{
    uint32_t nblocks = launch_blocks(a);
    if (nblocks > a.blk_hi)
        nblocks = a.blk_hi;
    return nblocks;
}

// Global block b: block k of stream st, n of the stream's total bytes, off()
// bytes into its input `in`.
struct BlockAt {
    uint32_t st, k;
    uint64_t total;
    const void *in;
    uint32_t n;
    SNAPMI_LANE_FN uint64_t off() const { return (uint64_t)k * kMaxBlock; }
};
SNAPMI_LANE_FN BlockAt locate_block(const CompressArgs &a, uint32_t b)
{
    // stream lookup: blk_first[st] <= b < blk_first[st + 1]
    uint32_t lo = 0, hi = a.n_streams;
    // (a batch of one-block streams - pages, frame chunks: block b IS
    // stream b, and two loads say so instead of log2(n) dependent ones)
    if (b < a.n_streams && a.blk_first[b] == b && a.blk_first[b + 1] > b) {
        lo = b;
        hi = b + 1;
    }
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (a.blk_first[mid] <= b)
            lo = mid;
        else
            hi = mid;
    }
    BlockAt at;
    at.st = lo;
    at.k = b - a.blk_first[lo];
    at.total = a.in_lens[lo];
    at.in = a.in_ptrs[lo];
    const uint64_t avail = at.total - at.off();
    at.n = avail < kMaxBlock ? (uint32_t)avail : kMaxBlock;
    return at;
}

// A stream of nb blocks from global block `first` / with nb - 1 slots from
// slot `first`: inside what the host sized?  (k_plan_compress rejects a stream
// for which either is false, and whoever writes for the whole stream -
// k_compact, k_stream_lens - asks the same.)
SNAPMI_LANE_FN bool blocks_fit(const CompressArgs &a, uint32_t first,
                               uint64_t nb)
{
    return (uint64_t)first + nb <= a.host_blocks;
}
SNAPMI_LANE_FN bool slots_fit(const CompressArgs &a, uint32_t first,
                              uint64_t nb)
{
    return (uint64_t)first + (nb - 1) <= a.host_slots;
}

// Where the compressed bytes of block b (= at) go, into dst (P: the caller's
// kind of byte pointer).  Block 0 of a stream: the caller's output behind
// varint(total), written here where `header` says so (one lane of the
// wavefront).  A later block: its final position when the sizes of the blocks
// in front are known (a.direct: k_scan_sizes has run; not asked with
// kSlotsOnly, for a kernel of scratch-slot launches only), else a scratch
// slot, from where k_compact moves it.  false: the stream was rejected by
// k_plan_compress (E_ARGUMENT), no destination, nothing written.  (The direct
// rule tests the stream's blocks, as the plan did; the slot rule the block's
// own slot: what of a rejected stream still has a slot is never moved.)
template <bool kSlotsOnly = false, class P>
SNAPMI_LANE_FN bool block_dest(const CompressArgs &a, const BlockAt &at,
                               uint32_t b, bool header, P &dst)
{
    if (at.k == 0) {
        dst = (P)a.out_ptrs[at.st];
        if (header)
            put_varint(dst, at.total);
        dst += varint_len(at.total);
    } else if (!kSlotsOnly && a.direct) {
        const uint32_t first = a.blk_first[at.st];
        if (!blocks_fit(a, first, stream_blocks(at.total)))
            return false;
        dst = (P)a.out_ptrs[at.st] + varint_len(at.total) +
              (a.blk_off[b] - a.blk_off[first]);
    } else {
        const uint32_t slot = a.slot_first[at.st] + at.k - 1;
        if (slot >= a.host_slots)
            return false;
        dst = (P)a.scratch + (uint64_t)slot * kSlotBytes;
    }
    return true;
}

// Hash table of a block of n bytes in a table of at most cap entries: the
// reference's sizing (src/compress.rs:491-518) - 256 entries, doubled while
// below both; a hash is the product's top 32 - shift bits.
struct TableShape {
    uint32_t shift, size;
};
SNAPMI_LANE_FN TableShape table_shift(uint32_t n, uint32_t cap)
{
    TableShape t{32 - 8, 256};
    while (t.size < cap && t.size < n) {
        t.shift--;
        t.size *= 2;
    }
    return t;
}

} // namespace snapmi

#endif
