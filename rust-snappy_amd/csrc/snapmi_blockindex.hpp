// snapmi_blockindex.hpp -- the block index of raw streams
// (snapmi_compress_batch_indexed / snapmi_decompress_batch_indexed), in plain
// C++ that the host code, the kernels and a CPU test
// (tests/blockindex_host.cpp) compile alike:
//
//   bi_entries        entries a stream of `len` input bytes owns
//   bi_stream_indexed whether a compressed stream and the entries it was
//                     given pass the rule (a hint is never trusted: anything
//                     else is an ordinary stream of the batch launch)
//   bi_piece          input and output range of piece k of an indexed stream
//   bi_range_*        the rules of a range read (snapmi_decompress_ranges_indexed),
//                     bi_range_groups how the host cuts a call into groups
//   bi_write_*        the rules of a range write (snapmi_write_ranges_indexed)
//   bi_append_*       the rules of an append (snapmi_append_indexed)
//   bi_update_groups  how both cut their named streams into groups
//   bi_build          the index of a stream that came without one: the
//                     sequential definition of snapmi_build_block_index
//
// Layout: stream i owns index[first[i], first[i + 1]): blocks + 1 entries,
// blocks = ceil(len / 64 KiB); entry j is the offset, inside the stream's
// compressed bytes, of the first element of block j - entry 0 the length of
// the varint header, the last entry the compressed length.
//
// No HIP types, no allocation.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "snapmi_element.hpp" // elem_step

#if defined(__HIPCC__)
#define SNAPMI_BI_HD __host__ __device__
#else
#define SNAPMI_BI_HD
#endif

namespace snapmi {

// input bytes per block of the encoders (kMaxBlock), output bytes per piece
// of the decoder (kStreamChunk)
constexpr uint64_t kBiBlock = 65536;

SNAPMI_BI_HD inline uint64_t bi_blocks(uint64_t len)
{
    return len / kBiBlock + (len % kBiBlock ? 1 : 0);
}

SNAPMI_BI_HD inline uint64_t bi_entries(uint64_t len)
{
    return bi_blocks(len) + 1;
}

// The varint at the head of in[0, in_len): its bytes (0: none that the
// decoders accept - truncated, more than 64 bits, or a length above
// 2^32 - 1) and its value.
SNAPMI_BI_HD inline uint32_t bi_header(const uint8_t *in, uint64_t in_len,
                                       uint64_t *dlen)
{
    uint64_t v = 0;
    for (uint32_t k = 0; k < 10 && k < in_len; k++) {
        const uint8_t b = in[k];
        v |= (uint64_t)(b & 0x7F) << (7 * k);
        if (b < 0x80) {
            if (v > 0xFFFFFFFFull)
                return 0;
            *dlen = v;
            return k + 1;
        }
    }
    return 0;
}

// Is the stream in[0, in_len) with room for `cap` bytes of output, which owns
// index[first, next) of an index of index_entries entries, indexed?  All of:
// at least 3 entries (two blocks) inside the index; entry 0 is the length of
// the varint header; the entries strictly increase; the last one is in_len;
// their count is ceil(dlen / 64 KiB) + 1; dlen <= cap.
SNAPMI_BI_HD inline bool bi_stream_indexed(const uint8_t *in, uint64_t in_len,
                                           uint64_t cap,
                                           const uint64_t *index,
                                           uint64_t first, uint64_t next,
                                           uint64_t index_entries)
{
    if (next > index_entries || first > next || next - first < 3)
        return false;
    const uint64_t count = next - first;
    uint64_t dlen = 0;
    const uint32_t hdr = bi_header(in, in_len, &dlen);
    if (hdr == 0 || dlen > cap || count != bi_entries(dlen))
        return false;
    const uint64_t *e = index + first;
    if (e[0] != hdr || e[count - 1] != in_len)
        return false;
    for (uint64_t j = 1; j < count; j++)
        if (e[j] <= e[j - 1])
            return false;
    return true;
}

// Piece k (k < entries - 1) of an indexed stream of dlen output bytes whose
// entries are e[]: input [in_off, in_off + in_len) into output
// [out_off, out_off + out_len).
struct BiPiece {
    uint64_t in_off, in_len, out_off, out_len;
};

SNAPMI_BI_HD inline BiPiece bi_piece(const uint64_t *e, uint64_t dlen,
                                     uint64_t k)
{
    BiPiece p;
    p.in_off = e[k];
    p.in_len = e[k + 1] - e[k];
    p.out_off = k * kBiBlock;
    const uint64_t end = (k + 1) * kBiBlock < dlen ? (k + 1) * kBiBlock : dlen;
    p.out_len = end - p.out_off;
    return p;
}

// the largest s in [0, n) with first[s] <= e (first[0] <= e is the caller's
// to check): the stream entry e belongs to when first[] is what compress
// wrote.  Whatever first[] holds, the answer is below n; the caller checks
// first[s] <= e < first[s + 1].
SNAPMI_BI_HD inline uint32_t bi_find_stream(const uint64_t *first, uint32_t n,
                                            uint64_t e)
{
    uint32_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (first[mid] <= e)
            lo = mid;
        else
            hi = mid;
    }
    return lo;
}

// ---------------------------------------------------------------------
// Range reads (snapmi_decompress_ranges_indexed): range [off, off + len) of a
// stream's OUTPUT, delivered by the pieces of the blocks it touches.
// ---------------------------------------------------------------------
// Blocks the range touches: *k0 the first, the return value their number - 0
// for an empty range and for one whose end passes 2^64 (which no stream holds:
// the call fails it).
SNAPMI_BI_HD inline uint64_t bi_range_blocks(uint64_t off, uint64_t len,
                                             uint64_t *k0)
{
    *k0 = off / kBiBlock;
    if (len == 0 || off + len < off)
        return 0;
    return (off + len - 1) / kBiBlock - *k0 + 1;
}

// Is touched block k an EDGE block - cut by the range, decoded into a room of
// scratch and copied from there - or does [k * 64 KiB, (k + 1) * 64 KiB) lie
// wholly inside the range, so that its piece decodes straight into the
// caller's buffer?  Told from the range alone (the host sizes the scratch
// without the streams): a stream's short last block is an edge block unless
// the range ends on a multiple of 64 KiB.
SNAPMI_BI_HD inline bool bi_range_edge(uint64_t off, uint64_t len, uint64_t k)
{
    return k * kBiBlock < off || off + len - k * kBiBlock < kBiBlock;
}

// Edge blocks of the range: 0, 1 or 2 (only the first and the last touched
// block can be cut).
SNAPMI_BI_HD inline uint32_t bi_range_edges(uint64_t off, uint64_t len)
{
    uint64_t k0;
    const uint64_t cnt = bi_range_blocks(off, len, &k0);
    if (cnt == 0)
        return 0;
    const uint32_t head = bi_range_edge(off, len, k0) ? 1 : 0;
    if (cnt == 1)
        return head;
    return head + (bi_range_edge(off, len, k0 + cnt - 1) ? 1 : 0);
}

// The room of edge block k among the range's edge rooms: 0 for the first
// touched block, and for the last one 1 when the first is an edge block too.
SNAPMI_BI_HD inline uint32_t bi_range_edge_slot(uint64_t off, uint64_t len,
                                                uint64_t k)
{
    const uint64_t k0 = off / kBiBlock;
    return k != k0 && bi_range_edge(off, len, k0) ? 1 : 0;
}

// The LOCAL index rule of a range read, in two parts.  The stream's part: a
// stream in[0, in_len) whose header (hdr bytes) announces dlen and which owns
// index[first, next) of an index of index_entries entries is usable when its
// entries lie inside the index and number bi_entries(dlen), entry 0 is the
// header's length and the last entry is in_len.  (A one-block stream with its
// 2 entries passes, unlike under bi_stream_indexed.)
SNAPMI_BI_HD inline bool bi_range_stream_usable(uint64_t in_len, uint32_t hdr,
                                                uint64_t dlen,
                                                const uint64_t *index,
                                                uint64_t first, uint64_t next,
                                                uint64_t index_entries)
{
    if (next > index_entries || first > next ||
        next - first != bi_entries(dlen))
        return false;
    return index[first] == hdr && index[next - 1] == in_len;
}

// The block's part, for every touched block k of a usable stream with entries
// e[]: e[k] < e[k + 1] <= in_len.  Blocks the range does not touch are not
// looked at.
SNAPMI_BI_HD inline bool bi_range_block_usable(const uint64_t *e,
                                               uint64_t in_len, uint64_t k)
{
    return e[k] < e[k + 1] && e[k + 1] <= in_len;
}

// The first touched block that fails the block's part, or ~0 when none does.
SNAPMI_BI_HD inline uint64_t bi_range_first_bad_block(const uint64_t *e,
                                                      uint64_t in_len,
                                                      uint64_t off,
                                                      uint64_t len)
{
    uint64_t k0;
    const uint64_t cnt = bi_range_blocks(off, len, &k0);
    for (uint64_t k = k0; k < k0 + cnt; k++)
        if (!bi_range_block_usable(e, in_len, k))
            return k;
    return ~0ull;
}

// What an edge block hands to the caller: bytes [from, from + n) of its room
// go to byte `to` of the range's buffer.
struct BiSpan {
    uint64_t from, to, n;
};

SNAPMI_BI_HD inline BiSpan bi_range_span(uint64_t off, uint64_t len,
                                         uint64_t k)
{
    const uint64_t lo = k * kBiBlock > off ? k * kBiBlock : off;
    // (the block's end may pass 2^64 only where the range's cannot)
    const uint64_t hi = off + len - k * kBiBlock < kBiBlock
                            ? off + len
                            : (k + 1) * kBiBlock;
    BiSpan s;
    s.from = lo - k * kBiBlock;
    s.to = lo - off;
    s.n = hi - lo;
    return s;
}

// Pieces of a call of m ranges, from the host's arrays: the touched blocks of
// all of them (saturates at 2^64 - 1).
SNAPMI_BI_HD inline uint64_t bi_range_pieces(const uint64_t *off,
                                             const uint64_t *len, size_t m)
{
    uint64_t pieces = 0;
    for (size_t r = 0; r < m; r++) {
        uint64_t k0;
        const uint64_t c = bi_range_blocks(off[r], len[r], &k0);
        pieces = pieces + c < pieces ? ~0ull : pieces + c;
    }
    return pieces;
}

// The groups of a range call: the ranges are cut, in order, into groups whose
// edge rooms (64 KiB each) fit `scratch_bytes`; a range has at most two, which
// the floor of the option holds, and a range that alone needs more than the
// scratch is a group of its own.  The groups follow each other on the stream
// and reuse the rooms and the descriptor list.
// ranges [r0, r0 + mg), their pieces and their edge rooms
struct BiRangeGroup {
    uint32_t r0, mg;
    uint64_t pieces, rooms;
};

// the most pieces and rooms any group holds
struct BiRangeMax {
    uint64_t pieces, rooms;
};

// groups[] has m places.  Returns the number of groups (0 for m == 0).
SNAPMI_BI_HD inline size_t bi_range_groups(const uint64_t *off,
                                           const uint64_t *len, size_t m,
                                           uint64_t scratch_bytes,
                                           BiRangeGroup *groups,
                                           BiRangeMax *max)
{
    max->pieces = max->rooms = 0;
    const uint64_t room_cap = scratch_bytes / kBiBlock;
    size_t count = 0;
    for (size_t r = 0; r < m; r++) {
        uint64_t k0;
        const uint64_t c = bi_range_blocks(off[r], len[r], &k0);
        const uint32_t e = bi_range_edges(off[r], len[r]);
        if (count == 0 || groups[count - 1].rooms + e > room_cap)
            groups[count++] = BiRangeGroup{(uint32_t)r, 0, 0, 0};
        BiRangeGroup &g = groups[count - 1];
        g.mg++;
        g.pieces += c;
        g.rooms += e;
        max->pieces = g.pieces > max->pieces ? g.pieces : max->pieces;
        max->rooms = g.rooms > max->rooms ? g.rooms : max->rooms;
    }
    return count;
}

// ---------------------------------------------------------------------
// Range writes (snapmi_write_ranges_indexed): write [off, off + len) replaces
// that part of a stream's OUTPUT.  The blocks the writes touch are decoded
// (when a write cuts them), patched and compressed again; every other block
// keeps its compressed bytes, which move by what the touched blocks in front
// of them grew or shrank.
// ---------------------------------------------------------------------
// What is wrong with the host's write list, or 0.  Writes of len == 0 are not
// looked at.  The others are sorted by (stream, off) and do not overlap;
// stream < n; off + len does not wrap.
constexpr int kBiWriteOk = 0, kBiWriteWraps = 1, kBiWriteNoStream = 2,
              kBiWriteOrder = 3;

SNAPMI_BI_HD inline int bi_write_check(const uint32_t *stream,
                                       const uint64_t *off,
                                       const uint64_t *len, size_t m,
                                       uint64_t n, size_t *bad)
{
    bool any = false;
    uint32_t ps = 0;
    uint64_t pend = 0; // end of the last write looked at
    for (size_t w = 0; w < m; w++) {
        if (len[w] == 0)
            continue;
        *bad = w;
        if (off[w] + len[w] < off[w])
            return kBiWriteWraps;
        if (stream[w] >= n)
            return kBiWriteNoStream;
        if (any && (stream[w] < ps || (stream[w] == ps && off[w] < pend)))
            return kBiWriteOrder;
        any = true;
        ps = stream[w];
        pend = off[w] + len[w];
    }
    return kBiWriteOk;
}

// The touched blocks of a checked write list, write by write: a walk that
// remembers the last block of the write in front, which the next write of the
// same stream may share - a shared block counts once, for the first of them.
struct BiWriteWalk {
    bool any = false;
    uint32_t stream = 0;
    uint64_t last = 0;
};

// Blocks the (non-empty) write adds to the list: *k0 the first, the return
// value their number (0: its only block is the one the write in front ended
// in).
SNAPMI_BI_HD inline uint64_t bi_write_touch(BiWriteWalk &w, uint32_t stream,
                                            uint64_t off, uint64_t len,
                                            uint64_t *k0)
{
    uint64_t k;
    uint64_t c = bi_range_blocks(off, len, &k);
    if (c == 0) {
        *k0 = k;
        return 0;
    }
    const uint64_t last = k + c - 1;
    if (w.any && w.stream == stream && w.last == k) {
        k++;
        c--;
    }
    w.any = true;
    w.stream = stream;
    w.last = last;
    *k0 = k;
    return c;
}

// Is touched block k, whose FIRST write is [off, off + len), an EDGE block -
// decoded into a room, patched there and compressed from there - or COVERED:
// [k * 64 KiB, (k + 1) * 64 KiB) lies inside the write, which is then the
// block's only one, and the block is compressed straight from the write's
// bytes?  Told from the writes alone, as bi_range_edge: a stream's short last
// block is an edge block unless the write ends on a multiple of 64 KiB.  (A
// block that two writes share is cut by both of them.)
SNAPMI_BI_HD inline bool bi_write_edge(uint64_t off, uint64_t len, uint64_t k)
{
    return bi_range_edge(off, len, k);
}

// What a write puts into touched block k: bytes [to, to + n) of its source go
// to byte `from` of the block (bi_range_span with the copy turned round).
SNAPMI_BI_HD inline BiSpan bi_write_span(uint64_t off, uint64_t len,
                                         uint64_t k)
{
    return bi_range_span(off, len, k);
}

// The index rule of a write: bi_range_stream_usable, and the block's part for
// EVERY block of the stream - each one is copied or replaced.  The first
// block that fails it, or ~0.
SNAPMI_BI_HD inline uint64_t bi_write_first_bad_block(const uint64_t *e,
                                                      uint64_t in_len,
                                                      uint64_t blocks)
{
    for (uint64_t k = 0; k < blocks; k++)
        if (!bi_range_block_usable(e, in_len, k))
            return k;
    return ~0ull;
}

// The splice, by definition: the stream's new entries from its old ones e[]
// (blocks + 1 of them), the ascending list tk[nt] of its touched blocks and
// their new compressed sizes tsize[nt] (without a varint); hdr_new is the
// length of varint(dlen).  Returns the new length (the last new entry).
SNAPMI_BI_HD inline uint64_t bi_write_splice(const uint64_t *e,
                                             uint64_t blocks,
                                             const uint64_t *tk,
                                             const uint64_t *tsize,
                                             uint64_t nt, uint32_t hdr_new,
                                             uint64_t *e_new)
{
    uint64_t pos = hdr_new, t = 0;
    for (uint64_t k = 0; k < blocks; k++) {
        e_new[k] = pos;
        if (t < nt && tk[t] == k)
            pos += tsize[t++];
        else
            pos += e[k + 1] - e[k];
    }
    e_new[blocks] = pos;
    return pos;
}

// ... and as the kernels compute it, an entry at a time: a block moves by
// what the touched blocks in front of it changed.  tcum[j] is the sum, over
// the touched blocks tk[0 .. j), of (new size - old size), modulo 2^64;
// tcum[nt] the stream's total.
SNAPMI_BI_HD inline uint64_t bi_write_below(const uint64_t *tk, uint64_t nt,
                                            uint64_t k)
{
    uint64_t lo = 0, hi = nt; // touched blocks below k
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (tk[mid] < k)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}

SNAPMI_BI_HD inline uint64_t bi_write_entry(const uint64_t *e, uint64_t k,
                                            const uint64_t *tk,
                                            const uint64_t *tcum, uint64_t nt,
                                            uint32_t hdr_old, uint32_t hdr_new)
{
    return e[k] + hdr_new - hdr_old + tcum[bi_write_below(tk, nt, k)];
}

// The last verdict: the new stream fits its buffer (an exact cap passes).
SNAPMI_BI_HD inline bool bi_write_fits(uint64_t cap, uint64_t new_len)
{
    return new_len <= cap;
}

// ---------------------------------------------------------------------
// Appends (snapmi_append_indexed): `add` bytes behind the dlen bytes of a
// stream's OUTPUT.  The old FULL blocks [0, kf) keep their compressed bytes;
// a short last block - the TAIL - is decoded into a room, the first source
// bytes are laid behind it and the room is compressed as the first NEW block;
// every further new block is compressed straight from the source.
// ---------------------------------------------------------------------
// Entries the stream owns in the new index, whatever becomes of it.
SNAPMI_BI_HD inline uint64_t bi_append_entries(uint64_t dlen, uint64_t add)
{
    return bi_entries(dlen + add);
}

// kf: the old full blocks, which are copied.
SNAPMI_BI_HD inline uint64_t bi_append_full(uint64_t dlen)
{
    return dlen / kBiBlock;
}

// Bytes of the tail (0: the old length is a multiple of 64 KiB - 0 included -
// and nothing is decoded).
SNAPMI_BI_HD inline uint64_t bi_append_tail(uint64_t dlen)
{
    return dlen % kBiBlock;
}

// Source bytes that fill the tail's room.
SNAPMI_BI_HD inline uint64_t bi_append_fill(uint64_t dlen, uint64_t add)
{
    const uint64_t rem = bi_append_tail(dlen);
    if (rem == 0)
        return 0;
    return add < kBiBlock - rem ? add : kBiBlock - rem;
}

// New blocks of a stream that `add` bytes are appended to (0 for add == 0:
// nobody names the stream).  dlen + add does not wrap: bi_append_check.
SNAPMI_BI_HD inline uint64_t bi_append_blocks(uint64_t dlen, uint64_t add)
{
    return add ? bi_blocks(dlen + add) - bi_append_full(dlen) : 0;
}

// New block j (j < bi_append_blocks): source bytes [off, off + len) go into
// it.  room: it is the tail's block - the bytes are laid at byte in_len - len
// of the room and the compressor reads room[0, in_len); else the compressor
// reads them where they are, in_len == len.
struct BiAppendBlock {
    bool room;
    uint64_t off, len, in_len;
};

SNAPMI_BI_HD inline BiAppendBlock bi_append_block(uint64_t dlen, uint64_t add,
                                                  uint64_t j)
{
    const uint64_t rem = bi_append_tail(dlen);
    const uint64_t fill = bi_append_fill(dlen, add);
    BiAppendBlock b;
    if (rem && j == 0) {
        b.room = true;
        b.off = 0;
        b.len = fill;
        b.in_len = rem + fill;
        return b;
    }
    b.room = false;
    b.off = fill + (rem ? j - 1 : j) * kBiBlock;
    b.len = add - b.off < kBiBlock ? add - b.off : kBiBlock;
    b.in_len = b.len;
    return b;
}

// What is wrong with the host's lists, or 0: h_out_lens[i] + h_app_len[i]
// wraps (*bad: the stream), or n + index_entries + new entries + new blocks
// is not below 2^31.  *entries: the new index's total; *blocks: the new
// blocks of the call (both saturate at 2^64 - 1).
constexpr int kBiAppendOk = 0, kBiAppendWraps = 1, kBiAppendTooMany = 2;

SNAPMI_BI_HD inline int bi_append_check(const uint64_t *out_lens,
                                        const uint64_t *app_len, size_t n,
                                        uint64_t index_entries,
                                        uint64_t *entries, uint64_t *blocks,
                                        size_t *bad)
{
    uint64_t e = 0, b = 0;
    for (size_t i = 0; i < n; i++) {
        if (out_lens[i] + app_len[i] < out_lens[i]) {
            *bad = i;
            return kBiAppendWraps;
        }
        const uint64_t ce = bi_append_entries(out_lens[i], app_len[i]);
        const uint64_t cb = bi_append_blocks(out_lens[i], app_len[i]);
        e = e + ce < e ? ~0ull : e + ce;
        b = b + cb < b ? ~0ull : b + cb;
    }
    *entries = e;
    *blocks = b;
    const uint64_t lim = 0x7FFFFFFFull;
    if ((uint64_t)n > lim || index_entries > lim || e > lim || b > lim ||
        (uint64_t)n + index_entries + e + b > lim)
        return kBiAppendTooMany;
    return kBiAppendOk;
}

// The index rule of an append: bi_range_stream_usable, and the block's part
// for every OLD block - the full ones are copied, the tail is decoded.
SNAPMI_BI_HD inline uint64_t bi_append_first_bad_block(const uint64_t *e,
                                                       uint64_t in_len,
                                                       uint64_t blocks)
{
    return bi_write_first_bad_block(e, in_len, blocks);
}

// The splice, by definition: the stream's new entries from its old ones e[]
// (kf + 1 of them are looked at) and the compressed sizes nsize[nb] of its
// new blocks (without a varint); hdr_new is the length of varint(dlen + add).
// e_new has kf + nb + 1 places.  Returns the new length (the last new entry).
SNAPMI_BI_HD inline uint64_t bi_append_splice(const uint64_t *e, uint64_t kf,
                                              const uint64_t *nsize,
                                              uint64_t nb, uint32_t hdr_new,
                                              uint64_t *e_new)
{
    uint64_t pos = hdr_new;
    for (uint64_t k = 0; k < kf; k++) {
        e_new[k] = pos;
        pos += e[k + 1] - e[k];
    }
    for (uint64_t j = 0; j < nb; j++) {
        e_new[kf + j] = pos;
        pos += nsize[j];
    }
    e_new[kf + nb] = pos;
    return pos;
}

// ... and as the kernels compute it, an entry at a time: an old entry moves
// by what the header grew; a new one lies behind the old full blocks by the
// running sum of the new blocks in front of it.  ncum[j] is the sum of the
// sizes of the new blocks [0, j), ncum[nb] their total.
SNAPMI_BI_HD inline uint64_t bi_append_entry(const uint64_t *e, uint64_t k,
                                             uint64_t kf,
                                             const uint64_t *ncum,
                                             uint32_t hdr_old,
                                             uint32_t hdr_new)
{
    if (k <= kf)
        return e[k] + hdr_new - hdr_old;
    return e[kf] + hdr_new - hdr_old + ncum[k - kf];
}

// The last verdict: the new stream fits its buffer (an exact cap passes).
SNAPMI_BI_HD inline bool bi_append_fits(uint64_t cap, uint64_t new_len)
{
    return bi_write_fits(cap, new_len);
}

// ---------------------------------------------------------------------
// The groups of an update (a range write or an append): the named streams -
// those a write touches, those bytes are appended to - are cut, in order, into
// groups of whole streams whose compress slots (kBiSlot bytes for every block
// that goes through the compressor) and rooms (64 KiB for every block that is
// decoded first) fit `scratch_bytes`; a stream that needs more than that is a
// group of its own.  The groups follow each other on the stream and reuse the
// scratch, so the rooms of a group are numbered from 0.
// ---------------------------------------------------------------------
// max_compress_len(64 KiB), rounded up to 16 (kSlotBytes of the device code)
constexpr uint64_t kBiSlot = 76496;

// named streams [t0, t0 + tg), their blocks [b0, b0 + bg), and their rooms
struct BiUpdateGroup {
    uint32_t t0, tg, b0, bg, rooms;
};

// the most streams, blocks and rooms any group holds
struct BiUpdateMax {
    uint64_t tg, bg, rooms;
};

// b0[ts + 1]: the first block of every named stream (b0[ts]: all blocks);
// rooms[ts]: the rooms of each.  groups[] has ts places; room0[t] becomes the
// first room of stream t inside its group - its rooms take the numbers from
// there, ascending in block order.  Returns the number of groups (0 for
// ts == 0).
SNAPMI_BI_HD inline size_t bi_update_groups(const uint32_t *b0,
                                            const uint32_t *rooms, size_t ts,
                                            uint64_t scratch_bytes,
                                            BiUpdateGroup *groups,
                                            uint32_t *room0, BiUpdateMax *max)
{
    max->tg = max->bg = max->rooms = 0;
    size_t count = 0;
    uint64_t bytes = 0;
    for (size_t t = 0; t < ts; t++) {
        const uint32_t nt = b0[t + 1] - b0[t];
        const uint64_t need =
            (uint64_t)nt * kBiSlot + (uint64_t)rooms[t] * kBiBlock;
        if (count == 0 || bytes + need > scratch_bytes) {
            groups[count++] = BiUpdateGroup{(uint32_t)t, 0, b0[t], 0, 0};
            bytes = 0;
        }
        BiUpdateGroup &g = groups[count - 1];
        room0[t] = g.rooms;
        g.tg++;
        g.bg += nt;
        g.rooms += rooms[t];
        bytes += need;
        max->tg = g.tg > max->tg ? g.tg : max->tg;
        max->bg = g.bg > max->bg ? g.bg : max->bg;
        max->rooms = g.rooms > max->rooms ? g.rooms : max->rooms;
    }
    return count;
}

// ---------------------------------------------------------------------
// Building the index of a stream that came without one
// (snapmi_build_block_index): a walk from element to element that notes where
// the chain stands when exactly k * 64 KiB have been produced.  bi_build is
// the definition; the kernels (the scan's cuts in snapmi_longstream.hip and
// k_index_walk in snapmi_index.hip) must reproduce it.  The hop over one
// element is elem_step of snapmi_element.hpp.
//
// The walk reads tag bytes and literal length bytes only.  Copy offsets are
// not looked at: the builder finds boundaries, it does not say whether the
// stream decodes - the decoders distrust every index anyway.
// ---------------------------------------------------------------------
constexpr int kBiBuilt = 1;     // SNAPMI_INDEX_BUILT: entries as compress writes them
constexpr int kBiUnaligned = 2; // ... _UNALIGNED: whole, but an element straddles a boundary
constexpr int kBiCorrupt = 3;   // ... _CORRUPT: no header, or the chain does not end at (in_len, dlen)
constexpr int kBiMissized = 4;  // ... _MISSIZED: not the lengths the host's copies said

// The walk of a stream of two blocks and more whose header (hdr bytes) has
// been read: put(k, p) for every interior k (0 < k < blocks) at which an
// element starts at p with exactly k * 64 KiB produced, in ascending k.
// kBiBuilt when the chain is whole - every element fits, it ends at in_len
// with dlen produced - and every interior k was put; kBiUnaligned when it is
// whole and an element straddles a boundary; else kBiCorrupt.  (What was put
// before a verdict other than kBiBuilt is the caller's to take back.)
template <class At, class Put>
SNAPMI_BI_HD inline int bi_walk(At &&at, uint64_t in_len, uint32_t hdr,
                                uint64_t dlen, Put &&put)
{
    const uint64_t blocks = bi_blocks(dlen);
    uint64_t p = hdr, out = 0, k = 1;
    bool aligned = true;
    while (p < in_len) {
        if (k < blocks && out > k * kBiBlock) { // the last element straddled
            aligned = false;
            k = (out + kBiBlock - 1) / kBiBlock;
        }
        if (k < blocks && out == k * kBiBlock) {
            if (aligned)
                put(k, p);
            k++;
        }
        // (out <= dlen < 2^32 here: the sums below cannot wrap)
        if (!elem_step(at, in_len, p, out) || out > dlen)
            return kBiCorrupt;
    }
    if (p != in_len || out != dlen)
        return kBiCorrupt;
    // (every interior boundary lies below dlen: one that was not stood on
    // was straddled - by the last element, if k is still behind)
    return aligned && k >= blocks ? kBiBuilt : kBiUnaligned;
}

// The index of the stream in[0, in_len), which the caller says announces
// dlen, into e[bi_entries(dlen)].  kBiBuilt: e[] is what
// snapmi_compress_batch_indexed writes - the varint's length, the offset of
// the element that starts where exactly k * 64 KiB have been produced for
// every interior k, in_len.  Any other verdict: all entries 0, which fails
// both bi_stream_indexed and bi_range_stream_usable - such a stream is
// decoded whole, and a range on it has no usable index.
// A stream of at most one block (dlen <= 64 KiB) is not walked: a header that
// parses gives {hdr, in_len} - which bi_range_stream_usable accepts - and
// kBiBuilt; dlen == 0 has the one entry {hdr}, and only when in_len == hdr
// (else kBiCorrupt).
SNAPMI_BI_HD inline int bi_build(const uint8_t *in, uint64_t in_len,
                                 uint64_t dlen, uint64_t *e)
{
    const uint64_t n = bi_entries(dlen);
    for (uint64_t j = 0; j < n; j++)
        e[j] = 0;
    uint64_t announced = 0;
    const uint32_t hdr = bi_header(in, in_len, &announced);
    if (hdr == 0)
        return kBiCorrupt;
    if (announced != dlen)
        return kBiMissized;
    if (dlen == 0) {
        if (in_len != hdr)
            return kBiCorrupt;
        e[0] = hdr;
        return kBiBuilt;
    }
    if (dlen > kBiBlock) {
        const int st = bi_walk([in](uint64_t i) { return (uint32_t)in[i]; },
                               in_len, hdr, dlen,
                               [e](uint64_t k, uint64_t p) { e[k] = p; });
        if (st != kBiBuilt) {
            for (uint64_t j = 0; j < n; j++)
                e[j] = 0;
            return st;
        }
    }
    e[0] = hdr;
    e[n - 1] = in_len;
    return kBiBuilt;
}

} // namespace snapmi
