// snapmi_framewalk.hpp -- the walk over the chunk headers of a framed stream
// (reference FrameDecoder::read, src/read.rs:111-236), in plain C++ that the
// kernels of snapmi_framedec.hip, the host code of the host-memory batch calls
// (snapmi_hostbatch.hip) and a CPU test (tests/framewalk_host.cpp) compile
// alike:
//
//   frame_hop        one chunk: the identifier, the chunk types, the length
//                    limits, the stale-10-byte rule
//   frame_walk       hop by hop to the first header the reader rejects
//   frame_chunk_len  the length a data chunk announces
//   frame_index_walk the regular cases only (snapmi_frame_index_host)
//   frame_index_*    the check of a lone stream's side index, entry by entry
//   frame_nowait_*   the rules of the no-wait decode: which front decides,
//                    when the caller's bound is exceeded, what pads the table
//   frame_walk_host  what the host learns of a stream while it stages it: the
//                    walk's verdict, a list entry per data chunk and the
//                    room - an upper bound on what the device may write
//
// The pointer type is a template parameter: device code walks global memory
// through address-space pointers, the host plain ones.  No HIP types, no
// allocation.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "snapmi.h"

#if defined(__HIPCC__)
#define SNAPMI_FW_HD __host__ __device__
#else
#define SNAPMI_FW_HD
#endif

namespace snapmi {

constexpr uint32_t kMaxChunk = 76490;            // reference src/frame.rs:12
constexpr uint32_t kFwMaxBlock = 1u << 16;       // reference src/lib.rs:97
constexpr uint64_t kFwMaxInput = 0xFFFFFFFFull;  // reference src/lib.rs:93

struct FrameChunk { // one data chunk of a framed stream (decode side)
    uint64_t payload_off; // offset of the payload in the stream
    uint32_t payload_len;
    uint32_t crc;   // stored masked crc
    uint32_t type;  // 0 compressed, 1 stored
    uint32_t pad;
};

// One data chunk as the host lists it for the device (k_fbd_from_list): the
// stream it belongs to, where its header lies and the header word itself
// (type | length << 8).
struct FwEntry {
    uint64_t off;
    uint32_t stream;
    uint32_t hd;
};

// little-endian dword at any alignment (one global_load_dword on the device)
template <class P> SNAPMI_FW_HD inline uint32_t fw_ld32(P p)
{
    uint32_t v;
    __builtin_memcpy(&v, p, 4);
    return v;
}

SNAPMI_FW_HD inline snapmi_error frame_err(int kind, uint64_t fa, uint64_t fb)
{
    snapmi_error e;
    e.kind = kind;
    e.reserved = 0;
    e.a = fa;
    e.b = fb;
    e.c = 0;
    return e;
}

// A compressed chunk whose payload is shorter than 10 bytes and holds no
// varint terminator (every byte >= 0x80; an empty payload too).  The
// reference calls decompress_len on its WHOLE 76 490-byte scratch buffer
// `src` (src/read.rs:216), so the varint continues into whatever earlier
// reads left there: this chunk's own 4 header bytes at src[0..4) (read.rs:118),
// and the bodies of earlier stream-identifier / skippable / padding /
// compressed chunks (read.rs:151,157,168,214; stored chunks go to `dst`).
// The outcome then is TooBig, UnsupportedChunkLength, or - when the phantom
// length is acceptable - whatever Decoder::decompress says about the real
// payload: Empty or Header (src/decompress.rs:80-83).  Rare and always an
// error, so the model of src[0..10) is rebuilt here by walking the stream
// `in` again from its start up to `stop` (the offset of this chunk's header);
// `stale` is src[0..10) when the walk started.
template <class P>
SNAPMI_FW_HD inline snapmi_error frame_short_varint(P in, const uint8_t *stale,
                                                    uint64_t stop)
{
    uint8_t m[10];
    for (int k = 0; k < 10; k++)
        m[k] = stale[k];
    uint64_t r = 0;
    for (;;) { // every chunk before `stop` was accepted by the walk
        const uint32_t hd = fw_ld32(in + r);
        for (int k = 0; k < 4; k++)
            m[k] = (uint8_t)(hd >> (8 * k));
        const uint32_t ty = hd & 0xFF;
        const uint64_t len = hd >> 8;
        uint64_t body = r + 4, blen = len; // bytes read into src[0..blen)
        if (ty == 0x00) {
            body = r + 8;
            blen = len - 4;
        } else if (ty == 0x01) {
            blen = 0;
        }
        for (uint64_t k = 0; k < blen && k < 10; k++)
            m[k] = in[body + k];
        if (r == stop)
            break;
        r += 4 + len;
    }
    // decompress_len(&src): read_varu64 (src/bytes.rs:73-90) over m[0..10)
    uint64_t v = 0;
    uint32_t shift = 0;
    bool ok = false;
    for (int k = 0; k < 10; k++) {
        const uint64_t b = m[k];
        if (b < 0x80) {
            v |= b << shift;
            ok = true;
            break;
        }
        v |= (b & 0x7F) << shift;
        shift += 7;
    }
    const uint64_t sn = (fw_ld32(in + stop) >> 8) - 4;
    if (!ok)
        return frame_err(SNAPMI_HEADER, 0, 0);
    if (v > kFwMaxInput)
        return frame_err(SNAPMI_TOO_BIG, v, kFwMaxInput);
    if (v > kFwMaxBlock) // read.rs:217-222
        return frame_err(SNAPMI_UNSUPPORTED_CHUNK_LENGTH, v, 0);
    // Decoder::decompress(&src[0..sn]), src/decompress.rs:80-83
    return frame_err(sn == 0 ? SNAPMI_EMPTY : SNAPMI_HEADER, 0, 0);
}

// true when the payload [p, p + pl) needs frame_short_varint
template <class P> SNAPMI_FW_HD inline bool short_varint(P p, uint64_t pl)
{
    if (pl >= 10)
        return false;
    for (uint64_t k = 0; k < pl; k++)
        if (p[k] < 0x80)
            return false;
    return true;
}

// One hop of the walk: the chunk whose header lies at r (r < in_len), checks
// in the reference's order.  Returns the error the reader stops with, or kind
// SNAPMI_OK with r behind the chunk; *data says that it was a data chunk, c.
// seen_ident: the identifier has been met (every stream must begin with it);
// `stale` as frame_short_varint.
template <class P>
SNAPMI_FW_HD inline snapmi_error frame_hop(P in, uint64_t in_len,
                                           const uint8_t *stale, uint64_t &r,
                                           bool &seen_ident, bool &data,
                                           FrameChunk &c)
{
    data = false;
    if (in_len - r < 4)
        return frame_err(SNAPMI_E_UNEXPECTED_EOF, 0, 0);
    const uint32_t hd = fw_ld32(in + r);
    r += 4;
    const uint32_t ty = hd & 0xFF;
    const uint64_t len = hd >> 8;
    if (!seen_ident) { // :123-128
        if (ty != 0xFF)
            return frame_err(SNAPMI_STREAM_HEADER, ty, 0);
        seen_ident = true;
    }
    if (len > kMaxChunk) // :129-135
        return frame_err(SNAPMI_UNSUPPORTED_CHUNK_LENGTH, len, 0);
    if (ty >= 0x02 && ty <= 0x7F) // :138-142
        return frame_err(SNAPMI_UNSUPPORTED_CHUNK_TYPE, ty, 0);
    if ((ty >= 0x80 && ty <= 0xFD) || ty == 0xFE) { // skippable, padding
        if (in_len - r < len)
            return frame_err(SNAPMI_E_UNEXPECTED_EOF, 0, 0);
        r += len;
    } else if (ty == 0xFF) { // :159-172
        if (len != 6)
            return frame_err(SNAPMI_UNSUPPORTED_CHUNK_LENGTH, len, 1);
        if (in_len - r < 6)
            return frame_err(SNAPMI_E_UNEXPECTED_EOF, 0, 0);
        const uint8_t body[6] = {'s', 'N', 'a', 'P', 'p', 'Y'};
        uint64_t got = 0;
        bool same = true;
        for (int k = 0; k < 6; k++) {
            const uint8_t b = in[r + k];
            got |= (uint64_t)b << (8 * k);
            same = same && b == body[k];
        }
        if (!same)
            return frame_err(SNAPMI_STREAM_HEADER_MISMATCH, got, 0);
        r += 6;
    } else { // 0x00 compressed / 0x01 stored: :173-235
        if (len < 4)
            return frame_err(SNAPMI_UNSUPPORTED_CHUNK_LENGTH, len, 0);
        if (in_len - r < 4)
            return frame_err(SNAPMI_E_UNEXPECTED_EOF, 0, 0);
        const uint32_t crc = fw_ld32(in + r);
        r += 4;
        const uint64_t pl = len - 4;
        if (ty == 0x01 && pl > kFwMaxBlock) // :182-187
            return frame_err(SNAPMI_UNSUPPORTED_CHUNK_LENGTH, pl, 0);
        if (in_len - r < pl)
            return frame_err(SNAPMI_E_UNEXPECTED_EOF, 0, 0);
        if (ty == 0x00 && short_varint(in + r, pl)) // read.rs:216
            return frame_short_varint(in, stale, r - 8);
        c.payload_off = r;
        c.payload_len = (uint32_t)pl;
        c.crc = crc;
        c.type = ty;
        c.pad = 0;
        data = true;
        r += pl;
    }
    return frame_err(SNAPMI_OK, 0, 0);
}

// Sequential walk over the chunk headers of one framed stream
// in[0, in_len): reference FrameDecoder::read, src/read.rs:111-236 (`flags`
// and `stale` as in snapmi_frame_decompress_ex).  Every hop depends on the
// previous header, so a stream is walked by one thread.  on_data(k, chunk) is
// called for data chunk k (0, 1, ...) in front of the first structural error;
// returns that error (kind SNAPMI_OK at a clean end) and *nd = the data
// chunks in front of it.
template <class P, class OnData>
SNAPMI_FW_HD inline snapmi_error frame_walk(P in, uint64_t in_len,
                                            uint32_t flags,
                                            const uint8_t *stale, uint32_t &nd,
                                            OnData on_data)
{
    uint64_t r = 0;
    nd = 0;
    bool seen_ident = (flags & SNAPMI_FRAME_CONTINUATION) != 0;
    while (r != in_len) { // clean EOF, :119-121
        bool data;
        FrameChunk c;
        const snapmi_error e =
            frame_hop(in, in_len, stale, r, seen_ident, data, c);
        if (e.kind != SNAPMI_OK)
            return e;
        if (data) {
            on_data(nd, c);
            nd++;
        }
    }
    return frame_err(SNAPMI_OK, 0, 0);
}

// decompressed length of data chunk c, whose payload starts at p: reference
// src/read.rs:181-187 (stored) and :215-222 (compressed: decompress_len, then
// dn <= 65536); 0 and *e on an error
template <class P>
SNAPMI_FW_HD inline uint64_t frame_chunk_len(P p, const FrameChunk &c,
                                             snapmi_error &e)
{
    e = frame_err(SNAPMI_OK, 0, 0);
    if (c.type > 1) { // only reachable through a bad side index or list
        e.kind = SNAPMI_UNSUPPORTED_CHUNK_TYPE;
        e.a = c.pad;
        return 0;
    }
    if (c.type == 1)
        return c.payload_len;
    uint64_t acc = 0;
    uint32_t shift = 0;
    bool ok = false;
    for (uint32_t k = 0; k < c.payload_len; k++) {
        const uint32_t b = p[k];
        if (shift >= 64)
            break;
        if (b < 0x80) {
            acc |= (uint64_t)b << shift;
            ok = true;
            break;
        }
        acc |= (uint64_t)(b & 0x7F) << shift;
        shift += 7;
    }
    if (c.payload_len == 0) {
        // reference: decompress_len of the scratch reads a stale byte;
        // the decode of the empty payload then fails with Empty
        e.kind = SNAPMI_EMPTY;
    } else if (!ok) {
        e.kind = SNAPMI_HEADER;
    } else if (acc > kFwMaxInput) {
        e.kind = SNAPMI_TOO_BIG;
        e.a = acc;
        e.b = kFwMaxInput;
    } else if (acc > kFwMaxBlock) {
        e.kind = SNAPMI_UNSUPPORTED_CHUNK_LENGTH;
        e.a = acc;
    } else {
        return acc;
    }
    return 0;
}

// The regular cases of the walk, without the rules that need history or a
// payload (snapmi_frame_index_host): 0 and *n_chunks = data chunks for a
// stream that is a run of well-formed chunks from its identifier to its end,
// 1 for anything else.  offsets (cap entries, may be NULL) receives the data
// chunks' header offsets and, behind them, in_len.
inline int frame_index_walk(const uint8_t *in, uint64_t in_len,
                            uint64_t *offsets, uint64_t cap,
                            uint64_t *n_chunks)
{
    uint64_t r = 0, nd = 0;
    bool seen_ident = false;
    while (r != in_len) {
        if (in_len - r < 4)
            return 1;
        const uint32_t ty = in[r];
        const uint64_t len = fw_ld32(in + r) >> 8;
        const uint64_t at = r;
        r += 4;
        if (!seen_ident && ty != 0xFF)
            return 1;
        seen_ident = true;
        if (len > kMaxChunk || (ty >= 0x02 && ty <= 0x7F) ||
            in_len - r < len)
            return 1;
        if (ty == 0xFF) {
            const uint8_t body[6] = {'s', 'N', 'a', 'P', 'p', 'Y'};
            if (len != 6)
                return 1;
            for (int k = 0; k < 6; k++)
                if (in[r + k] != body[k])
                    return 1;
        } else if (ty <= 0x01) {
            if (len < 4 || (ty == 0x01 && len - 4 > kFwMaxBlock))
                return 1;
            if (offsets) {
                if (nd + 1 >= cap)
                    return 1;
                offsets[nd] = at;
            }
            nd++;
        }
        r += len;
    }
    if (offsets) {
        if (nd + 1 > cap)
            return 1;
        offsets[nd] = in_len;
    }
    *n_chunks = nd;
    return 0;
}

// ---------------------------------------------------------------------
// The side index of a lone stream (snapmi_frame_decompress[_ex]).  The index
// is the caller's: it is taken as a hint, never trusted.  A header that is not
// an in-bounds data chunk ending exactly at the next index entry (the entries
// must tile the stream from the identifier to its end: other chunk types in
// between are the walk's business), or a chunk only the walk can judge
// (frame_short_varint), sends the whole stream to the walk, which owns every
// error report.
// ---------------------------------------------------------------------

// a record that decodes to nothing: what stands in the chunk table for an
// index entry that failed its check and, in a no-wait decode, behind the
// stream's last chunk (frame_chunk_len answers type 0xFF with length 0 and
// reads no payload byte)
SNAPMI_FW_HD inline FrameChunk frame_no_chunk()
{
    FrameChunk c;
    c.payload_off = 0;
    c.payload_len = 0;
    c.crc = 0;
    c.type = 0xFF;
    c.pad = 0;
    return c;
}

// What the index as a whole must get right, besides its entries: the stream
// begins with the identifier (unless it was seen before), and an index
// without entries tiles nothing - only a stream that ends right behind its
// identifier (or an empty continuation) has no chunks.
template <class P>
SNAPMI_FW_HD inline bool frame_index_start(P in, uint64_t in_len,
                                           uint32_t flags, uint32_t n_index)
{
    const bool cont = (flags & SNAPMI_FRAME_CONTINUATION) != 0;
    if (!cont) {
        const uint8_t ident[10] = {0xFF, 0x06, 0x00, 0x00, 's',
                                   'N',  'a',  'P',  'p',  'Y'};
        bool ok = in_len >= 10;
        for (int k = 0; ok && k < 10; k++)
            ok = in[k] == ident[k];
        if (!ok)
            return false; // the walk reports what is wrong with the start
    }
    return n_index != 0 || in_len == (cont ? 0u : 10u);
}

// Entry i < n_index (index has n_index + 1 entries; none behind index[i + 1]
// is read): true and the chunk c when it passes, false and a record that
// decodes to nothing when not.
template <class P>
SNAPMI_FW_HD inline bool frame_index_entry(P in, uint64_t in_len,
                                           uint32_t flags,
                                           const uint64_t *index,
                                           uint32_t n_index, uint32_t i,
                                           FrameChunk &c)
{
    const uint64_t r = index[i];
    c = frame_no_chunk();
    if (!(in_len >= 8 && r <= in_len - 8))
        return false;
    const uint32_t hd = fw_ld32(in + r);
    const uint32_t ty = hd & 0xFF, len = hd >> 8;
    const bool good =
        ty <= 1 && len >= 4 && len <= kMaxChunk && len <= in_len - r - 4 &&
        !(ty == 1 && len - 4 > kFwMaxBlock) &&
        index[i + 1] == r + 4 + len && // nothing unseen in between
        (i + 1 < n_index || index[i + 1] == in_len) &&
        (i > 0 || r == ((flags & SNAPMI_FRAME_CONTINUATION) ? 0u : 10u)) &&
        !(ty == 0 && short_varint(in + r + 8, len - 4));
    if (good) {
        c.type = ty;
        c.payload_len = len - 4;
        c.crc = fw_ld32(in + r + 4);
        c.payload_off = r + 8;
    }
    return good;
}

// ---------------------------------------------------------------------
// The no-wait decode (SNAPMI_FRAME_NO_WAIT): the caller bounds the data
// chunks by n_chunks, the host sizes the chunk table and every launch from
// that bound and enqueues the fronts back to back - the side index if one
// was given, else the parallel walk if the stream is long enough, then the
// sequential walk.  A front decides when it ends without handing the stream
// on (meta[2] == 0); a front behind one that has decided leaves at once.  The
// order on the stream is the only synchronisation.
// ---------------------------------------------------------------------
enum FrameFront : uint32_t {
    kFrontIndex = 1,    // the side index
    kFrontParallel = 2, // the parallel walk
    kFrontWalk = 3,     // the sequential walk
    kFrontExceeded = 4, // the deciding front counted more than n_chunks
};

// `handed_on`: meta[2] as a front left it (0, or who must judge instead)
SNAPMI_FW_HD inline bool frame_front_decided(uint32_t handed_on)
{
    return handed_on == 0;
}

// What a no-wait decode's fronts came to.  first_front: the front the host
// enqueued first (kFrontWalk when the walk was the only one); walk_ran: the
// sequential walk did not find the stream decided; found: data chunks the
// deciding front counted in front of the stream's first structural error;
// cap: n_chunks.
struct FrameNowait {
    uint32_t front;  // FrameFront, for info "frame_nowait_front"
    bool exceeded;   // the promise is broken: {SNAPMI_E_ARGUMENT, found, cap}
                     // wins over every other verdict, nothing is decoded
    uint32_t chunks; // records [0, chunks) of the table are the stream's
    uint32_t pad_lo; // records [pad_lo, cap) become frame_no_chunk()
};

SNAPMI_FW_HD inline FrameNowait frame_nowait_rule(uint32_t first_front,
                                                  bool walk_ran,
                                                  uint32_t found, uint32_t cap)
{
    FrameNowait x;
    x.exceeded = found > cap;
    x.front = x.exceeded                               ? kFrontExceeded
              : first_front == kFrontWalk || walk_ran ? kFrontWalk
                                                       : first_front;
    // (a front that counted too many has left records undefined - the
    // parallel walk emits none, the sequential walk those below cap: none
    // may reach the kernels behind)
    x.chunks = x.exceeded ? 0 : found;
    x.pad_lo = x.chunks;
    return x;
}

// the verdict of a broken promise
SNAPMI_FW_HD inline snapmi_error frame_nowait_exceeded(uint32_t found,
                                                       uint32_t cap)
{
    return frame_err(SNAPMI_E_ARGUMENT, found, cap);
}

// What the host learns of one fresh stream before the device sees it.
struct FwStream {
    snapmi_error e;  // the walk's verdict (kind SNAPMI_OK: the stream is a
                     // run of chunks the reader accepts, from start to end)
    uint64_t room;   // sum of the lengths the data chunks in front of that
                     // verdict announce: the decoder writes no chunk behind
                     // it and no chunk longer than it announces, so no more
                     // than this whatever the payloads hold
    uint32_t chunks; // data chunks in front of the verdict
};

// emit(header offset, header word) is called per data chunk, in order.
template <class Emit>
inline FwStream frame_walk_host(const uint8_t *in, uint64_t in_len, Emit emit)
{
    const uint8_t fresh[10] = {0};
    FwStream x;
    x.room = 0;
    x.e = frame_walk(in, in_len, 0, fresh, x.chunks,
                     [&](uint32_t, const FrameChunk &c) {
                         snapmi_error ce;
                         x.room += frame_chunk_len(in + c.payload_off, c, ce);
                         emit(c.payload_off - 8,
                              c.type | ((c.payload_len + 4) << 8));
                     });
    return x;
}

} // namespace snapmi
