// snapmi_element.hpp -- the Snappy element format, once: what a tag byte
// says, the hop over one element, the header, and the reference's element
// loop (src/decompress.rs:75-95, 130-343: which check fails with which three
// fields) by one thread over flat memory.  Plain C++ over a source of bytes,
// no HIP types: the kernels and a host program (tests/element_host.cpp,
// tests/test_element_cpu.py) compile the same text.
//
// An element is a tag byte and what follows it; its type is tag & 3:
//   0, literal: n6 = tag >> 2 < 60: n6 + 1 bytes follow; n6 = 60..63:
//      n6 - 59 length bytes (length - 1, little endian), then the bytes;
//   1, copy:    4 + (n6 & 7) bytes from offset (tag >> 5) << 8 | 1 byte;
//   2 / 3:      n6 + 1 bytes from an offset of 2 / 4 bytes.
#ifndef SNAPMI_ELEMENT_HPP
#define SNAPMI_ELEMENT_HPP

#include <stdint.h>

#include "../../include/snapmi.h"
#include "snapmi_tiny.hpp" // SNAPMI_LANE_FN

namespace snapmi {

constexpr uint64_t kMaxInput = 0xFFFFFFFFull; // reference src/lib.rs:93

SNAPMI_LANE_FN uint32_t copy_offset_bytes(uint32_t type) // behind the tag
{
    return type == 1 ? 1 : (type == 2 ? 2 : 4);
}
SNAPMI_LANE_FN uint32_t copy_length(uint32_t tag)
{
    return (tag & 3) == 1 ? 4 + ((tag >> 2) & 7) : 1 + (tag >> 2);
}
// the high bits of a copy-1's offset (TagEntry::offset, :433-474)
SNAPMI_LANE_FN uint32_t copy1_high(uint32_t tag) { return (tag >> 5) << 8; }
// bytes an element produces / occupies, as far as the tag alone says: 0 for
// a literal with length bytes
SNAPMI_LANE_FN uint32_t tag_produced(uint32_t tag)
{
    return tag & 3 ? copy_length(tag) : (tag < 240 ? (tag >> 2) + 1 : 0);
}
SNAPMI_LANE_FN uint32_t tag_encoded(uint32_t tag)
{
    return tag & 3 ? 1 + copy_offset_bytes(tag & 3)
                   : (tag < 240 ? (tag >> 2) + 2 : 0);
}

// a pointer as a source of bytes: at(i) is byte i
template <class P> struct BytesAt {
    P p;
    SNAPMI_LANE_FN uint32_t operator()(uint64_t i) const { return p[i]; }
};
template <class P> SNAPMI_LANE_FN BytesAt<P> bytes_at(P p)
{
    return BytesAt<P>{p};
}

// hop over the element at p (tag and literal length bytes only); false if it
// does not fit in the stream
template <class At>
SNAPMI_LANE_FN bool elem_step(At &&at, uint64_t in_len, uint64_t &p,
                              uint64_t &out)
{
    const uint32_t tag = at(p);
    const uint32_t type = tag & 3;
    if (type == 0) {
        const uint32_t n6 = tag >> 2;
        uint64_t len = n6 + 1, hd = 1;
        if (n6 >= 60) { // n6 - 59 length bytes
            const uint32_t nb = n6 - 59;
            if (p + 1 + nb > in_len)
                return false;
            uint32_t v = 0;
            for (uint32_t k = 0; k < nb; k++)
                v |= (uint32_t)at(p + 1 + k) << (8 * k);
            len = (uint64_t)v + 1;
            hd = 1 + nb;
        }
        if (in_len - (p + hd) < len)
            return false;
        p += hd + len;
        out += len;
    } else {
        const uint32_t cnb = copy_offset_bytes(type);
        if (p + 1 + cnb > in_len)
            return false;
        p += 1 + cnb;
        out += copy_length(tag);
    }
    return true;
}

// reference bytes::read_varu64, src/bytes.rs:73-90 (the header's length, 0 =
// invalid)
template <class At>
SNAPMI_LANE_FN uint32_t varint_read(At &&at, uint64_t n, uint64_t *value)
{
    uint64_t acc = 0;
    uint32_t shift = 0;
    for (uint64_t i = 0; i < n; i++) {
        const uint32_t b = at(i);
        if (shift >= 64)
            return 0;
        if (b < 0x80) {
            *value = acc | ((uint64_t)b << shift);
            return (uint32_t)i + 1;
        }
        acc |= (uint64_t)(b & 0x7F) << shift;
        shift += 7;
    }
    return 0;
}

// A failed check writes its error to errs[i] (errs null: nowhere) and
// returns the kind.
SNAPMI_LANE_FN int elem_fail(snapmi_error *errs, uint64_t i, int kind,
                             uint64_t a, uint64_t b, uint64_t c)
{
    if (errs) {
        errs[i].kind = kind;
        errs[i].reserved = 0;
        errs[i].a = a;
        errs[i].b = b;
        errs[i].c = c;
    }
    return kind;
}

// Header::read, src/decompress.rs:362-374: the kind; on success hdr and dlen
template <class At>
SNAPMI_LANE_FN int header_read(At &&at, uint64_t in_len, uint32_t *hdr,
                               uint64_t *dlen, snapmi_error *errs, uint64_t i)
{
    uint64_t v = 0;
    const uint32_t h = varint_read(at, in_len, &v);
    if (h == 0)
        return elem_fail(errs, i, SNAPMI_HEADER, 0, 0, 0);
    if (v > kMaxInput)
        return elem_fail(errs, i, SNAPMI_TOO_BIG, v, kMaxInput, 0);
    *hdr = h;
    *dlen = v;
    return SNAPMI_OK;
}

// One descriptor of the batch decoder from its prologue (Decoder::decompress
// and Header::read, src/decompress.rs:75-95,362-374; a stored frame chunk,
// src/read.rs:173-199) to HeaderMismatch (:149-157), over flat memory:
// in[0, in_len) into out[0, cap).  mode: 0 a raw stream, 1 a stored chunk,
// 2 a headerless piece (its elements produce exactly cap bytes), 3 another
// launch's (true, nothing written).  True: *produced bytes were written;
// false: the error is in errs[i].  Literals move 16 bytes at a time where both
// buffers allow it, copies bytewise and in order (they may overlap).
template <class CP, class MP>
SNAPMI_LANE_FN bool lane_decode(CP in, uint64_t in_len, uint32_t mode, MP out,
                                uint64_t cap, uint64_t *produced,
                                snapmi_error *errs, uint64_t i)
{
    *produced = 0;
    if (mode == 3)
        return true;
    if (mode == 1) {
        if (in_len > cap)
            return !elem_fail(errs, i, SNAPMI_BUFFER_TOO_SMALL, cap, in_len, 0);
        for (uint64_t k = 0; k < in_len; k++)
            out[k] = in[k];
        *produced = in_len;
        return true;
    }
    uint32_t hdr = 0;
    uint64_t dst_len = cap;
    if (mode != 2) {
        if (in_len == 0)
            return !elem_fail(errs, i, SNAPMI_EMPTY, 0, 0, 0);
        if (header_read(bytes_at(in), in_len, &hdr, &dst_len, errs, i) != SNAPMI_OK)
            return false;
        if (dst_len > cap)
            return !elem_fail(errs, i, SNAPMI_BUFFER_TOO_SMALL, cap, dst_len, 0);
    }
    CP src = in + hdr;
    const uint64_t src_len = in_len - hdr;
    uint64_t s = 0, d = 0;
    while (s < src_len) {
        const uint32_t tag = src[s];
        s += 1;
        if ((tag & 3) == 0) { // read_literal, :161-228
            uint64_t len = (tag >> 2) + 1;
            if (len >= 61) {
                const uint32_t nb = (uint32_t)len - 60;
                if (s + 4 > src_len)
                    return !elem_fail(errs, i, SNAPMI_LITERAL, 4, src_len - s,
                                      dst_len - d);
                uint32_t raw;
                __builtin_memcpy(&raw, src + s, 4);
                // (u64: a length field of 0xFFFFFFFF + 1 must not wrap)
                len = (uint64_t)(nb == 4 ? raw : raw & ((1u << (8 * nb)) - 1)) +
                      1;
                s += nb;
            }
            if (src_len - s < len || dst_len - d < len)
                return !elem_fail(errs, i, SNAPMI_LITERAL, len, src_len - s,
                                  dst_len - d);
            uint64_t k = 0;
            for (; k + 16 <= len; k += 16) {
                struct {
                    uint32_t w[4];
                } t;
                __builtin_memcpy(&t, src + s + k, 16);
                __builtin_memcpy(out + d + k, &t, 16);
            }
            for (; k < len; k++)
                out[d + k] = src[s + k];
            s += len;
            d += len;
        } else { // read_copy + TagEntry::offset, :233-343,433-474
            const uint32_t nb = copy_offset_bytes(tag & 3);
            const uint32_t len = copy_length(tag);
            uint64_t offset = (tag & 3) == 1 ? copy1_high(tag) : 0;
            if (s + nb > src_len)
                return !elem_fail(errs, i, SNAPMI_COPY_READ, nb, src_len - s, 0);
            uint32_t v = 0;
            for (uint32_t k = 0; k < nb; k++)
                v |= (uint32_t)src[s + k] << (8 * k);
            offset |= v;
            s += nb;
            if (d <= offset - 1) // wrapping, also catches offset == 0
                return !elem_fail(errs, i, SNAPMI_OFFSET, offset, d, 0);
            if (d + len > dst_len)
                return !elem_fail(errs, i, SNAPMI_COPY_WRITE, len, dst_len - d, 0);
            for (uint32_t k = 0; k < len; k++)
                out[d + k] = out[d - offset + k];
            d += len;
        }
    }
    if (d != dst_len)
        return !elem_fail(errs, i, SNAPMI_HEADER_MISMATCH, dst_len, d, 0);
    *produced = dst_len;
    return true;
}

} // namespace snapmi

#endif
