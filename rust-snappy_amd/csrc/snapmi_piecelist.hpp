// snapmi - the piece-descriptor slab: what launch_decompress reads when the
// "streams" of a launch are pieces the device cut itself (the long streams of
// a batch, indexed decode, range reads).  P slots, an array per field:
//   c_in [P] c_inlen [P] c_out [P] c_cap [P] c_outlen [P]   8 bytes a slot
//   c_err [P]                                                snapmi_error
//   c_mode [P]                                               a byte
// The one host-side description of it: snapmi_streamplan.hpp sizes sd_desc
// with it, the callers turn a base address into pointers with it, and every
// argument block that carries a list holds one PieceList.
// Plain functions, no HIP (tests/test_piecelist_cpu.py); the kernels never
// compute these addresses, they are handed the pointers and store and check a
// slot through piece_put / piece_whole of snapmi_device.hpp.
#pragma once
#include <cstddef>
#include <cstdint>

struct snapmi_error; // include/snapmi.h

namespace snapmi {

constexpr size_t kPieceErrBytes = 32; // sizeof(snapmi_error)
constexpr size_t kPieceSlotBytes = 8 * 5 + kPieceErrBytes + 1;

// byte offsets of the seven arrays of a slab of P slots; `total` is what to
// reserve for it (64 bytes of slack behind the modes)
struct PieceOffsets {
    size_t c_in, c_inlen, c_out, c_cap, c_outlen, c_err, c_mode, total;
};

inline PieceOffsets piece_offsets(size_t P)
{
    PieceOffsets o;
    o.c_in = 0;
    o.c_inlen = P * 8;
    o.c_out = P * 16;
    o.c_cap = P * 24;
    o.c_outlen = P * 32;
    o.c_err = P * 40;
    o.c_mode = P * (40 + kPieceErrBytes);
    o.total = P * kPieceSlotBytes + 64;
    return o;
}

struct PieceList {
    const void **c_in;
    uint64_t *c_inlen;
    void **c_out;
    uint64_t *c_cap;
    uint64_t *c_outlen;
    snapmi_error *c_err;
    uint8_t *c_mode;
};

// the slab of P slots at `base` (8-byte aligned: the allocator's are 256)
inline PieceList piece_list(void *base, size_t P)
{
    const PieceOffsets o = piece_offsets(P);
    uint8_t *const d = (uint8_t *)base;
    PieceList l;
    l.c_in = (const void **)(d + o.c_in);
    l.c_inlen = (uint64_t *)(d + o.c_inlen);
    l.c_out = (void **)(d + o.c_out);
    l.c_cap = (uint64_t *)(d + o.c_cap);
    l.c_outlen = (uint64_t *)(d + o.c_outlen);
    l.c_err = (snapmi_error *)(d + o.c_err);
    l.c_mode = d + o.c_mode;
    return l;
}

// the list of the slots of `l` from `first` on: a stream's own pieces inside
// the slab of its plan
inline PieceList piece_list_from(const PieceList &l, size_t first)
{
    PieceList s;
    s.c_in = l.c_in + first;
    s.c_inlen = l.c_inlen + first;
    s.c_out = l.c_out + first;
    s.c_cap = l.c_cap + first;
    s.c_outlen = l.c_outlen + first;
    // (snapmi_error is only named here)
    s.c_err = (snapmi_error *)((uint8_t *)l.c_err + first * kPieceErrBytes);
    s.c_mode = l.c_mode + first;
    return s;
}

} // namespace snapmi
