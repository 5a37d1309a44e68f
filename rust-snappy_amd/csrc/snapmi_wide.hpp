// snapmi_wide.hpp -- the wavefront decoder's shared parts: one wavefront per
// raw stream, its state in SGPRs.  The lane-order helpers, the 4 KiB ring of
// recent output in LDS (Ring2), the state (Wide), the stream prologue and
// epilogue (open_stream / close_stream) and the sequential decoder that
// finishes - and names the error of - every stream the window loops
// (snapmi_wide2.hpp, snapmi_wide3.hpp) hand over.  Kernels: snapmi_wide.hip.
#pragma once

#include "snapmi_device.hpp"
#include "snapmi_element.hpp"
#include "snapmi_kernels.hpp"

namespace snapmi {

namespace {

// The reference's element-at-a-time loop (src/decompress.rs:130-343), state
// in SGPRs, bytes moved by the lanes.  Used to finish a stream once the wide
// path has met something irregular; resumes at (s, d).
// The checks are lane_decode's (snapmi_element.hpp), in its order and with its
// fields, WRITTEN OUT: through a shared function these kernels, held to 64
// VGPRs, leave the parent's registers (profiles/decoder_split_resources.md).
__device__ __forceinline__ void decode_sequential(const DecompressArgs &a,
                                               uint64_t st, uint32_t lane,
                                               gcptr src,
                                               uint64_t src_len, gptr dst,
                                               uint64_t dst_len, uint64_t s,
                                               uint64_t d)
{
    ByteWindow win;
    win.init(src, src_len);
    uint64_t pend = 0; // dst[pend..d) may still be in flight (stores)

    while (s < src_len) {
        const uint32_t w = win.get32(s); // tag + the 3 bytes after it
        const uint32_t tag = w & 0xFF;
        s += 1;
        if ((tag & 3) == 0) {
            // reference read_literal, src/decompress.rs:161-228
            uint64_t len = (tag >> 2) + 1;
            if (len >= 61) {
                if (s + 4 > src_len)
                    SNAPMI_FAIL(lane == 0, , SNAPMI_LITERAL, 4, src_len - s,
                                dst_len - d);
                const uint32_t nb = (uint32_t)len - 60;
                const uint32_t raw = win.get32(s);
                len = (uint64_t)(nb == 4 ? raw
                                         : raw & ((1u << (8 * nb)) - 1)) +
                      1;
                s += nb;
            }
            if (src_len - s < len || dst_len - d < len)
                SNAPMI_FAIL(lane == 0, , SNAPMI_LITERAL, len, src_len - s,
                            dst_len - d);
            gcptr from = src + s;
            gptr to = dst + d;
            for (uint64_t i = 4 * lane; i + 4 <= len; i += 4 * kWave)
                st32u(to + i, ld32u(from + i));
            const uint64_t t = len & ~3ull;
            if (lane < (len & 3))
                to[t + lane] = from[t + lane];
            s += len;
            d += len;
        } else {
            // reference read_copy + TagEntry::offset,
            // src/decompress.rs:233-343,433-474
            const uint32_t kind = tag & 3;
            const uint32_t nb = kind == 1 ? 1 : (kind == 2 ? 2 : 4);
            const uint32_t len =
                kind == 1 ? 4 + ((tag >> 2) & 7) : 1 + (tag >> 2);
            uint64_t offset = kind == 1 ? (uint64_t)(tag >> 5) << 8 : 0;
            if (s + 4 <= src_len) {
                if (nb == 1)
                    offset |= (w >> 8) & 0xFF;
                else if (nb == 2)
                    offset |= (w >> 8) & 0xFFFF;
                else
                    offset |= win.get32(s);
            } else if (nb == 1) {
                if (s >= src_len)
                    SNAPMI_FAIL(lane == 0, , SNAPMI_COPY_READ, 1, src_len - s,
                                0);
                offset |= (w >> 8) & 0xFF;
            } else if (nb == 2) {
                if (s + 1 >= src_len)
                    SNAPMI_FAIL(lane == 0, , SNAPMI_COPY_READ, 2, src_len - s,
                                0);
                offset |= (w >> 8) & 0xFFFF;
            } else {
                SNAPMI_FAIL(lane == 0, , SNAPMI_COPY_READ, 4, src_len - s, 0);
            }
            s += nb;
            if (d <= offset - 1) // wrapping, also catches offset == 0
                SNAPMI_FAIL(lane == 0, , SNAPMI_OFFSET, offset, d, 0);
            const uint64_t end = d + len;
            if (end > dst_len)
                SNAPMI_FAIL(lane == 0, , SNAPMI_COPY_WRITE, len, dst_len - d,
                            0);

            // Source bytes are dst[d-offset .. min(d, d-offset+len)).  If
            // any of them may still be an in-flight store of this wave,
            // drain the stores first.
            const uint64_t from0 = d - offset;
            const uint64_t src_end = offset < len ? d : from0 + len;
            if (src_end > pend) {
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
                pend = d;
            }
            if (lane < len) {
                uint32_t i = lane;
                if (offset < len) {
                    // pattern replication: i mod offset, exact for i,offset<64
                    const uint32_t o = (uint32_t)offset;
                    const uint32_t q =
                        (uint32_t)(((float)lane + 0.5f) *
                                   __builtin_amdgcn_rcpf((float)o));
                    i = lane - q * o;
                }
                dst[d + lane] = dst[from0 + i];
            }
            d = end;
        }
    }
    if (d != dst_len)
        SNAPMI_FAIL(lane == 0, , SNAPMI_HEADER_MISMATCH, dst_len, d, 0);
    if (lane == 0) {
        set_error(a.errs, st, SNAPMI_OK, 0, 0, 0);
        a.out_lens[st] = dst_len;
    }
}

// Inclusive prefix sum over the wave: six v_add_u32_dpp.  (Through the
// update_dpp builtin every step is a v_mov_dpp plus an add - the compiler
// does not fold them - and the decoders' window loop is bound by VALU issue.)
// A DPP operand written by the instruction in front needs two wait states;
// the compiler cannot see into the asm, so the first pad also covers the
// worst case in front of it (a VALU write of EXEC: five wait states).
__device__ __forceinline__ uint32_t wave_inclusive_add(uint32_t v)
{
    asm volatile(
        "s_nop 4\n\t"
        "v_add_u32_dpp %0, %0, %0 row_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
        "s_nop 1\n\t"
        "v_add_u32_dpp %0, %0, %0 row_shr:2 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
        "s_nop 1\n\t"
        "v_add_u32_dpp %0, %0, %0 row_shr:4 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
        "s_nop 1\n\t"
        "v_add_u32_dpp %0, %0, %0 row_shr:8 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
        "s_nop 1\n\t"
        "v_add_u32_dpp %0, %0, %0 row_bcast:15 row_mask:0xa bank_mask:0xf\n\t"
        "s_nop 1\n\t"
        "v_add_u32_dpp %0, %0, %0 row_bcast:31 row_mask:0xc bank_mask:0xf\n\t"
        "s_nop 1"
        : "+v"(v));
    return v;
}

__device__ __forceinline__ uint32_t popc_below(uint64_t mask)
{
    // number of set bits of `mask` strictly below this lane
    return __builtin_amdgcn_mbcnt_hi(
        (uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0));
}

// 16 bytes as two qwords
struct B16x {
    uint64_t lo, hi;
};

// 8 bytes at src[pos..] for a stream of avail >= 8 readable bytes; bytes at
// or past `avail` read as zero.  Branch-free: the load address is clamped
// into the stream and the value shifted back into place.
__device__ __forceinline__ uint64_t ld64c(gcptr src, uint64_t pos,
                                          uint64_t avail)
{
    const uint64_t pc = pos < avail - 8 ? pos : avail - 8;
    uint64_t v;
    __builtin_memcpy(&v, src + pc, 8);
    const uint64_t sh = pos - pc; // 0 inside the stream
    return sh < 8 ? v >> (8 * sh) : 0;
}

// ---------------------------------------------------------------------
// One wavefront per raw stream: the wide path.
//
// Two window loops share the stream prologue, a 4 KiB ring of recent output
// in LDS and the hand-over to the sequential decoder:
//
// decode_windows2 (second generation; k_decompress_streams2 and the last
// bytes of every stream in k_decompress_streams3) - 64 compressed bytes per
// window, an element is copied by the lane that sits on its first byte:
//
//   1. every lane decodes the element that would start at its byte of the
//      64-byte window, and loads 16 literal bytes speculatively;
//   2. the real element starts are the orbit of lane 0 under "next element"
//      (one ds_bpermute per round, see the loop) - no compaction, the
//      records stay where they were decoded;
//   3. a DPP scan of the output lengths over the start lanes places every
//      element; the window is cut after 2048 output bytes (kWinMax), so a
//      4 KiB ring of recent output in LDS always keeps 2 KiB of history that
//      the window's own writes cannot touch;
//   4. ONE lane-parallel copy step: every element whose source is complete
//      before the window (literals; copies from in front of it) is copied by
//      its lane, 16 bytes per trip - source: the speculative literal bytes,
//      the ring, or HBM for what the ring no longer holds - and stored to
//      the ring as WHOLE 16-byte pieces, last piece first: overlapping lanes
//      of one DS store are applied in ascending lane order, so the excess
//      bytes of a short element are overwritten by the elements that follow;
//   5. the few elements that read the window's own output or repeat a short
//      period are swept in stream order, each by the whole wave (lane k =
//      byte k, k mod offset for overlaps);
//   6. the ring goes to HBM 256 bytes at a time (one dword per lane), so
//      global stores are whole aligned lines instead of 64 byte stores.
//
// decode_windows3 (third generation, the default) - 256 compressed bytes per
// window and one ELEMENT per lane; described at the function.
//
// Both loops are bound by instruction issue - VALU (a wave64 integer
// instruction holds its SIMD for four cycles) and the CU's one scalar unit
// about equally, the LDS pipeline third (tests/hw/lds_cost.hip) - so they are
// written for few instructions: predicates are 64-bit lane masks in SGPRs,
// combined with scalar ALU operations and handed back to the vector side as
// they are (inverse ballot); positions are 32-bit (no scalar 64-bit compare
// exists); tests that only matter near the end of the input sit behind one
// uniform branch; addresses are a uniform base plus a 32-bit lane offset.
//
// Everything irregular - a failed check, an element cut off by the end of
// the input - stops the wide path at a window boundary: the ring is stored
// and the sequential decoder above finishes the stream from (s, d) with the
// reference's exact error.  tests/model_decoder.py and tests/model_decoder3.py
// restate the two loops lane by lane on the CPU (test infrastructure, not
// used here).
// ---------------------------------------------------------------------
#define SNAPMI_RING 4096 // experiment builds: 8192 / 16384 (make ring_variants)
constexpr uint32_t kRing2 = SNAPMI_RING;
constexpr uint32_t kWinMax = 2048;

__device__ __forceinline__ uint32_t lds_ld32(const l_u8 *p)
{
    uint32_t v;
    __builtin_memcpy(&v, p, 4);
    return v;
}
__device__ __forceinline__ void lds_st32(l_u8 *p, uint32_t v)
{
    __builtin_memcpy(p, &v, 4);
}

struct Ring2 {
    l_u8 *rg;       // kRing2 bytes + a 16-byte mirror of its first 16
    gptr dst;
    uint32_t lane;
    uint32_t gflush; // dst[0, gflush) has been stored
    uint32_t fenced; // ... and those stores are known to be complete

    // ring[0,16) again behind the end: unaligned reads may run past it
    __device__ __forceinline__ void mirror() const
    {
        if (lane < 4)
            lds_st32(rg + kRing2 + 4 * lane, lds_ld32(rg + 4 * lane));
    }
    // whole 256-byte pieces of dst[gflush, d), one dword per lane
    __device__ __forceinline__ void flush_chunks(uint32_t d)
    {
        while (gflush + 256 <= d) {
            const uint32_t p = gflush + 4 * lane;
            st32u(dst + p, lds_ld32(rg + (p & (kRing2 - 1))));
            gflush += 256;
        }
    }
    // everything up to `upto`, bytewise (before a long literal, at the end,
    // when the sequential decoder takes over)
    __device__ __forceinline__ void flush_partial(uint32_t upto)
    {
        for (uint32_t p = gflush + lane; p < upto; p += kWave)
            dst[p] = rg[p & (kRing2 - 1)];
        gflush = upto;
    }
    // a far source must be a completed store
    __device__ __forceinline__ void fence_for(uint32_t limit)
    {
        if (limit > fenced) {
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
            fenced = gflush;
        }
    }
};

// The wide path's state: everything uniform (SGPRs).
struct Wide {
    gcptr src;        // elements (behind the varint header)
    gptr dst;
    uint64_t src_len, dst_len;
    uint64_t st;      // stream index
    // Positions are 32-bit: there is no scalar 64-bit compare, each one in
    // a window loop would be two VALU instructions.  dst_len < 2^32 by the
    // format; a compressed stream of 4 GiB or more (legal, if every element
    // is tiny) is left to the sequential decoder as a whole, and so is an
    // output within 4 KiB of 2^32 (window arithmetic like d + W + 16 must
    // not wrap).
    uint32_t slen, dlen;
    uint32_t s, d;    // positions in src / dst
    uint32_t ring_lo; // the ring holds dst[max(ring_lo, d - 4096), d)
    Ring2 R;
    PROF(
    uint64_t n_win = 0, n_elem = 0, n_dep = 0, n_fence = 0, n_far = 0,
             n_trip = 0, n_run = 0, n_win3 = 0;
    )
    __device__ __forceinline__ bool too_big() const
    {
        return src_len > 0xFFE00000ull || dst_len > 0xFFFFF000ull;
    }
};

// Stored chunk, header, capacity (reference Decoder::decompress,
// src/decompress.rs:75-95).  False: the stream is finished (copied, or its
// error is written).
// (lane_decode's prologue, WRITTEN OUT for the same reason.)
__device__ __forceinline__ bool open_stream(const DecompressArgs &a,
                                            const uint32_t lane, Wide &x,
                                            l_u8 *ring_mem,
                                            const uint32_t slot)
{
    const uint64_t st = a.order[slot]; // slot: position in the sorted order
    gcptr in = (gcptr)a.in_ptrs[st];
    const uint64_t in_len = a.in_lens[st];
    const bool piece = a.modes && a.modes[st] == 2;

    if (a.modes && a.modes[st] == 3)
        return false; // another launch decodes this stream
    if (a.modes && a.modes[st] == 1) {
        // stored frame chunk (reference src/read.rs:173-199): the payload is
        // the data (wave_copy)
        const uint64_t cap0 = a.out_caps[st];
        if (in_len > cap0)
            SNAPMI_FAIL(lane == 0, false, SNAPMI_BUFFER_TOO_SMALL, cap0,
                        in_len, 0);
        wave_copy<false>((gptr)a.out_ptrs[st], in, in_len, lane);
        if (lane == 0) {
            set_error(a.errs, st, SNAPMI_OK, 0, 0, 0);
            a.out_lens[st] = in_len;
        }
        return false;
    }
    uint32_t hdr = 0;
    uint64_t dst_len = 0;
    if (piece) { // elements [in, in + in_len) produce exactly out_caps bytes
        dst_len = a.out_caps[st];
    } else {
        if (in_len == 0)
            SNAPMI_FAIL(lane == 0, false, SNAPMI_EMPTY, 0, 0, 0);
        snapmi_error *e = lane == 0 ? a.errs : nullptr;
        if (read_header(in, in_len, &hdr, &dst_len, e, st) != SNAPMI_OK) {
            if (lane == 0)
                a.out_lens[st] = 0;
            return false;
        }
    }
    // the header came through vector loads: pin it (and everything derived
    // from it) to SGPRs so the decoder state is scalar
    hdr = uni(hdr);
    dst_len = uni64(dst_len);
    const uint64_t cap = a.out_caps[st];
    if (dst_len > cap)
        SNAPMI_FAIL(lane == 0, false, SNAPMI_BUFFER_TOO_SMALL, cap, dst_len, 0);
    x.st = st;
    x.src = in + hdr;
    x.src_len = in_len - hdr;
    x.dst = (gptr)a.out_ptrs[st];
    x.dst_len = dst_len;
    x.slen = (uint32_t)x.src_len;
    x.dlen = (uint32_t)dst_len;
    x.s = x.d = x.ring_lo = 0;
    x.R.rg = ring_mem;
    x.R.dst = x.dst;
    x.R.lane = lane;
    x.R.gflush = 0;
    x.R.fenced = 0;
    return true;
}

// The end of a stream: what the wide path has in the ring is stored; an
// irregular stream is finished (and its error named) by the sequential
// decoder; HeaderMismatch, reference src/decompress.rs:149-157.
__device__ __forceinline__ void close_stream(const DecompressArgs &a,
                                             const uint32_t lane, Wide &x,
                                             const bool irregular)
{
    const uint64_t st = x.st;
    x.R.flush_partial(x.d);
    if (irregular) {
        decode_sequential(a, st, lane, x.src, x.src_len, x.dst, x.dst_len,
                          x.s, x.d);
        return;
    }
    PROF(
    if (lane == 0 && a.prof) {
        atomicAdd(&a.prof[7], (unsigned long long)x.n_win3);
        atomicAdd(&a.prof[8], (unsigned long long)x.n_run);
        atomicAdd(&a.prof[9], (unsigned long long)x.n_far);
        atomicAdd(&a.prof[10], (unsigned long long)x.n_win);
        atomicAdd(&a.prof[11], (unsigned long long)x.n_trip);
        atomicAdd(&a.prof[12], (unsigned long long)x.n_elem);
        atomicAdd(&a.prof[13], (unsigned long long)x.n_fence);
        atomicAdd(&a.prof[14], (unsigned long long)x.n_dep);
        atomicAdd(&a.prof[15], 1ull);
    }
    )
    if (x.d != x.dst_len)
        SNAPMI_FAIL(lane == 0, , SNAPMI_HEADER_MISMATCH, x.dst_len, x.d, 0);
    if (lane == 0) {
        set_error(a.errs, st, SNAPMI_OK, 0, 0, 0);
        a.out_lens[st] = x.dst_len;
    }
}
} // namespace

} // namespace snapmi
