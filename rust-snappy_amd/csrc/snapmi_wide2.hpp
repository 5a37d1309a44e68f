// snapmi_wide2.hpp -- the wavefront decoder's second-generation window loop
// (described in snapmi_wide.hpp): the last bytes of every stream in
// k_decompress_streams3, and all of k_decompress_streams2.
#pragma once

#include "snapmi_wide.hpp"

namespace snapmi {

namespace {
// The second-generation window loop from (x.s, x.d) to the end of the
// input.  True: something irregular, the sequential decoder takes over.
__device__ __forceinline__ bool decode_windows2(Wide &x, const uint32_t lane)
{
    gcptr src = x.src;
    gptr dst = x.dst;
    const uint64_t src_len = x.src_len;
    const uint32_t slen = x.slen, dlen = x.dlen;
    uint32_t s = x.s, d = x.d, ring_lo = x.ring_lo;
    Ring2 &R = x.R;
    l_u8 *const rg = R.rg;
    // streams too short for the 8-byte window loads go to the sequential
    // decoder at once; so does the first failed check
    bool irregular = src_len < 8;
    uint64_t w = irregular || s >= slen
                     ? 0
                     : ld64c(src, (uint64_t)s + lane, src_len); // src[s+lane..]
    while (!irregular && s < slen) {
        COUNT(x.n_win);
        // bytes of input left, as far as this window can see (<= 2^20)
        const uint32_t rem = slen - s < (1u << 20) ? slen - s : 1u << 20;
        // ---- 1. the element that would start at src[s + lane] ------------
        const uint32_t tag = (uint32_t)w & 0xFF;
        const uint32_t b14 = (uint32_t)(w >> 8); // the 4 bytes after the tag
        const uint32_t type = tag & 3, n6 = tag >> 2;
        const bool is_lit = type == 0;
        // The bytes behind the tag hold a little-endian number of nb bytes:
        // the rest of a literal's length (nb = 0..4, reference read_literal,
        // src/decompress.rs:161-228) or a copy's offset (nb = 1, 2, 4,
        // TagEntry::offset / read_copy, :233-250,433-474) - one extraction
        // for both (this loop is bound by VALU issue: every instruction that
        // goes is 0.4 % of the kernel)
        const uint32_t lnb = (n6 > 59 ? n6 : 59) - 59; // extra length bytes
        const uint32_t cnb = type + (type == 3);        // 1, 2, 4
        const uint32_t sh = 32 - 8 * (is_lit ? lnb : cnb);
        const uint32_t ext = (b14 << (sh & 31)) >> (sh & 31); // (nb = 0: unused)
        const uint32_t lraw = lnb ? ext : n6; // length - 1
        const uint32_t hd = 1 + lnb;
        // Predicates live as 64-bit lane masks in SGPRs and are combined
        // there: a __ballot of a compound per-lane bool costs two VALU
        // instructions on top of its compares (the bool is materialised and
        // compared again), a scalar AND of two simple ballots costs none.
        const uint64_t M_lit = __ballot(is_lit);
        // literals of more than 64 bytes: not in a window
        const uint64_t M_lng = M_lit & __ballot(lraw >= 64);
        const uint32_t clen = type == 1 ? 4 + (n6 & 7) : 1 + n6;
        const uint32_t off = ext | (type == 1 ? (tag & 0xE0u) << 3 : 0);
        const uint32_t olen = is_lit ? lraw + 1 : clen;      // if !lng
        const uint32_t enc = is_lit ? hd + lraw + 1 : 1 + cnb; // if !lng
        // the whole element lies inside the input (:189-217 src side, CopyRead)
        // (an extended literal length is read as 4 bytes: :189-198)
        // (a window with 160 bytes of input in front of it - all but the
        // last two or three of a stream - needs none of the per-lane tests:
        // lane + 5 + 64 + 16 <= rem whatever the element)
        const bool deep = rem >= 160;
        const uint64_t M_fits =
            deep ? ~M_lng
                 : ~M_lng & __ballot(lane < rem && enc <= rem - lane &&
                                     !(is_lit && lnb && lane + 5 > rem));
        // 16 literal bytes, speculatively (only windows well inside the input)
        const bool inner = rem >= 64 + 5 + 16;
        B16x lit16;
        // (uniform base + 32-bit lane offset: the load takes the base from
        // SGPRs and no 64-bit vector adds are spent on the address)
        const gcptr win_src = src + s;
        if (inner) {
            __builtin_memcpy(&lit16, win_src + (lane + hd), 16);
        } else {
            lit16.lo = lit16.hi = 0;
        }
        // ---- 2. element starts: the orbit of lane 0 under "next" ----------
        // A ds_bpermute costs the CU's one LDS pipeline about as much as
        // seven VALU instructions cost its four SIMDs (tests/hw/lds_cost.hip:
        // 6.4 cycles), so the discovery moves ONE dword per round: the wave
        // is two halves of 32 positions, and a lane's set R (32 bits, its own
        // half) holds the first nodes of its chain INCLUDING the frontier -
        // the node not yet expanded, which is the set's highest bit because
        // chains run forward.  One round: R |= R[frontier].  After k rounds a
        // set holds 2^k + 1 nodes; a half has at most 16 (every element has
        // two bytes or more), so four rounds finish it.  A lane whose element
        // ends its chain - long literal, behind the input, or reaching into
        // the other half / out of the window - has no frontier beyond itself
        // and fetches its own set.  The two halves are strung together by
        // the scalar unit afterwards.
        const uint32_t nx = lane + enc;
        const uint64_t T = M_lng | (deep ? 0 : __ballot(lane >= rem));
        const uint64_t M_stay = ~T & __ballot((nx ^ lane) < 32);
        uint32_t Rr = (1u << (lane & 31)) |
                      (__builtin_amdgcn_inverse_ballot_w64(M_stay)
                           ? 1u << (nx & 31)
                           : 0);
        const int c4 = (int)((lane | 31) << 2);
#pragma unroll
        for (uint32_t k = 0; k < 4; k++) {
            const int sel = c4 - 4 * (int)__builtin_clz(Rr);
            Rr |= (uint32_t)__builtin_amdgcn_ds_bpermute(sel, (int)Rr);
        }
        uint64_t S = rdlane(Rr, 0);
        {
            // the last start of the lower half: does its element lead into
            // the upper half?
            const uint32_t t0 = 31 - (uint32_t)__builtin_clz((uint32_t)S);
            const uint32_t nx0 = rdlane(nx, t0);
            if (!((T >> t0) & 1) && nx0 < kWave)
                S |= (uint64_t)rdlane(Rr, nx0) << 32;
        }
        // ---- 3. placement, window cut, checks ------------------------------
        const uint64_t M_elem = S & M_fits;
        const uint32_t o =
            __builtin_amdgcn_inverse_ballot_w64(M_elem) ? olen : 0;
        const uint32_t incl = wave_inclusive_add(o);
        // the window ends in front of the first start that is a long literal
        // or does not fit, and after kWinMax output bytes
        const uint64_t stop = S & ~M_fits;
        const uint64_t below =
            stop ? ((1ull << __builtin_ctzll(stop)) - 1) : ~0ull;
        const uint64_t K = M_elem & __ballot(incl <= kWinMax) & below;
        if (K == 0) {
            // lane 0 is a literal of more than 64 bytes: wave_copy
            const uint32_t lng0 = (uint32_t)M_lng & 1u;
            const uint64_t Lq = (uint64_t)rdlane(lraw, 0) + 1;
            const uint32_t h0 = rdlane(hd, 0);
            if (!lng0 || rem < h0 || slen - (s + h0) < Lq || dlen - d < Lq) {
                irregular = true; // the sequential decoder names the error
                break;
            }
            R.flush_partial(d);
            wave_copy<false>(dst + d, src + s + h0, Lq, lane);
            s += h0 + (uint32_t)Lq;
            d += (uint32_t)Lq;
            R.gflush = d;
            ring_lo = d; // these bytes are not in the ring
            if (s < slen)
                w = ld64c(src, (uint64_t)s + lane, src_len);
            continue;
        }
        const uint32_t last = 63 - (uint32_t)__builtin_clzll(K);
        const uint32_t W = rdlane(incl, last);         // output of the window
        const uint32_t cur = last + rdlane(enc, last); // input consumed
        const uint32_t dstp = d + (incl - o);          // element's position
        // reference checks :209-217 (dst side), :245-250, :327-332
        const uint64_t M_cpy = K & ~M_lit;
        if (W > dlen - d ||
            (M_cpy & (__ballot(off == 0) | __ballot(off > dstp))) != 0) {
            irregular = true;
            break;
        }
        PROF(
        x.n_elem += __builtin_popcountll(K);
        )
        // next window's bytes: issued now, consumed after the expand
        // (plain unaligned loads while the next window lies inside the
        // input - a uniform test; the clamped form only at the stream's end)
        uint64_t w_next;
        if (slen - s >= cur + kWave + 8)
            __builtin_memcpy(&w_next, src + (s + cur) + lane, 8);
        else
            w_next = ld64c(src, (uint64_t)s + cur + lane, src_len);

        // ---- 4. the lane-parallel copy step --------------------------------
        const uint32_t q = dstp - off;               // copy source (if cpy)
        // (a copy that a lane moves by itself does not overlap its source:
        // olen <= off, it reads olen bytes)
        const uint32_t qe = q + olen;
        // (whole 16-byte pieces are stored: up to 15 bytes behind the window's
        // output may be clobbered too)
        const uint32_t dW = d + W + 16;
        uint32_t safe_lo = dW > kRing2 ? dW - kRing2 : 0;
        safe_lo = safe_lo > ring_lo ? safe_lo : ring_lo;
        const uint64_t M_ring = __ballot(q >= safe_lo);
        // 16-byte loads from HBM must stay inside the buffers: an element
        // that ends within 15 bytes of the input's / the output's end is
        // left to the sweep, which moves exactly its bytes
        // (for a literal near the end of the input the exact figure, for a
        // copy from HBM 64: elements of a window have at most 64 bytes)
        // lanes that copy their element themselves: literals (with their 16
        // speculative bytes inside the input), copies whose whole source lies
        // in front of the window, in the ring's safe part or stored already
        const uint64_t M_litok =
            deep ? M_lit
                 : (inner ? M_lit & __ballot(lane + hd + ((olen + 15) & ~15u) <=
                                             rem)
                          : 0);
        const uint64_t M_src = __ballot(qe <= d) & __ballot(olen <= off);
        const uint64_t M_farok =
            dlen >= 64 ? __ballot(qe <= R.gflush) & __ballot(q <= dlen - 64)
                       : 0;
        const uint64_t M_lw =
            K &
            (M_litok | (~M_lit & M_src & (M_ring | M_farok)));
        const uint64_t M_far = M_lw & ~M_lit & ~M_ring; // source in HBM
        const uint64_t M_rng = M_lw & ~M_lit & M_ring;  // source in the ring
        {
            if (M_far) {
                PROF(
                x.n_far += __builtin_popcountll(M_far);
                )
                if ((M_far & __ballot(qe > R.fenced)) != 0) {
                    R.fence_for(0xFFFFFFFFu);
                    COUNT(x.n_fence);
                }
            }
            // Every lane stores WHOLE 16-byte pieces with one ds_write_b128:
            // the bytes past an element's end land on the following elements,
            // whose lanes are higher and whose stores of the same instruction
            // therefore win (overlapping lanes of one DS store are applied in
            // ascending lane order: tests/hw/lds_write_order.hip, checked at
            // context creation).  The pieces go last to first, so the excess
            // of an element's last piece is repaired by the first pieces of
            // its successors, which are all written by the last trip.
            const uint64_t M_g16 = M_lw & __ballot(olen > 16);
            const uint32_t top =
                M_g16 == 0 ? 0
                           : ((M_g16 & __ballot(olen > 48))
                                  ? 48
                                  : ((M_g16 & __ballot(olen > 32)) ? 32 : 16));
            // an element's own bytes wrap around the ring's end only in a
            // window whose output does (uniform)
            const bool wraps = (d & (kRing2 - 1)) + W > kRing2;
            for (uint32_t c = top;; c -= 16) {
                const uint64_t M_act = c == 0 ? M_lw : M_lw & __ballot(c < olen);
                if (M_act != 0) {
                    COUNT(x.n_trip);
                    // source: 16 bytes from the literal, the ring, or HBM
                    // (a lane that loads nothing below stores nothing either:
                    // whatever v starts with - the literal bytes of trip 0 -
                    // is never seen)
                    B16x v = lit16;
                    if (c != 0 && __builtin_amdgcn_inverse_ballot_w64(
                                      M_act & M_lit)) {
                        __builtin_memcpy(&v, win_src + (lane + hd + c), 16);
                    }
                    if ((M_act & M_far) != 0 &&
                        __builtin_amdgcn_inverse_ballot_w64(M_act & M_far))
                        __builtin_memcpy(&v, dst + (q + c), 16);
                    if (__builtin_amdgcn_inverse_ballot_w64(M_act & M_rng)) {
                        // (only the lanes that need it: the LDS serves a wave's
                        // scattered unaligned reads a few lanes per cycle)
                        // (one unaligned 16-byte read costs the LDS one
                        // cycle per lane, two 8-byte reads two:
                        // tests/hw/lds_cost.hip; it may run into the mirror)
                        __builtin_memcpy(&v, rg + ((q + c) & (kRing2 - 1)), 16);
                    }
                    const uint32_t wa = (dstp + c) & (kRing2 - 1);
                    // (rare) the element's own bytes wrap around the ring's
                    // end: those lanes store bytewise, after the others
                    uint64_t M_strad = 0;
                    uint32_t m = 16;
                    if (wraps) {
                        m = olen - c < 16 ? olen - c : 16;
                        M_strad = M_act & __ballot(wa + m > kRing2);
                    }
                    if (__builtin_amdgcn_inverse_ballot_w64(M_act & ~M_strad))
                        __builtin_memcpy(rg + wa, &v, 16); // may reach the mirror
                    if (M_strad != 0 &&
                        __builtin_amdgcn_inverse_ballot_w64(M_strad)) {
                        for (uint32_t j = 0; j < m; j++) {
                            const uint64_t part = j < 8 ? v.lo : v.hi;
                            rg[(wa + j) & (kRing2 - 1)] =
                                (uint8_t)(part >> (8 * (j & 7)));
                        }
                    }
                }
                if (c == 0)
                    break;
            }
        }
        // ---- 5. the sweep: elements that depend on this window -------------
        uint64_t dep = K & ~M_lw;
        while (dep) {
            COUNT(x.n_dep);
            const uint32_t i = (uint32_t)__builtin_ctzll(dep);
            dep &= dep - 1;
            const uint32_t ni = rdlane(olen, i), di = rdlane(dstp, i);
            uint32_t val = 0;
            if ((M_lit >> i) & 1) {
                // (only windows at the very end of the input, `inner` false)
                if (lane < ni)
                    val = src[s + i + rdlane(hd, i) + lane];
            } else {
                const uint32_t qi = rdlane(q, i), oi = rdlane(off, i);
                const uint32_t nsrc = ni < oi ? ni : oi;
                uint32_t kk = lane;
                if (oi < ni) { // overlapping: byte k repeats byte k mod oi
                    const uint32_t quo = (uint32_t)(
                        ((float)lane + 0.5f) *
                        __builtin_amdgcn_rcpf((float)oi));
                    kk = lane - quo * oi;
                }
                const bool in_ring = qi >= safe_lo;
                if (!in_ring) {
                    // bytes the ring has lost that are not stored yet (only
                    // right after a long literal): store them first
                    if (qi + nsrc > R.gflush)
                        R.flush_partial(di);
                    if (qi + nsrc > R.fenced) {
                        R.fence_for(0xFFFFFFFFu);
                        COUNT(x.n_fence);
                    }
                }
                if (lane < ni)
                    val = in_ring ? (uint32_t)rg[(qi + kk) & (kRing2 - 1)]
                                  : (uint32_t)dst[qi + kk];
            }
            if (lane < ni)
                rg[(di + lane) & (kRing2 - 1)] = (uint8_t)val;
        }
        // The mirror of ring[0,16) behind the ring's end, once per window (a
        // uniform test): the window's stores - whole 16-byte pieces, so up to
        // d + W + 16 - touched ring[0,16), or spilled over the end into the
        // mirror.  Within the window nobody reads through it what these
        // stores changed: such a source lies below safe_lo; the sweep and the
        // flush address the ring bytewise / dword-aligned.
        {
            const uint32_t a0 = d & (kRing2 - 1);
            if (a0 < 16 || a0 + W + 16 > kRing2)
                R.mirror();
        }
        // ---- 6. advance; whole 256-byte pieces go to HBM -------------------
        d += W;
        s += cur;
        w = w_next;
        R.flush_chunks(d);
    }
    x.s = s;
    x.d = d;
    x.ring_lo = ring_lo;
    return irregular;
}
} // namespace

} // namespace snapmi
