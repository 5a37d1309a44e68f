// snapmi_wide3.hpp -- the wavefront decoder's third-generation window loop,
// the default: 256 compressed bytes per window, one ELEMENT per lane.
#pragma once

#include "snapmi_wide.hpp"

namespace snapmi {

namespace {
// ---------------------------------------------------------------------
// The third-generation window loop: kG3 x 64 compressed bytes per window,
// one ELEMENT per lane.
//
// The second generation spends its instructions on lanes that hold no
// element: every lane decodes "the element that would start at my byte" in
// full (offset, length, checks, source classes), and one lane in four or five
// is a real start.  Instruction issue - vector and scalar - is what bounds
// the loop, so here the expensive part runs on real elements only:
//
//   1. LENGTHS.  A window is kG3 groups of 64 input bytes; lane l looks at
//      the TAG bytes at s + 64 g + l, just far enough to know how many
//      compressed bytes the element there would take (tag only: a literal
//      with length bytes - 61 bytes or more - always ends a window).
//   2. STARTS.  Per group one ds_bpermute per round, four rounds (a lane's
//      32-bit set of its 32-byte sub-window, frontier as the highest bit:
//      R |= R[frontier]); the 2 kG3 sub-windows are strung together by the
//      scalar unit (two v_readlane each).
//   3. COMPACTION.  The t-th start of the window goes to lane t: rank by
//      population count, position through a 64 kG3-byte table in LDS.
//   4. DECODE, PLACEMENT, CHECKS as in the second generation, but every lane
//      below the element count holds a real element (40 of 64 lanes on the
//      corpus instead of 14).
//   5. COPY.  Every element whose source is complete before the window -
//      literals, copies from in front of it - is copied by its lane, as in
//      the second generation: 16 bytes per trip, whole-piece stores resolved
//      by lane order, the far sources of the whole window requested at once.
//      Then the LATE elements - copies that read the window's own output
//      (2.3 per window on text, 8 on html) or overlap themselves - are moved
//      one by one, in stream order, by the whole wave (lane k = byte k).
//
// A window needs kTail3 bytes of input in front of it, so that none of its
// loads can leave the input; the last bytes of a stream (and streams shorter
// than that) are decode_windows2's.  True: something irregular.
// ---------------------------------------------------------------------
#define SNAPMI_G3 4
constexpr uint32_t kG3 = SNAPMI_G3;
static_assert(kG3 == 2 || kG3 == 4,
              "positions in a window are masked with 64 kG3 - 1; 8 groups do "
              "not fit 64 VGPRs");
// the last position (64 kG3 - 1), a tag, 60 literal bytes read as whole
// 16-byte pieces
constexpr uint32_t kTail3 = 64 * kG3 + 1 + 64 + 16;

__device__ __forceinline__ bool decode_windows3(Wide &x, const uint32_t lane,
                                                l_u8 *const postab)
{
    gcptr src = x.src;
    gptr dst = x.dst;
    const uint32_t slen = x.slen, dlen = x.dlen;
    uint32_t s = x.s, d = x.d, ring_lo = x.ring_lo;
    Ring2 &R = x.R;
    l_u8 *const rg = R.rg;
    bool irregular = false;
    uint32_t tg[kG3]; // tag bytes of the window at s, one per group
    bool have = false;
    const int c4 = (int)((lane | 31) << 2);
    const uint32_t self = 1u << (lane & 31);

    while (slen - s >= kTail3) {
        COUNT(x.n_win3);
        const gcptr win_src = src + s;
        if (!have) {
#pragma unroll
            for (uint32_t g = 0; g < kG3; g++)
                tg[g] = win_src[64 * g + lane];
        }
        // ---- 1. lengths, 2. starts -------------------------------------
        uint32_t nx[kG3], Rr[kG3];
#pragma unroll
        for (uint32_t g = 0; g < kG3; g++) {
            const uint32_t t = tg[g], type = t & 3;
            const uint32_t pos = 64 * g + lane;
            // copies take 2, 3, 5 bytes; a literal its tag and n6 + 1 bytes;
            // a literal with length bytes (n6 >= 60) ends every chain: its
            // "next" lies behind the window
            uint32_t enc =
                type ? (0x05030200u >> (8 * type)) & 0xFF : (t >> 2) + 2;
            enc = (t & 0xF3) == 0xF0 ? 255 : enc;
            nx[g] = pos + enc;
            // (the chain stays in this lane's 32-byte sub-window)
            Rr[g] = self | ((nx[g] ^ pos) < 32 ? 1u << (nx[g] & 31) : 0);
        }
#pragma unroll
        for (uint32_t k = 0; k < 4; k++) {
#pragma unroll
            for (uint32_t g = 0; g < kG3; g++) {
                const int sel = c4 - 4 * (int)__builtin_clz(Rr[g]);
                Rr[g] |= (uint32_t)__builtin_amdgcn_ds_bpermute(sel,
                                                                (int)Rr[g]);
            }
        }
        // the sub-windows, strung together: sub-window k is entered at its
        // byte e; its last start's element leads into a later one (or out
        // of the window)
        uint32_t S32[2 * kG3];
#pragma unroll
        for (uint32_t kk = 0; kk < 2 * kG3; kk++)
            S32[kk] = 0;
        {
            uint32_t k = 0, e = 0;
#pragma unroll
            for (uint32_t kk = 0; kk < 2 * kG3; kk++) {
                if (k == kk) {
                    const uint32_t g = kk >> 1, half = 32 * (kk & 1);
                    const uint32_t Sk = rdlane(Rr[g], half + e);
                    S32[kk] = Sk;
                    const uint32_t lt = 31 - (uint32_t)__builtin_clz(Sk);
                    const uint32_t nxa = rdlane(nx[g], half + lt);
                    k = nxa >> 5;
                    e = nxa & 31;
                }
            }
        }
        uint64_t S[kG3];
#pragma unroll
        for (uint32_t g = 0; g < kG3; g++)
            S[g] = ((uint64_t)S32[2 * g + 1] << 32) | S32[2 * g];
        // ---- 3. compaction ---------------------------------------------
        uint32_t base = 0;
#pragma unroll
        for (uint32_t g = 0; g < kG3; g++) {
            // (a lane that is no start writes behind the table: a select is
            // cheaper than an exec region - the scalar unit is what is short)
            const uint32_t r = __builtin_amdgcn_inverse_ballot_w64(S[g])
                                   ? base + popc_below(S[g])
                                   : 64 * kG3 + lane;
            postab[r] = (uint8_t)(64 * g + lane);
            base += (uint32_t)__builtin_popcountll(S[g]);
        }
        const uint32_t n_el = base < kWave ? base : kWave;
        const uint64_t M_act = n_el == kWave ? ~0ull : (1ull << n_el) - 1;
        // (lanes behind the last element read what an earlier window left:
        // any position in the window will do, they are masked by M_act)
        const uint32_t pos = postab[lane] & (64 * kG3 - 1);
        // ---- 4. the element, in full -----------------------------------
        uint64_t w;
        __builtin_memcpy(&w, win_src + pos, 8);
        B16x lit16;
        __builtin_memcpy(&lit16, win_src + (pos + 1), 16);
        const uint32_t tag = (uint32_t)w & 0xFF;
        const uint32_t b14 = (uint32_t)(w >> 8); // the 4 bytes after the tag
        const uint32_t type = tag & 3, n6 = tag >> 2;
        const uint64_t M_lit = __ballot(type == 0);
        const uint64_t M_lng = M_act & M_lit & __ballot(n6 >= 60);
        // a copy's offset: 1, 2 or 4 bytes behind the tag (TagEntry::offset /
        // read_copy, reference src/decompress.rs:233-250,433-474)
        const uint32_t cnb = type + (type == 3);
        const uint32_t sh = 32 - 8 * cnb;
        const uint32_t ext = (b14 << (sh & 31)) >> (sh & 31);
        const uint32_t off = ext | (type == 1 ? (tag & 0xE0u) << 3 : 0);
        // output bytes: a literal's and a long copy's n6 + 1, copy-1's 4..11
        const uint32_t olen = type == 1 ? 4 + (n6 & 7) : 1 + n6;
        const uint32_t enc = type == 0 ? n6 + 2 : 1 + cnb;
        const uint64_t M_el = M_act & ~M_lng;
        const uint32_t o =
            __builtin_amdgcn_inverse_ballot_w64(M_el) ? olen : 0;
        const uint32_t incl = wave_inclusive_add(o);
        // the window ends in front of a literal with length bytes, and after
        // kWinMax output bytes
        const uint64_t below =
            M_lng ? ((1ull << __builtin_ctzll(M_lng)) - 1) : ~0ull;
        const uint64_t K = M_el & __ballot(incl <= kWinMax) & below;
        if (K == 0) {
            // lane 0 is a literal with length bytes (reference read_literal,
            // src/decompress.rs:161-228): moved by the whole wave
            const uint32_t lnb = rdlane(n6, 0) - 59; // 1..4 length bytes
            const uint32_t b0 = rdlane(b14, 0);
            const uint64_t Lq =
                (uint64_t)(lnb == 4 ? b0 : b0 & ((1u << (8 * lnb)) - 1)) + 1;
            const uint32_t h0 = 1 + lnb;
            if (slen - (s + h0) < Lq || dlen - d < Lq) {
                irregular = true; // the sequential decoder names the error
                break;
            }
            R.flush_partial(d);
            wave_copy<false>(dst + d, src + s + h0, Lq, lane);
            s += h0 + (uint32_t)Lq;
            d += (uint32_t)Lq;
            R.gflush = d;
            ring_lo = d; // these bytes are not in the ring
            have = false;
            continue;
        }
        // (K is a prefix of the lanes)
        const uint32_t nK = (uint32_t)__builtin_popcountll(K);
        const uint32_t W = rdlane(incl, nK - 1);       // output of the window
        const uint32_t cur = rdlane(pos, nK - 1) + rdlane(enc, nK - 1);
        const uint32_t dstp = d + (incl - o);          // element's position
        // reference checks :209-217 (dst side), :245-250, :327-332
        const uint64_t M_cpy = K & ~M_lit;
        if (W > dlen - d ||
            (M_cpy & (__ballot(off == 0) | __ballot(off > dstp))) != 0) {
            irregular = true;
            break;
        }
        PROF(
        x.n_elem += nK;
        )
        // next window's tags: issued now, consumed after the copy step
        uint32_t tgn[kG3];
        const bool have_next = slen - (s + cur) >= kTail3;
        if (have_next) {
#pragma unroll
            for (uint32_t g = 0; g < kG3; g++)
                tgn[g] = win_src[cur + 64 * g + lane];
        } else {
#pragma unroll
            for (uint32_t g = 0; g < kG3; g++)
                tgn[g] = 0;
        }
        // ---- 5. the copy step, in in-order runs ------------------------
        const uint32_t q = dstp - off; // copy source (if cpy)
        const uint32_t qe = q + olen;  // (its end, for a copy that does not
                                       // overlap itself)
        // (whole 16-byte pieces are stored: up to 15 bytes behind the window's
        // output may be clobbered too)
        const uint32_t dW = d + W + 16;
        uint32_t safe_lo = dW > kRing2 ? dW - kRing2 : 0;
        safe_lo = safe_lo > ring_lo ? safe_lo : ring_lo;
        const uint64_t M_ring = __ballot(q >= safe_lo);
        // A source in HBM must have been stored, and its 16-byte loads must
        // stay inside the buffer.  Both hold by construction while the ring
        // is whole (a far source ends 1968 bytes or more in front of d, the
        // stores lag d by less than 256); only behind a long literal, whose
        // bytes are not in the ring, must the lanes be asked.
        const bool whole = ring_lo + kRing2 <= dW;
        const uint64_t M_farok =
            whole ? ~0ull
                  : (dlen >= 64 ? __ballot(qe <= R.gflush) &
                                      __ballot(q <= dlen - 64)
                                : 0);
        // LATE elements are moved one by one, in stream order, by the whole
        // wave, after everything else: copies that read this window's own
        // output (qe > d: that includes a copy that overlaps itself) and
        // sources neither in the ring nor stored.  (2.3 per window on text,
        // 8 on html: a loop of in-order RUNS of lanes - whole-piece stores
        // per run - was measured first and cost the scalar unit five times
        // as much per dependent element.)
        const uint64_t M_late =
            M_cpy & (__ballot(qe > d) | ~(M_ring | M_farok));
        const uint64_t M_lw = K & ~M_late; // copied by their own lanes, now
        // an element's own bytes wrap around the ring's end only in a
        // window whose output does (uniform)
        const uint32_t r0 = d & (kRing2 - 1);
        const bool wraps = r0 + W > kRing2;
        const uint64_t M_far = M_lw & M_cpy & ~M_ring; // source in HBM
        const uint64_t M_rng = M_lw & M_cpy & M_ring;  // ... in the ring
        // The first piece of every element whose source is not in the ring:
        // literal bytes are here already (lit16); far sources are an L2 miss
        // each (64 bytes from HBM or the MALL, a microsecond or two), and
        // that latency is what a wave waits for most - all of them at once.
        B16x v0 = lit16;
        if (M_far) {
            PROF(
            x.n_far += __builtin_popcountll(M_far);
            )
            // sources in HBM must be completed stores
            if ((M_far & __ballot(qe > R.fenced)) != 0) {
                R.fence_for(0xFFFFFFFFu);
                COUNT(x.n_fence);
            }
            if (__builtin_amdgcn_inverse_ballot_w64(M_far))
                __builtin_memcpy(&v0, dst + q, 16);
        }
        // Every lane stores WHOLE 16-byte pieces with one ds_write_b128 per
        // trip, last piece first; the excess of a short element lands on
        // the elements behind it - higher lanes of the same instruction,
        // which win (see decode_windows2), or late elements, which are
        // written afterwards.
        const uint64_t M_g16 = M_lw & __ballot(olen > 16);
        if (!wraps && M_g16 == 0) {
            // the usual window: one piece per element, no wrap
            COUNT(x.n_trip);
            B16x v = v0;
            if (__builtin_amdgcn_inverse_ballot_w64(M_rng))
                __builtin_memcpy(&v, rg + (q & (kRing2 - 1)), 16);
            if (__builtin_amdgcn_inverse_ballot_w64(M_lw))
                __builtin_memcpy(rg + (dstp & (kRing2 - 1)), &v, 16);
        } else {
            const uint32_t top =
                M_g16 == 0 ? 0
                           : ((M_g16 & __ballot(olen > 48))
                                  ? 48
                                  : ((M_g16 & __ballot(olen > 32)) ? 32 : 16));
            for (uint32_t c = top;; c -= 16) {
                const uint64_t M_actc =
                    c == 0 ? M_lw : M_lw & __ballot(c < olen);
                if (M_actc != 0) {
                    COUNT(x.n_trip);
                    B16x v = v0;
                    if (c != 0) {
                        if (__builtin_amdgcn_inverse_ballot_w64(M_actc & M_lit))
                            __builtin_memcpy(&v, win_src + (pos + 1 + c), 16);
                        if ((M_actc & M_far) != 0 &&
                            __builtin_amdgcn_inverse_ballot_w64(M_actc & M_far))
                            __builtin_memcpy(&v, dst + (q + c), 16);
                    }
                    if (__builtin_amdgcn_inverse_ballot_w64(M_actc & M_rng))
                        __builtin_memcpy(&v, rg + ((q + c) & (kRing2 - 1)),
                                         16);
                    const uint32_t wa = (dstp + c) & (kRing2 - 1);
                    // (rare) the element's own bytes wrap around the ring's
                    // end: those lanes store bytewise, after the others
                    uint64_t M_strad = 0;
                    uint32_t m = 16;
                    if (wraps) {
                        m = olen - c < 16 ? olen - c : 16;
                        M_strad = M_actc & __ballot(wa + m > kRing2);
                    }
                    if (__builtin_amdgcn_inverse_ballot_w64(M_actc & ~M_strad))
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
        // the late elements: lane k = byte k of the element (exactly its
        // bytes, addressed bytewise: no mirror)
        uint64_t late = M_late;
        if ((M_late & ~M_ring) == 0) {
            // (the usual case: every late source is in the ring)
            while (late) {
                COUNT(x.n_dep);
                const uint32_t i = (uint32_t)__builtin_ctzll(late);
                late &= late - 1;
                const uint32_t F = rdlane(dstp, i), ni = rdlane(olen, i);
                const uint32_t qi = rdlane(q, i), oi = F - qi;
                uint32_t kk = lane;
                if (oi < ni) { // overlapping: byte k repeats byte k mod oi
                    const uint32_t quo = (uint32_t)(
                        ((float)lane + 0.5f) *
                        __builtin_amdgcn_rcpf((float)oi));
                    kk = lane - quo * oi;
                }
                if (lane < ni)
                    rg[(F + lane) & (kRing2 - 1)] =
                        rg[(qi + kk) & (kRing2 - 1)];
            }
        }
        while (late) {
            COUNT(x.n_dep);
            const uint32_t i = (uint32_t)__builtin_ctzll(late);
            late &= late - 1;
            const uint32_t F = rdlane(dstp, i), ni = rdlane(olen, i);
            const uint32_t qi = rdlane(q, i), oi = F - qi;
            uint32_t kk = lane;
            if (oi < ni) { // overlapping: byte k repeats byte k mod oi
                const uint32_t quo = (uint32_t)(
                    ((float)lane + 0.5f) * __builtin_amdgcn_rcpf((float)oi));
                kk = lane - quo * oi;
            }
            const bool in_ring = qi >= safe_lo;
            if (!in_ring) {
                const uint32_t nsrc = ni < oi ? ni : oi;
                // bytes the ring has lost that are not stored yet (only
                // right after a long literal): store them first
                if (qi + nsrc > R.gflush)
                    R.flush_partial(F);
                if (qi + nsrc > R.fenced) {
                    R.fence_for(0xFFFFFFFFu);
                    COUNT(x.n_fence);
                }
            }
            if (lane < ni) {
                const uint32_t val =
                    in_ring ? (uint32_t)rg[(qi + kk) & (kRing2 - 1)]
                            : (uint32_t)dst[qi + kk];
                rg[(F + lane) & (kRing2 - 1)] = (uint8_t)val;
            }
        }
        // the mirror for the next window (see decode_windows2)
        if (r0 < 16 || r0 + W + 16 > kRing2)
            R.mirror();
        // ---- 6. advance; whole 256-byte pieces go to HBM -----------------
        d += W;
        s += cur;
#pragma unroll
        for (uint32_t g = 0; g < kG3; g++)
            tg[g] = tgn[g];
        have = have_next;
        R.flush_chunks(d);
    }
    x.s = s;
    x.d = d;
    x.ring_lo = ring_lo;
    return irregular;
}
} // namespace

} // namespace snapmi
