"""Round-level model of the lane match finder with up to four probes a round
(match_blocks in rust-snappy_amd/csrc/snapmi_lane.hip): one lane, one
block.  tests/model_match_lane.py stays the model of the plain and the
two-probe round; this one takes a depth of 1..4 and a round at which the depth
changes from 1 to `depth`, in the middle of a block or not.

A round of depth D, in the kernel's order:
  * the entry of the round's probe and the entries of the up to D - 1 probes
    that follow if it and its successors miss are read BEFORE anything the
    round writes.  A further probe exists only while its position is known at
    the start of the round - the skip schedule of src/compress.rs:207-216;
    after a copy, s + 1 - and while its 12 bytes lie in the 16 bytes the lane
    holds in registers: a cumulative distance of at most 3;
  * probe k sees what probes 0..k-1 of the round and the chain insert at
    s - 1 wrote, by forwarding, the newest write first;
  * an entry is written only when its probe is consumed; a probe that hits
    leaves the entries fetched behind it unused;
  * every consumed probe applies `s_next > s_limit`.
The per-lane state between rounds is the same at every depth, so the depth may
change between any two rounds.  The window, the stalls and the token buffers
are not modelled (they do not change what is computed).
tests/test_model_match_multi_cpu.py compares the stream the tokens encode to
with the oracle's."""
import numpy as np

from model_match_lane import _common, _put_copy, _put_literal

PROBE, CHAIN, EXTEND = 0, 1, 2


def _hashes(block, shift):
    """hash of the four bytes at every position (zero padded at the end)."""
    buf = np.frombuffer(bytes(block) + b"\0\0\0", dtype=np.uint8)
    w = (buf[:-3].astype(np.uint64) | buf[1:-2].astype(np.uint64) << 8 |
         buf[2:-1].astype(np.uint64) << 16 | buf[3:].astype(np.uint64) << 24)
    return (((w * 0x1E35A7BD) & 0xFFFFFFFF) >> shift).astype(np.int64).tolist()


def lane_tokens(block, depth=1, switch_round=0):
    """Tokens (literal_len, copy_len, offset) of one block of >= 17 bytes; the
    rounds it took; how many of them ran at a depth above 1.  Rounds
    0 .. switch_round - 1 run at depth 1 (None: all of them)."""
    assert 1 <= depth <= 4
    n = len(block)
    shift, tsize = 24, 256
    while tsize < 16384 and tsize < n:
        shift -= 1
        tsize *= 2
    s_limit = n - 15
    first12 = block[0:12]
    H = _hashes(block, shift)
    table = {}               # slot -> (12 bytes at the position, position)
    tokens = []
    s, s_next, skip, mode, next_emit = 1, 2, 33, PROBE, 0
    p = c = mpos = mcand = 0
    rounds = multi = 0

    def lookup(entry, bytes12):
        """(hit, cand, common length up to 12); entry None = the reference's
        fresh table: position 0."""
        cand_bytes, cand = (entry if entry is not None else (first12, 0))
        if cand_bytes[0:4] == bytes12[0:4]:
            return True, cand, _common(cand_bytes, bytes12, 12)
        return False, cand, 0

    while True:
        D = depth if switch_round is not None and rounds >= switch_round else 1
        rounds += 1
        multi += D > 1
        matched = advance = tail = finished = False
        mend = 0
        if mode <= CHAIN:
            was_chain = mode == CHAIN
            s0 = s
            hprev, hcur = H[s0 - 1], H[s0]
            # ---- the loads of the round, before any of its stores
            A = table.get(hcur)
            further = []         # (distance, slot, 12 bytes, entry as read)
            if D > 1:
                d = 1 if was_chain else s_next - s
                sk = 32 if was_chain else skip
                for _ in range(D - 1):
                    if d > 3:
                        break
                    at = s0 + d
                    h = H[at] if at < n else 0
                    further.append((d, h, block[at:at + 12], table.get(h)))
                    step = sk >> 5
                    d += step
                    sk += step
            # ---- what the round writes, oldest first; forwarded newest first
            written = []

            def forwarded(h, entry):
                for hh, e in reversed(written):
                    if hh == h:
                        return e
                return entry

            if was_chain:
                e_prev = (bytes(block[s0 - 1:s0 + 11]), s0 - 1)
                table[hprev] = e_prev
                written.append((hprev, e_prev))
            cur12 = bytes(block[s0:s0 + 12])
            hit, cand, m = lookup(forwarded(hcur, A), cur12)
            table[hcur] = (cur12, s0)
            written.append((hcur, (cur12, s0)))
            if not hit and was_chain:
                s_next, skip = s0 + 1, 32
            k = 0
            while True:
                if hit:
                    mpos, mcand = s, cand
                    if m < 12:
                        matched, mend = True, s + m
                    else:
                        p, c, mode = s + 12, cand + 12, EXTEND
                        tail = p + 16 > n
                    break
                if k == len(further):
                    advance = True
                    break
                # the probe missed: its advance, then the probe at the new s
                # with the entry fetched for it
                d, h, t, Ak = further[k]
                k += 1
                s = s_next
                step = skip >> 5
                s_next = s + step
                skip += step
                mode = PROBE
                assert s == s0 + d
                if s_next > s_limit:
                    finished = True
                    break
                assert len(t) == 12
                hit, cand, m = lookup(forwarded(h, Ak), t)
                e = (bytes(t), s)
                table[h] = e
                written.append((h, e))
        else:
            m = _common(block[c:c + 16], block[p:p + 16], 16)
            if m < 16:
                matched, mend = True, p + m
            else:
                p += 16
                c += 16
                tail = p + 16 > n
        if tail:
            while p < n and block[p] == block[c]:
                p += 1
                c += 1
            matched, mend = True, p
        if matched:
            tokens.append((mpos - next_emit, mend - mpos, mpos - mcand))
            s = mend
            next_emit = mend
            mode = CHAIN
            if s >= s_limit:
                finished = True
        if advance:
            s = s_next
            step = skip >> 5
            s_next = s + step
            skip += step
            mode = PROBE
            if s_next > s_limit:
                finished = True
        if finished:
            if next_emit < n:
                tokens.append((n - next_emit, 0, 0))
            return tokens, rounds, multi


def compress_one_block_stream(data, depth=1, switch_round=0):
    """The raw stream of an input of at most 65536 bytes; rounds; rounds at a
    depth above 1."""
    n = len(data)
    out = bytearray()
    v = n
    while v >= 128:
        out.append((v & 127) | 128)
        v >>= 7
    out.append(v)
    if n == 0:
        return bytes(out), 0, 0
    if n < 17:
        _put_literal(out, data)
        return bytes(out), 0, 0
    tokens, rounds, multi = lane_tokens(data, depth, switch_round)
    at = 0
    for lit, ln, off in tokens:
        if lit:
            _put_literal(out, data[at:at + lit])
            at += lit
        if ln:
            _put_copy(out, off, ln)
            at += ln
    assert at == n
    return bytes(out), rounds, multi
