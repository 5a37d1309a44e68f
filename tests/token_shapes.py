"""Inputs built to land on the places where the compressors' token path makes
a decision, and the parser that proves they do - TEST INFRASTRUCTURE, pure
Python, no GPU.

The token path (rust-snappy_amd/csrc/snapmi_lane.hip, snapmi_window.hpp) hands
k_encode_tokens the reference's greedy parse as tokens (literal, copy,
offset): four bytes each in pages of 512, the ones that do not fit (literal
>= 1 024, copy > 64) in an exception list in pages of 256.  tokens() reads
that parse back out of a compressed stream, so a test can say how many
tokens, how many exceptions and which lengths an input really holds - the
oracle decides, not the builder's intention.

The builders do not compute the reference's probe schedule (the stride of
the skip loop grows with every miss, src/compress.rs:207-216): they lay out
bytes that SHOULD parse to a planned token list, ask the oracle
(oracle_lib.compress) and keep a block only when tokens() of the oracle's
stream IS the plan, token for token.  A length the schedule never probes is
found that way to be unreachable and the nearest reachable one is taken on
each side of the threshold (REACHABLE below; literal_edges() searches,
tests/test_token_shapes_cpu.py compares and prints).

Families (the_set()): "grid" - one token at every literal edge x copy edge x
offset edge the parse can reach, as the first token of a block, in its
middle and in front of its final literal, in blocks of 4-8 KiB and of more
than 8 KiB; "dense" - 64 KiB blocks of more than 15 000 tokens; "exceptions"
- 64 KiB blocks of more than 800 exceptions, the three kinds mixed, and an
exception at token 63, 64, 511 and 512; "streams" - blocks of the three in
streams of 2, 3 and 5 blocks.
"""
import functools
import random

import oracle_lib as O

BLOCK = 65536
EXC_LITERAL, EXC_COPY = 1024, 64    # literal >= / copy > : an exception
TOK_PAGE, EXC_PAGE = 512, 256       # kTokPage, kExcPage


# ---------------------------------------------------------------- the parser
def _varint(n):
    out = bytearray()
    while n >= 0x80:
        out.append((n & 0x7F) | 0x80)
        n >>= 7
    out.append(n)
    return bytes(out)


def elements(compressed):
    """(kind, length, offset) of every element of a raw Snappy stream; kind 0
    is a literal (offset 0), 1 / 2 / 3 a copy with 1 / 2 / 4 offset bytes."""
    buf = bytes(compressed)
    s = 0
    while buf[s] >= 0x80:
        s += 1
    s += 1
    out = []
    n = len(buf)
    while s < n:
        tag = buf[s]
        s += 1
        kind = tag & 3
        if kind == 0:
            length = (tag >> 2) + 1
            if length > 60:
                nb = length - 60
                length = int.from_bytes(buf[s:s + nb], "little") + 1
                s += nb
            out.append((0, length, 0))
            s += length
        elif kind == 1:
            out.append((1, 4 + ((tag >> 2) & 7), (tag >> 5) << 8 | buf[s]))
            s += 1
        elif kind == 2:
            out.append((2, (tag >> 2) + 1, buf[s] | buf[s + 1] << 8))
            s += 2
        else:
            out.append((3, (tag >> 2) + 1,
                        int.from_bytes(buf[s:s + 4], "little")))
            s += 4
    assert s == n, (s, n)
    return out


def tokens(compressed):
    """The greedy parse behind a raw Snappy stream the reference's encoder
    wrote: a list of tokens (literal, copy, offset), copy 0 for a literal
    with no copy behind it (a block's last bytes).

    A literal element opens a token.  Consecutive copy elements with the same
    offset, where the piece before was one of 64 or 60 bytes, are ONE match:
    emit_copy (src/compress.rs:323-357) cuts a match of more than 64 bytes
    into such pieces.  The merge is exact, not a guess: a match is maximal -
    it ends where the next byte differs from the byte `offset` back, or at
    the block's end - so it cannot be followed directly by another match at
    the same offset (that would be the same match going on), and behind a
    block's end the next block begins with a literal."""
    out = []
    lit = None          # an open literal without its copy yet
    merge = False       # the element before was a copy piece of 64 or 60
    for kind, n, off in elements(compressed):
        if kind == 0:
            if lit is not None:
                out.append((lit, 0, 0))
            lit, merge = n, False
            continue
        if merge and lit is None and out[-1][2] == off:
            out[-1] = (out[-1][0], out[-1][1] + n, off)
        else:
            out.append((lit or 0, n, off))
        lit, merge = None, n in (64, 60)
    if lit is not None:
        out.append((lit, 0, 0))
    return out


def block_tokens(compressed):
    """tokens() cut into the 64 KiB blocks of the input (no token crosses
    one: every block is compressed on its own)."""
    blocks, cur, covered = [], [], 0
    for t in tokens(compressed):
        cur.append(t)
        covered += t[0] + t[1]
        assert covered <= BLOCK, covered
        if covered == BLOCK:
            blocks.append(cur)
            cur, covered = [], 0
    if cur:
        blocks.append(cur)
    return blocks


def is_exception(tok):
    return tok[0] >= EXC_LITERAL or tok[1] > EXC_COPY


def exceptions(toks):
    return sum(1 for t in toks if is_exception(t))


def pages(toks):
    """Pool pages the token path needs for a block of these tokens at the
    least: ceil(tokens / 512) + ceil(exceptions / 256)."""
    return -(-len(toks) // TOK_PAGE) + -(-exceptions(toks) // EXC_PAGE)


def token_parts(L, C, O):
    """The reference's emit rules for one token (emit_literal,
    src/compress.rs:433-474; emit_copy, :323-369) as the arithmetic
    token_bytes() and TokenSink::flush() of snapmi_compress_dev.hpp carry:
    (literal tag bytes, copies of 64, copies of 60, last piece's length, last
    piece's bytes)."""
    lt = 0 if L == 0 else (1 if L <= 60 else (2 if L <= 256 else 3))
    n64 = (C - 4) >> 6 if C >= 68 else 0
    rem = C - (n64 << 6)
    mid = 1 if rem > 64 else 0
    fin_len = rem - 60 * mid
    fin = 0 if C == 0 else (2 if fin_len <= 11 and O <= 2047 else 3)
    return lt, n64, mid, fin_len, fin


def encode(data, toks):
    """The stream of `data` from its tokens by the emit rules above, in plain
    Python: what tokens() took apart, put together again."""
    out = bytearray(_varint(len(data)))
    at = 0
    for L, C, O in toks:
        lt, n64, mid, fin_len, fin = token_parts(L, C, O)
        if lt == 1:
            out.append((L - 1) << 2)
        elif lt == 2:
            out += bytes((60 << 2, L - 1))
        elif lt == 3:
            out += bytes((61 << 2, (L - 1) & 255, (L - 1) >> 8))
        out += data[at:at + L]
        at += L + C
        out += bytes((63 << 2 | 2, O & 255, O >> 8)) * n64
        out += bytes((59 << 2 | 2, O & 255, O >> 8)) * mid
        if fin == 2:
            out += bytes(((O >> 8) << 5 | (fin_len - 4) << 2 | 1, O & 255))
        elif fin == 3:
            out += bytes(((fin_len - 1) << 2 | 2, O & 255, O >> 8))
    assert at == len(data), (at, len(data))
    return bytes(out)


# --------------------------------------------------------------- the builder
class _Builder:
    """Bytes that should parse to self.plan.  token(L, C, O): L fresh random
    bytes, then C bytes equal to those O back, then a byte that differs - so
    the match is C long if the parse finds it at that position at all, which
    it does only if the position is one the skip loop probes and the source
    one it inserted; the caller asks the oracle."""

    def __init__(self, rng, n):
        self.rng = rng
        self.n = n          # the block's final length: it sizes the table
        self.buf = bytearray()
        self.plan = []
        self.avoid = None   # the byte that would make the last copy longer

    def _fresh(self, n):
        lit = bytearray(self.rng.randbytes(n))
        while n and lit[0] == self.avoid:
            lit[0] = self.rng.randrange(256)
        return lit

    def token(self, L, C, O):
        """False: no such token here (its source would lie before the
        block).  O "max": the largest offset there is, the block's start."""
        buf = self.buf
        p = len(buf) + L
        if O == "max":
            O = p
        q = p - O
        if O < 1 or q < 0:
            return False
        buf += self._fresh(L)
        if L and q >= 1:
            # the byte in front of the copy differs from the one in front of
            # its source: the match does not begin a byte early
            bad = {buf[q - 1]} | ({self.avoid} if L == 1 else set())
            while buf[p - 1] in bad:
                buf[p - 1] = self.rng.randrange(256)
        if C <= O:
            buf += buf[p - O:p - O + C]
        else:                   # an overlapping run
            for _ in range(C):
                buf.append(buf[len(buf) - O])
        self.avoid = buf[len(buf) - O]
        self.plan.append((L, C, O))
        return True

    def unit(self, u, longest=8):
        """One short token of u bytes in all (10 <= u <= 30 + longest): a
        literal of 6 to 30 bytes - the skip loop probes every position of it
        - and a copy of 4 to `longest` bytes of that literal's second byte
        on."""
        c = self.rng.randrange(max(4, u - 30), min(longest, u - 6) + 1)
        ok = self.token(u - c, c, u - c - 1)
        assert ok

    def filler(self, nbytes):
        """nbytes (>= 10) of such tokens, ending with a copy.  Laid out some
        1 500 bytes at a time and each stretch shown to the oracle (two
        strings may share a slot of the hash table, and then a source is
        gone): one that does not parse to its plan is made again."""
        assert nbytes >= 10, nbytes

        def stretch(left):
            while left:
                if left > 180:
                    u = self.rng.randrange(14, 91)
                elif left > 90:
                    u = left // 2
                else:
                    u = left
                self.unit(u, 60)
                left -= u
        while nbytes:
            now = nbytes if nbytes < 2000 else 1500
            self._confirmed(lambda: stretch(now))
            nbytes -= now

    def units(self, count):
        """`count` tokens of 12 to 19 bytes, confirmed 64 at a time."""
        while count:
            now = min(count, 64)
            self._confirmed(lambda: [self.unit(self.rng.randrange(12, 20))
                                     for _ in range(now)])
            count -= now

    def _confirmed(self, make):
        keep = len(self.buf), len(self.plan), self.avoid
        for attempt in range(50):
            make()
            if attempt == 49 or self.prefix_ok():
                return          # (the 50th: as it is, ok() will say no)
            del self.buf[keep[0]:]
            del self.plan[keep[1]:]
            self.avoid = keep[2]

    def prefix_ok(self):
        """The oracle parses what is there so far to the plan, in a block
        with the table of the final one (random bytes behind it up to the
        length that gives that table: src/compress.rs:491-518)."""
        m = self.n if self.n <= 8192 else 8193
        pad = max(m - len(self.buf), 20)
        if len(self.buf) + pad > self.n:
            return True     # the end of the block: ok() decides
        tail = self._fresh(pad)
        got = tokens(O.compress(bytes(self.buf + tail)))
        return got == self.plan + [(pad, 0, 0)]

    def final(self, F):
        if F:
            self.buf += self._fresh(F)
            self.plan.append((F, 0, 0))
        self.avoid = None

    def ok(self):
        """The oracle parses the bytes to the plan, token for token."""
        return tokens(O.compress(bytes(self.buf))) == self.plan


# ------------------------------------------------------------------ the grid
LIT_THRESHOLDS = ((60, 61), (64, 65), (256, 257), (1023, 1024))
COPY_EDGES = (4, 11, 12, 64, 65, 67, 68, 71, 72, 75, 76)
OFFSET_EDGES = (1, 2, 3, 4, 2047, 2048, "max")
# the final literal behind the last copy: none, and lengths on both sides of
# the encoder's 16-byte pieces and of its lane copy (a final literal of up to
# 64 bytes that is no multiple of 16 takes the encoder's slow path, P + Lp > n
# in TokenSink::flush(); a literal with a copy behind it never does - the copy
# and what follows are 16 bytes at the least, src/compress.rs:20)
FINALS = (0, 1, 15, 16, 17, 64, 65)
PLACES = ("first", "middle", "last")

# The literal lengths the reference's parse can give a token WITH a copy next
# to each threshold, (nearest at or below the lower side, nearest at or above
# the upper side), as literal_edges() finds them with the oracle; the CPU test
# asserts that the search still finds exactly these and prints them.  The skip
# loop probes every position for 32 misses, then every 2nd for 16, every 3rd
# ...: behind a match (and at a block's start, where the first probe is
# position 1) a literal of 60 or 64 bytes cannot end in a copy - 59 / 61 and
# 63 / 65 are the sides that exist - nor one of 256, 1 023 or 1 024.  The
# lengths 60, 64, 256, 1 023 and 1 024 themselves occur only as a block's
# FINAL literal (no copy), which the "final" family below builds at each.
REACHABLE = {
    "first": {(60, 61): (59, 61), (64, 65): (63, 65),
              (256, 257): (254, 262), (1023, 1024): (999, 1031)},
    "after_match": {(60, 61): (59, 61), (64, 65): (63, 65),
                    (256, 257): (254, 262), (1023, 1024): (999, 1031)},
}


def _block(rng, n, first=None, middle=None, last=None, final=20, lead=None):
    """A block of n bytes: the token `first` at its start, `middle` behind at
    least `lead` bytes (2 100 by default: offsets of 2 048 exist there),
    `last` in front of the final literal of `final` bytes, short tokens
    between them.  Returns the builder, or None when it cannot be laid out
    or the oracle does not confirm `first` or `middle` where they end."""
    b = _Builder(rng, n)
    b.marks = {}
    if first is not None:
        b.marks["first"] = 0
        if not b.token(*first) or not b.prefix_ok():
            return None
    if lead is None:
        lead = 2100
    if middle is not None:
        at = max(lead, len(b.buf) + 40 + middle[0])
        if middle[2] != "max" and middle[2] > middle[0] + 1:
            # its source behind what is there already
            at = max(at, len(b.buf) + 10 + middle[2])
        _fill_to(b, at - middle[0], middle)
        b.marks["middle"] = len(b.plan)
        if not b.token(*middle) or not b.prefix_ok():
            return None
    end = n - final - (last[0] + last[1] if last else 0)
    if end - len(b.buf) < 10:
        return None
    _fill_to(b, end, last)
    if last is not None:
        b.marks["last"] = len(b.plan)
        if not b.token(*last):
            return None
    b.final(final)
    assert len(b.buf) == n
    return b


def _fill_to(b, end, tok):
    """Short tokens up to position `end`, where the token `tok` is to begin.
    Where its source lies inside them, one of their copies ends exactly
    there: the parse inserts that position whatever else it does."""
    if tok is not None and tok[2] != "max":
        q = end + tok[0] - tok[2]
        if q - len(b.buf) >= 10 and end - q >= 10:
            b.filler(q - len(b.buf))
    b.filler(end - len(b.buf))


def _needs(tok):
    return 2100 if tok[2] in (2047, 2048) else 200


def _try(place, tok, final=20, seeds=3):
    """Can the parse give `tok` at `place`?  A small block of its own per
    seed; True when the oracle parses one to its plan."""
    for seed in range(seeds):
        rng = random.Random(f"{place}-{tok}-{final}-{seed}")
        lead = _needs(tok)
        n = lead + 2 * (tok[0] + tok[1]) + 400
        b = _block(rng, n, lead=lead, final=final, **{place: tok})
        if b is not None and b.ok():
            return True
    return False


@functools.lru_cache(maxsize=None)
def literal_edges():
    """{"first" | "after_match": {threshold: (below, above)}}: for every
    literal threshold the nearest reachable literal length of a token with a
    copy on each side, searched with the oracle."""
    found = {}
    for name, place in (("first", "first"), ("after_match", "middle")):
        found[name] = {}
        for lo, hi in LIT_THRESHOLDS:
            w = max(6, hi // 16)
            reach = [L for L in range(lo - w, hi + w + 1)
                     if _try(place, (L, 8, "max" if place == "first"
                                     else L + 1))]
            below = max((L for L in reach if L <= lo), default=None)
            above = min((L for L in reach if L >= hi), default=None)
            found[name][(lo, hi)] = (below, above)
    return found


def literal_values(place):
    """The literal lengths of the grid at a place: 1, 3 (the shortest behind
    which every offset of 1 to 4 has a source the parse inserted), the two
    sides of every threshold and - behind a match - 0."""
    edges = literal_edges()["first" if place == "first" else "after_match"]
    vals = {1, 3} | {v for pair in edges.values() for v in pair
                     if v is not None}
    if place != "first":
        vals.add(0)
    return sorted(vals)


@functools.lru_cache(maxsize=None)
def grid_targets():
    """{place: [(token, final)]}: every literal value x copy edge x offset
    edge the oracle's parse can give at that place ("max": the block's first
    byte as the source), the final literal behind a "last" token chosen in
    turn among FINALS (a short copy cannot lie within 15 bytes of the block's
    end: src/compress.rs:20, the next final that works is taken).  What is
    not here is unreachable: unreachable_targets() counts it."""
    out = {p: [] for p in PLACES}
    k = 0
    for place in PLACES:
        for L in literal_values(place):
            for C in COPY_EDGES:
                for Oe in OFFSET_EDGES:
                    tok = (L, C, Oe)
                    if place != "last":
                        if _try(place, tok, seeds=6):
                            out[place].append((tok, None))
                        continue
                    for j in range(len(FINALS)):
                        F = FINALS[(k + j) % len(FINALS)]
                        if _try(place, tok, final=F):
                            out[place].append((tok, F))
                            k += 1
                            break
    return out


def unreachable_targets():
    total = {p: len(literal_values(p)) * len(COPY_EDGES) * len(OFFSET_EDGES)
             for p in PLACES}
    return {p: total[p] - len(grid_targets()[p]) for p in PLACES}


class Block:
    """One block of the set: its bytes, the token list the oracle confirmed
    (plan) and where the tokens it was built for lie (marks: {place: index
    into plan}; asked: {place: (L, C, offset edge)})."""

    def __init__(self, family, cls, builder, asked=None, final=None):
        self.family, self.cls = family, cls
        self.data = bytes(builder.buf)
        self.plan = list(builder.plan)
        self.marks = dict(getattr(builder, "marks", {}))
        self.asked = asked or {}
        self.final = final


def _grid_size(cls, i):
    if cls == "small":      # 4 097 .. 8 192 bytes: k_match_spans_8k's class
        return 8192 if i % 16 == 0 else 4097 + (i % 5) * 101
    return 16385 + i if i % 32 == 0 else 8193 + (i % 7) * 53


def _grid_block(cls, i, want, attempts=8):
    """A block of class cls with the targets want = {place: (token, final)}
    (any of the three places), confirmed by the oracle, or None."""
    toks = {p: w[0] for p, w in want.items()}
    final = want["last"][1] if "last" in want else 20
    need = sum(t[0] + t[1] for t in toks.values()) + 2100 + 120 + final
    n = max(_grid_size(cls, i), need)
    if cls == "small" and n > 8192:
        return None
    for attempt in range(attempts):
        rng = random.Random(f"grid-{cls}-{i}-{sorted(toks)}-{attempt}")
        b = _block(rng, n, final=final, **toks)
        if b is not None and b.ok():
            return Block("grid", cls, b, toks, final)
    return None


GRID_DROPPED = []    # targets no block of a class could be built for


@functools.lru_cache(maxsize=None)
def grid():
    """The grid's blocks: every target of grid_targets() once in a block of
    4-8 KiB and once in a block of more than 8 KiB, three to a block (one per
    place) where the oracle confirms them together and alone otherwise; then
    the blocks whose FINAL literal has each length the literal thresholds
    name (the one place those lengths can occur)."""
    targets = grid_targets()
    out = []
    for cls in ("small", "large"):
        # at most one "max" to a block: the first of them takes the empty
        # slot of the hash table that stands for the block's first bytes
        queue = {p: list(targets[p]) for p in PLACES}

        def is_max(p, w):       # its source is the block's first bytes
            return w[0][2] == "max" or (p == "first" and w[0][2] == w[0][0])

        i = 0
        while any(queue.values()):
            want, has_max = {}, False
            for k in range(len(PLACES)):
                p = PLACES[(i + k) % len(PLACES)]
                # (the place whose turn it is takes a "max" if it has one)
                pick = [j for j, w in enumerate(queue[p])
                        if is_max(p, w) == (k == 0)] or \
                       [j for j, w in enumerate(queue[p])
                        if not (has_max and is_max(p, w))]
                if pick:
                    want[p] = queue[p].pop(pick[0])
                    has_max = has_max or is_max(p, want[p])
            i += 1
            blk = _grid_block(cls, i, want) if want else None
            if blk is not None:
                out.append(blk)
                continue
            for p, w in want.items():
                blk = _grid_block(cls, i, {p: w}, attempts=40)
                if blk is None:     # (a source that depends on the company)
                    GRID_DROPPED.append((cls, p, w))
                else:
                    out.append(blk)
        for i, F in enumerate(v for pair in LIT_THRESHOLDS for v in pair):
            for attempt in range(8):
                rng = random.Random(f"final-{cls}-{F}-{attempt}")
                b = _block(rng, _grid_size(cls, i + 1), final=F)
                if b.ok():
                    break
            else:
                raise AssertionError((cls, F))
            out.append(Block("final", cls, b, final=F))
    return out


@functools.lru_cache(maxsize=None)
def _long_literal():
    """The first literal length from 4 000 on that a token with a copy can
    have (the skip loop probes one position in 126 there)."""
    for L in range(4000, 4300):
        if _try("first", (L, 8, "max"), seeds=1):
            return L
    raise AssertionError("no literal of 4 000 to 4 300 bytes is reachable")


@functools.lru_cache(maxsize=None)
def full_blocks():
    """64 KiB blocks whose last copy has the largest offset a block admits -
    its source is the block's first byte - and ends 0, 1, 15, 16, 17, 64 and
    65 bytes in front of the block's end.  Behind 2 to 6 KiB of short tokens
    and an exception the block is literals of some 4 000 bytes with a copy of
    8 behind each (few probes: the empty slot of the hash table that stands
    for the block's first bytes has to survive them all); the last token's
    literal is 3 bytes, since behind a long one the skip loop's stride would
    carry it past the block's end (src/compress.rs:212-216)."""
    out = []
    copies = (76, 76, 64, 65, 67, 68, 72)
    Lb = _long_literal()
    for F, C in zip(FINALS, copies):
        fixed = 61 + 65 + 1031 + 76 + 300 + 3 + C + F
        k = (BLOCK - fixed - 2000) // (Lb + 8)
        for attempt in range(40):
            rng = random.Random(f"full-{F}-{attempt}")
            b = _Builder(rng, BLOCK)
            b.token(61, 65, 60)
            b.filler(BLOCK - fixed - k * (Lb + 8))
            b.token(1031, 76, 2048)
            if not b.prefix_ok():
                continue
            for _ in range(k):
                b.token(Lb, 8, Lb + 1)
            b.filler(300)
            mark = len(b.plan)
            b.token(3, C, "max")
            b.final(F)
            assert len(b.buf) == BLOCK
            if b.ok():
                blk = Block("full", "full", b, final=F)
                blk.marks = {"last": mark}
                out.append(blk)
                break
        else:
            raise AssertionError(F)
    return out


# ----------------------------------------------------------------- the dense
DENSE_BLOCKS, DENSE_MIN_TOKENS = 128, 15000


def _dense_block(seed):
    rng = random.Random(f"dense-{seed}")
    words = [rng.randbytes(4) for _ in range(16 if seed % 2 else 64)]
    return b"".join(rng.choices(words, k=BLOCK // 4))


@functools.lru_cache(maxsize=None)
def dense():
    """128 blocks of 65 536 bytes, each 16 384 four-byte words drawn from a
    dictionary of 16 (odd seeds) or 64 words: at least 15 000 tokens each
    (counted, seeds that give fewer are passed over).  Returns (blocks, their
    oracle streams, token counts)."""
    blocks, comps, counts = [], [], []
    seed = 0
    while len(blocks) < DENSE_BLOCKS:
        data = _dense_block(seed)
        seed += 1
        comp = O.compress(data)
        count = len(tokens(comp))
        if count >= DENSE_MIN_TOKENS:
            blocks.append(data)
            comps.append(comp)
            counts.append(count)
        assert seed < 4 * DENSE_BLOCKS
    return blocks, comps, counts


# ------------------------------------------------------------ the exceptions
EXC_MIN = 800


def _phrase_block(seed, kinds):
    rng = random.Random(f"phrases-{seed}-{kinds}")
    phrases = [rng.randbytes(rng.randrange(65, 71)) for _ in range(kinds)]
    buf = bytearray()
    while len(buf) < BLOCK:
        buf += rng.choice(phrases)
    return bytes(buf[:BLOCK])


@functools.lru_cache(maxsize=None)
def exception_blocks():
    """[(name, data)] of 65 536-byte blocks:
    "phrases-*": a few distinct phrases of 65 to 70 bytes in random order - at
    least 800 copies of more than 64 bytes, so all four exception pages;
    "mixed": the three kinds of exception in turn - long literal with a short
    copy, short literal with a long copy, both long - between short tokens;
    "at-K": short tokens and one exception that is token K of the block, K =
    63, 64 (the edges of the encoder's first pass of 64 tokens), 511 and 512
    (the edge of the first token page)."""
    out = []
    seed = 0
    while len(out) < 2:
        data = _phrase_block(seed, 5 + seed % 4)
        seed += 1
        assert seed < 64
        if exceptions(tokens(O.compress(data))) >= EXC_MIN:
            out.append((f"phrases-{seed - 1}", data))
    for attempt in range(8):
        b = _Builder(random.Random(f"mixed-{attempt}"), BLOCK)
        # (sources the parse is sure to have inserted: the last byte of
        # the copy in front, or the literal's own first bytes)
        kinds = ((1031, 5, 1032), (3, 200, 3), (1031, 300, 1032),
                 (999, 65, 1000), (262, 64, 263), (1, 1000, 1))
        k = 0
        b.filler(2200)
        while len(b.buf) < BLOCK - 3000:
            b.token(*kinds[k % len(kinds)])
            b.filler(40 + k % 50)
            k += 1
        b.filler(BLOCK - len(b.buf) - 1031)
        b.final(1031)
        if b.ok():
            out.append(("mixed", bytes(b.buf)))
            break
    else:
        raise AssertionError("mixed")
    for K in (63, 64, 511, 512):
        for attempt in range(8):
            b = _Builder(random.Random(f"at-{K}-{attempt}"), BLOCK)
            b.units(K)
            b.token(5, 100, 6)
            if not b.prefix_ok():
                continue
            b.filler(BLOCK - len(b.buf) - 17)
            b.final(17)
            if b.ok() and is_exception(b.plan[K]):
                out.append((f"at-{K}", bytes(b.buf)))
                break
        else:
            raise AssertionError(K)
    return out


# ------------------------------------------------------------------- the set
class Case:
    """One input of the set: name, family, data, the oracle's stream and its
    tokens per block."""

    def __init__(self, name, family, data, comp=None, made_of=None):
        self.name, self.family, self.data = name, family, data
        self.comp = O.compress(data) if comp is None else comp
        self._blocks = None
        self.made_of = made_of  # one-block cases whose blocks these are

    @property
    def blocks(self):
        if self._blocks is None and self.made_of:
            self._blocks = [c.blocks[0] for c in self.made_of]
        if self._blocks is None:
            self._blocks = block_tokens(self.comp)
        return self._blocks

    def __repr__(self):
        return f"<{self.name} {len(self.data)}>"


class TheSet:
    def __init__(self):
        self.grid_blocks = grid()
        self.full = full_blocks()
        self.grid = [Case(f"grid-{b.family}-{b.cls}-{i}", "grid", b.data)
                     for i, b in enumerate(self.grid_blocks + self.full)]
        d_blocks, d_comps, self.dense_counts = dense()
        self.dense = [Case(f"dense-{i}", "dense", d, c)
                      for i, (d, c) in enumerate(zip(d_blocks, d_comps))]
        self.dense_stream = Case("dense-stream", "dense", b"".join(d_blocks),
                                 made_of=self.dense)
        self.exceptions = [Case(name, "exceptions", d)
                           for name, d in exception_blocks()]
        exc = [d for _, d in exception_blocks()]
        full = [b.data for b in self.full]
        small = next(b.data for b in self.grid_blocks
                     if b.cls == "small" and len(b.data) < 4200)
        parts = {
            "stream-2": [d_blocks[0], exc[0]],
            "stream-3": [full[0], exc[1], d_blocks[1]],
            "stream-5": [d_blocks[2], exc[2], full[1], exc[3], d_blocks[3]],
            "stream-5b": [exc[4], exc[5], d_blocks[5], exc[6], full[6]],
            "stream-grid-last": [d_blocks[4], exc[0], small],
        }
        self.streams = [Case(name, "streams", b"".join(p))
                        for name, p in parts.items()]

    def dense_and_exceptions(self):
        return self.dense + [self.dense_stream] + self.exceptions

    def everything(self):
        return self.grid + self.dense_and_exceptions() + self.streams

    def single_blocks(self):
        return [c for c in self.everything() if len(c.data) <= BLOCK]


@functools.lru_cache(maxsize=None)
def the_set():
    """The whole set with its oracle streams, built once per process."""
    return TheSet()
