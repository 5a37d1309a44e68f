"""Raw streams built at the edges of the wave decoders' window loops
(csrc/snapmi_wide3.hpp, snapmi_wide2.hpp, decode_sequential): what
tests/token_shapes.py is for the compressors.

Every stream is built from explicit elements (foreign.varint / lit / copy)
and carries the output it must produce.  A Builder follows the third
generation's window rule while it appends (a window ends after 64 elements,
in front of the element that starts at input position 256 or later, in front
of the element that would pass 2048 output bytes, and at a literal with
length bytes), so an element can be put at a chosen place of a window, of the
ring and of the output.  Whether the place was hit is not the builder's to
say: the lane-level model (tests/model_decoder3.py) reports the events of a
stream, and a stream stays in a family only when the model saw one of the
events the family is named for (the_set()).

The window loop runs only while kTail3 = 337 bytes of input are left, so a
stream ends in a pad of 60-byte literals of random bytes: the element under
test is the window loop's, not the tail's.

Families (the_set()):
  overlap    every (offset 1..64, length 1..64) moved by the late loops, as
             copy-2 and copy-4 (copy-1 where 4 <= length <= 11), one stream
             per offset, a short literal of fresh bytes in front of each;
             the pairs with offset >= length once more as own-lane copies
             ("own_lane-*": at the head of a window, behind a three-byte
             literal with a length byte); the overlapping pairs once more
             through the late loop that asks every element where its source
             is ("general_loop-*"); and one more copy of the pairs cut into
             streams under 256 compressed bytes, in turn with an output of at
             most 256 bytes ("lds-*") and of more ("short_wide-*"), and the
             lengths up to 10 in streams of 256..511 compressed bytes with at
             most 512 of output ("small-*")
  foreign_whole  no literal over 60 bytes, more than 70 000 bytes of output:
             copy-2 / copy-4 at the offsets around 2 KiB, 4 KiB and 64 KiB
             and at the stream's first byte, windows of more than 64 starts;
             "-aligned": the same with an element boundary at every 64 KiB
  ring       sources around safe_lo, ring reads from the ring's last 15
             bytes, elements that wrap the ring's end in every piece, windows
             that start in the ring's first 16 bytes and close to its end
  cuts       64 / 65 starts, 2048 / 2049 bytes, chosen start positions,
             literals with length bytes in all forms and places
  behind_long_literal   what only a window behind such a literal sees
  handover   337 / 336 bytes left at a window boundary (and the second
             generation's 160 / 159)
  beyond     the shortest padded stream of each family above one step past
             valid, the bad element in front of the pad so that the window
             loop meets it: out is None, the oracle names the error.  The
             handover family ends without a pad and has no such variant.
"""
import functools
import random

import foreign
import model_decoder as M2
import model_decoder3 as M3

PAD = 6           # literals of 60 bytes behind the element under test
R = M3.R


class Case:
    def __init__(self, name, comp, out, pairs=()):
        self.name, self.comp, self.out = name, comp, out
        self.pairs = frozenset(pairs)     # (offset, length, kind) it holds
        self.stats3 = None                # the third-generation model's

    def __repr__(self):
        return "<%s: %d -> %s>" % (self.name, len(self.comp),
                                   None if self.out is None else len(self.out))


class Builder:
    def __init__(self, seed):
        self.rng = random.Random(seed)
        self.els = []             # element bytes, in order
        self.out = bytearray()
        self.pairs = set()
        # the window the next element would join: elements, input bytes and
        # output bytes it holds so far
        self.w_el = self.w_in = self.w_out = 0
        self.s = 0                # input bytes so far (behind the header)
        self.win_starts = []      # where the rule says a window starts

    # ---- the window rule ------------------------------------------------
    def _joins(self, n_out):
        return not (self.w_el == 64 or self.w_in >= 256
                    or self.w_out + n_out > M3.WMAX)

    def peek(self, n_out):
        """Where in its window's output an element of n_out bytes would
        start, were it appended now."""
        return self.w_out if self._joins(n_out) else 0

    def at_window_start(self):
        return self.w_el == 0 or self.w_el == 64 or self.w_in >= 256

    def _place(self, enc, n_out, ends_window):
        at = self.s
        self.s += enc
        if ends_window:           # ... and is moved in a step of its own
            self.win_starts.append(at)
            self.w_el = self.w_in = self.w_out = 0
            return
        if self.w_el == 0 or not self._joins(n_out):
            self.win_starts.append(at)
            self.w_el = self.w_in = self.w_out = 0
        self.w_el += 1
        self.w_in += enc
        self.w_out += n_out

    @property
    def d(self):
        return len(self.out)

    # ---- elements -------------------------------------------------------
    def lit(self, n, form=None):
        data = self.rng.randbytes(n)
        el = foreign.lit(data, form)
        self._place(len(el), n, el[0] >> 2 >= 60)
        self.els.append(el)
        self.out += data
        return self

    def copy(self, off, n, kind=2):
        assert 1 <= off <= self.d, (off, self.d)
        el = foreign.copy(off, n, kind)
        self._place(len(el), n, False)
        self.els.append(el)
        for _ in range(n):
            self.out.append(self.out[-off])
        self.pairs.add((off, n, kind))
        return self

    def grow_to(self, t):
        """Output up to exactly t: 64-byte copies, a fresh literal now and
        then so that the bytes have no period."""
        assert t >= self.d
        if self.d < 64:
            self.lit(min(60, t - self.d))
            if t - self.d > 0:
                self.lit(min(60, t - self.d))
        k = 0
        while t - self.d >= 64 + 61:
            k += 1
            if k % 6 == 0:
                self.lit(self.rng.randrange(3, 14))
            else:
                self.copy(self.rng.randrange(64, min(self.d, 3000) + 1), 64)
        while t > self.d:
            self.lit(min(60, t - self.d))
        return self

    def new_window(self):
        """Literals of 60 bytes until the next element starts a window."""
        while not self.at_window_start():
            self.lit(60)
        return self

    def start_window_at(self, t):
        """The next element starts a window, at output position t exactly,
        and no literal with length bytes was needed (the ring stays whole)."""
        self.grow_to(t - 549)
        self.new_window()         # at most five literals of 60
        r = t - self.d
        assert 249 <= r <= 549 and self.at_window_start()
        for part in ((r,) if r <= 492 else (r // 2, r - r // 2)):
            self._exact_window(part)
        assert self.d == t and self.at_window_start(), (self.d, t)
        return self

    def _exact_window(self, w):
        """One whole window of exactly w output bytes, 249 <= w <= 492: up
        to two copies of 64, a copy of n, four literals of 60, one of x."""
        for j in (0, 1, 2):
            lo_x = max(1, 11 - 3 * (j + 1))
            n = w - 64 * j - 240 - lo_x
            x = lo_x
            if n > 64:
                x += n - 64
                n = 64
            if n >= 1 and x <= 60:
                break
        else:
            raise AssertionError(w)
        d0 = self.d
        for _ in range(j):
            self.copy(777, 64)
        self.copy(777, n)
        for _ in range(4):
            self.lit(60)
        self.lit(x)
        assert self.d - d0 == w and self.at_window_start()

    def reach(self, t):
        """Inside the current window: output up to exactly t with a few
        64-byte copies and one literal (at most 8 elements)."""
        assert 0 <= t - self.d <= 450
        while t - self.d >= 64:
            self.copy(300, 64)
        if t > self.d:
            self.lit(t - self.d)
        return self

    # ---- the stream -----------------------------------------------------
    def finish(self, name, pad=PAD):
        core = list(self.els), len(self.out)
        for _ in range(pad):
            self.lit(60)
        body = b"".join(self.els)
        c = Case(name, foreign.varint(len(self.out)) + body, bytes(self.out),
                 self.pairs)
        c.core = core             # (elements, output) in front of the pad
        c.win_starts = list(self.win_starts)
        c.pad = b"".join(self.els[len(core[0]):])
        return c


# ---------------------------------------------------------------- overlap
def kinds_of(o, n):
    return (2, 4, 1) if 4 <= n <= 11 else (2, 4)


def overlap_stream(o):
    """Every length at offset o as a LATE element: overlapping (o < n) by
    itself, the others by their place - behind o - n bytes of the window's
    own output and more."""
    b = Builder(1000 + o)
    b.lit(60)
    b.lit(max(4, o - 59))
    for n in range(1, 65):
        for kind in kinds_of(o, n):
            b.lit(b.rng.randrange(1, 5))
            while n <= o and b.peek(n) <= o - n:
                b.lit(min(60, o - n + 1 - b.peek(n)))
            b.copy(o, n, kind)
    return b.finish("overlap-%d" % o)


def own_lane_stream():
    """The pairs with offset >= length copied by their own lanes: a window's
    first elements, each behind at most offset - length bytes of its output.
    A literal of one byte written with a length byte (three bytes) ends the
    window; the sources then lie in front of the ring's history (HBM)."""
    b = Builder(2000)
    b.grow_to(200)
    left = sorted(((o - n, n, o) for o in range(1, 65)
                   for n in range(1, o + 1)))
    k = 0
    while left:
        b.lit(1, form=1)
        while True:
            f = b.w_out
            pick = next((p for p in left if p[0] >= f), None)
            if pick is None or not b._joins(pick[1]) and b.w_el:
                break
            left.remove(pick)
            k += 1
            b.copy(pick[2], pick[1], 4 if k % 3 == 0 else 2)
    return b.finish("own_lane")


def general_loop_stream(part):
    """The overlapping pairs through the late loop that asks every element
    where its source is (taken when one late source of the window is not in
    the ring): each pair opens a window behind a three-byte literal with a
    length byte, so its source is in HBM, and comes once more behind two
    fresh bytes, its source now the ring."""
    b = Builder(2100 + part)
    b.grow_to(130)
    k = 0
    for o in range(1, 64):
        for n in range(o + 1, 65):
            k += 1
            if k % 4 != part:
                continue
            kind = 2 if (o + n) % 2 else 4
            b.lit(1, form=1 + k % 3)
            b.copy(o, n, kind)
            b.lit(2)
            b.copy(o, n, 6 - kind)
    return b.finish("general_loop-%d" % part)


# stream classes of the plan (tests/error_variants.py): (name, compressed
# bytes at most, output at most, output more than)
LDS = ("lds", 255, 256, 0)
SHORT_WIDE = ("short_wide", 240, 1 << 20, 256)
SMALL = ("small", 500, 512, 0)


def short_streams(classes, o, lengths):
    """The copies of offset o cut into short streams, one after the other in
    the class that its offset and its lengths (eight to a block) select."""
    out = []
    b = None
    block = None
    for n in lengths:
        for kind in kinds_of(o, n):
            el = len(foreign.copy(o, n, kind)) + 2
            if block != (n - 1) // 8 % len(classes) or b.s + el + 2 > cls[1] \
                    or b.d + 1 + n > cls[2]:
                block = (n - 1) // 8 % len(classes)
                cls = classes[(block + o) % len(classes)]
                b = Builder(3000 + 64 * len(out) + o)
                out.append((cls, b))
                b.lit(min(o, 60))
                if o > 60:
                    b.lit(o - 60)
            b.lit(1)
            b.copy(o, n, kind)
    cases = []
    for i, (cls, b) in enumerate(out):
        while b.d <= cls[3]:
            b.copy(o, 64)
        cases.append(b.finish("%s-%d-%d" % (cls[0], o, i), pad=0))
    return cases


# ---------------------------------------------------------- foreign_whole
FAR_OFFSETS = [1, 2047, 2048, 4095, 4096, 4097, 65535, 65536, 65537]


def foreign_whole_stream(seed):
    b = Builder(seed)
    b.grow_to(70000 + 97 * (seed % 7))
    for rep, n in enumerate((64, 17, 5, 33)):
        for off in FAR_OFFSETS + [None]:
            for kind in (4, 2):
                o = b.d if off is None else off
                if kind == 2 and o >= 65536:
                    continue
                b.copy(o, n, kind)
                b.lit(1 + (rep + o) % 9)
        # a window of more than 64 starts that holds copy-4 elements
        b.new_window()
        for i in range(80):
            if i % 9 == 4:
                b.copy(FAR_OFFSETS[(i // 9 + rep) % 9], 20 + i % 7, 4)
            else:
                b.copy(1 + (i * 37) % 1500, 4 + i % 8, 1)
    return b.finish("foreign_whole-%d" % seed)


def foreign_aligned_stream():
    """The same offsets in a stream with an element boundary at every
    multiple of 64 KiB of output: one a block index can be built for."""
    b = Builder(8100)
    for block in (1, 2):
        b.grow_to(65536 * block)
        for i, off in enumerate(FAR_OFFSETS + [None]):
            o = b.d if off is None else off
            if o <= b.d:
                b.copy(o, 64 - i, 4)
                b.lit(5)
    return b.finish("foreign_whole-aligned")


# ------------------------------------------------------------------- ring
def placed_window(b, copies, lits=None):
    """A whole window of copies at chosen sources: `copies` is a list of
    (length, kind, q_of) where q_of(d, W, safe_lo, dstp) names the source;
    literals of 60 bytes behind them end the window."""
    b.new_window()
    enc = sum(len(foreign.copy(1, n, kind)) for n, kind, _ in copies)
    k = -(-(256 - enc) // 61) if lits is None else lits
    d, W = b.d, sum(n for n, _, _ in copies) + 60 * k
    assert W <= M3.WMAX and d + W + 16 >= R
    safe_lo = d + W + 16 - R
    for n, kind, q_of in copies:
        b.copy(b.d - q_of(d, W, safe_lo, b.d), n, kind)
    for _ in range(k):
        b.lit(60)
    assert b.d == d + W and b.at_window_start()


def ring_safe_lo_stream():
    b = Builder(4001)
    b.grow_to(9000)
    for n in (16, 40, 64, 5):
        placed_window(b, [(n, 2, lambda d, W, lo, p, k=k: lo + k)
                        for k in (-1, 0, 1)] +
                    [(n, 4, lambda d, W, lo, p, k=k, n=n: lo + k - n)
                     for k in (-1, 0, 1)] +
                    [(n, 2, lambda d, W, lo, p, n=n: lo - n // 2)])
    return b.finish("ring-safe_lo")


def ring_tail_stream():
    """Ring reads that start in each of the ring's last 15 bytes, in a window
    that starts right behind a wrap and in one far from it."""
    b = Builder(4002)
    for m, r0 in ((2, 40), (3, 1800), (4, 3000)):
        b.start_window_at(R * m + r0)
        placed_window(b, [(16 if j % 2 else 19, 2,
                         lambda d, W, lo, p, j=j, m=m: R * m - j)
                        for j in range(1, 16)])
    return b.finish("ring-tail")


def ring_wrap_stream(as_copy):
    """An element whose own bytes wrap the ring's end in its piece c, with
    k bytes of the piece in front of the wrap."""
    b = Builder(4003 + as_copy)
    m = 1
    for c in (0, 16, 32, 48):
        for k in (1, 8, 15, 16):
            n = 64 if as_copy else 60
            if c + k >= n:
                continue
            m += 1
            t = R * m - c - k
            b.grow_to(t - 500)
            b.new_window()
            if t - b.d > 450:
                b.lit(60).new_window()
            b.reach(t)
            if as_copy:
                b.copy(2000, n, 2 if k % 2 else 4)
            else:
                b.lit(n)
            b.lit(7)
    return b.finish("ring-wrap-%s" % ("copy" if as_copy else "literal"))


def ring_start_stream(which):
    """Windows that start in the ring's first 16 bytes / so close to its end
    that their 16-byte pieces pass it; behind each a ring read through the
    mirror they had to refresh."""
    b = Builder(4010 + which)
    W = 300
    starts = range(16) if which == 0 else (
        R - W - 17, R - W - 16, R - W - 15, R - W, R - 200, R - 17, R - 16,
        R - 15, R - 1)
    for r0 in starts:
        m = (b.d + 1400 - r0) // R + 1
        b.start_window_at(R * m + r0)
        for _ in range(5):
            b.lit(60)
        top = R * (m + 1)
        b.grow_to(max(b.d, top + 16))
        b.new_window()
        b.copy(b.d - (top - 6), 16).copy(b.d - (top - 15), 33, 4)
    return b.finish("ring-start-%s" % ("lo" if which == 0 else "hi"))


# ------------------------------------------------------------------- cuts
def cuts_counts_stream():
    b = Builder(5001)
    b.grow_to(400)
    for twos in (61, 62):            # 64 and 65 starts in 256 bytes
        b.new_window()
        for i in range(twos):
            b.copy(1 + 5 * i, 4 + i % 8, 1)
        b.lit(60).lit(60).lit(60)
    b.new_window()
    for _ in range(32):              # W == 2048, ended by a long literal
        b.copy(100, 64)
    b.lit(70)
    for _ in range(32):              # 2049: the 33rd element is cut
        b.copy(100, 64)
    b.copy(100, 1)
    b.new_window()
    for _ in range(33):              # 33 copies of 64
        b.copy(100, 64, 4)
    return b.finish("cuts-counts")


def cuts_positions_stream():
    b = Builder(5002)
    b.grow_to(200).new_window()
    # starts at 31, 63 and 255; elements across 32, 64 and the window's end
    b.lit(30).copy(9, 20).lit(28).copy(77, 64, 4).lit(60).lit(60).lit(60)
    b.copy(33, 4, 1).copy(34, 5, 1).copy(150, 40, 4)
    assert b.w_in == 260
    # starts at 32, 64 and 255: a 60-byte literal across the window's end
    b.lit(31).copy(9, 20).lit(28).copy(50, 30).lit(60).lit(60).lit(60)
    b.lit(4).lit(60)
    assert b.w_in == 316
    return b.finish("cuts-positions")


def cuts_long_literal_stream(form):
    """Literals with `form` length bytes - minimal or not - at lane 0, in
    mid-window and at position 255."""
    b = Builder(5010 + form)
    b.grow_to(150)
    for n in (1, 60, 61, 256, 300):
        if n > 256 ** form:
            continue
        b.new_window().lit(n, form)                    # lane 0
        b.lit(10).copy(5, 9).lit(n, form)              # mid-window
        b.new_window()
        b.lit(60).lit(60).lit(60).lit(60).lit(10)      # 255 bytes
        assert b.w_in == 255
        b.lit(n, form)
        b.copy(3, 7)
    return b.finish("cuts-long-literal-form%d" % form)


def cuts_literal_to_the_end():
    b = Builder(5020)
    b.grow_to(500).copy(1, 30).lit(400)
    return b.finish("cuts-literal-to-the-end", pad=0)


# ------------------------------------------------------ behind_long_literal
def behind_stream():
    b = Builder(6001)
    b.grow_to(6000)
    b.lit(100).copy(3000, 40).copy(3100, 64, 4).lit(9)  # own-lane, far
    b.new_window()
    b.lit(100).copy(50, 33).copy(140, 64).lit(3)      # inside its bytes
    b.new_window()
    b.lit(100).lit(30).copy(40, 20).copy(77, 64, 4)   # across its end
    b.new_window()
    b.lit(61).copy(7, 40).lit(5).copy(13, 64)         # overlapping, from it
    return b.finish("behind-sources")


def behind_end_stream():
    """A source in the output's last 64 bytes: literals of one byte with four
    length bytes keep 337 bytes of input behind it."""
    b = Builder(6002)
    b.grow_to(1000)
    b.lit(100).copy(1, 1, 4).copy(30, 2, 4)
    for _ in range(57):
        b.lit(1, form=4)
    return b.finish("behind-output-end", pad=0)


# --------------------------------------------------------------- handover
def handover_streams():
    out = []
    for last in (31, 30):            # 337 and 336 bytes behind a boundary
        b = Builder(7000 + last)
        b.grow_to(900).copy(64, 64).copy(1, 9, 1).new_window()
        for _ in range(5):
            b.lit(60)
        b.lit(last)
        out.append(b.finish("handover3-%d" % (306 + last), pad=0))
    # the second generation: its windows are the model's to place
    found = {}
    for x in range(1, 61):
        b = Builder(7100)
        b.grow_to(700).copy(64, 64).copy(2, 9, 1)
        b.lit(60).lit(60).lit(x)
        c = b.finish("handover2-%d" % x, pad=0)
        st = M2.Stats()
        M2.decode(c.comp, st)
        for ev in ("window_at_tail", "handover_at_tail"):
            if st.events[ev] and ev not in found:
                found[ev] = c
    return out + sorted(found.values(), key=lambda c: c.name)


# ----------------------------------------------------------------- beyond
def beyond(case):
    """`case` one step past valid, the pad still behind the bad element."""
    els, d = case.core
    body = b"".join(els)
    pad_out = 60 * PAD
    name = "beyond-" + case.name

    def stream(extra, n_out, pad=case.pad, pad_n=pad_out):
        return foreign.varint(d + n_out + pad_n) + body + extra + pad

    return [
        Case(name + "-offset-dstp+1", stream(foreign.copy(d + 1, 9, 4), 9),
             None),
        Case(name + "-offset-0", stream(foreign.copy(0, 9, 2), 9), None),
        Case(name + "-header-short",
             foreign.varint(len(case.out) - 1) + case.comp[
                 len(foreign.varint(len(case.out))):], None),
        Case(name + "-literal-long",
             stream(bytes([61 << 2]) + len(case.pad).to_bytes(2, "little"),
                    len(case.pad) + 1, pad_n=0), None),
    ]


# ---------------------------------------------------------------- the set
# events of tests/model_decoder3.py a family is named for: a stream that
# reports none of them is not kept
NAMED_FOR = {
    "overlap": (),                 # held to its pairs instead (below)
    "foreign_whole": ("copy4_whole", "off_gt_64k_whole", "cap64"),
    "ring": ("src_straddles_safe_lo", "ring_read_into_mirror",
             "wrap_bytewise", "mirror_lo", "mirror_hi"),
    "cuts": ("cap64", "starts_64", "wmax_cut", "w_is_wmax", "start_at_255",
             "longlit_form1", "longlit_form2", "longlit_form3",
             "longlit_form4"),
    "behind_long_literal": ("far_own_lane_not_whole", "late_not_ring"),
    "handover": ("window_at_tail", "handover_at_tail"),
}


def model3(case):
    if case.stats3 is None:
        case.stats3 = M3.Stats()
        case.result3 = M3.decode(case.comp, case.stats3)
    return case.stats3


def build_set():
    fam = {
        "overlap": [overlap_stream(o) for o in range(1, 65)]
        + [own_lane_stream()] + [general_loop_stream(p) for p in range(4)],
        "foreign_whole": [foreign_whole_stream(s) for s in (8001, 8002)]
        + [foreign_aligned_stream()],
        "ring": [ring_safe_lo_stream(), ring_tail_stream(),
                 ring_wrap_stream(True), ring_wrap_stream(False),
                 ring_start_stream(0), ring_start_stream(1)],
        "cuts": [cuts_counts_stream(), cuts_positions_stream()]
        + [cuts_long_literal_stream(f) for f in (1, 2, 3, 4)]
        + [cuts_literal_to_the_end()],
        "behind_long_literal": [behind_stream(), behind_end_stream()],
        "handover": handover_streams(),
    }
    short = []
    for o in range(1, 65):
        short += short_streams((LDS, SHORT_WIDE), o, range(1, 65))
        short += short_streams((SMALL,), o, list(range(1, 11)) * 2)
    return fam, short


@functools.lru_cache(maxsize=None)
def the_set():
    """{family: [Case]}; "overlap_short" holds the streams of the
    lane-per-stream classes, which no window loop decodes."""
    fam, short = build_set()
    kept = {}
    for name, cases in fam.items():
        named = NAMED_FOR[name]
        kept[name] = []
        for c in cases:
            ev = model3(c).events
            if name == "handover" and c.name.startswith("handover2"):
                kept[name].append(c)       # the second generation's
            elif not named or any(ev[k] for k in named):
                kept[name].append(c)
    # overlap: every stream must have had its pairs moved by the late loops
    # or copied by their own lanes
    kept["overlap"] = [c for c in kept["overlap"]
                       if {(o, n) for o, n, _ in c.pairs} <=
                       (c.stats3.late_overlap | c.stats3.late_apart
                        | c.stats3.own_lane)]
    kept["overlap_short"] = short
    # (a stream without a pad - the handover family, the literal that fills
    # its stream - has no room for a bad element that the window loop would
    # still decode: no variant of those)
    kept["beyond"] = [v for name in fam
                      for c in sorted((c for c in kept[name] if c.pad),
                                      key=lambda c: len(c.comp))[:1]
                      for v in beyond(c)]
    return kept


def valid_cases():
    s = the_set()
    return [c for name in s if name != "beyond" for c in s[name]]


def long_stream(admits):
    """The valid streams of the window families as ONE stream (every family
    refers back into its own output only, so the elements can be appended),
    repeated until admits(compressed length, output length): (stream, out).
    Cut into pieces that start with an empty ring, every family meets the
    window loop's not-whole path here."""
    body, out = bytearray(), bytearray()
    while not admits(len(body) + 5, len(out)):
        for cases in window_families().values():
            for c in cases:
                body += c.comp[M3.read_varint(c.comp)[1]:]
                out += c.out
    return foreign.varint(len(out)) + bytes(body), bytes(out)


def window_families():
    """The families the window loops decode (all but the short streams)."""
    s = the_set()
    return {k: v for k, v in s.items() if k not in ("beyond",
                                                    "overlap_short")}
