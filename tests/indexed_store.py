"""A store of indexed raw streams that lives through many calls, as a model:
what snapmi_compress_batch_indexed, snapmi_write_ranges_indexed,
snapmi_append_indexed, snapmi_build_block_index and the two indexed readers
must answer when each call is handed the streams and the index the call before
it wrote.

Store composes the models of the single calls (writeindex_ref.expect,
appendindex_ref.expect, rangeindex_ref.expect, indexbuild_ref.build, the
oracle) and rewrites none of them.  SCENARIO / SCENARIO_FAIL are the chains the
CPU test proves complete and the GPU tests run on the device; play() is the
model's answer to every step of one.  No torch here: the CPU test imports
this."""
import functools
import random

import appendindex_ref as A
import blockindex_ref as B
import indexbuild_ref as I
import oracle_lib as O
import rangeindex_ref as R
import writeindex_ref as W

BLOCK = B.BLOCK
OK = (0, 0, 0, 0)
SLACK = 37      # bytes of capacity behind the length a stream is to take
NO_CAP = 1 << 40
MAX_LEN = 400000        # no stream of a scenario grows past this
MAX_STEP_BLOCKS = 40    # no step of a scenario touches more blocks


@functools.lru_cache(maxsize=None)
def oracle(data):
    """(O.compress(data), B.expected_index(data)), once per value."""
    return O.compress(data), B.expected_index(data)


def firsts(entries):
    out = [0]
    for e in entries:
        out.append(out[-1] + len(e))
    return out


class Store:
    """Per stream: the plain data, the compressed stream and its index
    entries.  One method per call kind; each takes what the call takes,
    returns what the call must answer and then applies the caller's rule: a
    stream that succeeded takes the new bytes and entries, one that failed -
    or that no write or append named - keeps the old ones."""

    def __init__(self):
        self.data, self.streams, self.entries = [], [], []

    @property
    def n(self):
        return len(self.data)

    @property
    def first(self):
        return firsts(self.entries)

    @property
    def flat(self):
        return [e for idx in self.entries for e in idx]

    @property
    def lens(self):
        return [len(d) for d in self.data]

    def snapshot(self):
        return list(self.data), list(self.streams), [list(e) for e in
                                                     self.entries]

    def compress_indexed(self, datas):
        """-> (streams, first, flat index)."""
        self.data = [bytes(d) for d in datas]
        self.streams = [oracle(d)[0] for d in self.data]
        self.entries = [list(oracle(d)[1]) for d in self.data]
        return list(self.streams), self.first, self.flat

    def write(self, writes, caps=None):
        """writes: (stream, off, bytes) sorted by (stream, off).  -> (per
        stream (new bytes or None, new entries or None, error), the new flat
        index, (write_blocks, write_blocks_decoded, write_streams_ok,
        write_streams_failed))."""
        caps = [NO_CAP] * self.n if caps is None else caps
        res, new_index = W.expect(self.streams, self.flat, self.first, writes,
                                  caps, O.compress, W.decode_piece,
                                  W.header_error)
        named = [w for w in writes if len(w[2])]
        t = W.touched([(s, o, len(b)) for s, o, b in named])
        touched_streams = sorted({w[0] for w in named})
        failed = sum(1 for s in touched_streams if res[s][0] is None)
        counters = (len(t), sum(int(q[3]) for q in t),
                    len(touched_streams) - failed, failed)
        for s, (new, ne, err) in enumerate(res):
            if new is not None:
                self.data[s] = W.patched(
                    self.data[s], [(o, b) for t_, o, b in named if t_ == s])
                self.streams[s], self.entries[s] = new, list(ne)
        assert new_index == self.flat  # a failed stream's old entries: copied
        return res, new_index, counters

    def append(self, appends, old_lens=None, caps=None):
        """appends[i]: the bytes appended to stream i (empty: not named);
        old_lens: the host's copy of the lengths (default: the true ones).
        -> (per stream (new bytes or None, new entries, error), the new
        first[], the new flat index, (append_blocks, append_blocks_decoded,
        append_streams_ok, append_streams_failed))."""
        old_lens = self.lens if old_lens is None else list(old_lens)
        caps = [NO_CAP] * self.n if caps is None else caps
        res, nf, new_index = A.expect(
            self.streams, self.flat, self.first, old_lens, appends, caps,
            O.compress, A.decode_piece, A.header_error)
        counters = A.counters(old_lens, appends, res)
        for s, (new, ne, err) in enumerate(res):
            if new is not None:
                self.data[s] = self.data[s] + bytes(appends[s])
                self.streams[s], self.entries[s] = new, list(ne)
        return res, nf, new_index, counters

    def rebuild(self):
        """snapmi_build_block_index on the current streams alone -> (status
        per stream, first, flat index)."""
        built = [I.build(st, len(d)) for st, d in zip(self.streams, self.data)]
        entries = [e for _, e in built]
        return ([s for s, _ in built], firsts(entries),
                [x for e in entries for x in e])

    def read(self, ranges):
        """-> (the decoded data of every stream, per range (bytes or None,
        error))."""
        got = R.expect(self.streams, self.flat, self.first, ranges,
                       W.decode_piece, W.header_error, self.data)
        return list(self.data), got


# ------------------------------------------------------------ the payloads
def text(n, at=0):
    return A.text(n, at)


def zeros(n, at=0):
    return bytes(n)


def rnd(n, at=0):
    return random.Random(1000 + at).randbytes(n)


CLASSES = {"t": text, "z": zeros, "r": rnd}

#                 0  1    2      3      4      5      6       7       8
INITIAL = [("t", 0), ("t", 1), ("t", 127), ("t", 16383), ("t", 65535),
           ("z", 65536), ("r", 65537), ("t", 131072), ("t", 200000),
           ("z", 150000)]
N = len(INITIAL)

# One line per step: ("append", [(class, bytes) per stream]) and ("write",
# [[(off, class, bytes), ...] per stream]); an offset below 0 counts from the
# stream's end.  Every step names every stream, and the classes alternate per
# stream, so that the compressed size of a block moves both ways.
STEPS = [
    ("compress",),
    # 0 -> 100 (onto the empty stream), 128, 128 (1 -> 2 header bytes), 16 384
    # (2 -> 3), 65 536 and 196 608 (tails filled exactly), aligned 65 536 and
    # 131 072, three streams over two new blocks
    ("append", [("t", 100), ("t", 127), ("z", 1), ("t", 1), ("z", 1),
                ("r", 70000), ("z", 131071), ("t", 3000), ("r", 100000),
                ("t", 50000)]),
    # inside a short last block; zeros over the random block 1 and random over
    # the zero block 2 that the append made; 16 bytes across 65 536; whole
    # blocks 1 and 2 with both neighbours cut; across an append's seam
    ("write", [[(10, "r", 16)], [(0, "z", 128)], [(127, "r", 1)],
               [(16000, "t", 384)], [(65535, "r", 1)], [(65536, "z", 65536)],
               [(131072, "r", 65536)], [(65528, "r", 16)],
               [(60000, "z", 140000)], [(149990, "r", 20)]]),
    # behind tails the write rewrote (0, 2, 7, 8); 100 -> 65 536 exactly
    ("append", [("z", 65436), ("t", 16256), ("r", 1000), ("z", 60000),
                ("t", 65536), ("t", 10), ("t", 1), ("r", 70000), ("z", 30000),
                ("z", 100000)]),
    ("rebuild",),
    ("read",),
    # the other way: text and random where zeros were, zeros where random was
    ("write", [[(0, "t", 65536)], [(100, "r", 3000)], [(0, "z", 1128)],
               [(65530, "t", 16)], [(65536, "z", 65536)],
               [(65536, "r", 65536)], [(131072, "z", 65536), (196608, "t", 1)],
               [(134067, "t", 10)], [(290000, "r", 40000)],
               [(0, "t", 1), (-1, "t", 1)]]),
    ("fail",),      # (SCENARIO_FAIL's two calls go here)
    ("append", [("r", 65537), ("z", 49152), ("t", 200000), ("r", 1),
                ("z", 1), ("z", 61062), ("t", 70000), ("z", 100),
                ("t", 69990), ("r", 20)]),
    # into the blocks that append made; whole block 1 of stream 2 with both
    # neighbours cut
    ("write", [[(-1, "t", 1)], [(30000, "z", 35536)], [(1000, "z", 140000)],
               [(-1, "t", 1)], [(131070, "r", 3)], [(135528, "t", 16)],
               [(261608, "z", 1000)], [(-100, "r", 100)], [(329990, "z", 20)],
               [(240000, "t", 60020)]]),
    ("append", [("t", 5), ("r", 70000), ("r", 1), ("z", 300), ("t", 65535),
                ("t", 3), ("z", 10), ("t", 60000), ("r", 1), ("z", 5000)]),
    ("rebuild",),
    ("write", [[(65530, "z", 12)], [(-70000, "t", 50)], [(100000, "r", 50)],
               [(-300, "r", 300)], [(-65535, "z", 65535)], [(-3, "r", 3)],
               [(-10, "t", 10)], [(-60000, "z", 100)], [(-1, "t", 1)],
               [(-5000, "r", 64)]]),
    ("append", [("r", 3), ("z", 1), ("t", 100), ("t", 7), ("r", 2), ("z", 9),
                ("r", 50), ("r", 1), ("z", 1), ("t", 33)]),
    # whole streams and whole tails, to their last byte
    ("write", [[(65528, "r", 16)], [(65536, "z", 70001)],
               [(131072, "t", 65536)], [(0, "z", 76692)], [(196608, "t", 2)],
               [(0, "t", 100)], [(262144, "r", 4525)], [(200000, "z", 64173)],
               [(-8, "r", 8)], [(131071, "t", 2)]]),
    ("append", [("z", 65535), ("t", 60000), ("z", 1), ("r", 5), ("z", 65534),
                ("r", 4), ("t", 1), ("z", 1), ("r", 8), ("t", 9)]),
    ("read",),
]

# The two calls of SCENARIO_FAIL, in which three streams fail.  The write:
# stream 5 with an output cap one below its need (BUFFER_TOO_SMALL {cap,
# need}), stream 8 written behind its end (E_ARGUMENT {off, len, dlen});
# streams 3 and 7 succeed beside them and nobody names the rest.  The append
# that follows it: the host's old_len of stream 2 is one too large (E_ARGUMENT
# {s, dlen, old_len}); streams 7 and 9 succeed.  The steps behind them append
# to and write into every stream, the three included.
FAIL_WRITE = {3: [(70000, "r", 100)], 5: [(100, "t", 3000)],
              7: [(65000, "z", 1000)], 8: [(-1, "t", 2)]}
FAIL_WRITE_SHORT_CAP = 5
FAIL_WRITE_BEHIND_END = 8
FAIL_APPEND = {2: ("t", 500), 7: ("z", 10), 9: ("t", 1000)}
FAIL_APPEND_OLD_LEN = 2


def build(fail, initial=None, steps=None):
    """The concrete steps of STEPS: dicts with "kind" and, for a write,
    "writes" [(stream, off, bytes)]; for an append, "appends" [bytes per
    stream] and "old_lens" (the host's copy); for a read, "ranges" [(stream,
    off, len)] - one across every seam between old and appended bytes, one
    inside every block a write touched.  fail: with the two calls of
    SCENARIO_FAIL.  initial / steps: INITIAL and STEPS, or lists like them."""
    initial = INITIAL if initial is None else initial
    steps = STEPS if steps is None else steps
    lens = [n for _, n in initial]
    seams, blocks = set(), set()
    out, uid = [], [0]

    def payload(cls, n):
        uid[0] += 1
        return CLASSES[cls](n, 977 * uid[0])

    def write_step(per_stream, short=(), behind=()):
        writes = []
        for s, ws in per_stream:
            for off, cls, n in ws:
                off = off + lens[s] if off < 0 else off
                assert s in behind or off + n <= lens[s], (s, off, n, lens[s])
                writes.append((s, off, payload(cls, n)))
                if s not in behind and s not in short:
                    cnt, k0 = R.blocks(off, n)
                    blocks.update((s, k) for k in range(k0, k0 + cnt))
        return dict(kind="write", writes=writes, short=list(short))

    def append_step(per_stream, liar=None):
        appends = [b""] * len(initial)
        old_lens = list(lens)
        for s, (cls, n) in per_stream:
            appends[s] = payload(cls, n)
            if s == liar:
                old_lens[s] += 1
                continue
            if lens[s]:
                seams.add((s, lens[s]))
            lens[s] += n
        return dict(kind="append", appends=appends, old_lens=old_lens)

    for step in steps:
        kind = step[0]
        if kind == "compress":
            uid[0] += 1
            out.append(dict(kind="compress",
                            datas=[CLASSES[c](n, 1000 * i)
                                   for i, (c, n) in enumerate(initial)]))
        elif kind == "write":
            out.append(write_step(list(enumerate(step[1]))))
        elif kind == "append":
            out.append(append_step(list(enumerate(step[1]))))
        elif kind == "fail":
            if fail:
                out.append(write_step(sorted(FAIL_WRITE.items()),
                                      short=[FAIL_WRITE_SHORT_CAP],
                                      behind=[FAIL_WRITE_BEHIND_END]))
                out[-1]["fails"] = True
                out.append(append_step(sorted(FAIL_APPEND.items()),
                                       liar=FAIL_APPEND_OLD_LEN))
                out[-1]["fails"] = True
        elif kind == "rebuild":
            out.append(dict(kind="rebuild"))
        else:
            ranges = []
            for s, p in sorted(seams):
                lo = max(p - 70, 0)
                ranges.append((s, lo, min(140, lens[s] - lo)))
            for s, k in sorted(blocks):
                lo = k * BLOCK + min(100, lens[s] - k * BLOCK - 1)
                ranges.append((s, lo, min(64, lens[s] - lo,
                                          (k + 1) * BLOCK - lo)))
            out.append(dict(kind="read", ranges=ranges))
    return out


SCENARIO = build(False)
SCENARIO_FAIL = build(True)

# More blocks in one call than a segment of the "lanes_segmented" configuration
# holds (lane_segment_blocks cannot go below 64): three streams, an append of
# 68 new blocks behind a short tail, a write over 68 blocks of one stream and
# 66 of another, an append of 67.  Not part of the chains above, which stay
# under 40 blocks a step.
SEGMENT = 64
INITIAL_LONG = [("t", 70 * BLOCK + 1000), ("r", 3000), ("z", BLOCK)]
STEPS_LONG = [
    ("compress",),
    ("append", [("z", 10), ("t", 67 * BLOCK + 5), ("r", 1)]),
    ("write", [[(65000, "r", 66 * BLOCK + 1000)], [(2000, "z", 65 * BLOCK)],
               [(0, "t", 5)]]),
    ("append", [("t", 3), ("z", 66 * BLOCK), ("t", 2 * BLOCK)]),
    ("rebuild",),
    ("read",),
]
SCENARIO_LONG = build(False, INITIAL_LONG, STEPS_LONG)


# ------------------------------------------------------------ the model's run
class Played:
    """What the model says of one step.  n: the number of streams; before /
    after: (data, streams, entries) of every stream; caps: the output capacities the call gets
    (exact need + SLACK; a stream nobody names: 64; step["short"]: one below
    the need); res / new_first / new_index / counters / status / first / flat
    / decoded / ranges: the call's answers, as Store gives them."""

    def __init__(self, step, before):
        self.step, self.kind, self.before = step, step["kind"], before


def play(scenario):
    """[Played] of every step of the scenario."""
    store, out = Store(), []
    for step in scenario:
        p = Played(step, store.snapshot())
        kind = step["kind"]
        p.n = len(step["datas"]) if kind == "compress" else store.n
        if kind == "compress":
            p.streams, p.first, p.flat = store.compress_indexed(step["datas"])
            p.caps = [O.max_compress_len(len(d)) for d in step["datas"]]
        elif kind == "write":
            trial = Store()
            trial.data, trial.streams, trial.entries = store.snapshot()
            need, _, _ = trial.write(step["writes"])
            p.caps = [len(r[0]) + SLACK if r[0] is not None else 64
                      for r in need]
            for s in step["short"]:
                p.caps[s] = len(need[s][0]) - 1
            p.res, p.new_index, p.counters = store.write(step["writes"],
                                                         p.caps)
        elif kind == "append":
            trial = Store()
            trial.data, trial.streams, trial.entries = store.snapshot()
            need, _, _, _ = trial.append(step["appends"], step["old_lens"])
            p.caps = [len(r[0]) + SLACK if r[0] is not None else 64
                      for r in need]
            p.res, p.new_first, p.new_index, p.counters = store.append(
                step["appends"], step["old_lens"], p.caps)
        elif kind == "rebuild":
            p.status, p.first, p.flat = store.rebuild()
        else:
            p.decoded, p.ranges = store.read(step["ranges"])
        p.after = store.snapshot()
        out.append(p)
    return out
