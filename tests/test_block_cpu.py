"""The compressor's block rules on the CPU: csrc/snapmi_block.hpp compiled
into a stand-alone program (tests/block_host.cpp) that asks locate_block,
block_dest, launch_blocks / segment_blocks and table_shift over plain host
arrays.  Every answer is compared with a model written out here - a linear
walk over the streams, nothing taken from the header - for batches of
one-block streams (the lookup's shortcut), one-block streams around a
multi-block one (where the shortcut must stop), streams without blocks in
between, a batch that the plan on the device counts larger than the host
sized it (nothing of the excess may get a destination, nothing else may
change), batches whose blocks are inside the launch and whose slots are not
(block_dest itself has to refuse), with final positions (direct) and with
scratch slots.  The same
program runs once more with -fsanitize=address,undefined."""
import subprocess

import pytest

from conftest import ROOT

B = 65536
SLOT = 76496          # kSlotBytes
MAX_TABLE = 16384


def varint(v):
    out = bytearray()
    while v >= 0x80:
        out.append((v & 0x7F) | 0x80)
        v >>= 7
    out.append(v)
    return bytes(out)


def plan(lens, small_limit):
    """blk_first, slot_first as k_plan_compress leaves them."""
    blk_first, slot_first = [0], [0]
    for n in lens:
        nb = 0 if n == 0 or n < small_limit else (n + B - 1) // B
        blk_first.append(blk_first[-1] + nb)
        slot_first.append(slot_first[-1] + max(nb - 1, 0))
    return blk_first, slot_first


class Case:
    def __init__(self, name, lens, small_limit=0, direct=0, host_lens=None,
                 blk_hi=None):
        self.name, self.lens, self.direct = name, lens, direct
        self.blk_first, self.slot_first = plan(lens, small_limit)
        # the host sizes the launch from ITS copy of the lengths
        hb, hs = plan(lens if host_lens is None else host_lens, small_limit)
        self.host_blocks, self.host_slots = hb[-1], hs[-1]
        blocks = self.blk_first[-1]
        self.blk_lo = 0
        self.blk_hi = blocks + 7 if blk_hi is None else blk_hi
        self.sizes = [(b * 7919 + 13) % 70000 + 1 for b in range(blocks)]
        self.blk_off = [0]
        for s in self.sizes:
            self.blk_off.append(self.blk_off[-1] + s)

    def text(self):
        nums = ([len(self.lens), self.direct, self.host_blocks,
                 self.host_slots, self.blk_lo, self.blk_hi] + self.lens
                + self.blk_first + self.slot_first + self.blk_off)
        return "batch " + " ".join(str(x) for x in nums) + "\n"

    def want(self):
        """The answer's lines, by a walk over the streams."""
        blocks = self.blk_first[-1]
        launch = min(blocks, self.host_blocks)
        lines = ["launch %d %d" % (launch, min(launch, self.blk_hi))]
        heads = [b"\xee" * 10 for _ in self.lens]
        b = 0
        for st, total in enumerate(self.lens):
            nb = self.blk_first[st + 1] - self.blk_first[st]
            for k in range(nb):
                n = min(B, total - k * B)
                if b >= launch:
                    where = "past"
                elif k == 0:
                    # block 0 is written in place, whatever became of the
                    # stream: the caller's buffer has room, the error is set
                    heads[st] = (varint(total) + heads[st])[:10]
                    where = "out %d %d" % (st, len(varint(total)))
                elif self.direct:
                    if self.blk_first[st] + (total + B - 1) // B \
                            > self.host_blocks:
                        where = "none"
                    else:
                        where = "out %d %d" % (
                            st, len(varint(total))
                            + sum(self.sizes[self.blk_first[st]:b]))
                else:
                    slot = self.slot_first[st] + k - 1
                    where = ("none" if slot >= self.host_slots
                             else "slot %d" % (slot * SLOT))
                lines.append("%d %d %d %d %d %d %s" % (b, st, k, total, n,
                                                       k * B, where))
                b += 1
        assert b == blocks
        return lines + ["head " + h.hex() for h in heads]


def cases():
    out = []
    for direct in (0, 1):
        d = "direct" if direct else "slots"
        out.append(Case("one-block-" + d, [1, B, 17, B - 1] * 8,
                        direct=direct))
        out.append(Case("around-multi-" + d, [B] * 5 + [3 * B + 1] + [B] * 5,
                        direct=direct))
        out.append(Case("no-blocks-" + d, [0, B + 1, 0, 0, 2 * B, 5],
                        direct=direct))
        out.append(Case("no-blocks-small-" + d, [0, B + 1, 0, 0, 2 * B, 5],
                        small_limit=256, direct=direct))
        # the device counts one stream more than the host sized
        out.append(Case("excess-stream-" + d, [B + 1, 2 * B, 3 * B],
                        direct=direct, host_lens=[B + 1, 2 * B, 0]))
        # ... a stream longer than the host sized: it straddles host_blocks
        out.append(Case("excess-length-" + d, [B + 1, 4 * B, B],
                        direct=direct, host_lens=[B + 1, 2 * B, 0]))
        # blocks inside the launch whose slots are not: the device sees one
        # stream where the host sized four one-block streams (no slot at
        # all), and two streams whose slots straddle what the host sized
        out.append(Case("no-slots-" + d, [4 * B], direct=direct,
                        host_lens=[B] * 4))
        out.append(Case("slots-straddle-" + d, [3 * B, 3 * B], direct=direct,
                        host_lens=[3 * B, B, B, B]))
        # a segment that ends inside the batch
        out.append(Case("segment-" + d, [B] * 5 + [3 * B + 1] + [B] * 5,
                        direct=direct, blk_hi=6))
    return out


CASES = cases()
TABLE_NS = [15, 16, 17, 255, 256, 257, 8191, 8192, 8193, 16384, 16385, 65536]
TABLE_CAPS = [16384, 8192]


def build(tmp, name, extra):
    exe = tmp / name
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror"]
                          + extra
                          + ["-I", str(ROOT / "include"),
                             str(ROOT / "tests" / "block_host.cpp"),
                             "-o", str(exe)])
    return exe


def run(exe):
    text = "".join(c.text() for c in CASES) + "".join(
        "table %d %d\n" % (n, cap) for cap in TABLE_CAPS for n in TABLE_NS)
    out = subprocess.run([str(exe)], input=text, capture_output=True,
                         text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stdout.splitlines()
    answer = {}
    at = 0
    for c in CASES:
        count = 1 + c.blk_first[-1] + len(c.lens)
        answer[c.name] = lines[at:at + count]
        at += count
    answer["table"] = lines[at:]
    return answer


@pytest.fixture(scope="module")
def answer(tmp_path_factory):
    return run(build(tmp_path_factory.mktemp("block"), "block_host", []))


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_every_block_as_the_walk_says(answer, case):
    got, want = answer[case.name], case.want()
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g == w, case.name


def test_shortcut_stops_at_the_multi_block_stream():
    """What the second batch is for: blk_first[b] == b holds for the five
    streams in front and for no block behind them but the long stream's
    first, and the walk puts three blocks behind it into stream 5."""
    c = next(c for c in CASES if c.name == "around-multi-slots")
    assert [b for b in range(c.blk_first[-1])
            if b < len(c.lens) and c.blk_first[b] == b] == [0, 1, 2, 3, 4, 5]
    assert [ln.split()[1] for ln in c.want()[1:1 + 14]] == (
        ["0", "1", "2", "3", "4"] + ["5"] * 4 + ["6", "7", "8", "9", "10"])


@pytest.mark.parametrize("direct", [0, 1])
def test_excess_gets_no_destination_and_changes_nothing_else(answer, direct):
    d = "direct" if direct else "slots"
    c = next(c for c in CASES if c.name == "excess-stream-" + d)
    assert c.blk_first[-1] > c.host_blocks and c.slot_first[-1] > c.host_slots
    got = answer[c.name]
    blocks = [ln.split() for ln in got[1:1 + c.blk_first[-1]]]
    assert [t[6] for t in blocks if t[1] == "2"] == ["past"] * 3
    # the blocks of the other streams: as in the batch without the excess
    alone = Case("alone", [B + 1, 2 * B], direct=direct)
    assert got[1:1 + alone.blk_first[-1]] == alone.want()[
        1:1 + alone.blk_first[-1]]
    assert got[-1] == "head " + "ee" * 10        # not a byte of its output
    # a stream that begins inside the launch and ends outside of it: its
    # later blocks get nothing where positions are final, and only slots the
    # host sized where they are not
    c = next(c for c in CASES if c.name == "excess-length-" + d)
    where = [ln.split()[6] for ln in answer[c.name][1:1 + c.blk_first[-1]]
             if ln.split()[1] == "1"]
    assert where == ["out", "none" if direct else "slot", "past", "past"]
    assert all(ln.endswith("past")
               for ln in answer[c.name][1 + 4:1 + c.blk_first[-1]])


def where(answer, name):
    c = next(c for c in CASES if c.name == name)
    return [ln.split()[6] for ln in answer[name][1:1 + c.blk_first[-1]]]


def test_the_rule_itself_says_no(answer):
    """Blocks that ARE inside the launch and still get no destination: it is
    block_dest that refuses them, by each of its two tests - the block's slot
    against host_slots where blocks go to slots, the stream's blocks against
    host_blocks where positions are final."""
    # four blocks in a launch of four, not one slot: block 0 in place, the
    # others nowhere; with final positions the stream fits and all four go out
    assert where(answer, "no-slots-slots") == ["out", "none", "none", "none"]
    assert where(answer, "no-slots-direct") == ["out"] * 4
    # slots 0, 1 of stream 0 exist, slots 2, 3 of stream 1 do not
    assert where(answer, "slots-straddle-slots") == [
        "out", "slot", "slot", "out", "none", "none"]
    assert where(answer, "slots-straddle-direct") == ["out"] * 6
    # the stream that ends outside host_blocks, with final positions
    assert where(answer, "excess-length-direct")[2:4] == ["out", "none"]
    for name in ("no-slots-slots", "slots-straddle-slots"):
        c = next(c for c in CASES if c.name == name)
        assert c.blk_first[-1] == c.host_blocks     # nothing is "past"


def test_table_shift_is_the_references(answer):
    """reference src/compress.rs:491-518: 256 entries, doubled while below
    both the block's length and the cap; the hash keeps the top log2(size)
    bits."""
    want = []
    for cap in TABLE_CAPS:
        for n in TABLE_NS:
            size = 256
            while size < n:
                size *= 2
            size = min(size, cap)
            want.append("%d %d" % (32 - (size.bit_length() - 1), size))
    assert answer["table"] == want


def test_sanitizers_clean(tmp_path, answer):
    """The same program with -fsanitize=address,undefined gives the same
    answer and exits clean."""
    exe = build(tmp_path, "block_host_san",
                ["-g", "-fsanitize=address,undefined",
                 "-fno-sanitize-recover=all"])
    assert run(exe) == answer
