"""The lane match finder's round with up to four probes
(tests/model_match_lane_multi.py: the order of table reads, writes and
forwarding of match_blocks at a run-time depth) must give the oracle's stream
- at every depth, with the depth raised at round 0, in the middle of a block
and never - on every 64 KiB block of the corpus, on the blocks of
tests/token_shapes.py and on 200 random and structured blocks of 17 bytes to
64 KiB.  Depth 1 must be the plain model's rounds and depth 2 the speculating
model's.  Prints the rounds per depth and input: what the kernel's gain in a
latency-bound phase is estimated from."""
import random

import pytest

import model_match_lane as M1
import model_match_lane_multi as M
import oracle_lib as O
import token_shapes as T

BLOCK = 65536
DEPTHS = (1, 2, 3, 4)


def _switches(rng, data):
    """round 0, a random round inside the block, never"""
    _, plain, _ = M.compress_one_block_stream(data, 1)
    return (0, rng.randrange(1, max(2, plain)), None)


def _check(data, want, depth, switch):
    got, rounds, multi = M.compress_one_block_stream(data, depth, switch)
    assert got == want, (depth, switch, len(data), bytes(data[:24]).hex())
    if depth == 1 or switch is None:
        assert multi == 0
    elif switch == 0:
        assert multi == rounds
    return rounds, multi


def _corpus_blocks():
    for path in sorted(O.CORPUS.iterdir()):
        if path.suffix in (".snappy", ".rawsnappy") or path.name == "COPYING":
            continue
        data = path.read_bytes()
        for at in range(0, len(data), BLOCK):
            if len(data) - at >= 17:
                yield path.name, data[at:at + BLOCK]


def test_every_corpus_block_at_every_depth():
    """Depth 1 once (it is "never" at every depth), depths 2..4 from round 0
    and from a random round of the block."""
    rng = random.Random(5)
    per_file = {}
    for name, data in _corpus_blocks():
        want = O.compress(data)
        sw = _switches(rng, data)
        row = per_file.setdefault(name, [0] * 5)
        row[0] += 1
        row[1] += _check(data, want, 1, 0)[0]
        _check(data, want, 4, None)
        for depth in (2, 3, 4):
            row[depth] += _check(data, want, depth, 0)[0]
            rounds, multi = _check(data, want, depth, sw[1])
            assert 0 < multi <= rounds
    print("\nrounds per block at depth 1, and depth 2..4 as a share of them")
    tot = [0] * 5
    for name, row in per_file.items():
        tot = [a + b for a, b in zip(tot, row)]
        print(f"  {name:28s} {row[0]:3d} blocks {row[1] // row[0]:6d}  " +
              "  ".join(f"{row[d] / row[1]:.3f}" for d in (2, 3, 4)))
    print(f"  {'all':28s} {tot[0]:3d} blocks {tot[1] // tot[0]:6d}  " +
          "  ".join(f"{tot[d] / tot[1]:.3f}" for d in (2, 3, 4)))
    # the more probes a round resolves, the fewer rounds
    assert tot[4] < tot[3] < tot[2] < 0.85 * tot[1]


def _made_blocks():
    rng = random.Random(23)
    blob = b"".join(d for _, d in _corpus_blocks())
    out = []
    sizes = [17, 18, 19, 20, 31, 32, 33, 47, 48, 63, 64, 65, 100, 255, 256,
             257, 1000, 4096, 5000, BLOCK - 1, BLOCK]
    while len(sizes) < 200:
        sizes.append(rng.choice((rng.randrange(17, 200),
                                 rng.randrange(200, 5000),
                                 rng.randrange(5000, 30000))))
    for i, n in enumerate(sizes):
        kind = i % 5
        if kind == 0:        # a cut of the corpus
            at = rng.randrange(0, len(blob) - n)
            out.append(blob[at:at + n])
        elif kind == 1:      # a tiny alphabet: consecutive positions share slots
            alpha = rng.choice((1, 2, 3, 4))
            out.append(bytes(rng.randrange(alpha) for _ in range(n)))
        elif kind == 2:      # noise
            out.append(bytes(rng.randrange(256) for _ in range(n)))
        elif kind == 3:      # a period
            unit = bytes(rng.randrange(256)
                         for _ in range(rng.choice((1, 2, 3, 5, 13, 37))))
            out.append((unit * (n // len(unit) + 1))[:n])
        else:                # text with noise between
            at = rng.randrange(0, len(blob) - n)
            mixed = bytearray(blob[at:at + n])
            for _ in range(n // 50):
                mixed[rng.randrange(n)] = rng.randrange(256)
            out.append(bytes(mixed))
    return out


def test_made_blocks_at_every_depth_and_switch():
    rng = random.Random(29)
    blocks = _made_blocks()
    assert len(blocks) == 200
    for data in blocks:
        want = O.compress(data)
        for depth in DEPTHS:
            for switch in _switches(rng, data):
                _check(data, want, depth, switch)


def test_token_shape_blocks():
    """Every one-block case of the set (the streams are made of them), each at
    one depth and one switch, all combinations in turn."""
    rng = random.Random(31)
    cases = T.the_set().single_blocks()
    combos = [(d, k) for d in (2, 3, 4) for k in (0, 1)]
    seen = set()
    for i, case in enumerate(cases):
        if len(case.data) < 17:
            continue
        depth, k = combos[i % len(combos)]
        switch = 0 if k == 0 else rng.randrange(1, 2000)
        _check(case.data, case.comp, depth, switch)
        seen.add((case.family, depth, k))
    for family in ("grid", "dense", "exceptions"):
        assert {(family, d, k) for d, k in combos} <= seen, family


@pytest.mark.parametrize("depth,spec", [(1, False), (2, True)])
def test_depths_1_and_2_are_the_two_existing_rounds(depth, spec):
    """Same tokens in the same number of rounds as model_match_lane."""
    blocks = [d for _, d in _corpus_blocks()][::7] + _made_blocks()[::9]
    assert len(blocks) > 20
    for data in blocks:
        a, ra = M1.lane_tokens(data, spec)
        b, rb, _ = M.lane_tokens(data, depth, 0)
        assert (a, ra) == (b, rb), len(data)
