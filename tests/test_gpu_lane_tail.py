"""GPU suite: the lane match finder at up to four probes a round (options
lane_tail_probes, lane_tail_idle_pct; tests/model_match_lane_multi.py is the
round as a model).  Every compress call must give the oracle's bytes and
lengths, and the bytes of the same context at lane_tail_probes 0 - in the lane
kernel alone on one and on two wavefronts and in the lane wavefronts of
k_match_both, at depths 2, 3 and 4, with the multi-probe round from the first
round on (lane_tail_idle_pct 0) and from the moment one per cent of the lanes
are out of work (1).  The batches mix block lengths inside every group of 64, so
short blocks end and the ticket runs out while the other lanes of their
wavefront are in the middle of a block, and the depth changes there: 256
blocks cut from the corpus (four times that for k_match_both, whose window
wavefronts take the first 512 blocks) and the set of tests/token_shapes.py.  The test
build counts the rounds that ran above the launch's own depth
(ctx.info("lane_multi_rounds")): zero at lane_tail_probes 0, not zero
otherwise - the proof that the form under test ran."""
import random

import pytest
import torch

import oracle_lib as O
import token_shapes as T

pytestmark = pytest.mark.gpu

KERNELS = ("lanes-1w", "lanes-2w", "both")
DEPTHS = (2, 3, 4)
IDLE_PCTS = (0, 1)

_made = {}


def _cut_streams():
    """256 one-block streams cut from the corpus files: in every group of 64,
    blocks under kMinNonLiteral (17 bytes), of a few dozen bytes, of a few
    KiB and of up to 64 KiB, in shuffled order."""
    rng = random.Random(41)
    files = [p.read_bytes() for p in sorted(O.CORPUS.iterdir())
             if p.suffix not in (".snappy", ".rawsnappy")
             and p.name != "COPYING"]
    out = []
    for group in range(4):
        sizes = ([rng.randrange(1, 17) for _ in range(6)] +
                 [17, 18, 31, 32, 33, 64] +
                 [rng.randrange(17, 300) for _ in range(12)] +
                 [rng.randrange(300, 8192) for _ in range(16)] +
                 [rng.randrange(8193, 65536) for _ in range(12)] +
                 [65535, 65536] + [65536] * 10)
        assert len(sizes) == 64
        rng.shuffle(sizes)
        for n in sizes:
            data = rng.choice([f for f in files if len(f) >= n])
            at = rng.randrange(0, len(data) - n + 1)
            out.append(data[at:at + n])
    return out


def _batch(name):
    """(expected streams, inputs on the device), made once per process."""
    if name not in _made:
        from rust_snappy_amd import batch
        if name == "cuts":
            data = _cut_streams()
            want = [O.compress(d) for d in data]
        elif name == "cuts4":
            want, data = _batch("cuts")[0] * 4, _cut_streams() * 4
        else:
            cases = T.the_set().everything()
            data = [c.data for c in cases]
            want = [c.comp for c in cases]
        _made[name] = (want, batch.StreamBatch.from_bytes(data))
    return _made[name]


def _context(kernel, spill=False):
    import rust_snappy_amd as R
    c = R.raw.Context(0)
    c.set_option("compress_mode", 1)
    c.set_option("lane_min_blocks", 1)
    c.set_option("match_kernel", 0)
    c.set_option("small_table_kernel", 0)
    # (blocks under 256 bytes are the lane kernel's too)
    c.set_option("tiny_stream_kernel", 0)
    c.set_option("lane_coresident", 1 if kernel == "both" else 0)
    c.set_option("lane_coresident_min_blocks", 1)
    if kernel != "both":
        # the plain kernel as the launch's own round, on 64 or 128 lanes
        c.set_option("lane_speculate", 0)
        c.set_test_option("lane_max_waves", 1 if kernel == "lanes-1w" else 2)
    if spill:  # a page or two: nearly every block spills
        c.set_option("token_pool_pct", 1)
        c.set_option("token_pool_min_pages", 0)
    return c


def _compress(c, want, src):
    from rust_snappy_amd import batch
    dst, lens, errs = batch.compress(c, src)
    assert all(e == (0, 0, 0, 0) for e in errs)
    assert lens.tolist() == [len(w) for w in want]
    host = dst.data.cpu().numpy()
    got = [host[int(o):int(o) + int(n)].tobytes()
           for o, n in zip(dst.offsets, lens)]
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"stream {i} ({len(w)} bytes expected)"
    return got


def _check(kernel, depth, pct, name, spill=False):
    # (k_match_both: its 512 window wavefronts draw their first blocks from
    # the back before a lane wavefront has drawn from the front - of 256
    # blocks the lanes may see none; of four times the batch they get half)
    want, src = _batch("cuts4" if name == "cuts" and kernel == "both"
                       else name)
    with _context(kernel, spill) as c:
        c.set_option("lane_tail_probes", 0)
        off = _compress(c, want, src)
        assert c.last_kernel() == ("k_match_both" if kernel == "both"
                                   else "k_match_blocks")
        assert c.info("lane_multi_rounds") == 0
        c.set_option("lane_tail_probes", depth)
        c.set_option("lane_tail_idle_pct", pct)
        on = _compress(c, want, src)
        multi = c.info("lane_multi_rounds")
        spilled = c.info("token_blocks_spilled")
        print(f"\n{name} {kernel} depth {depth} idle {pct} %: "
              f"{multi} multi-probe rounds, {spilled} blocks spilled")
        assert on == off
        assert multi > 0
        if spill:
            assert spilled > 0
        # ... and off again: the plain round on the tables the other left
        c.set_option("lane_tail_probes", 1)
        assert _compress(c, want, src) == off
        assert c.info("lane_multi_rounds") == 0


@pytest.mark.parametrize("pct", IDLE_PCTS)
@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("kernel", KERNELS)
def test_corpus_cuts(built, kernel, depth, pct):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    _check(kernel, depth, pct, "cuts")


@pytest.mark.parametrize("pct", IDLE_PCTS)
@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("kernel", KERNELS)
def test_token_shapes(built, kernel, depth, pct):
    """The whole set of tests/token_shapes.py: a token at every edge of the
    token format, dense blocks, all exception pages, multi-block streams."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    _check(kernel, depth, pct, "shapes")


@pytest.mark.parametrize("kernel", ("lanes-1w", "lanes-2w"))
def test_blocks_spill_while_the_tail_form_runs(built, kernel):
    """A token pool of a page or two: nearly every block finds it empty in
    the middle of its rounds and goes on spilled.  (Not k_match_both: what its
    65 536 lanes keep in hand is a pool that this batch does not empty.)"""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    _check(kernel, 4, 1, "cuts", spill=True)
