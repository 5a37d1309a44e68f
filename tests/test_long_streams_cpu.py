"""The inputs of tests/test_gpu_long_streams.py, on the CPU.

tests/long_streams.py builds large raw streams from a pool of 64 KiB blocks
compressed once each.  Here: that construction is O.compress of the
concatenation, and every shape the GPU file decodes reaches the plan
geometry it is there for (csrc/snapmi_streamplan.hpp through
tests/streamplan_host.cpp), so that a change to the planner or to the shapes
cannot quietly shrink the GPU tests under the levels they target."""
import numpy as np
import pytest

import foreign
import long_streams as LS
import oracle_lib as O
from test_streamplan_cpu import P, plan  # noqa: F401 - P is a fixture

MIB = 1 << 20
SWITCH = 256 * MIB   # long bytes from which segments are 4 KiB


@pytest.fixture(scope="module")
def small_pool():
    return LS.Pool({k: 3 for k in LS.KINDS}, seed=7)


@pytest.mark.parametrize("tail", [0, 1, 7, 59, 61, 4000, 65535])
def test_construction_is_the_compression_of_the_concatenation(small_pool,
                                                               tail):
    p = small_pool
    rng = np.random.default_rng(tail)
    for nb, w in [(1, {"text": 1}), (2, {"random": 1}), (6, LS.MIX),
                  (9, {"zeros": 1, "runs": 1}), (5, {"noise": 1})]:
        idx = p.order(rng, nb, w)
        t = (p.tail(LS.KINDS[tail % len(LS.KINDS)], tail, rng) if tail
             else None)
        st = p.stream(idx, t)
        data = st.expected()
        assert len(data) == st.dlen == nb * LS.BLOCK + tail
        comp = st.bytes()
        assert len(comp) == st.in_len
        assert comp == O.compress(data), (nb, w, tail)
        assert O.decompress(comp) == data


def test_tail_only_stream(small_pool):
    rng = np.random.default_rng(3)
    st = small_pool.stream([], small_pool.tail("text", 1000, rng))
    assert st.bytes() == O.compress(st.expected())


def test_pool_blocks_distinct_and_neighbours_differ():
    p = LS.pool()
    assert len({r.tobytes() for r in p.raw}) == len(p.raw)
    for k in LS.KINDS:
        assert len(p.of_kind[k]) >= 2, k
    # every kind is there in a long order, and no block follows itself
    idx = p.order(np.random.default_rng(5), 20000, LS.MIX)
    assert not np.any(idx[1:] == idx[:-1])
    assert {p.kinds[i] for i in idx} == set(LS.KINDS)
    # the kinds are what they say: a literal, dense copies, text
    lens = {k: p.blen[p.of_kind[k]] for k in LS.KINDS}
    assert np.all(lens["random"] > LS.BLOCK)
    assert np.all(lens["zeros"] < 4096)
    assert np.all(lens["text"] < LS.BLOCK * 3 // 4)


def test_module_pool_construction():
    st = LS.mixed(9, 12, tail_len=12345)
    assert st.bytes() == O.compress(st.expected())
    st = LS.mixed(10, 3, weights={"random": 1}, tail_len=70, tail_kind="runs")
    assert st.bytes() == O.compress(st.expected())


def test_foreign_long_stream():
    comp, want = LS.foreign_long(1, lit_lens=(1 << 20, 70000))
    assert O.decompress(comp) == want
    # a literal with 3 length bytes, one with 4, copy-4 elements
    comp, want = LS.foreign_long(2)
    assert len(want) > (1 << 24)
    assert O.decompress(comp) == want
    assert b"\xfc" + ((1 << 24) + 6).to_bytes(4, "little") in comp
    assert b"\xf8" + ((1 << 20) - 1).to_bytes(3, "little") in comp


def geometry(P, lens, bounds, lone, forced=None):  # noqa: F811
    seg, groups = forced if forced else (0, 0)
    p = plan(P, lens, bounds, lone=lone, seg_log2=seg, scan_segs=groups)
    assert p is not None
    return p


# (seg_log2, scan_segs, nsuper3 lower bound, nsuper3 upper bound) per shape
LADDER_WANT = {
    "scan8": (10, 8, 2, 2),
    "scan16": (10, 16, 3, 8),
    "scan32": (10, 32, 8, 16),
    "under256": (10, 64, 60, 64),
    "over256": (12, 64, 16, 64),
    "4k-small": (12, 8, 2, 4),
    "spread3x2": (10, 64, 65, 1 << 30),
}


@pytest.mark.parametrize("name", list(LS.LADDER))
def test_ladder_geometry(P, name):  # noqa: F811
    target, forced = LS.LADDER[name]
    st = LS.ladder(name)
    assert st.dlen % LS.BLOCK != 0
    assert st.in_len >= target
    # the caller's buffer is exactly dlen: lone_stream_bound gives dlen
    p = geometry(P, [st.in_len], [st.dlen], True, forced)
    seg, scan, lo, hi = LADDER_WANT[name]
    g = p["slots"][0]
    assert (p["seg_log2"], p["scan_segs"]) == (seg, scan), (name, p)
    assert lo <= g["nsuper3"] <= hi, (name, g)
    if name == "spread3x2":
        assert p["grid_spread3"] >= 2
    if not forced:
        assert (st.in_len < SWITCH) == (seg == 10)


@pytest.mark.parametrize("tail", [False, True])
def test_limit_geometry(P, tail):  # noqa: F811
    st = LS.limit(tail)
    assert st.dlen == (1 << 32) - (1 if tail else LS.BLOCK)
    assert (1 << 30) < st.in_len < 1500 * MIB
    p = geometry(P, [st.in_len], [st.dlen], True)
    g = p["slots"][0]
    assert (p["seg_log2"], p["scan_segs"]) == (12, 64)
    assert g["nsuper3"] > 64 and p["grid_spread3"] >= 2
    assert g["kmax"] > 65536
    # pieces: 65535, or 65536 with the tail
    assert -(-st.dlen // LS.BLOCK) == (65536 if tail else 65535)


def batch_geometry(P, items, forced=None):  # noqa: F811
    """The plan of the streams k_long_plan takes from a batch of (Stream or
    bytes, cap) items, and how many it takes."""
    lens, bounds = [], []
    for src, cap in items:
        if isinstance(src, LS.Stream):
            n, dl = src.in_len, src.dlen
        else:
            n = len(src)
            try:
                dl = O.decompress_len(src) if n else 0
            except O.SnapError:
                continue
        if n >= (32 << 10) and dl <= cap and LS.long_stream_rule(n, dl):
            lens.append(n)
            bounds.append(dl)
    return geometry(P, lens, bounds, False, forced), len(lens)


def test_batch_limit_geometry(P):  # noqa: F811
    p, nl = batch_geometry(P, LS.batch_items("long4096"))
    assert nl == 4096 and p["seg_log2"] == 10
    assert len(LS.batch_items("long4096")) <= 16384
    for st, _ in LS.batch_items("long4096"):
        if isinstance(st, LS.Stream):
            assert (33 << 10) <= st.in_len <= (80 << 10)
    _, nl = batch_geometry(P, LS.batch_items("long4097"))
    assert nl == 4097
    for name, n in (("n16384", 16384), ("n16385", 16385)):
        items = LS.batch_items(name)
        assert len(items) == n
        _, nl = batch_geometry(P, items)
        assert 0 < nl <= 4096


def test_batch_mixed_geometry(P):  # noqa: F811
    items = LS.batch_items("mixed")
    p, nl = batch_geometry(P, items, (10, 0))
    assert nl > 1000
    assert max(g["nsuper3"] for g in p["slots"]) > 64
    assert p["grid_spread3"] > len(p["slots"])   # two for the big one
    exact = [s for s, _ in items
             if isinstance(s, LS.Stream) and s.in_len == 32 << 10]
    assert len(exact) >= 1000
    assert sum(1 for s, c in items
               if isinstance(s, LS.Stream) and c == s.dlen - 1) >= 4


@pytest.mark.parametrize("side", ["under", "over"])
def test_batch_natural_geometry(P, side):  # noqa: F811
    items = LS.batch_items(side + "256")
    p, nl = batch_geometry(P, items)
    streams = [s for s, _ in items if isinstance(s, LS.Stream)]
    assert nl == len(streams) > 1   # every one of them is taken
    total = sum(s.in_len for s in streams)
    assert abs(total - SWITCH) < 4 * MIB
    assert (total < SWITCH) == (side == "under")
    assert p["seg_log2"] == (10 if side == "under" else 12)


def test_scan_segs_by_size_cover_8_to_64(P):  # noqa: F811
    got = set()
    for name, (_, forced) in LS.LADDER.items():
        if forced is None or forced[1] == 0:
            st = LS.ladder(name)
            got.add(geometry(P, [st.in_len], [st.dlen], True,
                             forced)["scan_segs"])
    assert got == {8, 16, 32, 64}


def test_error_streams_reach_their_positions():
    for name in LS.ERROR_CASES:
        comp, cap, where = LS.error_case(name, materialize=False)
        if name == "beyond2g":
            assert where > (1 << 31)
        assert cap > 0


def test_error_cases_against_oracle_small():
    """The mutations of error_case on a small stream give the errors they
    are named for (the GPU file compares the kernels with the oracle on the
    full ones)."""
    st = LS.mixed(30, 6, tail_len=5000)
    for name in LS.ERROR_CASES:
        if name == "beyond2g":
            continue
        comp, cap = LS.mutate(st, name)
        with pytest.raises(O.SnapError) as e:
            O.decompress(comp, cap)
        kind = e.value.name
        want = {"last_block": "Offset", "two_blocks": "Offset",
                "hdr+1": "HeaderMismatch", "hdr+65536": "HeaderMismatch",
                "cut": None, "hdr-1": None, "hdr-65536": None}[name]
        if want:
            assert kind == want, (name, e.value)
    # two corrupt blocks: the first in stream order is reported
    comp, cap = LS.mutate(st, "two_blocks")
    with pytest.raises(O.SnapError) as e:
        O.decompress(comp, cap)
    assert e.value.c == 0 and e.value.b < 2 * LS.BLOCK


def test_varint_roundtrip():
    for v in (0, 127, 128, (1 << 32) - 1, (1 << 32) - LS.BLOCK):
        b = foreign.varint(v)
        assert O.decompress_len(b + b"\x00") == v
