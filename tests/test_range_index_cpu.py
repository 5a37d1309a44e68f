"""The range-read rules on the CPU: csrc/snapmi_blockindex.hpp, compiled into
a stand-alone program (tests/rangeindex_host.cpp - the source the kernels and
the host entry point compile), against tests/rangeindex_ref.py over the
shapes of the GPU tests and seeded random draws that include the 2^64 edge;
the exports and bindings of the two calls."""
import random
import subprocess

import pytest

import blockindex_ref as B
import rangeindex_ref as R
from conftest import ROOT

U64 = 1 << 64
DLENS = [0, 1000, 65536, 131072, 200000, 70000]
SHAPES = [(0, 1), (65535, 2), (100, 300), (65536, 65536), (1000, 189000),
          (0, 0), (65536, 0), (U64 - 1, 1), (U64 - 1, 0), (0, U64 - 1),
          (1, U64 - 1), (U64 - 65536, 65536), (U64 - 65537, 65536),
          (65536, 1), (65535, 1), (0, 65536), (0, 65537), (131071, 2)]
SHAPES += [(0, d) for d in DLENS] + [(d - 1, 1) for d in DLENS if d]
SHAPES += [(d, 0) for d in DLENS] + [(d, 1) for d in DLENS]


def build(tmp_path_factory, name, extra):
    exe = tmp_path_factory.mktemp(name) / "rangeindex_host"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror",
                           *extra,
                           str(ROOT / "tests" / "rangeindex_host.cpp"),
                           "-o", str(exe)])

    def run(lines):
        out = subprocess.run([str(exe)], input="".join(s + "\n"
                                                       for s in lines),
                             capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stderr
        rows = [[int(t) for t in ln.split()]
                for ln in out.stdout.splitlines()]
        assert len(rows) == len(lines)
        return rows
    return run


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    return build(tmp_path_factory, "rangeindex", [])


def draws(seed, count):
    rng = random.Random(seed)
    edge_vals = [0, 1, 65535, 65536, 65537, U64 - 1, U64 - 2, U64 - 65536,
                 U64 - 65537, 1 << 32, (1 << 32) - 1, 1 << 63]
    out = []
    for _ in range(count):
        kind = rng.randrange(4)
        if kind == 0:
            off, n = rng.choice(edge_vals), rng.choice(edge_vals)
        elif kind == 1:
            off = rng.randrange(0, 1 << 20)
            n = rng.randrange(0, 1 << 20)
        elif kind == 2:
            off = rng.randrange(0, 64) * 65536 + rng.choice([0, 0, 1, 65535])
            n = rng.randrange(0, 8) * 65536 + rng.choice([0, 0, 1, 65535])
        else:
            off = U64 - rng.randrange(1, 1 << 18)
            n = rng.randrange(0, 1 << 18)
        out.append((off, n))
    return out


def test_blocks_edges_and_spans(prog):
    cases = SHAPES + draws(20260101, 4000)
    rows = prog([f"B {o} {n}" for o, n in cases])
    probes, want = [], []
    for (o, n), row in zip(cases, rows):
        cnt, k0 = R.blocks(o, n)
        assert row == [cnt, k0, R.edges(o, n)], (o, n)
        # the first, the last and one inner touched block
        for k in sorted({k0, k0 + cnt - 1, k0 + cnt // 2} if cnt else ()):
            probes.append(f"E {o} {n} {k}")
            want.append([int(R.edge(o, n, k)), R.edge_slot(o, n, k),
                         *R.span(o, n, k)])
    assert prog(probes) == want
    # the identities the kernels rest on
    for o, n in cases:
        cnt, k0 = R.blocks(o, n)
        if cnt == 0 or cnt > 64:
            continue
        covered, rooms = 0, set()
        for k in range(k0, k0 + cnt):
            a, to, m = R.span(o, n, k)
            assert to == covered and 0 < m <= 65536 and a + m <= 65536
            covered += m
            if R.edge(o, n, k):
                assert k in (k0, k0 + cnt - 1)
                rooms.add(R.edge_slot(o, n, k))
            else:
                assert (a, m) == (0, 65536)
        assert covered == n
        assert sorted(rooms) == list(range(R.edges(o, n)))
    assert R.blocks(1000, 189000) == (3, 0) and R.edges(1000, 189000) == 2
    assert R.blocks(65536, 65536) == (1, 1) and R.edges(65536, 65536) == 0
    assert R.blocks(65535, 2) == (2, 0) and R.edges(65535, 2) == 2
    assert R.blocks(U64 - 1, 1) == (0, (U64 - 1) // 65536)


def test_pieces_sum_saturates(prog):
    sets = [[], [(0, 0)], SHAPES, draws(7, 50),
            [(0, U64 - 1)] * 70000]
    lines = [f"P {len(s)} " + " ".join(f"{o} {n}" for o, n in s)
             for s in sets]
    rows = prog(lines)
    for s, row in zip(sets, rows):
        assert row == [R.pieces([o for o, _ in s], [n for _, n in s])]
    assert rows[-1] == [U64 - 1]


def test_groups(prog, tmp_path_factory):
    """bi_range_groups, which snapmi_decompress_ranges_indexed cuts a call
    with, against room_groups - the model the GPU tests count groups with -
    and the pieces and rooms of every group summed from the per-range rules;
    the same lines through a build with -fsanitize=address,undefined."""
    floor, big = 128 << 10, 1 << 30
    none, one, two, wide = (0, 65536), (1, 10), (65535, 2), (1, 131072)
    empty, wraps = (70000, 0), (U64 - 1, 2)
    assert [R.edges(*r) for r in (none, one, two, wide, empty, wraps)] == \
        [0, 1, 2, 2, 0, 0]
    lists = [
        [],
        [none, one, two, wide, empty, wraps],
        [wraps, empty, wide, none, two, one, one, none, empty, two],
        [one, one, one],              # a group closes exactly when full
        [one, none, one, empty, one, one, two],
        [two, one, one, one],         # the first range alone fills the floor
        [wide, wide, none, wide],
        [none] * 5, [empty] * 3, [wraps],
        [(1000, 189000)] * 3 + [(0, 1 << 20), (5, (1 << 20) + 7)],
    ]
    lists += [[r] for r in (none, one, two, wide, empty, wraps)]   # m = 1
    rng = random.Random(20261020)
    for _ in range(300):
        lists.append(rng.choices([none, one, two, wide, empty, wraps]
                                 + draws(rng.randrange(1 << 30), 12),
                                 k=rng.randrange(1, 41)))
    cases = [(sc, rs) for rs in lists for sc in (floor, big)]
    # (a few at scratch sizes in between, a partial room included)
    cases += [(sc, rs) for rs in lists[:40] for sc in (3 * 65536, 327679)]
    lines, want = [], []
    for sc, rs in cases:
        offs, lens = [o for o, _ in rs], [n for _, n in rs]
        lines.append(f"G {sc} {len(rs)} " + " ".join(f"{o} {n}"
                                                     for o, n in rs))
        groups = R.room_groups(offs, lens, sc)
        rows = [(g[0], len(g), sum(R.blocks(*rs[r])[0] for r in g),
                 sum(R.edges(*rs[r]) for r in g)) for g in groups]
        assert [r for g in groups for r in g] == list(range(len(rs)))
        want.append([len(rows), max([q[2] for q in rows], default=0),
                     max([q[3] for q in rows], default=0),
                     *[v for q in rows for v in q]])
    got = prog(lines)
    assert got == want
    sanitized = build(tmp_path_factory, "rangeindex_sanitized",
                      ["-g", "-fsanitize=address,undefined",
                       "-fno-sanitize-recover=all"])
    assert sanitized(lines) == want
    # what the lists were chosen for, at the floor
    by = {(sc, tuple(rs)): w for (sc, rs), w in zip(cases, want)}
    assert by[floor, (one, one, one)] == [2, 2, 2, 0, 2, 2, 2, 2, 1, 1, 1]
    assert by[floor, (two, one, one, one)][:3] == [3, 2, 2]
    assert by[floor, (two, one, one, one)][3:7] == [0, 1, 2, 2]
    assert by[big, (two, one, one, one)] == [1, 5, 5, 0, 4, 5, 5]
    assert by[floor, (wraps,)] == [1, 0, 0, 0, 1, 0, 0]


def test_local_index_rule(prog):
    lines, want = [], []

    def usable(in_len, hdr, dlen, idx, first, nxt):
        lines.append(f"U {in_len} {hdr} {dlen} {first} {nxt} {len(idx)} "
                     + " ".join(map(str, idx)))
        want.append([int(R.stream_usable(in_len, hdr, dlen, idx, first, nxt,
                                         len(idx)))])
        return want[-1][0]

    def bad_block(e, in_len, off, n):
        lines.append(f"K {in_len} {off} {n} " + " ".join(map(str, e)))
        k = R.first_bad_block(e, in_len, off, n)
        want.append([U64 - 1 if k is None else k])
        return k

    for dlen in DLENS:
        hdr = len(B.varint(dlen))
        blocks = B.entries(dlen) - 1
        in_len = hdr + 100 * blocks
        good = [hdr + 100 * k for k in range(blocks)] + [in_len]
        if dlen == 0:
            good = [1]
            in_len = 1
        n = len(good)
        # a one-block stream with its 2 entries is usable (not "indexed")
        assert usable(in_len, hdr, dlen, good, 0, n)
        assert usable(in_len, hdr, dlen, [9] * 3 + good + [9], 3, 3 + n)
        assert not usable(in_len, hdr, dlen, good, 0, n - 1)   # count
        assert not usable(in_len, hdr, dlen, good + [5], 0, n + 1)
        assert not usable(in_len, hdr, dlen, good[:-1], 0, n)  # past the end
        assert not usable(in_len, hdr, dlen, good, 1, 0)       # reversed
        assert not usable(in_len, hdr, dlen, good, U64 - 1, n)
        assert not usable(in_len, hdr, dlen, [0] * n, 0, n)    # all zero
        assert not usable(in_len, hdr + 1, dlen, good, 0, n)   # entry 0
        assert not usable(in_len + 1, hdr, dlen, good, 0, n)   # last entry
        if blocks < 2:
            continue
        # the block's part looks at the touched blocks only
        for off, ln in [(0, dlen), (0, 1), (dlen - 1, 1), (65535, 2),
                        (65536, 65536), (1000, dlen - 1001)]:
            assert bad_block(good, in_len, off, ln) is None
            swapped = good[:1] + [good[2], good[1]] + good[3:]
            cnt, k0 = R.blocks(off, ln)
            k = bad_block(swapped, in_len, off, ln)
            touched = set(range(k0, k0 + cnt))
            # entries 1 and 2 swapped: blocks 0 (if blocks > 2 the pair
            # (e0, e2) still rises), 1 and 2 can be hit
            assert (k is None) == (not ({1} & touched)), (off, ln, k)
            beyond = good[:-1] + [in_len + 7]
            k = bad_block(beyond, in_len, off, ln)
            assert (k is None) == (blocks - 1 not in touched)
    rows = prog(lines)
    assert rows == want


def test_binding_exposes_the_two_calls(built):
    from rust_snappy_amd import _lib, batch, raw
    L = _lib.load()
    P = _lib.load_product()
    names = {s[0] for s in _lib.SYMBOLS}
    for name in ("snapmi_range_pieces", "snapmi_decompress_ranges_indexed"):
        assert name in names
        assert hasattr(L, name) and hasattr(P, name)
    # host code: no GPU needed
    for s in ([], SHAPES, draws(3, 200)):
        offs, lens = [o for o, _ in s], [n for _, n in s]
        assert raw.range_pieces(offs, lens) == R.pieces(offs, lens)
    assert raw.range_pieces([1000], [189000]) == 3
    assert callable(batch.read_ranges)
    assert callable(raw.decompress_ranges_indexed)
