"""The inputs of tests/token_shapes.py hold what they were built to hold - the
oracle's parse says so, not the builder - and the parser that reads that parse
is exact: re-encoding its tokens by the reference's emit rules gives the
oracle's stream back byte for byte.  The window kernel's walk
(tests/span_wave_host.cpp: the text of snapmi_span.hpp on the host) runs on
every single-block input of the set and must give the oracle's stream too.
Prints the reachable-length table and the measured counts (pytest -s)."""
import ctypes as C
import subprocess

import pytest

import oracle_lib as O
import token_shapes as T
from conftest import ROOT


@pytest.fixture(scope="module")
def S():
    return T.the_set()


def test_reachable_literal_lengths_are_the_recorded_ones():
    found = T.literal_edges()
    print()
    for where, edges in found.items():
        for (lo, hi), (below, above) in edges.items():
            print(f"literal {lo}/{hi} {where}: reachable {below} and {above}")
    assert found == T.REACHABLE
    # every threshold has a reachable length on both sides, at both places
    for edges in found.values():
        for (lo, hi), (below, above) in edges.items():
            assert below is not None and below <= lo
            assert above is not None and above >= hi
    # what the docstring of REACHABLE says of 60: no token with a copy has it
    assert not T._try("first", (60, 8, "max"))
    assert not T._try("middle", (60, 8, 61))


def test_grid_holds_every_target_at_every_place_in_both_classes(S):
    targets = T.grid_targets()
    print("\ngrid targets reachable", {p: len(v) for p, v in targets.items()},
          "unreachable", T.unreachable_targets(),
          "blocks", len(S.grid_blocks))
    assert T.GRID_DROPPED == []
    seen = {(cls, p): set() for cls in ("small", "large") for p in T.PLACES}
    finals = {"small": set(), "large": set()}
    end_literals = {"small": set(), "large": set()}
    sizes = {"small": set(), "large": set()}
    for blk, case in zip(S.grid_blocks, S.grid):
        toks = case.blocks[0]
        assert toks == blk.plan and len(case.blocks) == 1
        n = len(blk.data)
        assert 4096 < n <= 8192 if blk.cls == "small" else n > 8192
        sizes[blk.cls].add(n)
        if blk.family == "final":
            assert toks[-1] == (blk.final, 0, 0)
            end_literals[blk.cls].add(blk.final)
            continue
        at = [0]
        for t in toks:
            at.append(at[-1] + t[0] + t[1])
        for place, idx in blk.marks.items():
            L, Cc, Oe = blk.asked[place]
            got = toks[idx]
            assert got[:2] == (L, Cc), (place, got)
            assert got[2] == (at[idx] + L if Oe == "max" else Oe)
            if place == "first":
                assert idx == 0
            if place == "last":
                assert at[idx + 1] + blk.final == n
                assert len(toks) == idx + (2 if blk.final else 1)
                finals[blk.cls].add(blk.final)
            if place == "middle":
                assert 0 < idx < len(toks) - 2
            seen[(blk.cls, place)].add(blk.asked[place])
    for (cls, place), got in seen.items():
        assert got == {t for t, _ in targets[place]}, (cls, place)
        # every edge of the issue's list, or its recorded neighbour
        lits = {t[0] for t in got}
        assert lits == set(T.literal_values(place))
        assert {t[1] for t in got} == set(T.COPY_EDGES)
        want_offs = set(T.OFFSET_EDGES)
        if place == "first":    # no source 2 047 back in front of a literal
            want_offs -= {2047, 2048}   # of 1 031 bytes at a block's start
        assert {t[2] for t in got} == want_offs, (cls, place)
        # the copy1 / copy2 edge, all four corners
        if place != "first":
            for Cc in (11, 12):
                for Oe in (2047, 2048):
                    assert any(t[1:] == (Cc, Oe) for t in got)
    for cls in ("small", "large"):
        assert finals[cls] == set(T.FINALS), (cls, finals[cls])
        assert end_literals[cls] == {60, 61, 64, 65, 256, 257, 1023, 1024}
    assert 8192 in sizes["small"] and 8193 in sizes["large"]
    # the largest offset a 64 KiB block admits, at every final literal
    for blk in S.full:
        tok = blk.plan[blk.marks["last"]]
        assert len(blk.data) == T.BLOCK and tok[2] >= T.BLOCK - 76 - 65 - 3
        assert tok[2] == T.BLOCK - blk.final - tok[1]
    assert {b.final for b in S.full} == set(T.FINALS)


def test_dense_blocks_hold_fifteen_thousand_tokens(S):
    assert len(S.dense) == T.DENSE_BLOCKS == 128
    counts = [len(c.blocks[0]) for c in S.dense]
    print("\ndense tokens per block: min", min(counts), "max", max(counts))
    assert counts == S.dense_counts
    assert min(counts) >= T.DENSE_MIN_TOKENS == 15000
    assert max(counts) <= 16385
    assert all(len(c.data) == T.BLOCK for c in S.dense)
    assert len(set(c.data for c in S.dense)) == 128
    # token pages at full density: 30 pages and more of the 33 a block has
    assert min(-(-n // T.TOK_PAGE) for n in counts) >= 30
    # (the stream of the 128: parsed on its own, not taken from the blocks)
    stream = T.block_tokens(S.dense_stream.comp)
    assert stream == [c.blocks[0] for c in S.dense] == S.dense_stream.blocks


def test_exception_blocks_reach_all_four_pages_and_the_token_indices(S):
    by = {c.name: c for c in S.exceptions}
    print()
    for c in S.exceptions:
        assert len(c.data) == T.BLOCK and len(c.blocks) == 1
        print(c.name, "tokens", len(c.blocks[0]), "exceptions",
              T.exceptions(c.blocks[0]))
    phrases = [c for c in S.exceptions if c.name.startswith("phrases")]
    assert len(phrases) == 2
    for c in phrases:
        n = T.exceptions(c.blocks[0])
        assert n >= T.EXC_MIN == 800 and n > 3 * T.EXC_PAGE
        assert n <= 1008
    mixed = by["mixed"].blocks[0]
    assert any(t[0] >= 1024 and 0 < t[1] <= 64 for t in mixed)
    assert any(t[0] < 1024 and t[1] > 64 for t in mixed)
    assert any(t[0] >= 1024 and t[1] > 64 for t in mixed)
    assert mixed[-1][0] >= 1024 and mixed[-1][1] == 0   # a final literal too
    for K in (63, 64, 511, 512):
        toks = by[f"at-{K}"].blocks[0]
        assert [i for i, t in enumerate(toks) if T.is_exception(t)] == [K]


def test_streams_and_the_size_of_the_set(S):
    blocks = {c.name: len(c.blocks) for c in S.streams}
    assert sorted(blocks.values()) == [2, 3, 3, 5, 5]
    last = S.streams[-1]
    assert last.name == "stream-grid-last"
    assert 4096 < len(last.data) % T.BLOCK < 4200
    assert last.blocks[-1] in [b.plan for b in S.grid_blocks]
    for c in S.streams:     # exceptions in blocks at a position k > 0
        assert any(T.exceptions(b) for b in c.blocks[1:]), c.name
    # ... all four exception pages and 30 token pages there too
    assert sum(1 for c in S.streams for b in c.blocks[1:]
               if T.exceptions(b) > 3 * T.EXC_PAGE) >= 3
    assert sum(1 for c in S.streams for b in c.blocks[1:]
               if len(b) >= T.DENSE_MIN_TOKENS) >= 3
    assert len(S.dense_stream.blocks) == 128
    everything = S.everything()
    assert all(len(c.data) >= 4096 for c in everything)
    total = sum(len(c.data) for c in everything)
    print("\nthe set:", len(everything), "inputs,", total, "bytes")
    assert total < 26 << 20


def test_tokens_reencoded_are_the_oracle_stream(S):
    """tokens() loses nothing: the reference's emit rules over its tokens give
    the oracle's stream back - the whole set (the 128 dense blocks within the
    stream that strings them together: the same blocks, the same tokens) and
    the corpus."""
    for c in S.grid + [S.dense_stream] + S.exceptions + S.streams:
        toks = T.tokens(c.comp)
        assert toks == [t for b in c.blocks for t in b]
        assert T.encode(c.data, toks) == c.comp, c.name
    for name, data in O.corpus_round():
        comp = O.compress(data)
        assert T.encode(data, T.tokens(comp)) == comp, name


def test_token_parts_is_the_reference_emit_rule():
    """Every literal length to 1 100 and 65 536, every copy length to 300, at
    offsets on both sides of 2 047 / 2 048: the size token_parts() gives is
    the size of the oracle's elements - for tokens made to order here."""
    import random
    rng = random.Random(1)
    for Cc in list(range(4, 300)):
        for Oo in (1, 5, 2047, 2048, 5000):
            lt, n64, mid, fin_len, fin = T.token_parts(0, Cc, Oo)
            assert 64 * n64 + 60 * mid + fin_len == Cc and 4 <= fin_len <= 64
            assert fin == (2 if fin_len <= 11 and Oo < 2048 else 3)
            assert mid == 0 or 5 <= fin_len <= 7
    for L in list(range(1, 1100)) + [65535, 65536]:
        data = rng.randbytes(L)
        comp = O.compress(data)
        if L >= 17 and T.tokens(comp) != [(L, 0, 0)]:
            continue
        assert T.encode(data, [(L, 0, 0)]) == comp, L


@pytest.fixture(scope="module")
def span(tmp_path_factory):
    so = tmp_path_factory.mktemp("span_shapes") / "span_wave_host.so"
    subprocess.check_call(
        ["g++", "-O2", "-shared", "-fPIC", "-std=c++17",
         "-I", str(ROOT / "rust-snappy_amd" / "csrc"),
         str(ROOT / "tests" / "span_wave_host.cpp"), "-o", str(so)])
    L = C.CDLL(str(so))
    L.span_wave_compress.restype = C.c_uint32
    L.span_wave_compress.argtypes = [C.c_char_p, C.c_uint32, C.c_char_p,
                                     C.c_uint32, C.POINTER(C.c_uint64)]

    def run(data):
        cap = len(data) + len(data) // 6 + 64
        out = C.create_string_buffer(cap)
        st = (C.c_uint64 * 16)()
        r = L.span_wave_compress(bytes(data), len(data), out, cap, st)
        assert r < 0x80000000, hex(r)
        return out.raw[:r]
    return run


def test_window_walk_gives_the_oracle_stream_on_every_single_block(S, span):
    """span_walk / span_par_walk of snapmi_span.hpp and the emit functions of
    snapmi_tiny.hpp on the host, over every one-block input of the set (not
    thinned: the emulator takes them all in a few seconds)."""
    singles = S.single_blocks()
    assert len(singles) == len(S.grid) + len(S.dense) + len(S.exceptions)
    for c in singles:
        assert span(c.data) == c.comp, c.name
