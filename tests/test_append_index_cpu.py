"""The append rules on the CPU: bi_append_* of csrc/snapmi_blockindex.hpp,
compiled into a stand-alone program (tests/appendindex_host.cpp - the source
the kernels and the host entry point compile) plainly and under the
sanitizers, against tests/appendindex_ref.py; the splice identity - the old
full blocks' bytes in front of the oracle's bytes of the new blocks ARE the
oracle's stream of old data followed by appended data - that the call's
contract rests on; the export and the binding of the call."""
import random
import subprocess

import pytest

import appendindex_ref as A
import blockindex_ref as B
import oracle_lib as O
from conftest import ROOT

U64 = 1 << 64
NONE = U64 - 1
GRID = [(d, a) for d in A.OLD_LENS for a in A.APPENDS]


def build(tmp_path_factory, name, extra):
    exe = tmp_path_factory.mktemp(name) / "appendindex_host"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror",
                           *extra,
                           str(ROOT / "tests" / "appendindex_host.cpp"),
                           "-o", str(exe)])

    def run(lines):
        out = subprocess.run([str(exe)],
                             input="".join(s + "\n" for s in lines),
                             capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stderr
        rows = [[int(t) for t in ln.split()]
                for ln in out.stdout.splitlines()]
        assert len(rows) == len(lines)
        return rows
    return run


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def prog(request, tmp_path_factory):
    """The stand-alone program, and the same under
    -fsanitize=address,undefined: every test below runs through both."""
    extra = [] if request.param == "plain" else [
        "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    return build(tmp_path_factory, "appendindex_" + request.param, extra)


def pairs():
    rng = random.Random(1)
    extra = [(rng.randrange(1 << 20), rng.randrange(1 << 20))
             for _ in range(200)]
    return GRID + extra + [(2**32 - 1, 1), (2**32 - 1, 0), (0, 2**32),
                           (65536 * 7, 65536 * 3), (U64 - 2, 1)]


def test_layout_tail_and_new_blocks(prog):
    ps = pairs()
    rows = prog([f"L {d} {a}" for d, a in ps])
    probes, want = [], []
    for (d, a), row in zip(ps, rows):
        assert row == [A.entries(d, a), A.full(d), A.tail(d), A.fill(d, a),
                       A.blocks(d, a)], (d, a)
        nb = A.blocks(d, a)
        # the entries are the old full blocks, the new blocks and one
        if a:
            assert A.entries(d, a) == A.full(d) + nb + 1
        if nb > 100:
            continue
        # the new blocks tile the source; only the first may be the tail's
        pos = 0
        for j in range(nb):
            room, off, ln, in_len = A.block(d, a, j)
            assert off == pos and ln > 0 and in_len <= 65536
            assert room == (j == 0 and A.tail(d) != 0)
            assert in_len == ln + (A.tail(d) if room else 0)
            assert in_len == 65536 or j == nb - 1
            pos += ln
            probes.append(f"B {d} {a} {j}")
            want.append([int(room), off, ln, in_len])
        assert pos == a
    assert prog(probes) == want
    by = {p: (A.full(p[0]), A.tail(p[0]), A.fill(*p), A.blocks(*p))
          for p in GRID}
    assert by[(0, 1)] == (0, 0, 0, 1)
    assert by[(65535, 1)] == (0, 65535, 1, 1)
    assert by[(65535, 2)] == (0, 65535, 1, 2)
    assert by[(65536, 65537)] == (1, 0, 0, 2)
    assert by[(200000, 200000)] == (3, 3392, 62144, 4)
    assert by[(127, 0)] == (0, 127, 0, 0)
    assert A.block(65535, 2, 1) == (False, 1, 1, 1)


def test_host_checks_wrap_and_limit(prog):
    rng = random.Random(2)
    lists = [[], [(0, 0)], [(5, 0), (0, 7)], GRID[:20], GRID,
             [(U64 - 1, 1)], [(3, 4), (U64 - 5, 5)], [(1, U64 - 1)],
             [(U64 - 2, 1)], [(U64 - 65536, 65535)],
             [((1 << 31) * 65536, 0)], [(0, (1 << 30) * 65536)],
             [(65536 * ((1 << 31) - 2), 65536)]]
    for _ in range(50):
        lists.append([(rng.randrange(1 << 22), rng.choice([0, rng.randrange(
            1 << 22)])) for _ in range(rng.randrange(1, 9))])
    cases = [(ie, ls) for ls in lists for ie in (0, 77)]
    # exactly at the limit, and one below: n + index_entries + entries + blocks
    one = [(65536, 65536)]                      # 3 entries, 1 new block
    for ie in ((1 << 31) - 1 - 5, (1 << 31) - 1 - 4, (1 << 31) - 1 - 6,
               1 << 31, U64 - 1):
        cases.append((ie, one))
    rows = prog([f"C {ie} {len(ls)} " + " ".join(f"{d} {a}" for d, a in ls)
                 for ie, ls in cases])
    for (ie, ls), row in zip(cases, rows):
        assert row == list(A.check([d for d, _ in ls], [a for _, a in ls],
                                   ie)), (ie, ls)
    by = {(ie, tuple(ls)): A.check([d for d, _ in ls], [a for _, a in ls], ie)
          for ie, ls in cases}
    assert by[(0, ((U64 - 1, 1),))] == (A.WRAPS, 0, 0, 0)
    assert by[(0, ((3, 4), (U64 - 5, 5)))] == (A.WRAPS, 1, 0, 0)
    assert by[(0, ((U64 - 2, 1),))][0] == A.TOO_MANY   # (no wrap: too long)
    assert by[((1 << 31) - 1 - 5, tuple(one))] == (0, 0, 3, 1)
    assert by[((1 << 31) - 1 - 4, tuple(one))][0] == A.TOO_MANY
    assert by[(0, ((65536 * ((1 << 31) - 2), 65536),))][0] == A.TOO_MANY
    assert by[(77, tuple(GRID))][0] == 0


def test_index_rule_over_every_old_block(prog):
    lines, want = [], []
    for blocks in (1, 2, 4, 70):
        good = [3 + 100 * k for k in range(blocks + 1)]
        in_len = good[-1]
        cases = [(good, in_len), (good, in_len - 1), ([0] * (blocks + 1),
                                                      in_len)]
        for k in range(blocks):
            e = list(good)
            e[k + 1] = e[k]                      # an empty block
            cases.append((e, in_len))
        for e, ln in cases:
            lines.append(f"K {ln} {blocks} " + " ".join(map(str, e)))
            first = next((k for k in range(blocks)
                          if not (e[k] < e[k + 1] <= ln)), None)
            want.append([NONE if first is None else first])
    assert prog(lines) == want
    assert prog(["F 10 10", "F 9 10", "F 0 0", "F 11 10"]) == [[1], [0], [1],
                                                                [1]]


def test_splice_entries(prog):
    rng = random.Random(3)
    lines, want = [], []
    for _ in range(300):
        kf = rng.choice([0, 1, 2, 16, 300])
        nb = rng.choice([1, 2, 3, 40])
        hdr_old = rng.choice([1, 2, 3, 5])
        hdr_new = rng.choice([hdr_old, hdr_old + 1])
        e = [hdr_old]
        for _ in range(kf + 1):                  # (a tail behind the full ones)
            e.append(e[-1] + rng.randrange(1, 70000))
        nsize = [rng.randrange(1, 76490) for _ in range(nb)]
        lines.append(" ".join(map(str, ["X", hdr_old, hdr_new, kf, nb]
                                  + e[:kf + 1] + nsize)))
        ne = A.splice(e, kf, nsize, hdr_new)
        assert len(ne) == kf + nb + 1
        want.append(ne + ne)
    assert prog(lines) == want


@pytest.fixture(scope="module")
def case():
    return A.Case()


def test_splice_identity_against_the_oracle(case):
    """varint(new length), the old bytes [hdr, e[kf]) and the oracle's
    streams of the new blocks without their varints are the oracle's stream
    of old data followed by appended data, and the running sums are its index:
    what makes the call's yardstick exact."""
    checked = 0
    for a in A.APPENDS:
        extra = A.text(a, 777)
        appends = [extra] * case.n
        res, nf, new_index = A.expect(
            case.comps, case.flat, case.first, case.old_lens, appends,
            [1 << 40] * case.n, O.compress, A.decode_piece, A.header_error)
        assert nf == A.new_first(case.old_lens, [a] * case.n)
        for s, old in enumerate(case.inputs):
            out, ne, err = res[s]
            assert err == A.OK, (s, a, err)
            if a == 0:
                assert out is None and ne == case.index[s]
                continue
            assert out == O.compress(old + extra), (len(old), a)
            assert ne == B.expected_index(old + extra), (len(old), a)
            assert new_index[nf[s]:nf[s + 1]] == ne
            # ... spelled out: the three parts
            e, kf = case.index[s], A.full(len(old))
            new = (old + extra)[kf * 65536:]
            assert out == (B.varint(len(old) + a) + case.comps[s][e[0]:e[kf]]
                           + b"".join(B.block_streams(new)))
            checked += 1
    assert checked == len(A.OLD_LENS) * (len(A.APPENDS) - 1)


def test_model_precedence_of_failures(case):
    """The model's own order of the reasons: header, announced length, too
    big, index, piece, cap."""
    S = A.OLD_LENS.index(200000)

    def one(s, add, comps=None, flat=None, first=None, old_lens=None,
            cap=1 << 40):
        appends = [b""] * case.n
        appends[s] = add
        res, nf, ni = A.expect(
            comps or case.comps, flat or case.flat, first or case.first,
            old_lens or case.old_lens, appends, [cap] * case.n, O.compress,
            A.decode_piece, A.header_error)
        assert ni[nf[s]:nf[s + 1]] == res[s][1]
        return res[s]

    bad = list(case.comps)
    bad[S] = b"\xff" * 11 + bad[S][11:]
    lens = list(case.old_lens)
    lens[S] += 1
    # (a header that does not parse comes before the announced length)
    assert one(S, b"a", comps=bad, old_lens=lens)[2] == A.header_error(bad[S])
    assert one(S, b"a", old_lens=lens)[2] == (101, S, 200000, 200001)
    forged = list(case.comps)
    forged[S] = B.varint(2**32 - 1)
    lens[S] = 2**32 - 1
    out, ne, err = one(S, b"a", comps=forged, old_lens=lens)
    assert err == (A.TOO_BIG, 2**32, 2**32 - 1, 0) and ne == [0] * 65537
    idx = case.index[S]
    flat, first = case.with_index(S, idx[:2] + [idx[1]] + idx[3:])
    assert one(S, b"a", flat=flat, first=first)[2] == (101, S, 1, 0)
    flat, first = case.with_index(S, [idx[0] + 1] + idx[1:])
    assert one(S, b"a", flat=flat, first=first)[2] == (101, S, 0, 0)
    need = len(one(S, b"abc")[0])
    assert one(S, b"abc", cap=need)[2] == A.OK
    assert one(S, b"abc", cap=need - 1)[2] == (2, need - 1, need, 0)
    assert one(S, b"abc", cap=need - 1)[1] == [0] * len(idx)
    lens = [200000] * 6
    adds = [200000] * 6
    assert A.groups(lens, adds, 1 << 30) == [[0, 1, 2, 3, 4, 5]]
    assert A.groups(lens, adds, A.FLOOR) == [[s] for s in range(6)]
    assert A.groups([65536, 1, 0], [1, 0, 1], 2 * A.SLOT) == [[0, 2]]
    assert A.counters([65536, 1, 7], [b"a", b"", b"b"],
                      [(b"x",), (None,), (None,)]) == (2, 1, 1, 1)


def groups_row(lens, adds, scratch):
    """What the program's G command answers, from the model: A.groups names
    the streams of every group; a named stream with a tail has one room, and
    the rooms of a group count from 0."""
    gs = A.groups(lens, adds, scratch)
    row, rooms_of = [len(gs)], []
    t0 = b0 = 0
    top = [0, 0, 0]
    for g in gs:
        bg = sum(A.blocks(lens[s], adds[s]) for s in g)
        tails = [int(A.tail(lens[s]) != 0) for s in g]
        row += [t0, len(g), b0, bg, sum(tails)]
        top = [max(a, b) for a, b in zip(top, (len(g), bg, sum(tails)))]
        r = 0
        for tail in tails:
            rooms_of.append(r if tail else 2**32 - 1)
            r += tail
        t0 += len(g)
        b0 += bg
    return row + top + rooms_of


def test_groups_of_named_streams(prog):
    """bi_update_groups, as snapmi_append_indexed calls it, against A.groups:
    whole named streams until the scratch is full, a stream that needs more
    than the scratch alone in its group, the rooms numbered from 0 in every
    group."""
    six = ([200000] * 6, [200000] * 6)
    lone = ([1, 65536, 10, 5, 70000], [1, 0, 65536 * 5, 1, 1])
    cases = [(*six, A.FLOOR), (*six, 1 << 30),
             ([65536, 1, 0], [1, 0, 1], 2 * A.SLOT), (*lone, A.FLOOR),
             (*lone, 2 * A.FLOOR), ([7, 8], [0, 0], A.FLOOR)]
    rng = random.Random(22)
    for _ in range(300):
        n = rng.randrange(1, 9)
        lens = [rng.choice(A.OLD_LENS + [rng.randrange(1 << 18)])
                for _ in range(n)]
        adds = [rng.choice([0, 1, 65536, rng.randrange(1, 1 << 18)])
                for _ in range(n)]
        cases.append((lens, adds, rng.randrange(A.FLOOR, 8 * A.FLOOR + 1)))
    rows = prog([f"G {scratch} {len(lens)} " +
                 " ".join(f"{d} {a}" for d, a in zip(lens, adds))
                 for lens, adds, scratch in cases])
    for (lens, adds, scratch), row in zip(cases, rows):
        assert row == groups_row(lens, adds, scratch), (lens, adds, scratch)
    # 200 000 more bytes behind 200 000: the tail's room and four new blocks
    assert rows[0] == [6] + [v for t in range(6) for v in (t, 1, 4 * t, 4, 1)
                             ] + [1, 4, 1] + [0] * 6
    assert rows[1] == [1, 0, 6, 0, 24, 6, 6, 24, 6, 0, 1, 2, 3, 4, 5]
    assert rows[2] == [1, 0, 2, 0, 2, 0, 2, 2, 0, 2**32 - 1, 2**32 - 1]
    # six new blocks behind ten bytes: more than the scratch, a group of its
    # own between its neighbours, which share theirs when they fit
    assert A.groups(*lone, A.FLOOR) == [[0], [2], [3], [4]]
    assert A.groups(*lone, 2 * A.FLOOR) == [[0], [2], [3, 4]]
    assert rows[4] == [3, 0, 1, 0, 1, 1, 1, 1, 1, 6, 1, 2, 2, 7, 2, 2,
                       2, 6, 2, 0, 0, 0, 1]
    assert rows[5] == [0, 0, 0, 0]
    assert sum(len(A.groups(*c)) > 1 for c in cases[6:]) > 50
    assert sum(len(A.groups(*c)) == 1 for c in cases[6:]) > 50


def test_binding_exposes_the_call(built):
    from rust_snappy_amd import _lib, batch, raw
    L = _lib.load()
    P = _lib.load_product()
    names = {s[0] for s in _lib.SYMBOLS}
    assert "snapmi_append_indexed" in names
    assert hasattr(L, "snapmi_append_indexed")
    assert hasattr(P, "snapmi_append_indexed")
    header = (ROOT / "include" / "snapmi.h").read_text()
    assert "SNAPMI_API int snapmi_append_indexed(" in header
    for m in ("snapmi.map", "snapmi_test.map"):
        text = (ROOT / "rust-snappy_amd" / "csrc" / m).read_text()
        assert "snapmi_append_indexed;" in text
    assert callable(batch.append)
    assert callable(raw.append_indexed)
    # the entry count of the new index is the existing helper's, of the
    # summed lengths
    for d, a in GRID:
        assert raw.block_index_entries([d + a]) == A.entries(d, a)
