"""The chains of tests/indexed_store.py through the model alone: after every
step every stream is the oracle's stream of its data with the oracle's index,
whatever sequence of writes and appends made it - and the scenarios contain
what they are for, so that a later edit cannot hollow them out quietly."""
import pytest

import appendindex_ref as A
import blockindex_ref as B
import indexbuild_ref as I
import indexed_store as S
import rangeindex_ref as R
import writeindex_ref as W

BLOCK = S.BLOCK
OK = S.OK


@pytest.fixture(scope="module")
def played():
    return {"plain": S.play(S.SCENARIO), "fail": S.play(S.SCENARIO_FAIL),
            "long": S.play(S.SCENARIO_LONG)}


@pytest.mark.parametrize("name", ["plain", "fail", "long"])
def test_every_step_is_the_oracles_stream_and_index(played, name):
    mutating = 0
    for k, p in enumerate(played[name]):
        data, streams, entries = p.after
        for s in range(p.n):
            want = S.oracle(data[s])
            assert streams[s] == want[0], (name, k, p.kind, s)
            assert entries[s] == want[1], (name, k, p.kind, s)
        if p.kind in ("write", "append"):
            mutating += 1
            assert p.before != p.after, (name, k)
        if p.kind == "rebuild":
            assert p.status == [I.BUILT] * p.n, (name, k)
            assert p.first == S.firsts(entries), (name, k)
            assert p.flat == [e for idx in entries for e in idx], (name, k)
        if p.kind == "read":
            assert p.decoded == data
            for (s, off, n), (got, err) in zip(p.step["ranges"], p.ranges):
                assert err == OK and got == data[s][off:off + n], (name, k, s)
    assert 9 <= mutating <= 14 or name == "long"


def test_the_long_scenario_has_more_blocks_than_a_segment(played):
    """Every write and append of SCENARIO_LONG compresses more blocks than one
    token-path launch of the "lanes_segmented" configuration takes, and
    decodes a tail or an edge block beside them."""
    kinds = [p.kind for p in played["long"]]
    assert kinds == ["compress", "append", "write", "append", "rebuild",
                     "read"]
    for p in played["long"]:
        if p.kind in ("write", "append"):
            assert p.counters[0] > S.SEGMENT and p.counters[1] > 0
            assert p.counters[2:] == (p.n, 0)


@pytest.mark.parametrize("name", ["plain", "fail"])
def test_sizes_stay_small(played, name):
    """Ten streams of the initial lengths the issue names, none past 400 000
    bytes, no step over more than 40 blocks."""
    run = played[name]
    assert run[0].kind == "compress" and run[1].kind == "append"
    assert [len(d) for d in run[0].after[0]] == [
        0, 1, 127, 16383, 65535, 65536, 65537, 131072, 200000, 150000]
    d = run[0].after[0]
    assert d[5] == bytes(65536) and d[9] == bytes(150000)
    assert len(set(d[6])) == 256 and d[8] == A.text(200000, 8000)
    for k, p in enumerate(run):
        assert max(len(x) for x in p.after[0]) <= S.MAX_LEN, (name, k)
        if p.kind == "write":
            assert 0 < p.counters[0] <= S.MAX_STEP_BLOCKS, (name, k)
        if p.kind == "append":
            assert 0 < p.counters[0] <= S.MAX_STEP_BLOCKS, (name, k)
        if p.kind == "read":
            assert R.pieces([r[1] for r in p.step["ranges"]],
                            [r[2] for r in p.step["ranges"]]) <= 150


def test_the_plain_scenario_names_every_stream_in_every_step(played):
    """test_chain_enqueue_only hands each call's outputs to the next one
    verbatim: every write and every append names every stream, all succeed,
    and the first step behind the compress is an append, so that no stream is
    empty when the first write comes."""
    for k, p in enumerate(played["plain"]):
        if p.kind == "write":
            assert {w[0] for w in p.step["writes"] if w[2]} == set(
                range(S.N)), k
            assert p.counters[2:] == (S.N, 0), k
        if p.kind == "append":
            assert all(len(b) for b in p.step["appends"]), k
            assert p.step["old_lens"] == [len(d) for d in p.before[0]], k
            assert p.counters[2:] == (S.N, 0), k
        if p.kind in ("write", "append"):
            assert all(r[0] is not None and r[2] == OK for r in p.res), k


def coverage(run):
    """What the steps of a played scenario contain: a set of names."""
    seen = set()
    made_by_append, rewritten = set(), set()   # (stream, block)
    wrote = appended = False
    for p in run:
        data = p.before[0]
        if p.kind == "append":
            for s, add in enumerate(p.step["appends"]):
                if not add or p.res[s][0] is None:
                    continue
                appended = True
                old, new = len(data[s]), len(data[s]) + len(add)
                if old == 0:
                    seen.add("append onto the empty stream")
                if old % BLOCK and new % BLOCK == 0:
                    seen.add("append fills the tail exactly")
                if old % BLOCK == 0:
                    seen.add("append onto a block-aligned stream")
                    assert A.counters([old], [add], [p.res[s]])[1] == 0
                if old < 128 <= new < 16384:
                    seen.add("header 1 -> 2 bytes")
                    assert (p.before[2][s][0], p.res[s][1][0]) == (1, 2)
                if 128 <= old < 16384 <= new:
                    seen.add("header 2 -> 3 bytes")
                    assert (p.before[2][s][0], p.res[s][1][0]) == (2, 3)
                if old % BLOCK and (s, old // BLOCK) in rewritten:
                    seen.add("append behind a tail a write rewrote")
                made_by_append.update(
                    (s, k) for k in range(-(-old // BLOCK), -(-new // BLOCK)))
        if p.kind == "write":
            for s in range(S.N):
                mine = [(o, b) for t, o, b in p.step["writes"] if t == s and b]
                if not mine or p.res[s][0] is None:
                    continue
                wrote = True
                dlen = len(data[s])
                t = W.touched([(s, o, len(b)) for o, b in mine])
                for o, b in mine:
                    cnt, k0 = R.blocks(o, len(b))
                    covered = [k for k in range(k0, k0 + cnt)
                               if not R.edge(o, len(b), k)]
                    if covered and cnt == len(covered) + 2:
                        seen.add("whole blocks, both neighbours cut")
                    if len(b) == 16 and cnt == 2:
                        seen.add("16 bytes across a block boundary")
                    if cnt == 1 and k0 == dlen // BLOCK and dlen % BLOCK \
                            and o + len(b) < dlen:
                        seen.add("inside a short last block")
                old_e, new_e = p.before[2][s], p.res[s][1]
                for _, k, _, _ in t:
                    size = new_e[k + 1] - new_e[k]
                    was = old_e[k + 1] - old_e[k]
                    if size > 65536 and was < 4096:
                        seen.add("a block grows above 65 536")
                    if size < 4096 and was > 65536:
                        seen.add("a block shrinks below 4 096")
                    if (s, k) in made_by_append:
                        seen.add("write into a block an append made")
                    rewritten.add((s, k))
        if p.kind == "rebuild" and wrote and appended:
            seen.add("rebuild behind a write and an append")
    return seen


WANTED = {"append onto the empty stream", "append fills the tail exactly",
          "append onto a block-aligned stream", "header 1 -> 2 bytes",
          "header 2 -> 3 bytes", "whole blocks, both neighbours cut",
          "16 bytes across a block boundary", "inside a short last block",
          "a block grows above 65 536", "a block shrinks below 4 096",
          "write into a block an append made",
          "append behind a tail a write rewrote",
          "rebuild behind a write and an append"}


@pytest.mark.parametrize("name", ["plain", "fail"])
def test_the_scenario_contains_what_it_is_for(played, name):
    assert coverage(played[name]) == WANTED


def test_the_failures_and_the_successes_behind_them(played):
    """SCENARIO_FAIL is SCENARIO with a write and the append behind it put in
    the middle: three streams fail with exactly the tuples of
    include/snapmi.h, the other streams those calls name succeed, and the
    next steps append to and write into the same three streams."""
    plain, fail = played["plain"], played["fail"]
    at = [k for k, p in enumerate(fail) if p.step.get("fails")]
    assert len(at) == 2 and at[1] == at[0] + 1
    assert len(fail) == len(plain) + 2
    assert len(fail) // 3 <= at[0] <= 2 * len(fail) // 3  # in the middle
    rest = [p for p in fail if not p.step.get("fails")]
    assert [p.step for p in rest[:at[0]]] == [p.step for p in
                                              plain[:at[0]]]
    assert [p.kind for p in rest] == [p.kind for p in plain]
    w, a = fail[at[0]], fail[at[1]]
    assert (w.kind, a.kind) == ("write", "append")
    data, _, entries = w.before
    # the write: a cap one below the need, and a write behind the end
    s = S.FAIL_WRITE_SHORT_CAP
    need = w.caps[s] + 1
    assert w.res[s] == (None, None, (W.BUFFER_TOO_SMALL, need - 1, need, 0))
    s = S.FAIL_WRITE_BEHIND_END
    (off, b), = [(o, b) for t, o, b in w.step["writes"] if t == s]
    assert off < len(data[s]) < off + len(b)
    assert w.res[s] == (None, None,
                        (W.E_ARGUMENT, off, len(b), len(data[s])))
    named = {t for t, _, b in w.step["writes"] if b}
    ok = named - {S.FAIL_WRITE_SHORT_CAP, S.FAIL_WRITE_BEHIND_END}
    assert len(ok) >= 2 and all(w.res[t][0] is not None for t in ok)
    assert 0 < len(named) < S.N  # and streams nobody names
    assert w.counters[2:] == (len(ok), 2)
    # the append: the host's old_len of one stream is off by one
    s = S.FAIL_APPEND_OLD_LEN
    dlen = len(a.before[0][s])
    assert a.step["old_lens"][s] == dlen + 1 and a.step["appends"][s]
    cnt = B.entries(dlen + 1 + len(a.step["appends"][s]))
    assert a.res[s] == (None, [0] * cnt, (A.E_ARGUMENT, s, dlen, dlen + 1))
    named = {t for t, b in enumerate(a.step["appends"]) if b}
    assert len(named) >= 3 and all(a.res[t][0] is not None
                                   for t in named - {s})
    assert a.counters[2:] == (len(named) - 1, 1)
    # the three kept their bytes and entries ...
    three = (S.FAIL_WRITE_SHORT_CAP, S.FAIL_WRITE_BEHIND_END,
             S.FAIL_APPEND_OLD_LEN)
    for t in three:
        assert a.after[1][t] == w.before[1][t]
        assert a.after[2][t] == w.before[2][t]
    # ... and the very next steps append to them and write into them
    nxt = fail[at[1] + 1:at[1] + 3]
    assert sorted(p.kind for p in nxt) == ["append", "write"]
    for p in nxt:
        for t in three:
            assert p.res[t][0] is not None and p.res[t][2] == OK, (p.kind, t)
            assert p.after[1][t] != p.before[1][t]
