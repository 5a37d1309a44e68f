"""tests/decoder_shapes.py held to what it promises, without a GPU: every
stream decodes to the output its builder wrote down - by the oracle, by both
lane-level models and by the host build of lane_decode
(tests/element_host.cpp) - and the third-generation model met, in the family
named for it, every event of the fixed list below.  The list is written out
here and not derived from the set: an event the builders stop reaching fails
this file.  Prints the event table (pytest -s)."""
import struct
import subprocess
import zlib
from collections import Counter

import pytest

import decoder_shapes as D
import error_variants as V
import model_decoder as M2
import model_decoder3 as M3
import oracle_lib as O
from conftest import ROOT

PAIRS = {(o, n) for o in range(1, 65) for n in range(1, 65)}
OVERLAPPING = {(o, n) for o, n in PAIRS if o < n}
APART = PAIRS - OVERLAPPING

# event of tests/model_decoder3.py -> the family that must reach it
REQUIRED = [
    ("cap64", "cuts"), ("starts_64", "cuts"), ("wmax_cut", "cuts"),
    ("w_is_wmax", "cuts"), ("last_is_lit60", "cuts"),
    ("start_at_31", "cuts"), ("start_at_32", "cuts"), ("start_at_63", "cuts"),
    ("start_at_64", "cuts"), ("start_at_255", "cuts"),
    ("crosses_window_end", "cuts"), ("crosses_sub_window", "cuts"),
    ("crosses_group", "cuts"), ("copy_crosses_sub_window", "cuts"),
    ("copy_crosses_group", "cuts"),
    ("longlit_form1", "cuts"), ("longlit_form2", "cuts"),
    ("longlit_form3", "cuts"), ("longlit_form4", "cuts"),
    ("longlit_mid_window", "cuts"), ("longlit_at_255", "cuts"),
    ("trips_1", "overlap"), ("trips_2", "overlap"), ("trips_3", "overlap"),
    ("trips_4", "overlap"),
    ("cap64", "foreign_whole"), ("cap64_copy4_whole", "foreign_whole"),
    ("copy4_whole", "foreign_whole"), ("off_gt_64k_whole", "foreign_whole"),
    ("far_multi_piece", "foreign_whole"),
    ("win_not_whole", "behind_long_literal"),
    ("far_own_lane_not_whole", "behind_long_literal"),
    ("far_multi_piece", "behind_long_literal"),
    ("late_not_ring", "behind_long_literal"),
    ("late_flush_partial", "behind_long_literal"),
    ("late_src_near_end", "behind_long_literal"),
    ("src_straddles_safe_lo", "ring"), ("ring_read_into_mirror", "ring"),
    ("mirror_lo", "ring"), ("mirror_hi", "ring"),
    ("window_at_tail", "handover"), ("handover_at_tail", "handover"),
]
REQUIRED += [(("wrap_bytewise", c), "ring") for c in (0, 16, 32, 48)]
# ... with 1, 8 and 15 bytes of the piece in front of the ring's end (16
# bytes in front of it is a piece that fits: no bytewise store)
REQUIRED += [(("wrap_front", c, k), "ring")
             for c in (0, 16, 32, 48) for k in (1, 8, 15)]
REQUIRED += [(("ring_read_tail", k), "ring") for k in range(1, 16)]
REQUIRED += [((what, k), "ring") for what in ("q_at_safe_lo", "qe_at_safe_lo")
             for k in (-1, 0, 1)]
REQUIRED += [(("win_r0", r), "ring") for r in range(16)]
REQUIRED += [(("win_end_gap", g), "ring") for g in (-1, 0, 1)]


@pytest.fixture(scope="module")
def the_set():
    return D.the_set()


def family_events(cases):
    total = Counter()
    for c in cases:
        total.update(D.model3(c).events)
    return total


def test_no_stream_was_dropped(the_set):
    """the_set() keeps a stream only when the model saw what its family is
    named for: every stream the builders make must pass that."""
    fam, short = D.build_set()
    for name, cases in fam.items():
        assert [c.name for c in the_set[name]] == [c.name for c in cases]
    assert len(the_set["overlap_short"]) == len(short)
    assert len(the_set["beyond"]) >= 4 * 5
    size = sum(len(c.comp) for cases in the_set.values() for c in cases)
    print("streams", sum(len(v) for v in the_set.values()), "compressed",
          size)
    # (every later suite run decodes the set on several routes: it is to
    # stay in the low hundreds of KiB)
    assert size < 440 << 10


def test_oracle_gives_the_builders_output(the_set):
    for c in D.valid_cases():
        assert O.decompress(c.comp) == c.out, c.name
    for c in the_set["beyond"]:
        with pytest.raises(O.SnapError):
            O.decompress(c.comp)
    kinds = Counter()
    for c in the_set["beyond"]:
        try:
            O.decompress(c.comp)
        except O.SnapError as e:
            kinds[e.name] += 1
            if "offset-0" in c.name:
                assert e.name == "Offset" and e.a == 0, c.name
            if "offset-dstp+1" in c.name:
                assert e.name == "Offset" and e.a == e.b + 1, c.name
            if "literal-long" in c.name:
                assert e.name == "Literal" and e.a == e.b + 1, c.name
    assert kinds["Offset"] >= 10 and kinds["Literal"] >= 5, kinds


def test_the_builders_window_rule_is_the_models(the_set):
    """The builders place elements by following the window rule themselves
    (Builder._place); the model's trace must show the same windows, up to the
    one that hands over to the tail."""
    checked = 0
    for cases in D.window_families().values():
        for c in cases:
            got = [s for s, _, _, _ in D.model3(c).trace]
            assert got == c.win_starts[:len(got)], c.name
            assert got, c.name
            checked += len(got)
    assert checked > 5000


def check_model(M, tail, c, res):
    if res[0] == "ok":
        assert res[1] == c.out, c.name
        return
    _, s, d, prefix = res
    hdr = M.read_varint(c.comp)[1]
    assert len(c.comp) - hdr - s < tail, (c.name, s)
    assert prefix == c.out[:d], (c.name, s, d)


def test_third_generation_model_gives_the_builders_output(the_set):
    for c in D.valid_cases():
        D.model3(c)
        check_model(M3, M3.TAIL, c, c.result3)
    for name, cases in D.window_families().items():
        for c in cases:            # ... and the window loop did the work
            if c.name.startswith("handover2"):
                continue
            assert c.stats3.windows > 0, c.name


def test_second_generation_model_gives_the_builders_output(the_set):
    total = Counter()
    late = set()
    for c in D.valid_cases():
        st = M2.Stats()
        res = M2.decode(c.comp, st)
        # (the second generation has no tail: it leaves a valid stream only
        # when that is shorter than its first loads)
        check_model(M2, 8, c, res)
        if c in the_set["handover"]:
            total.update(st.events)
        if c in the_set["overlap"]:
            late |= st.late_overlap
    assert total["window_at_tail"] and total["handover_at_tail"], total
    assert late >= OVERLAPPING


def test_required_events(the_set):
    events = {name: family_events(cases)
              for name, cases in D.window_families().items()}
    missing = [(ev, fam) for ev, fam in REQUIRED if not events[fam][ev]]
    print()
    print("%-28s %-20s %s" % ("event", "family", "times"))
    for ev, fam in REQUIRED:
        print("%-28s %-20s %d" % (ev if isinstance(ev, str) else
                                  "%s %s" % (ev[0], list(ev[1:])), fam,
                                  events[fam][ev]))
    assert not missing, missing
    assert events["foreign_whole"]["copy4_whole"] > 0
    assert events["foreign_whole"]["off_gt_64k_whole"] > 0


def test_overlap_pairs(the_set):
    """Both late loops of the third generation moved all 2016 overlapping
    pairs; the pairs with offset >= length were late elements and own-lane
    elements; every pair came as copy-2 and copy-4, and as copy-1 where the
    format has one."""
    lo, la, own, general, ring_loop = set(), set(), set(), set(), set()
    kinds = set()
    for c in the_set["overlap"]:
        st = D.model3(c)
        lo |= st.late_overlap
        la |= st.late_apart
        own |= st.own_lane
        general |= st.late_general
        ring_loop |= st.late_ring_loop
        if c.name.startswith("overlap-"):
            kinds |= c.pairs
    print("overlapping pairs moved late: %d of %d; by the first late loop %d, "
          "by the second %d; offset >= length: late %d, own lane %d of %d"
          % (len(lo & OVERLAPPING), len(OVERLAPPING),
             len(ring_loop & OVERLAPPING), len(general & OVERLAPPING),
             len(la & APART), len(own & APART), len(APART)))
    assert len(OVERLAPPING) == 2016
    assert lo >= OVERLAPPING
    assert ring_loop >= OVERLAPPING      # each loop by itself, not the union
    assert general >= OVERLAPPING
    assert la >= APART and own >= APART
    want = {(o, n, k) for o, n in PAIRS for k in D.kinds_of(o, n)}
    assert kinds >= want
    # the short copies: every pair in the staged lane loop's class or in the
    # wavefront decoder's short class - every offset and every length in
    # both - and the short lengths in k_decompress_small's
    per_class = {"lds": set(), "short_wide": set(), "small": set()}
    for c in the_set["overlap_short"]:
        cls = c.name.split("-")[0]
        assert V.in_class(cls, c.comp), c.name
        per_class[cls] |= c.pairs
    assert per_class["lds"] | per_class["short_wide"] >= want
    for cls in ("lds", "short_wide"):
        assert {o for o, _, _ in per_class[cls]} == set(range(1, 65)), cls
        assert {n for _, n, _ in per_class[cls]} == set(range(1, 65)), cls
        assert {k for _, _, k in per_class[cls]} == {1, 2, 4}, cls
    assert per_class["small"] >= {p for p in want if p[1] <= 10}


# ---- the host build of lane_decode -----------------------------------------
def host_answers(tmp, cases):
    exe = tmp / "element_host"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror",
                           str(ROOT / "tests" / "element_host.cpp"),
                           "-o", str(exe)])
    path = tmp / "cases.bin"
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(cases)))
        for c in cases:
            f.write(struct.pack("<QI", O.decompress_len(c.comp),
                                len(c.comp)) + c.comp)
    out = subprocess.run([str(exe), str(path)], capture_output=True,
                         text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stdout.splitlines()
    assert len(lines) == 3 * len(cases)
    return lines[::3]


def test_lane_decode_on_the_host(the_set, tmp_path):
    cases = D.valid_cases() + the_set["beyond"]
    errors = 0
    for c, line in zip(cases, host_answers(tmp_path, cases)):
        if c.out is not None:
            want = "0 0 0 0 %d %d" % (len(c.out), zlib.crc32(c.out))
        else:
            with pytest.raises(O.SnapError) as e:
                O.decompress(c.comp)
            e = e.value
            want = "%d %d %d %d 0 %d" % (e.kind, e.a, e.b, e.c,
                                         zlib.crc32(b""))
            errors += 1
        assert line == "flat " + want, c.name
    assert errors == len(the_set["beyond"])
