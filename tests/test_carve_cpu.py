"""The frame layer's carved scratch buffers on the CPU: csrc/snapmi_carve.hpp
and the layout functions of csrc/snapmi_frame.hpp, compiled into a stand-alone
program (tests/carve_host.cpp).  Each buffer (fb_streams, fb_chunks, fr_desc,
fr_crc) has one layout function that the host runs twice - without a base for
the size, then on the buffer - so this checks what no compiler does: that
every array, with the count the KERNELS index (written out here, not taken
from the layouts), lies inside the measured size and apart from every other,
and that the measured size is no more than the formula the layouts replaced."""
import itertools
import subprocess

import pytest

from conftest import ROOT

ERR = 32           # sizeof(snapmi_error)
CANDS = 32         # kFwCands: candidates kept per segment of the parallel walk

NS = [1, 2, 64, 1000]
NSEGS = [0, 1, 5]


def shapes():
    out = []
    for n in NS:
        for total in (0, 1, n, 3 * n + 1):
            for seg in (0, 1, total):
                for nseg in NSEGS:
                    if (n, total, seg, nseg) not in out:
                        out.append((n, total, seg, nseg))
    return out


@pytest.fixture(scope="module")
def answer(tmp_path_factory):
    exe = tmp_path_factory.mktemp("carve") / "carve_host"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror",
                           "-I", str(ROOT / "include"),
                           str(ROOT / "tests" / "carve_host.cpp"),
                           "-o", str(exe)])
    S = shapes()
    out = subprocess.run([str(exe)],
                         input="".join("%d %d %d %d\n" % s for s in S),
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.splitlines()
    sizes = [int(t) for t in lines[0].split()]
    mixed = [[int(t) for t in ln.split()] for ln in lines[1:21]]
    end = lines[21].split()
    assert end[0] == "end"
    layouts = {}
    rest = lines[22:]
    assert len(rest) == 6 * len(S)
    for k, s in enumerate(S):
        for ln in rest[6 * k:6 * k + 6]:
            t = ln.split()
            arrays = [(t[i], int(t[i + 1]), int(t[i + 2]))
                      for i in range(4, len(t), 3)]
            layouts[(t[0],) + s] = (int(t[1]), int(t[2]), int(t[3]), arrays)
    return {"frame_chunk": sizes[0], "error": sizes[1], "mixed": mixed,
            "end": (int(end[1]), int(end[2])), "layouts": layouts}


# ------------------------------------------------------------ the Carver alone
def test_measuring_and_placing_end_together(answer):
    measured, placed = answer["end"]
    assert measured == placed > 0
    assert [(r[0], r[1]) for r in answer["mixed"]] == [
        (e, c) for c in (0, 1, 3, 17) for e in (1, 4, 8, 24, 32)]


def test_every_address_is_16_aligned(answer):
    for elem, count, before, after, off, mod in answer["mixed"]:
        assert mod == 0 and off % 16 == 0, (elem, count)
        assert off == before, (elem, count)   # bytes() ends on a boundary


def test_no_elements_no_bytes(answer):
    for elem, count, before, after, off, mod in answer["mixed"]:
        if count == 0:
            assert after == before, elem
        else:
            assert after == (off + elem * count + 15) // 16 * 16, (elem, count)


# ----------------------------------------------------------------- the layouts
def want_arrays(tag, n, total, seg, nseg, frame_chunk):
    """(name, element bytes, elements the kernels index) in the layout's
    order."""
    if tag == "streams":
        return [("counts", 8, n), ("first", 8, n + 1), ("serr", ERR, n),
                ("sidx", 4, n), ("first_bad", 4, n)]
    if tag == "lone":   # the batch of one, the scalars' places, the walk
        return [("counts", 8, 1), ("first", 8, 2), ("serr", ERR, 1),
                ("sidx", 4, 1), ("first_bad", 4, 1),
                ("in_ptrs", 8, 1), ("in_lens", 8, 1), ("out_ptrs", 8, 1),
                ("out_caps", 8, 1), ("meta", 4, 4),
                ("fw_cand", 8, nseg * CANDS * 3), ("fw_entry", 8, nseg + 1),
                ("fw_ncand", 4, nseg), ("fw_base", 4, nseg + 1)]
    if tag == "chunks":
        return [("chunks", frame_chunk, total), ("c_stream", 4, total),
                ("dlens", 8, total), ("offs", 8, total + 1),
                ("cerrs", ERR, total), ("derrs", ERR, total),
                ("c_in", 8, total), ("c_in_len", 8, total),
                ("c_out", 8, total), ("c_caps", 8, total),
                ("c_out_lens", 8, total), ("modes", 1, total),
                ("crcs", 4, total)]
    if tag in ("desc0", "desc1"):
        one = 1 if tag == "desc1" else 0
        return [("lone_in", 8, one), ("lone_len", 8, one),
                ("lone_out", 8, one),
                ("counts", 8, n), ("first", 8, n + 1), ("refused", 1, n),
                ("sbase", 8, n), ("c_in", 8, total), ("c_len", 8, total),
                ("c_stream", 4, total), ("carry", 8, 1),
                ("slot_ptrs", 8, seg), ("clens", 8, seg), ("crcs", 4, seg),
                ("sizes", 8, seg), ("offs", 8, seg + 1)]
    assert tag == "crc"
    return [("seg_first", 8, n + 1), ("acc", 4, n)]


def parent_formula(tag, n, total, seg, nseg, frame_chunk):
    """What the host code reserved for the buffer before the layouts."""
    if tag == "streams":
        return n * (8 + 8 + ERR + 4 + 4) + 8 + 16 * 8
    if tag == "lone":
        front = 4 * 8 + 16 + 16 * 16 + (nseg + 2) * (CANDS * 24 + 4 + 8 + 4)
        return 1 * (8 + 8 + ERR + 4 + 4) + 8 + 16 * 8 + front
    if tag == "chunks":
        return total * (frame_chunk + 4 + 8 + 8 + 2 * ERR + 8 + 8 + 8 + 8 + 8
                        + 1 + 4) + 8 + 16 * 16
    if tag in ("desc0", "desc1"):
        return (n * (8 + 8 + 1 + 8) + 8 + 3 * 8 + total * (8 + 8 + 4)
                + seg * (8 + 8 + 4 + 8 + 8) + 8 + 8 + 16 * 16)
    assert tag == "crc"
    return (n + 1) * 8 + n * 4 + 16


TAGS = ["streams", "lone", "chunks", "desc0", "desc1", "crc"]


def test_sizes_the_test_assumes(answer):
    assert answer["error"] == ERR
    assert answer["frame_chunk"] % 8 == 0 and answer["frame_chunk"] >= 24


@pytest.mark.parametrize("tag", TAGS)
def test_arrays_disjoint_and_inside(answer, tag):
    for s in shapes():
        measured, placed, base_mod, arrays = answer["layouts"][(tag,) + s]
        assert measured == placed and base_mod == 0, (tag, s)
        want = want_arrays(tag, *s, answer["frame_chunk"])
        assert [(a[0], a[1]) for a in arrays] == [(w[0], w[1]) for w in want]
        spans = []
        for (name, elem, off), (_, _, count) in zip(arrays, want):
            assert off % 16 == 0, (tag, s, name)
            assert 0 <= off and off + elem * count <= measured, (tag, s, name)
            spans.append((off, off + elem * count, name))
        for (lo, hi, a), (lo2, hi2, b) in itertools.combinations(spans, 2):
            assert hi <= lo2 or hi2 <= lo or lo == hi or lo2 == hi2, (
                tag, s, a, b)


@pytest.mark.parametrize("tag", TAGS)
def test_no_more_than_the_formula_it_replaced(answer, tag):
    for s in shapes():
        measured = answer["layouts"][(tag,) + s][0]
        assert measured <= parent_formula(tag, *s, answer["frame_chunk"]), (
            tag, s, measured)
