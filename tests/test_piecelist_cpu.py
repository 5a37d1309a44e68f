"""The piece-descriptor slab on the CPU: csrc/snapmi_piecelist.hpp, compiled
into a stand-alone program (tests/piecelist_host.cpp) - the one description
the long-stream plan, indexed decode and range reads size and address their
descriptor lists with.  For every slot count: the seven arrays are disjoint,
the 8-byte arrays are 8-byte aligned over a 256-byte aligned base, the last
byte lies inside the reported total, and plan_streams (snapmi_streamplan.hpp)
reports the same offsets for a plan of that many pieces.

No plan has ONE piece (a stream gets bound / 64 KiB + 2 of them), so the last
property is checked for every count but 1, and for 2 in its place."""
import subprocess

import pytest

from conftest import ROOT

COUNTS = [0, 1, 3, 64, 4097]
NONE = (1 << 64) - 1
# bytes of a slot of each array: c_in, c_inlen, c_out, c_cap, c_outlen (8),
# c_err (snapmi_error, 32), c_mode (1)
WIDTH = [8, 8, 8, 8, 8, 32, 1]


def build(tmp_path_factory, name, extra):
    exe = tmp_path_factory.mktemp(name) / "piecelist_host"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror",
                           *extra,
                           str(ROOT / "tests" / "piecelist_host.cpp"),
                           "-o", str(exe)])
    return exe


def run(exe, counts):
    out = subprocess.run([str(exe)], input="".join(f"{p}\n" for p in counts),
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    rows = [[int(t) for t in ln.split()] for ln in out.stdout.splitlines()]
    assert len(rows) == len(counts)
    return rows


@pytest.fixture(scope="module")
def rows(tmp_path_factory):
    exe = build(tmp_path_factory, "piecelist", [])
    counts = COUNTS + [2]
    return dict(zip(counts, run(exe, counts)))


def split(row):
    assert len(row) == 1 + 8 + 7 + 1 + 8
    return row[0], row[1:8], row[8], row[9:16], row[16], row[17:24], row[24]


def test_slot_bytes(rows):
    for p, row in rows.items():
        assert split(row)[0] == sum(WIDTH) == 8 * 5 + 32 + 1


@pytest.mark.parametrize("p", COUNTS)
def test_arrays_disjoint_aligned_inside(rows, p):
    _, offs, total, ptrs, base_mod, _, _ = split(rows[p])
    assert base_mod == 0
    assert ptrs == offs            # piece_list() follows piece_offsets()
    spans = [(o, o + w * p) for o, w in zip(offs, WIDTH)]
    for i, (lo, hi) in enumerate(spans):
        assert hi <= total, (p, i)
        for lo2, hi2 in spans[i + 1:]:
            assert hi <= lo2 or hi2 <= lo, (p, i)
    for o, w in zip(offs, WIDTH):
        if w >= 8:
            assert o % 8 == 0, (p, o)
    # the last byte of the slab: the last mode
    assert max(hi for _, hi in spans) == sum(WIDTH) * p <= total


@pytest.mark.parametrize("p", [0, 2, 3, 64, 4097])
def test_plan_streams_reports_the_same_offsets(rows, p):
    _, offs, total, _, _, plan, d_bytes = split(rows[p])
    assert plan == offs
    assert d_bytes == total


def test_no_plan_has_one_piece(rows):
    _, _, _, _, _, plan, d_bytes = split(rows[1])
    assert plan == [NONE] * 7 and d_bytes == NONE


def test_under_the_sanitizers(tmp_path_factory, rows):
    """The same program with -fsanitize=address,undefined: it writes the first
    and the last slot of every array of a slab of exactly `total` bytes."""
    exe = build(tmp_path_factory, "piecelist_san",
                ["-g", "-fsanitize=address,undefined",
                 "-fno-sanitize-recover=all"])
    counts = COUNTS + [2]
    assert dict(zip(counts, run(exe, counts))) == rows
