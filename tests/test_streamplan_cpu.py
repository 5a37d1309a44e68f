"""The long-stream decoder's plan (csrc/snapmi_streamplan.hpp), on the CPU:
segment size, scan groups, the pieces of a lone stream, the workgroups of
each launch and where every table and descriptor lies in the scratch, for a
lone stream (snapmi_decompress_stream) and for the long streams of a batch
(snapmi_decompress_batch); and the rule that sends a stream this way at all
(long_stream_rule), held against its restatement in long_streams.py.  The
GPU suite checks the bytes these launches produce; here the arithmetic that
routes, sizes and places them."""
import ctypes as C
import random
import subprocess
from pathlib import Path

import pytest

import long_streams as LS

ROOT = Path(__file__).resolve().parent.parent
KIB, MIB = 1 << 10, 1 << 20
DESC = 200       # a descriptor's bytes: sizeof(StreamArgs), see test_long_stream_rule
NTOT, NSLOT = 25, 13
PRE = ["scan", "super", "super3", "spread3", "spread2", "cuts", "pieces"]


@pytest.fixture(scope="module")
def P(tmp_path_factory):
    so = tmp_path_factory.mktemp("streamplan") / "streamplan_host.so"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-shared",
                           "-fPIC", str(ROOT / "tests" / "streamplan_host.cpp"),
                           "-o", str(so)])
    L = C.CDLL(str(so))
    u64, u32 = C.c_uint64, C.c_uint32
    L.t_seg_log2.restype = u32
    L.t_seg_log2.argtypes = [u32, u64]
    L.t_scan_segs.restype = u32
    L.t_scan_segs.argtypes = [u32, u64]
    L.t_lone_bound.restype = u64
    L.t_lone_bound.argtypes = [u64, u64]
    L.t_plan.restype = C.c_int
    L.t_plan.argtypes = [u32, C.POINTER(u64), C.POINTER(u64), C.c_int, u32,
                         u32, u64]
    L.t_long_stream_rule.restype = C.c_int
    L.t_long_stream_rule.argtypes = [u64, u64, u64]
    L.t_desc_size.restype = u64
    L.t_desc_size.argtypes = []
    return L


def constants(P):
    out = (C.c_uint64 * 8)()
    P.t_constants(out)
    names = ["seg", "entry", "seg_per_super", "cut_segs", "scan_segs",
             "scan_fill", "chunk", "pre"]
    return dict(zip(names, out))


def plan(P, lens, bounds, lone=False, seg_log2=0, scan_segs=0):
    """The plan as a dict (None when a stream is too long): totals, 'slots'
    (a dict per stream), 'pre' (a list per prefixed kernel)."""
    n = len(lens)
    a = (C.c_uint64 * n)(*lens)
    b = (C.c_uint64 * n)(*bounds)
    if not P.t_plan(n, a, b, int(lone), seg_log2, scan_segs, DESC):
        return None
    tot = (C.c_uint64 * NTOT)()
    P.t_totals(tot)
    names = (["seg_log2", "scan_segs"] + ["grid_" + k for k in PRE] +
             ["e_off", "e_bytes", "t_bytes", "pieces", "c_in", "c_inlen",
              "c_out", "c_cap", "c_outlen", "c_err", "c_mode", "d_bytes",
              "pre_off", "desc_bytes"])
    p = dict(zip(names, tot))
    sl = (C.c_uint64 * (NSLOT * n))()
    P.t_slots(sl)
    fields = ["nseg", "nsuper", "nsuper3", "kmax", "meta", "e1", "e2", "e3",
              "s1", "s2", "s3", "cuts", "entry"]
    p["slots"] = [dict(zip(fields, sl[j * NSLOT:(j + 1) * NSLOT]))
                  for j in range(n)]
    pr = (C.c_uint32 * (len(PRE) * (n + 1)))()
    P.t_pre(pr)
    p["pre"] = [list(pr[k * (n + 1):(k + 1) * (n + 1)])
                for k in range(len(PRE))]
    return p


def cdiv(a, b):
    return -(-a // b)


def want_geometry(in_len, bound, seg_log2):
    nseg = cdiv(in_len, 1 << seg_log2) + 1
    nsuper = cdiv(nseg, 64)
    nsuper3 = cdiv(nsuper, 64)
    return dict(nseg=nseg, nsuper=nsuper, nsuper3=nsuper3,
                kmax=bound // 65536 + 2)


def parent_bytes(geoms, lone):
    """t_bytes / d_bytes as the two callers computed them before the plan."""
    rows = sum(g["nseg"] + (g["nsuper"] + g["nsuper3"]) * 64 for g in geoms)
    blocks = sum(g["nseg"] + g["nsuper"] + g["nsuper3"] for g in geoms)
    if lone:
        (g,) = geoms
        t = 64 + rows * 8 * 16 + blocks * 16 + (g["kmax"] + 1) * 16
        d = (g["kmax"] + 1) * (40 + 32 + 1) + 64
    else:
        t = (64 + len(geoms) * 64 + rows * 8 * 16 + blocks * 16 +
             sum(g["kmax"] + 1 for g in geoms) * 16)
        d = sum(g["kmax"] for g in geoms) * (40 + 32 + 1) + 64
    return t, d


def check_plan(p, lens, bounds):
    """Geometry, prefixes, and every region inside its buffer, none
    overlapping another."""
    n = len(lens)
    slots = p["slots"]
    for j in range(n):
        want = want_geometry(lens[j], bounds[j], p["seg_log2"])
        assert {k: slots[j][k] for k in want} == want, j
    # workgroups per stream -> exclusive prefixes, the grid last
    wgs = {"scan": lambda g: cdiv(g["nseg"], p["scan_segs"]),
           "super": lambda g: g["nsuper"],
           "super3": lambda g: g["nsuper3"],
           "spread3": lambda g: cdiv(g["nsuper3"], 64),
           "spread2": lambda g: cdiv(g["nsuper"], 64),
           "cuts": lambda g: cdiv(g["nseg"], 512),
           "pieces": lambda g: cdiv(g["kmax"], 256)}
    for k, name in enumerate(PRE):
        acc, pre = 0, p["pre"][k]
        for j in range(n):
            assert pre[j] == acc, (name, j)
            acc += wgs[name](slots[j])
        assert pre[n] == acc == p["grid_" + name], name
    # sd_tables
    regions, e_regions = [], []
    for g in slots:
        regions.append((g["meta"], 64))
        for e, cnt in (("e1", g["nseg"]), ("e2", g["nsuper"]),
                       ("e3", g["nsuper3"])):
            e_regions.append((g[e], cnt * 16))
        regions += [(g["s1"], g["nseg"] * 8 * 16),
                    (g["s2"], g["nsuper"] * 64 * 8 * 16),
                    (g["s3"], g["nsuper3"] * 64 * 8 * 16),
                    (g["cuts"], (g["kmax"] + 1) * 16)]
    blocks = sum(g["nseg"] + g["nsuper"] + g["nsuper3"] for g in slots)
    assert p["e_bytes"] == blocks * 16
    # the e-tables of all streams are one run: the 0xFF fill covers them all
    pos = p["e_off"]
    for off, size in e_regions:
        assert off == pos
        pos += size
    assert pos == p["e_off"] + p["e_bytes"]
    assert p["slots"][0]["meta"] == 0  # snapmi_stream_decode_path reads it
    disjoint_inside(regions + e_regions, p["t_bytes"])
    # sd_desc: an array per field, every stream's pieces a run of each
    assert p["pieces"] == sum(g["kmax"] for g in slots)
    sizes = {"c_in": 8, "c_inlen": 8, "c_out": 8, "c_cap": 8, "c_outlen": 8,
             "c_err": 32, "c_mode": 1}
    entry = 0
    dregions = []
    for g in slots:
        assert g["entry"] == entry
        entry += g["kmax"]
        for f, sz in sizes.items():
            assert p[f] % min(sz, 8) == 0, f  # (snapmi_error: 8-aligned)
            dregions.append((p[f] + g["entry"] * sz, g["kmax"] * sz))
    disjoint_inside(dregions, p["d_bytes"])
    # the descriptor block: n descriptors, then the prefixes
    assert p["pre_off"] == n * DESC
    assert p["desc_bytes"] == p["pre_off"] + len(PRE) * (n + 1) * 4


def disjoint_inside(regions, total):
    last = 0
    for off, size in sorted(regions):
        assert off >= last, (off, last)
        last = off + size
    assert last <= total


def test_constants(P):
    assert constants(P) == dict(seg=4096, entry=8, seg_per_super=64,
                                cut_segs=512, scan_segs=64, scan_fill=1024,
                                chunk=65536, pre=7)


def test_segment_size(P):
    assert P.t_seg_log2(0, 0) == 10
    assert P.t_seg_log2(0, 256 * MIB - 1) == 10
    assert P.t_seg_log2(0, 256 * MIB) == 12
    assert P.t_seg_log2(0, 1 << 40) == 12
    for forced in (10, 12):
        for b in (0, 256 * MIB - 1, 256 * MIB, 3 << 30):
            assert P.t_seg_log2(forced, b) == forced


def test_scan_groups(P):
    # 64 segments a wavefront while that makes 1024 wavefronts, halved
    # while it does not, never below 8
    for segs in (64, 32, 16):
        edge = segs * 1024
        assert P.t_scan_segs(0, edge) == segs
        assert P.t_scan_segs(0, edge - 1) == segs // 2
        assert P.t_scan_segs(0, edge + 1) == segs
    assert P.t_scan_segs(0, 8 * 1024 - 1) == 8
    assert P.t_scan_segs(0, 0) == 8
    assert P.t_scan_segs(0, 1) == 8
    assert P.t_scan_segs(0, 1 << 40) == 64
    for forced in (8, 16, 64):
        assert P.t_scan_segs(forced, 1 << 20) == forced
        assert P.t_scan_segs(forced, 0) == forced


def test_lone_bound_and_pieces(P):
    # the caller's buffer, or 22x the input if that is smaller
    assert P.t_lone_bound(1000, 1 << 30) == 22000
    assert P.t_lone_bound(1000, 21999) == 21999
    assert P.t_lone_bound(1000, 22000) == 22000
    assert P.t_lone_bound(0, 5000) == 0
    # from 2^40 compressed bytes the input is not multiplied
    assert P.t_lone_bound((1 << 40) - 1, 1 << 62) == ((1 << 40) - 1) * 22
    assert P.t_lone_bound(1 << 40, 1 << 62) == 1 << 62
    assert P.t_lone_bound(1 << 41, 12345) == 12345
    for in_len, cap in ((0, 0), (100 * KIB, 150 * KIB), (100 * KIB, 1 << 40),
                        (7 * MIB + 3, 9 * MIB)):
        bound = P.t_lone_bound(in_len, cap)
        p = plan(P, [in_len], [bound], lone=True)
        assert p["slots"][0]["kmax"] == bound // 65536 + 2


def test_too_long(P):
    # kmax = bound / 64 KiB + 2 and nseg = ceil(len / seg) + 1 stay under
    # 2^30: 0x3FFFFFFF is the last that fits
    kmax_edge = (0x3FFFFFFF - 2) * 65536
    assert plan(P, [0], [kmax_edge + 65535], lone=True) is not None
    assert plan(P, [0], [kmax_edge + 65536], lone=True) is None
    nseg_edge = (0x3FFFFFFF - 1) << 12  # 4 KiB segments at this size
    assert plan(P, [nseg_edge], [0], lone=True) is not None
    assert plan(P, [nseg_edge + 1], [0], lone=True) is None
    assert plan(P, [1024, nseg_edge + 1], [0, 0]) is None


def test_lone_and_batch_scan_rules(P):
    # the lone stream's scan groups follow its segments (ceil + 1), a
    # batch's its long bytes per segment plus one per stream (floor + 1):
    # one segment apart unless the stream is a whole number of segments
    n = 65535 * KIB - 1  # 1 KiB segments: lone 65536 segments, batch 65535
    lone = plan(P, [n], [n * 2], lone=True)
    batch = plan(P, [n], [n * 2])
    assert lone["seg_log2"] == batch["seg_log2"] == 10
    assert lone["scan_segs"] == 64 and batch["scan_segs"] == 32
    n = 65536 * KIB
    assert plan(P, [n], [n], lone=True)["scan_segs"] == \
        plan(P, [n], [n])["scan_segs"] == 64
    # a batch: all its long bytes decide the segment size
    p = plan(P, [200 * MIB, 100 * MIB], [400 * MIB, 200 * MIB])
    assert p["seg_log2"] == 12
    assert p["scan_segs"] == P.t_scan_segs(0, (300 * MIB >> 12) + 2)


def test_overrides(P):
    p = plan(P, [300 * MIB], [600 * MIB], lone=True, seg_log2=10,
             scan_segs=16)
    assert p["seg_log2"] == 10 and p["scan_segs"] == 16
    check_plan(p, [300 * MIB], [600 * MIB])
    p = plan(P, [40 * KIB] * 3, [90 * KIB] * 3, seg_log2=12, scan_segs=64)
    assert p["seg_log2"] == 12 and p["scan_segs"] == 64
    check_plan(p, [40 * KIB] * 3, [90 * KIB] * 3)


@pytest.mark.parametrize("n", [1, 2, 3, 17, 255, 1000, 4096])
def test_batch_layout(P, n):
    rng = random.Random(n)
    lens, bounds = [], []
    for _ in range(n):
        ln = rng.choice([32 * KIB, 256 * KIB, 4 * MIB, 64 * MIB]) + \
            rng.randrange(-100, 100000)
        lens.append(ln)
        bounds.append(int(ln * rng.uniform(1.5, 21)))
    p = plan(P, lens, bounds)
    check_plan(p, lens, bounds)
    t, d = parent_bytes(p["slots"], lone=False)
    assert (p["t_bytes"], p["d_bytes"]) == (t, d)


@pytest.mark.parametrize("in_len,cap", [
    (32 * KIB, 48 * KIB), (100000, 1 << 30), (256 * MIB - 1, 1 << 33),
    (256 * MIB, 300 * MIB), (2 << 30, (2 << 30) + 5), (0, 0)])
def test_lone_layout(P, in_len, cap):
    bound = P.t_lone_bound(in_len, cap)
    p = plan(P, [in_len], [bound], lone=True)
    check_plan(p, [in_len], [bound])
    # the parent's sizes: the tables gain the 64 bytes of meta slack a batch
    # has; the pieces lose the whole-stream entry [kmax], which now travels
    # with the descriptor (73 bytes: five pointers / lengths, an error, a mode)
    t, d = parent_bytes(p["slots"], lone=True)
    assert p["t_bytes"] == t + 64
    assert p["d_bytes"] == d - 73


@pytest.mark.parametrize("in_len", [64 * KIB, 65536 * KIB, 300 * MIB])
def test_lone_is_a_batch_of_one(P, in_len):
    # a whole number of segments: the two scan rules agree too
    bound = 20 * in_len
    lone = plan(P, [in_len], [bound], lone=True)
    batch = plan(P, [in_len], [bound])
    assert lone == batch


def test_fixed_totals(P):
    # one 1 MiB stream of 3 MiB output: 1025 segments of 1 KiB
    p = plan(P, [MIB], [3 * MIB], lone=True)
    g = p["slots"][0]
    assert (g["nseg"], g["nsuper"], g["nsuper3"], g["kmax"]) == (1025, 17, 1,
                                                                 50)
    assert p["scan_segs"] == 8
    assert [p["grid_" + k] for k in PRE] == [129, 17, 1, 1, 1, 3, 1]
    assert p["t_bytes"] == 64 + 64 + (1025 + 18 * 64) * 128 + 1043 * 16 + \
        51 * 16
    assert p["d_bytes"] == 50 * 73 + 64


def test_long_stream_rule(P):
    """The C++ rule and long_streams.long_stream_rule agree around every edge
    of the rule - min_len and 256 KiB of input; an expansion of 1.5, of 22,
    and a piece and a half of output - and on seeded random pairs."""
    assert DESC == P.t_desc_size()
    min_len = 32 * KIB
    # (the 1.5 edge decides only from 64 KiB of input on, below 256 KiB, and
    # is hit exactly by an even length: 100 KiB)
    lens = [min_len - 1, min_len, min_len + 1, 100 * KIB, 100 * KIB + 1,
            256 * KIB - 1, 256 * KIB, 256 * KIB + 1, 3 * MIB]
    pairs = []
    for n in lens:
        dls = {3 * 65536 // 2 + d for d in (-1, 0, 1)}
        dls |= {(3 * n + 1) // 2 + d for d in (-2, -1, 0, 1)}
        dls |= set(range(22 * n - 22, 22 * n + 23))
        pairs += [(n, dl) for dl in sorted(dls)]
    rng = random.Random(20261020)
    for _ in range(2000):
        pairs.append((rng.randrange(1 << 33), rng.randrange(1 << 33)))
        pairs.append((int(2 ** rng.uniform(0, 33)), int(2 ** rng.uniform(0, 33))))
    seen = set()
    for n, dl in pairs:
        want = LS.long_stream_rule(n, dl, min_len)
        assert bool(P.t_long_stream_rule(n, dl, min_len)) == want, (n, dl)
        seen.add(want)
    assert seen == {True, False}
    # the default of the restatement is the library's (long_stream_min)
    assert LS.long_stream_rule(min_len, 3 * min_len) and \
        not LS.long_stream_rule(min_len - 1, 3 * min_len)
