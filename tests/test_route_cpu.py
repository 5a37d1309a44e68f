"""The compressor's routing (csrc/snapmi_route.hpp), on the CPU: which kernels
a batch runs for the options a context holds - DESIGN 4.1's table.  The GPU
suite forces each kernel with options and so tests the kernels; here the
choice the defaults make, and the choice every `cctx` configuration of
tests/conftest.py makes, row by row.  Options are MI355X's: 256 CUs, a device
that passed the LDS order self-check, snapmi_options.hpp's defaults."""
import ctypes as C
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent

# snapmi_options.hpp's defaults on an MI355X, pinned
MI355X = dict(compress_mode=1, lds_order_ok=1, num_cus=256,
              lane_min_blocks=20480, lane_segment_blocks=262144,
              lane_waves_per_cu=6, lane_max_waves=0, lane_coresident=1,
              lane_coresident_min_blocks=98304, small_table_kernel=1,
              small_table_min_blocks=256, small_batch_kernel=1, span_kernel=1,
              span_schedule=1, both_wave_cus=0, match_kernel=2,
              lane_speculate=1, lane_speculate_max_blocks=24576,
              lane_overlap_encode=0, tiny_stream_kernel=1,
              small_stream_kernel=1)
WINDOW = ["none", "k_compress_spans", "k_compress_span_lds",
          "k_compress_blocks", "k_compress_block_lds"]
MATCH = ["none", "k_match_spans", "k_match_both", "k_match_blocks"]
FIELDS = ["window_grid", "window_beside", "sched", "tokens", "small_grid",
          "nb_big", "direct", "post_ratio", "seg_blocks", "lanes",
          "stage_waves"]


@pytest.fixture(scope="module")
def P(tmp_path_factory):
    so = tmp_path_factory.mktemp("route") / "route_host.so"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-shared",
                           "-fPIC", str(ROOT / "tests" / "route_host.cpp"),
                           "-o", str(so)])
    L = C.CDLL(str(so))
    u64, u32 = C.c_uint64, C.c_uint32
    L.t_reset.restype = None
    L.t_default.restype = C.c_int64
    L.t_default.argtypes = [C.c_char_p]
    L.t_set.restype = C.c_int
    L.t_set.argtypes = [C.c_char_p, C.c_int64]
    L.t_route.restype = None
    L.t_route.argtypes = [u64, u64, C.c_int]
    L.t_get.restype = C.c_int64
    L.t_get.argtypes = [C.c_char_p]
    L.t_last_kernel.restype = C.c_char_p
    L.t_match_grid.restype = u32
    L.t_match_grid.argtypes = [u64]
    L.t_segment.restype = None
    L.t_segment.argtypes = [u64, u64, C.POINTER(u64)]
    L.t_prepare_lanes.restype = u32
    L.t_prepare_lanes.argtypes = [u64]
    L.t_small_stream_limit.restype = u64
    return L


# what the context finds out about an MI355X (not options)
DEVICE = dict(lds_order_ok=1, num_cus=256)


def _set(P, opts):
    """A fresh set of options - the table's own defaults - on an MI355X, then
    `opts`."""
    P.t_reset()
    for k, v in dict(DEVICE, **opts).items():
        assert P.t_set(k.encode(), v) == 0, k


def test_defaults_are_the_pinned_ones(P):
    """The routes below start from the option table's defaults: they are the
    values pinned here."""
    for k, v in MI355X.items():
        if k in DEVICE:
            assert DEVICE[k] == v, k
        else:
            assert P.t_default(k.encode()) == v, k


def route(P, blocks, cnt8=0, hint=False, **opts):
    """The route of a batch as a dict; 'segments': (lo, mid, hi, spec,
    match grid of each half - 0: no second half -, k_redo_spilled grid) of
    every token-path launch."""
    _set(P, opts)
    P.t_route(blocks, cnt8, int(hint))
    r = {f: P.t_get(f.encode()) for f in FIELDS}
    r["window"] = WINDOW[P.t_get(b"window")]
    r["match"] = MATCH[P.t_get(b"match")]
    r["last_kernel"] = P.t_last_kernel().decode()
    r["segments"] = []
    if r["tokens"]:
        out = (C.c_uint64 * 3)()
        for lo in range(0, blocks, r["seg_blocks"]):
            hi = min(lo + r["seg_blocks"], blocks)
            P.t_segment(lo, hi, out)
            mid, spec, redo = out
            r["segments"].append((lo, mid, hi, bool(spec),
                                  P.t_match_grid(mid - lo),
                                  P.t_match_grid(hi - mid) if mid < hi
                                  else 0, redo))
    return r


def prepare(P, blocks, **opts):
    _set(P, opts)
    return P.t_prepare_lanes(blocks)


def test_cfg2_runs_both_match_finders_in_one_launch(P):
    r = route(P, 146700)
    assert r["tokens"] and r["window"] == "none"
    assert r["match"] == r["last_kernel"] == "k_match_both"
    assert r["lanes"] == 65536 and r["stage_waves"] == 2
    assert r["direct"] and r["post_ratio"]
    assert r["segments"] == [(0, 146700, 146700, False, 256, 0, 256)]
    # (k_match_both from lane_coresident_min_blocks on)
    assert route(P, 98304)["match"] == "k_match_both"
    assert route(P, 98303)["match"] == "k_match_blocks"


def test_lane_kernel_from_lane_min_blocks_with_speculation_below_its_limit(P):
    r = route(P, 65536)
    assert r["match"] == r["last_kernel"] == "k_match_blocks"
    assert r["lanes"] == 65536 and r["direct"]
    assert r["segments"] == [(0, 65536, 65536, False, 1024, 0, 256)]
    r = route(P, 20480)
    assert r["match"] == r["last_kernel"] == "k_match_blocks"
    assert r["lanes"] == 20480 and r["stage_waves"] == 0
    assert r["segments"] == [(0, 20480, 20480, True, 320, 0, 256)]
    assert route(P, 24576)["segments"][0][3]
    r = route(P, 24577)
    assert r["lanes"] == 24640 and not r["segments"][0][3]


def test_window_kernel_below_lane_min_blocks(P):
    r = route(P, 20479)
    assert not r["tokens"] and r["match"] == "none"
    assert r["window"] == r["last_kernel"] == "k_compress_spans"
    assert r["window_grid"] == 256 and r["sched"] and not r["window_beside"]
    assert not r["direct"] and r["lanes"] == 0      # slots + k_compact
    r = route(P, 513)
    assert (r["window"], r["window_grid"], r["sched"]) == (
        "k_compress_spans", 103, False)
    # two blocks per CU and fewer: one block per CU, input in LDS as well
    r = route(P, 512)
    assert (r["window"], r["window_grid"], r["sched"]) == (
        "k_compress_span_lds", 256, False)
    assert r["last_kernel"] == "k_compress_spans"
    assert route(P, 10)["window_grid"] == 10


def test_blocks_of_at_most_8k_go_to_the_small_table_kernel(P):
    r = route(P, 300, cnt8=300)
    assert r["tokens"] and r["window"] == "none" and r["match"] == "none"
    assert r["small_grid"] == 30 and r["last_kernel"] == "k_match_spans_8k"
    assert r["lanes"] == 0 and r["stage_waves"] == 10 and r["direct"]
    assert r["segments"] == [(0, 300, 300, False, 0, 0, 60)]
    # fewer than small_table_min_blocks of them: the window kernel
    assert route(P, 600, cnt8=255)["window"] == "k_compress_spans"
    assert route(P, 300, cnt8=255)["window"] == "k_compress_span_lds"
    # beside the larger blocks' match finder, whose share they are not
    r = route(P, 1000, cnt8=900)
    assert (r["match"], r["small_grid"], r["nb_big"]) == ("k_match_spans",
                                                         90, 100)
    assert r["segments"] == [(0, 1000, 1000, False, 20, 0, 200)]
    r = route(P, 30000, cnt8=5000)
    assert (r["match"], r["small_grid"]) == ("k_match_blocks", 256)
    # (lanes for the whole segment, small blocks included)
    assert r["lanes"] == 30016 and r["stage_waves"] == 10


def test_no_blocks_runs_the_stream_kernels_only(P):
    r = route(P, 0)
    assert not r["tokens"] and r["window"] == "none"
    assert r["last_kernel"] == "k_compress_tiny" and not r["direct"]
    for tiny, small, limit in [(1, 1, 1024), (1, 2, 2048), (1, 0, 256),
                               (0, 1, 0), (0, 2, 0)]:
        _set(P, dict(tiny_stream_kernel=tiny, small_stream_kernel=small))
        assert P.t_small_stream_limit() == limit


def test_ratio_hint_sends_the_batch_to_the_window_match_finder(P):
    r = route(P, 146700, hint=True)
    assert r["match"] == r["last_kernel"] == "k_match_spans"
    assert r["lanes"] == 0 and r["stage_waves"] == 5 and r["direct"]
    assert r["segments"] == [(0, 146700, 146700, False, 256, 0, 256)]
    # only match_kernel 2 follows it
    assert route(P, 146700, hint=True, match_kernel=0)["match"] == \
        "k_match_both"
    # and k_post_ratio posts it from two lane_min_blocks on
    assert route(P, 40960)["post_ratio"]
    assert not route(P, 40959)["post_ratio"]
    assert not route(P, 146700, match_kernel=1)["post_ratio"]


def test_compress_mode_0_and_a_device_without_lds_order(P):
    r = route(P, 146700, compress_mode=0)
    assert not r["tokens"] and r["window"] == "k_compress_spans"
    assert r["window_grid"] == 256 and r["sched"]
    r = route(P, 10, lds_order_ok=0)
    assert r["tokens"] and r["window"] == "none"
    assert r["match"] == r["last_kernel"] == "k_match_blocks"
    assert r["lanes"] == 64 and r["direct"]
    assert r["segments"] == [(0, 10, 10, True, 1, 0, 2)]
    assert route(P, 10, lds_order_ok=0, compress_mode=0)["match"] == \
        "k_match_blocks"


def test_overlap_split_from_1_4_blocks_per_lane(P):
    opts = dict(lane_overlap_encode=1, lane_coresident=0)
    r = route(P, 146700, **opts)
    assert r["lanes"] == 98304 and not r["direct"]
    assert r["segments"] == [(0, 73350, 146700, False, 1536, 1536, 256)]
    r = route(P, 130000, **opts)
    assert r["segments"][0][:3] == (0, 130000, 130000)
    # (at exactly 1.4: 448 blocks on 320 lanes)
    opts.update(lane_max_waves=5, lane_min_blocks=1)
    assert route(P, 448, **opts)["segments"][0][:3] == (0, 224, 448)
    assert route(P, 447, **opts)["segments"][0][:3] == (0, 447, 447)


def test_compress_mode_2_puts_the_window_kernel_beside_one_segment_only(P):
    opts = dict(cctx_options("both"), lane_segment_blocks=64)
    r = route(P, 64, **opts)
    assert r["window_beside"] and not r["direct"]
    r = route(P, 200, **opts)
    assert r["window"] == "none" and r["direct"] and len(r["segments"]) == 4


# tests/conftest.py's cctx configurations (the options it sets; "_spill"
# changes the token pool only)
def cctx_options(param):
    opts = dict(
        compress_mode={"spans": 0, "spans_lds": 0, "waves": 0, "waves_lds": 0,
                       "lanes": 1, "lanes_segmented": 1, "lanes_overlap": 1,
                       "both": 2, "spans_match": 1, "small_tables": 1,
                       "small_tables_lanes": 1, "coresident": 1,
                       "spans_sched": 0}[param],
        lane_coresident=1 if param == "coresident" else 0,
        lane_coresident_min_blocks=1,
        small_table_kernel=1 if param.startswith("small_tables") else 0,
        small_table_min_blocks=1,
        match_kernel=1 if param == "spans_match" else 0,
        small_batch_kernel=2 if param in ("waves_lds", "spans_lds") else 0,
        span_kernel=0 if param in ("waves", "waves_lds") else 1,
        lane_min_blocks=1 << 30 if param == "small_tables" else 1,
        tiny_stream_kernel=0 if param in ("waves", "lanes_segmented") else 1,
        lane_overlap_encode=2 if param == "lanes_overlap" else 0)
    if param == "spans_sched":
        opts["span_schedule"] = 2
    if param == "lanes_segmented":
        opts.update(lane_segment_blocks=64, lane_speculate=0)
    return opts


@pytest.mark.parametrize("blocks", [1, 3, 200, 2000])
def test_cctx_configurations_run_the_kernels_they_name(P, blocks):
    def r(param, cnt8=0):
        return route(P, blocks, cnt8=cnt8, **cctx_options(param))

    grid = min(-(-blocks // 5), 256)
    for p in ("spans", "waves"):
        x = r(p)
        assert not x["tokens"] and x["window_grid"] == grid
        assert x["window"] == {"spans": "k_compress_spans",
                               "waves": "k_compress_blocks"}[p]
        assert x["sched"] == (p == "spans" and blocks > 1280)
        assert x["last_kernel"] == "k_compress_spans"
    assert r("spans_sched")["sched"]
    for p in ("spans_lds", "waves_lds"):
        x = r(p)
        assert x["window"] == {"spans_lds": "k_compress_span_lds",
                               "waves_lds": "k_compress_block_lds"}[p]
        assert x["window_grid"] == min(blocks, 256) and not x["tokens"]
    x = r("lanes")
    assert x["match"] == x["last_kernel"] == "k_match_blocks"
    assert x["window"] == "none" and x["direct"]
    assert x["segments"][0][3] == (blocks <= x["lanes"])
    x = r("lanes_segmented")
    seg = blocks if blocks <= 64 else -(-blocks // -(-blocks // 64))
    assert x["seg_blocks"] == seg and x["match"] == "k_match_blocks"
    assert len(x["segments"]) == -(-blocks // 64)
    assert not any(s[3] for s in x["segments"])
    x = r("lanes_overlap")
    assert not x["direct"]
    assert x["segments"] == [(0, blocks // 2 if blocks >= 2 else blocks,
                              blocks, True, x["lanes"] // 64,
                              x["lanes"] // 64 if blocks >= 2 else 0,
                              grid)]
    x = r("both")
    assert x["tokens"] and x["window"] == "k_compress_spans"
    assert x["window_beside"] and x["window_grid"] == min(grid, 128)
    assert not x["sched"] and not x["direct"]
    assert x["match"] == x["last_kernel"] == "k_match_blocks"
    x = r("spans_match")
    assert x["match"] == x["last_kernel"] == "k_match_spans"
    assert x["lanes"] == 0 and x["direct"]
    x = r("coresident")
    assert x["match"] == x["last_kernel"] == "k_match_both"
    assert x["lanes"] == 65536
    small = blocks // 2
    x = r("small_tables", cnt8=small)
    assert x["small_grid"] == min(-(-max(small, 1) // 10), 256) or not small
    # (a batch without such blocks: the window kernel, lane_min_blocks
    # being out of reach)
    assert x["last_kernel"] == ("k_compress_spans" if not small
                                else "k_match_spans")
    assert r("small_tables", cnt8=blocks)["last_kernel"] == "k_match_spans_8k"
    x = r("small_tables_lanes", cnt8=small)
    assert x["match"] == "k_match_blocks" and x["lanes"] == 64 * min(
        1536, -(-blocks // 64))


def test_prepare_keeps_its_own_rule(P):
    """snapmi_ctx_prepare's lane count: the launch's where both apply ..."""
    for blocks in (146700, 65536, 20480):
        assert prepare(P, blocks) == route(P, blocks)["lanes"]
    assert prepare(P, 20479) == 0
    assert prepare(P, 146700, compress_mode=0) == 0
    assert prepare(P, 146700, compress_mode=2) == 98304
    # ... and where it differs from what the launch then does
    assert prepare(P, 146700, match_kernel=1) == 65536
    assert route(P, 146700, match_kernel=1)["lanes"] == 0
    assert route(P, 146700, hint=True)["lanes"] == 0
    assert prepare(P, 10, compress_mode=0, lds_order_ok=0,
                   lane_min_blocks=1) == 0
    assert route(P, 10, compress_mode=0, lds_order_ok=0)["lanes"] == 64
