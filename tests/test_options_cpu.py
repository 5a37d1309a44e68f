"""The option table and the info names (csrc/snapmi_options.hpp), on the CPU:
what snapmi_ctx_set_option, snapmi_ctx_set_test_option and
snapmi_ctx_get_info accept, in the product library and in the test build,
without a context (which needs a device: tests/test_gpu_options.py).

Every default and every bound below is written out: they are what the parent
of the table - the fields of snapmi_ctx.hpp and the if-chains of
snapmi_api.hip - had, so that neither can move unnoticed.  Nothing expected
is read back from the table."""
import ast
import ctypes as C
import functools
import subprocess
import tempfile
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
INF = 2 ** 63 - 1     # no upper bound: any int64 from lo on

# name: (default, lo, hi) of the product library
PRODUCT = {
    "compress_mode": (1, 0, 1),
    "lane_min_blocks": (20480, 1, INF),
    "lane_segment_blocks": (262144, 64, 0x7FFFFFFF),
    "lane_table_spread": (1, 0, 1),
    "lane_table_tries": (2, 1, 16),
    "lane_table_budget_pct": (33, 1, 90),
    "token_pool_pct": (39, 1, 100),
    "token_pool_min_pages": (32768, 0, 0x7FFFFFFF),
    "span_schedule": (1, 0, 2),
    "lane_coresident": (1, 0, 1),
    "lane_coresident_min_blocks": (98304, 1, INF),
    "small_table_kernel": (1, 0, 1),
    "small_table_min_blocks": (256, 1, INF),
    "small_batch_kernel": (1, 0, 2),
    "lane_speculate": (1, 0, 1),
    "lane_tail_probes": (2, 0, 4),
    "lane_tail_idle_pct": (40, 0, 100),
    "span_kernel": (1, 1, 1),
    "match_kernel": (2, 0, 2),
    "match_spans_ratio_pct": (90, 1, 200),
    "release_scratch": (0, 0, 1),
    "batch_long_streams": (1, 0, 1),
    "both_wave_cus": (0, 0, 4096),
    "tiny_stream_kernel": (1, 0, 1),
    "small_stream_kernel": (1, 0, 2),
    "frame_parallel_walk_min": (4 << 20, 0, INF),
    "host_copy_kernel": (1, 0, 3),
    "host_encode_slice": (2048 << 20, 65536, INF),
    "host_decode_slice_chunks": (8192, 1, INF),
    "host_batch_slice": (16 << 20, 65536, INF),
    "range_scratch_bytes": (1 << 30, 128 << 10, INF),
    # one block's compress slot (kSlotBytes) and its room (kMaxBlock)
    "write_scratch_bytes": (1 << 30, 76496 + 65536, INF),
}
# the cross-checks of the test build: a wider interval through the same call
TEST_BUILD_WIDER = {"compress_mode": (0, 2), "span_kernel": (0, 1)}
# name: (default, lo, hi) of snapmi_ctx_set_test_option; default None: the
# name has no field, it acts on the context
TEST = {
    "lane_waves_per_cu": (6, 1, 32),
    "decode_many_min": (1 << 20, 0, INF),
    "lane_speculate_max_blocks": (24576, 0, INF),
    "lane_max_waves": (0, 0, 0x7FFFFFFF),
    "frame_crc_side_stream": (1, 0, 1),
    "lane_tables_uncached": (0, 0, 1),
    "lane_overlap_encode": (0, 0, 2),
    "frame_walk_segment": (32 << 20, 128 << 10, INF),
    "lane_table_probe": (0, 0, 1),
    "lane_tables_renew": (None, 1, 1),
    "lane_epoch_preset": (-1, -1, 0xFFFF),
    "index_build_route": (0, 0, 2),
    "index_build_group_streams": (4096, 1, 4096),
    "lds_order_ok": (None, 0, 1),
    "host_batch_direct_min": (1 << 20, 0, INF),
    "host_batch_pack_to_host": (1, 0, 1),
    "host_batch_listed": (1, 0, 1),
    "scratch_fill": (-1, -1, 255),
}
# accepted sets that are no interval: name: (test-only, default, members,
# the nearest non-members)
SETS = {
    "decode_kernel": (False, 3, [0, 3], [-1, 1, 2, 4]),
    "stream_seg_log2": (True, 0, [0, 10, 12], [-1, 1, 9, 11, 13]),
    "stream_scan_segs": (True, 0, [0, 8, 16, 32, 64],
                         [-1, 1, 7, 9, 15, 17, 31, 33, 63, 65]),
    "lane_table_stride_kib": (True, 0, [0, 256, 260, 2048, 4092, 4096],
                              [-1, 1, 4, 252, 255, 257, 258, 259, 4093, 4095,
                               4097, 4100]),
}
# ... and the one of them whose set is wider in the test build
DECODE_KERNEL_TEST_BUILD = ([0, 2, 3], [-1, 1, 4])

INFO = ["scratch_bytes", "token_scratch_bytes", "token_pool_pages",
        "token_pool_pct_now", "token_pages_asked", "token_blocks_spilled",
        "host_batch_slices", "host_batch_h2d_bytes", "host_batch_d2h_bytes",
        "host_batch_listed_slices", "index_streams_pieced",
        "index_streams_fallback", "range_pieces", "range_ranges_ok",
        "range_ranges_failed", "write_blocks", "write_blocks_decoded",
        "write_streams_ok", "write_streams_failed", "append_blocks",
        "append_blocks_decoded", "append_streams_ok", "append_streams_failed",
        "index_build_built", "index_build_unaligned", "index_build_corrupt",
        "index_build_missized", "index_build_walked", "frame_nowait_front"]
INFO_TEST_BUILD = ["lane_multi_rounds", "scratch_fill_buffers",
                   "scratch_fill_bytes", "scratch_fill_seen"]

ACCEPTED, UNKNOWN, REFUSED = 0, 1, 2


class Table:
    """tests/options_host.cpp, loaded."""

    def __init__(self, L):
        self.L = L
        self.options = {}       # name: (test_only, default or None)
        self.option_names = []  # as listed, duplicates and all
        for i in range(L.t_option_count()):
            name = L.t_option_name(i).decode()
            self.option_names.append(name)
            self.options[name] = (
                bool(L.t_option_test_only(i)),
                L.t_option_default(i) if L.t_option_has_field(i) else None)
        self.info_names = [L.t_info_name(i).decode()
                           for i in range(L.t_info_count())]
        self.info = {L.t_info_name(i).decode(): bool(L.t_info_test_only(i))
                     for i in range(L.t_info_count())}

    def has_option(self, name, test_only):
        """`name` is an option of that entry point."""
        return self.options.get(name, (None,))[0] is test_only

    def has_info(self, name, test_only=False):
        return self.info.get(name) is test_only

    def attempt(self, name, value, test_entry_point, test_build):
        """(verdict, what the field holds when accepted and there is one)"""
        stored = C.c_int64(-12345)
        r = self.L.t_option_try(name.encode(), value, int(test_entry_point),
                                int(test_build), C.byref(stored))
        return r, stored.value


@functools.lru_cache(maxsize=None)
def options_table():
    """The host program over the tables, built once per process (plain g++,
    no device); the tests of other modules that ask for a name come here."""
    so = Path(tempfile.mkdtemp(prefix="snapmi_options_")) / "options_host.so"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-shared",
                           "-fPIC", str(ROOT / "tests" / "options_host.cpp"),
                           "-o", str(so)])
    L = C.CDLL(str(so))
    u64, i64 = C.c_uint64, C.c_int64
    for f, res, args in (("t_option_count", u64, []),
                         ("t_option_name", C.c_char_p, [u64]),
                         ("t_option_test_only", C.c_int, [u64]),
                         ("t_option_has_field", C.c_int, [u64]),
                         ("t_option_default", i64, [u64]),
                         ("t_option_index", i64, [C.c_char_p]),
                         ("t_option_try", C.c_int,
                          [C.c_char_p, i64, C.c_int, C.c_int,
                           C.POINTER(i64)]),
                         ("t_info_count", u64, []),
                         ("t_info_name", C.c_char_p, [u64]),
                         ("t_info_test_only", C.c_int, [u64])):
        getattr(L, f).restype = res
        getattr(L, f).argtypes = args
    return Table(L)


@pytest.fixture(scope="module")
def T():
    return options_table()


def _intervals():
    """(name, test-only, lo, hi) of every interval entry above."""
    return ([(n, False, lo, hi) for n, (_, lo, hi) in PRODUCT.items()] +
            [(n, True, lo, hi) for n, (_, lo, hi) in TEST.items()])


def test_no_name_occurs_twice_and_the_names_are_these(T):
    assert len(T.option_names) == len(set(T.option_names))
    assert len(T.info_names) == len(set(T.info_names))
    product = set(PRODUCT) | {n for n, s in SETS.items() if not s[0]}
    test = set(TEST) | {n for n, s in SETS.items() if s[0]}
    assert not product & test
    assert {n for n, (t, _) in T.options.items() if not t} == product
    assert {n for n, (t, _) in T.options.items() if t} == test
    assert {n for n, t in T.info.items() if not t} == set(INFO)
    assert {n for n, t in T.info.items() if t} == set(INFO_TEST_BUILD)
    # an index by name finds the entry of that name
    for i, n in enumerate(T.option_names):
        assert T.L.t_option_index(n.encode()) == i
    assert T.L.t_option_index(b"no_such_option") == -1


def test_defaults_are_the_parents(T):
    want = {n: d for n, (d, _, _) in dict(PRODUCT, **TEST).items()}
    want.update({n: s[1] for n, s in SETS.items()})
    assert {n: d for n, (_, d) in T.options.items()} == want


def test_every_name_is_documented_where_it_belongs(T):
    header = (ROOT / "include" / "snapmi.h").read_text()
    test_h = (ROOT / "include" / "snapmi_test.h").read_text()
    raw = ast.parse((ROOT / "rust-snappy_amd" / "raw.py").read_text())
    doc = next(ast.get_docstring(f) for c in raw.body
               if isinstance(c, ast.ClassDef) and c.name == "Context"
               for f in c.body
               if isinstance(f, ast.FunctionDef) and f.name == "info")
    for name, (test_only, _) in T.options.items():
        assert f'"{name}"' in (test_h if test_only else header), name
    for name, test_only in T.info.items():
        assert f'"{name}"' in (test_h if test_only else header), name
        assert f'"{name}"' in doc, name


@pytest.mark.parametrize("test_build", [False, True])
def test_interval_bounds(T, test_build):
    for name, test_only, lo, hi in _intervals():
        if test_build:
            lo, hi = TEST_BUILD_WIDER.get(name, (lo, hi))
        inside = [lo, hi]
        outside = [v for v in (lo - 1, hi + 1) if -2 ** 63 <= v <= INF]
        assert outside, name
        for v in inside:
            r, stored = T.attempt(name, v, test_only, test_build)
            assert r == ACCEPTED, (name, v)
            # the field holds it (a bool: whether it is not 0; above 32 bits a
            # narrower field truncates, as the setters always did)
            if T.options[name][1] is not None and abs(v) < 2 ** 31:
                assert stored == v, (name, v, stored)
        for v in outside:
            assert T.attempt(name, v, test_only, test_build)[0] == REFUSED, \
                (name, v)


@pytest.mark.parametrize("test_build", [False, True])
def test_accepted_sets(T, test_build):
    for name, (test_only, _, members, others) in SETS.items():
        if name == "decode_kernel" and test_build:
            members, others = DECODE_KERNEL_TEST_BUILD
        for v in members:
            assert T.attempt(name, v, test_only, test_build) == (ACCEPTED, v), \
                (name, v)
        for v in others:
            assert T.attempt(name, v, test_only, test_build)[0] == REFUSED, \
                (name, v)


def test_product_build_refuses_the_cross_checks(T):
    for name, v in (("compress_mode", 2), ("span_kernel", 0),
                    ("decode_kernel", 2)):
        assert T.attempt(name, v, False, False)[0] == REFUSED, name
        assert T.attempt(name, v, False, True) == (ACCEPTED, v), name
    # and knows no test-only name, at a value the test entry point takes
    for name, (_, lo, _) in TEST.items():
        assert T.attempt(name, lo, False, False)[0] == UNKNOWN, name
    for name, (test_only, _, members, _) in SETS.items():
        if test_only:
            assert T.attempt(name, members[0], False, False)[0] == UNKNOWN


@pytest.mark.parametrize("test_build", [False, True])
def test_each_entry_point_knows_its_own_names_only(T, test_build):
    mine = {n: lo for n, _, lo, _ in _intervals()}
    mine.update({n: s[2][0] for n, s in SETS.items()})
    for name, (test_only, _) in T.options.items():
        v = mine[name]
        assert T.attempt(name, v, test_only, test_build)[0] == ACCEPTED, name
        assert T.attempt(name, v, not test_only, test_build)[0] == UNKNOWN, \
            name
    for entry in (False, True):
        assert T.attempt("no_such_option", 1, entry, test_build)[0] == UNKNOWN
        assert T.attempt("", 1, entry, test_build)[0] == UNKNOWN
