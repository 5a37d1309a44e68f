"""GPU suite: the routes the DEFAULT options take, at the smallest batches that
select them, with every stream compared.

The other GPU suites force each kernel onto batches of a few hundred blocks
with options, so a few hundred of the 65 536 lane tables are ever used, and
the tests that do fill the chip used to compare a sample of their streams.
Here the batch sizes are what snapmi_route.hpp asks for with
snapmi_options.hpp's defaults - derived from the route itself
(tests/route_host.cpp, built as tests/test_route_cpu.py builds it, on the
device's own CU count), not written down - plus a margin, so that lanes take
a second block.  Inputs are tiled from 64 to 256 payloads cut from the
compressible files of tests/golden/corpus (tests/tiled_batch.py), sizes mixed
inside every group of 64 consecutive blocks; the oracle compresses each
payload once and assert_all compares every length, every error record and
every byte of every stream on the device.  Each case asserts that
ctx.last_kernel() is what the CPU route says, that table_probe_log() names the
route's lane count (as mapped chunks from 16 384 lanes on), and prints the
kernel, the lanes, the number of streams compared, its time and the device
memory it held.

One context per case, closed before the next is made: it holds 17 to 26 GB of
lane tables."""
import ctypes as C
import re
import subprocess
import time
from pathlib import Path

import numpy as np
import pytest
import torch

import blockindex_ref as BI
import oracle_lib as O
import tiled_batch as TB

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
BLOCK = 65536
MARGIN = 2048           # blocks above a threshold
MATCH = ["none", "k_match_spans", "k_match_both", "k_match_blocks"]
# compressible, all of them: match_kernel 2 sends a context whose last batch
# compressed to 90 % or more to the window match finder
FILES = ["alice29.txt", "asyoulik.txt", "lcet10.txt", "plrabn12.txt", "html",
         "urls.10K", "geo.protodata", "kppkn.gtb",
         "Mark.Twain-Tom.Sawyer.txt"]


# ---------------------------------------------------------------------
# the route on the CPU
# ---------------------------------------------------------------------
@pytest.fixture(scope="module")
def P(tmp_path_factory):
    so = tmp_path_factory.mktemp("route") / "route_host.so"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-shared",
                           "-fPIC", str(ROOT / "tests" / "route_host.cpp"),
                           "-o", str(so)])
    L = C.CDLL(str(so))
    u64 = C.c_uint64
    L.t_reset.restype = None
    L.t_set.restype = C.c_int
    L.t_set.argtypes = [C.c_char_p, C.c_int64]
    L.t_default.restype = C.c_int64
    L.t_default.argtypes = [C.c_char_p]
    L.t_route.restype = None
    L.t_route.argtypes = [u64, u64, C.c_int]
    L.t_get.restype = C.c_int64
    L.t_get.argtypes = [C.c_char_p]
    L.t_last_kernel.restype = C.c_char_p
    L.t_segment.restype = None
    L.t_segment.argtypes = [u64, u64, C.POINTER(u64)]
    L.t_small_stream_limit.restype = u64
    return L


def route(P, blocks, cnt8=0, **opts):
    """The route of `blocks` blocks, cnt8 of them of at most 8 KiB, on this
    device with the default options and `opts`: match finder, last_kernel,
    lanes and the (lo, hi, speculating) of every launch."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    P.t_reset()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    for k, v in dict(lds_order_ok=1, num_cus=cus, **opts).items():
        assert P.t_set(k.encode(), v) == 0, k
    P.t_route(blocks, cnt8, 0)
    r = {"match": MATCH[P.t_get(b"match")],
         "last_kernel": P.t_last_kernel().decode(),
         "lanes": P.t_get(b"lanes"), "seg_blocks": P.t_get(b"seg_blocks"),
         "small_grid": P.t_get(b"small_grid"), "cus": cus, "segments": []}
    out = (C.c_uint64 * 3)()
    for lo in range(0, blocks, max(r["seg_blocks"], 1)):
        hi = min(lo + r["seg_blocks"], blocks)
        P.t_segment(lo, hi, out)
        r["segments"].append((lo, hi, bool(out[1])))
    return r


def smallest(P, wanted, lo=1, hi=1 << 21, **opts):
    """The smallest block count in [lo, hi] whose route satisfies `wanted`
    (which holds from there on)."""
    assert wanted(route(P, hi, **opts)) and not wanted(route(P, lo, **opts))
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if wanted(route(P, mid, **opts)):
            hi = mid
        else:
            lo = mid
    return hi


def batch_route(P, tb, **opts):
    """The route of a batch as snapmi_compress_batch counts it: streams under
    the small-stream limit have no blocks, a stream's last block counts as
    small when it has at most 8 KiB."""
    P.t_reset()
    for k, v in opts.items():
        assert P.t_set(k.encode(), v) == 0, k
    lens = tb.in_lens[tb.in_lens >= max(int(P.t_small_stream_limit()), 1)]
    nb = -(-lens // BLOCK)
    cnt8 = int(((lens - (nb - 1) * BLOCK) <= 8192).sum())
    return route(P, int(nb.sum()), cnt8, **opts), int(nb.sum()), cnt8


# ---------------------------------------------------------------------
# payloads and batches
# ---------------------------------------------------------------------
class Payloads:
    """Distinct payloads cut from the corpus, by class of size, and what the
    oracle makes of each."""

    def __init__(self, seed, classes):
        rng = np.random.default_rng(seed)
        files = [(O.CORPUS / f).read_bytes() for f in FILES]
        self.data, self.of = [], {}
        for name, sizes in classes.items():
            self.of[name] = np.arange(len(self.data),
                                      len(self.data) + len(sizes))
            for n in sizes:
                # (a stream of several blocks: a file twice over if need be)
                f = files[int(rng.integers(len(files)))]
                f = f * (n // len(f) + 1)
                at = int(rng.integers(0, len(f) - n + 1))
                self.data.append(f[at:at + n])
        t0 = time.perf_counter()
        self.comp = [O.compress(p) for p in self.data]
        print(f"\n{len(self.data)} payloads of {sum(map(len, self.data))} "
              f"bytes, the oracle's bytes of them in "
              f"{time.perf_counter() - t0:.2f} s")
        import rust_snappy_amd as R
        self.caps = [R.raw.max_compress_len(len(p)) for p in self.data]
        assert len(set(self.data)) == len(self.data)

    def __len__(self):
        return len(self.data)


def big_kinds(rng, count, pay):
    """`count` one-block streams of more than 8 KiB: in every 64 consecutive
    ones 63 of 8 193 .. 12 000 bytes and one full block, at a place that
    moves from group to group."""
    kind = rng.choice(pay.of["big"], count)
    i = np.arange(count)
    full = i % 64 == (i // 64 * 7) % 64
    kind[full] = rng.choice(pay.of["full"], int(full.sum()))
    return kind


def chip_batch(P):
    """Cases a, b and e: lane_coresident_min_blocks one-block streams of more
    than 8 KiB and the margin, and among them 4 000 blocks of at most 8 KiB
    (k_match_spans_8k's), 1 500 streams each under 256 bytes and under 1 KiB
    (k_compress_tiny's, k_compress_small's), 300 empty ones and 300 of two to
    four blocks with a short tail."""
    rng = np.random.default_rng(98304)
    pay = Payloads(1, {
        "big": rng.integers(8193, 12001, 176).tolist(),
        "full": [BLOCK] * 4,
        "small8k": [1024, 2048, 4096, 8191, 8192] +
        rng.integers(1024, 8193, 35).tolist(),
        "tiny": [1, 16, 17, 255] +
        rng.choice(np.arange(18, 255), 8, replace=False).tolist(),
        "small": [256, 511, 512, 1023] +
        rng.choice(np.arange(513, 1023), 8, replace=False).tolist(),
        "empty": [0],
        "multi": [BLOCK + 1, 2 * BLOCK + 17, 3 * BLOCK + 8192,
                  3 * BLOCK + 8193] +
        [int(b) * BLOCK + int(t) for b, t in zip(rng.integers(1, 4, 7),
                                                 rng.integers(1, 5000, 7))]})
    assert len(pay) == 256
    both = smallest(P, lambda r: r["match"] == "k_match_both")
    assert both == P.t_default(b"lane_coresident_min_blocks")
    kind = big_kinds(rng, both + MARGIN, pay)
    extras = np.concatenate([rng.choice(pay.of[name], count) for name, count
                             in (("small8k", 4000), ("tiny", 1500),
                                 ("small", 1500), ("empty", 300),
                                 ("multi", 300))])
    kind = np.insert(kind, rng.integers(0, kind.size + 1, extras.size),
                     extras)
    return pay, TB.TiledBatch(pay.data, kind), both


@pytest.fixture(scope="module")
def chip(built, P):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    made = chip_batch(P)
    yield made
    del made
    torch.cuda.empty_cache()


def product_context(**opts):
    """The shipped library (libsnapmi.so) with its default options and
    `opts`."""
    import rust_snappy_amd as R
    c = R.raw.Context(0, lib=R._lib.load_product())
    for k, v in opts.items():
        c.set_option(k, v)
    return c


class Case:
    """One context's calls, timed, with the device memory in use when each
    has returned (free memory then, against free memory at the start)."""

    def __init__(self, name, ctx):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        self.name, self.ctx = name, ctx
        self.free0 = torch.cuda.mem_get_info()[0]
        self.low = self.free0
        self.t0 = time.perf_counter()
        self.compared = 0

    def compress(self, tb, pay, seed, index=False):
        """Every stream of tb into a fresh slab; asserts the guards, every
        length, record and byte; returns (slab, out_lens[, first, index])."""
        import rust_snappy_amd as R
        slab = tb.outputs(pay.caps, seed=seed)
        out_lens = torch.full((tb.n,), -1, dtype=torch.int64, device="cuda")
        errs = torch.zeros(32 * tb.n, dtype=torch.uint8, device="cuda")
        extra = {}
        if index:
            entries = int((-(-tb.in_lens // BLOCK) + 1).sum())
            extra = dict(
                index_first=torch.full((tb.n + 1,), -1, dtype=torch.int64,
                                       device="cuda"),
                index=torch.full((entries,), -1, dtype=torch.int64,
                                 device="cuda"),
                index_cap=entries)
        R.raw.compress_batch(self.ctx, tb.d_in_ptrs, tb.d_in_lens, slab.d_ptrs,
                             slab.d_caps, out_lens, errs,
                             host_in_lens=tb.h_in_lens, **extra)
        self.ctx.synchronize()
        self.low = min(self.low, torch.cuda.mem_get_info()[0])
        slab.assert_guards(self.name)
        self.compared += TB.assert_all(slab.data, slab.d_offs, out_lens,
                                       tb.kind, pay.comp, errs=errs,
                                       what=self.name)
        if index:
            return slab, out_lens, extra["index_first"], extra["index"]
        return slab, out_lens

    def assert_route(self, r):
        """The context ran what the CPU route names, on that many lanes."""
        assert self.ctx.last_kernel() == r["last_kernel"], self.name
        log = self.ctx.table_probe_log()
        m = re.search(r"kept \d+ KiB apart, (\d+) lanes, (\d+) bytes", log)
        assert m and int(m.group(1)) == r["lanes"], (self.name, log)
        assert ("chunks:" in log) == (r["lanes"] >= 16384), (self.name, log)
        self.tables = int(m.group(2))

    def report(self, r, n, note=""):
        self.ctx.synchronize()
        torch.cuda.synchronize()
        self.low = min(self.low, torch.cuda.mem_get_info()[0])
        print(f"\n{self.name}: {self.ctx.last_kernel()} on {r['lanes']} lanes"
              f" ({r['cus']} CUs), launches {r['segments']}; "
              f"{self.compared} streams compared in calls of {n}; "
              f"{time.perf_counter() - self.t0:.2f} s, "
              f"{(self.free0 - self.low) / 2**30:.2f} GiB of device memory "
              f"held behind its calls - output slab, scratch and "
              f"{self.tables / 2**30:.2f} GiB of lane tables"
              f"{note}")


def assert_compressible(pay, tb):
    """The batch stays below match_spans_ratio_pct: the context's next call
    takes the same match finder."""
    comp = np.array([len(c) for c in pay.comp], dtype=np.int64)[tb.kind].sum()
    assert comp * 100 < 80 * tb.in_lens.sum()


# ---------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------
def test_a_defaults_fill_the_chip_with_both_match_finders(chip, P):
    """The shipped library, no option set: k_match_both on 4 x CUs x 64 lanes,
    tables as mapped chunks, more blocks than lanes; beside it
    k_match_spans_8k, k_compress_tiny and k_compress_small in the same call.
    Then the same streams in reverse order on the same context - every table
    is full of the first call's epochs - and all of that call's outputs
    decoded by a default context, 100 000 streams planned on many
    workgroups."""
    import rust_snappy_amd as R
    pay, tb, both = chip
    assert_compressible(pay, tb)
    r, blocks, cnt8 = batch_route(P, tb)
    assert r["match"] == r["last_kernel"] == "k_match_both"
    assert r["lanes"] == 4 * 64 * r["cus"] and r["small_grid"] > 0
    assert blocks - cnt8 >= both + MARGIN and len(r["segments"]) == 1
    with product_context() as c:
        case = Case("a: defaults", c)
        slab, out_lens = case.compress(tb, pay, seed=1)
        case.assert_route(r)
        log = c.table_probe_log()
        del slab, out_lens
        back = tb.reordered(tb.kind[::-1])
        slab, out_lens = case.compress(back, pay, seed=2)
        case.assert_route(r)
        assert c.table_probe_log() == log          # (the same tables)
        case.report(r, tb.n)
    assert case.compared == 2 * tb.n
    t0 = time.perf_counter()
    with R.raw.Context(0) as d:
        out = back.outputs([len(p) for p in pay.data], seed=3)
        got = torch.full((back.n,), -1, dtype=torch.int64, device="cuda")
        errs = torch.zeros(32 * back.n, dtype=torch.uint8, device="cuda")
        R.raw.decompress_batch(d, slab.d_ptrs, out_lens, out.d_ptrs,
                               out.d_caps, got, errs)
        d.synchronize()
        out.assert_guards("a: decode")
        n = TB.assert_all(out.data, out.d_offs, got, back.kind, pay.data,
                          errs=errs, what="a: decode")
    print(f"a: decode: {n} streams compared with their inputs, "
          f"{time.perf_counter() - t0:.2f} s")
    assert n == tb.n


def test_b_lane_kernel_alone_reuses_every_table(chip, P):
    """lane_coresident 0: k_match_blocks on 6 x CUs x 64 lanes, every chunk
    slot in use, and more blocks than lanes: tables are reused inside the
    launch at the full lane count."""
    pay, tb, both = chip
    r, blocks, cnt8 = batch_route(P, tb, lane_coresident=0)
    assert r["match"] == r["last_kernel"] == "k_match_blocks"
    assert r["lanes"] == 6 * 64 * r["cus"] < blocks - cnt8
    assert r["segments"] == [(0, blocks, False)]
    with product_context(lane_coresident=0) as c:
        case = Case("b: lane_coresident 0", c)
        case.compress(tb, pay, seed=4)
        case.assert_route(r)
        case.report(r, tb.n)
    assert case.compared == tb.n


def test_c_two_segments_by_default(built, P):
    """Just over lane_segment_blocks one-block streams of 1 100 to 2 000
    bytes with small_table_kernel 0: two equal launches of k_match_both, the
    second's offsets carried over from the first's."""
    opts = dict(small_table_kernel=0)
    two = smallest(P, lambda r: len(r["segments"]) >= 2, **opts)
    assert two == P.t_default(b"lane_segment_blocks") + 1
    rng = np.random.default_rng(262144)
    pay = Payloads(2, {"all": [1100, 2000] +
                       rng.integers(1100, 2001, 126).tolist()})
    tb = TB.TiledBatch(pay.data, rng.choice(len(pay), two + MARGIN))
    assert_compressible(pay, tb)
    r, blocks, _ = batch_route(P, tb, **opts)
    assert blocks == tb.n and r["match"] == r["last_kernel"] == "k_match_both"
    half = -(-tb.n // 2)
    assert r["segments"] == [(0, half, False), (half, tb.n, False)]
    with product_context(**opts) as c:
        case = Case("c: two segments", c)
        case.compress(tb, pay, seed=5)
        case.assert_route(r)
        case.report(r, tb.n)
    assert case.compared == tb.n
    del tb
    torch.cuda.empty_cache()


@pytest.mark.parametrize("which", ["speculating", "plain"])
def test_d_lane_kernel_in_its_own_range(built, P, which):
    """Blocks of more than 8 KiB, defaults: k_match_blocks_spec between
    lane_min_blocks and lane_speculate_max_blocks, the plain kernel just above
    (one block per lane either way: fewer blocks than the chip has lanes)."""
    first = smallest(P, lambda r: r["match"] != "none")
    plain = smallest(P, lambda r: not r["segments"][0][2], lo=first)
    assert first == P.t_default(b"lane_min_blocks")
    assert plain == P.t_default(b"lane_speculate_max_blocks") + 1
    count = (first + plain) // 2 + 37 if which == "speculating" else plain + 37
    rng = np.random.default_rng(count)
    pay = Payloads(3, {"big": rng.integers(8193, 12001, 62).tolist(),
                       "full": [BLOCK] * 2})
    tb = TB.TiledBatch(pay.data, big_kinds(rng, count, pay))
    r, blocks, cnt8 = batch_route(P, tb)
    assert (blocks, cnt8) == (count, 0)
    assert r["match"] == r["last_kernel"] == "k_match_blocks"
    assert r["segments"] == [(0, count, which == "speculating")]
    assert r["lanes"] == -(-count // 64) * 64
    with product_context() as c:
        case = Case(f"d: {which}", c)
        case.compress(tb, pay, seed=6)
        case.assert_route(r)
        case.report(r, tb.n)
    assert case.compared == tb.n
    del tb
    torch.cuda.empty_cache()


def test_e_defaults_with_the_block_index(chip, P):
    """Case a through snapmi_compress_batch_indexed: the same bytes, and
    every entry of every stream's index is blockindex_ref's."""
    pay, tb, both = chip
    r, _, _ = batch_route(P, tb)
    per_kind = [np.array(BI.expected_index(p), dtype=np.int64)
                for p in pay.data]
    count = np.array([len(e) for e in per_kind], dtype=np.int64)
    assert count.tolist() == [BI.entries(len(p)) for p in pay.data]
    at = np.concatenate([[0], np.cumsum(count)[:-1]])
    first = np.concatenate([[0], np.cumsum(count[tb.kind])])
    # entry j of stream i is entry j of its kind: tile the kinds' entries
    take = np.repeat(at[tb.kind] - first[:-1], count[tb.kind]) + \
        np.arange(first[-1])
    want = torch.from_numpy(np.concatenate(per_kind)[take]).cuda()
    with product_context() as c:
        case = Case("e: defaults, indexed", c)
        _, _, got_first, got = case.compress(tb, pay, seed=7, index=True)
        case.assert_route(r)
        assert torch.equal(got_first, torch.from_numpy(first).cuda())
        wrong = torch.nonzero(got != want).flatten()
        if wrong.numel():
            e = int(wrong[0])
            i = int(np.searchsorted(first, e, side="right")) - 1
            raise AssertionError(
                f"{wrong.numel()} of {want.numel()} index entries differ; "
                f"the first: entry {e - first[i]} of stream {i} (kind "
                f"{tb.kind[i]}) is {int(got[e])}, expected {int(want[e])}")
        case.report(r, tb.n, f"; {want.numel()} index entries compared")
    assert case.compared == tb.n


def test_the_comparison_sees_one_planted_byte_on_the_device(built):
    """tests/test_tiled_batch_cpu.py on the device the cases above compare
    on: a compressed batch passes; one bit flipped in the last byte of the
    last stream is reported with its stream and offset, a byte behind a
    stream's length is not, a byte in a gap fails the guard check."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    rng = np.random.default_rng(7)
    pay = Payloads(4, {"all": [0, 1, 300, 70000] +
                       rng.integers(1024, 12001, 60).tolist()})
    tb = TB.TiledBatch(pay.data, rng.integers(0, len(pay), 5000))
    with product_context() as c:
        slab, out_lens = Case("planted", c).compress(tb, pay, seed=8)
    last = tb.n - 1
    end = int(slab.offs[last]) + len(pay.comp[tb.kind[last]])
    assert end < int(slab.offs[last]) + pay.caps[tb.kind[last]]
    slab.data[end] ^= 0xFF                      # behind the length
    assert TB.assert_all(slab.data, slab.d_offs, out_lens, tb.kind,
                         pay.comp) == tb.n
    slab.data[end - 1] ^= 1
    with pytest.raises(AssertionError) as e:
        TB.assert_all(slab.data, slab.d_offs, out_lens, tb.kind, pay.comp,
                      what="planted")
    assert f"planted: 1 of {tb.n} streams differ" in str(e.value)
    assert (f"stream {last} kind {tb.kind[last]}: " in str(e.value) and
            f"first wrong byte at {len(pay.comp[tb.kind[last]]) - 1}"
            in str(e.value)), str(e.value)
    slab.assert_guards("planted")
    gap = int(slab.offs[2500]) - 1
    slab.data[gap] = 0
    with pytest.raises(AssertionError) as e:
        slab.assert_guards("planted")
    assert e.value.args[0] == ("planted", 1, gap)
