"""GPU suite: chains of calls on indexed raw streams, on every compressor
route.

tests/indexed_store.py is the model: a store of ten streams that is compressed
with its index once and then written into, appended to, re-indexed and read
for a dozen steps, each call taking the streams and the index that the call
before it wrote.  For streams whose blocks are self-contained every successful
write or append must give, bit for bit, O.compress of the patched or extended
data and B.expected_index of it (include/snapmi.h), whatever sequence of
calls came before - so every comparison here is byte or integer equality,
against the models of the single calls and against the oracle.

Every buffer is a gpu_buffers.Slab (exact capacities from the model plus a
small slack, guard bands, every alignment); the outputs are filled with the
guard byte and the index and length tensors with sentinels."""
import pytest
import torch

import indexed_store as S
from gpu_buffers import GUARD, Slab, read_errs, u64

pytestmark = pytest.mark.gpu

OK = S.OK
U64 = 1 << 64
FILL = U64 - 7  # what the index and length tensors hold before a call
PAD = 4         # sentinels behind every index


@pytest.fixture(scope="module", autouse=True)
def _gpu(built):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.fixture(scope="module")
def played():
    """The model's answers to every step of the scenarios, once."""
    return {"plain": S.play(S.SCENARIO), "fail": S.play(S.SCENARIO_FAIL),
            "long": S.play(S.SCENARIO_LONG)}


def filled(n, dtype=torch.int64, value=-7):
    return torch.full((n,), value, dtype=dtype, device="cuda")


def ints(t):
    return [x & (U64 - 1) for x in t.cpu().tolist()]


def flat(entries):
    return [e for idx in entries for e in idx]


# ------------------------------------------------ the device side of a step
class Buffers:
    """What one call of a chain reads and writes besides the streams and the
    index it is handed: sources, outputs, sentinels.  Made from the model's
    sizes alone, so all of a chain's can be allocated before its first
    call."""

    def __init__(self, p, k):
        self.p, self.k = p, k
        step, n = p.step, p.n
        kind = p.kind
        if kind == "compress":
            datas = step["datas"]
            self.src = Slab([max(len(d), 1) for d in datas], 5 * k + 1, datas)
            self.h_lens = torch.tensor([len(d) for d in datas],
                                       dtype=torch.int64)
            self.d_lens = self.h_lens.cuda()
            self.entries = len(p.flat)
            self.out = Slab(p.caps, 5 * k)
            self.out_lens, self.errs = filled(n), filled(32 * n, torch.uint8,
                                                         0x77)
            self.first = filled(n + 1)
            self.index = filled(self.entries + PAD)
        elif kind == "write":
            ws = step["writes"]
            self.src = Slab([max(len(w[2]), 1) for w in ws], 5 * k + 2,
                            [w[2] for w in ws])
            self.src_ptrs = [int(x) for x in self.src.d_ptrs.cpu().tolist()]
            self.entries = len(p.new_index)
            self.out = Slab(p.caps, 5 * k)
            self.out_lens, self.errs = filled(n), filled(32 * n, torch.uint8,
                                                         0x77)
            self.index = filled(self.entries + PAD)
        elif kind == "append":
            adds = step["appends"]
            self.src = Slab([max(len(b), 1) for b in adds], 5 * k + 2, adds)
            ptrs = [int(x) for x in self.src.d_ptrs.cpu().tolist()]
            self.src_ptrs = [x if b else 0 for x, b in zip(ptrs, adds)]
            self.entries = p.new_first[-1]
            self.out = Slab(p.caps, 5 * k)
            self.out_lens, self.errs = filled(n), filled(32 * n, torch.uint8,
                                                         0x77)
            self.first = filled(n + 1)
            self.index = filled(self.entries + PAD)
        elif kind == "rebuild":
            self.entries = len(p.flat)
            self.first = filled(n + 1)
            self.index = filled(self.entries + PAD)
            self.status = filled(n, torch.uint8, 0x77)
        else:
            self.out = Slab([len(d) for d in p.decoded], 5 * k)
            self.out_lens, self.errs = filled(n), filled(32 * n, torch.uint8,
                                                         0x77)
            rs = step["ranges"]
            self.r_out = Slab([r[2] for r in rs], 5 * k + 3)
            self.r_stream = torch.tensor([r[0] for r in rs],
                                         dtype=torch.int32, device="cuda")
            self.r_off = u64([r[1] for r in rs])
            self.r_len = u64([r[2] for r in rs])
            self.r_got = filled(len(rs))
            self.r_errs = filled(32 * len(rs), torch.uint8, 0x77)

    def enqueue(self, ctx, ptrs, lens, first, index, entries, between=None):
        """The call, on the streams (ptrs, lens) with the index (first, index,
        entries) - device tensors but for `entries`, the host's count."""
        from rust_snappy_amd import raw
        p, step = self.p, self.p.step
        if p.kind == "compress":
            raw.compress_batch(ctx, self.src.d_ptrs, self.d_lens,
                               self.out.d_ptrs, self.out.d_caps, self.out_lens,
                               self.errs, host_in_lens=self.h_lens,
                               index_first=self.first, index=self.index,
                               index_cap=self.entries)
        elif p.kind == "write":
            ws = step["writes"]
            raw.write_ranges_indexed(
                ctx, ptrs, lens, first, index, [w[0] for w in ws],
                [w[1] for w in ws], [len(w[2]) for w in ws], self.src_ptrs,
                self.out.d_ptrs, self.out.d_caps, self.out_lens, self.errs,
                self.index, index_entries=entries)
        elif p.kind == "append":
            raw.append_indexed(
                ctx, ptrs, lens, step["old_lens"], first, index,
                self.src_ptrs, [len(b) for b in step["appends"]],
                self.out.d_ptrs, self.out.d_caps, self.out_lens, self.errs,
                self.first, self.index, index_entries=entries,
                new_index_cap=self.entries)
        elif p.kind == "rebuild":
            _, streams, _ = p.before
            raw.build_block_index(
                ctx, ptrs, lens, [len(c) for c in streams],
                [len(d) for d in p.before[0]], self.first, self.index,
                self.status, index_cap=self.entries)
        else:
            raw.decompress_batch(ctx, ptrs, lens, self.out.d_ptrs,
                                 self.out.d_caps, self.out_lens, self.errs,
                                 index_first=first, index=index,
                                 index_entries=entries)
            if between:  # (between the two readers of a read step)
                between()
            rs = step["ranges"]
            raw.decompress_ranges_indexed(
                ctx, ptrs, lens, first, index, self.r_stream, self.r_off,
                self.r_len, [r[1] for r in rs], [r[2] for r in rs],
                self.r_out.d_ptrs, self.r_got, self.r_errs,
                index_entries=entries)

    # ---- what the call left, against the model
    def check_outputs(self, what):
        """The out slab, the lengths, the errors, the new index and its
        sentinels.  -> the error tuples."""
        p = self.p
        self.out.assert_guards(what)
        lens, errs = ints(self.out_lens), read_errs(self.errs)
        if p.kind == "compress":
            want = [(c, None, OK) for c in p.streams]
        else:
            want = p.res
        for s, (wbytes, _, werr) in enumerate(want):
            key = (what, s)
            n = 0 if wbytes is None else len(wbytes)
            assert errs[s] == werr, (key, errs[s], werr)
            assert lens[s] == n, (key, lens[s], n)
            got = self.out.bytes(s, n)
            if got != (wbytes or b""):
                at = next(i for i in range(n) if got[i] != wbytes[i])
                assert False, (key, "first differing byte", at,
                               "entries", p.after[2][s])
            if p.kind != "compress":
                # exactly [0, new length) is written - nothing for a stream
                # that failed or that nobody names
                rest = self.out.bytes(s, p.caps[s])[n:]
                assert rest == bytes([GUARD]) * len(rest), key
        index = ints(self.index)
        if p.kind == "compress":
            assert ints(self.first) == p.first, what
            assert index[:self.entries] == p.flat, what
        else:
            assert index[:self.entries] == p.new_index, what
            if p.kind == "append":
                assert ints(self.first) == p.new_first, what
        assert index[self.entries:] == [FILL] * PAD, what   # the sentinels
        return errs

    def check_oracle(self, what):
        """Every stream that succeeded is the oracle's stream of the model's
        data, with the oracle's index of it."""
        p = self.p
        data, streams, entries = p.after
        index = ints(self.index)
        nf = {"append": lambda: p.new_first, "compress": lambda: p.first,
              "write": lambda: S.firsts(p.before[2])}[p.kind]()
        for s in range(p.n):
            if p.kind != "compress" and p.res[s][0] is None:
                continue
            stream, idx = S.oracle(data[s])
            assert self.out.bytes(s, len(stream)) == stream, (what, s)
            assert index[nf[s]:nf[s + 1]] == idx, (what, s)

    def check_sources(self, what):
        p = self.p
        self.src.assert_guards(what)
        fill = {"compress": lambda: p.step["datas"],
                "write": lambda: [w[2] for w in p.step["writes"]],
                "append": lambda: p.step["appends"]}[p.kind]()
        for i, b in enumerate(fill):
            assert self.src.bytes(i, len(b)) == b, (what, i)

    def check_counters(self, ctx, what):
        p = self.p
        names = {"write": ("write_blocks", "write_blocks_decoded",
                           "write_streams_ok", "write_streams_failed"),
                 "append": ("append_blocks", "append_blocks_decoded",
                            "append_streams_ok", "append_streams_failed")}
        got = tuple(ctx.info(x) for x in names[p.kind])
        assert got == tuple(p.counters), (what, got, p.counters)

    def check_rebuild(self, what, first, index):
        """The index built from the streams alone is the carried one."""
        p = self.p
        assert self.status.cpu().tolist() == p.status == [1] * p.n, what
        assert ints(self.first) == p.first == ints(first), what
        got = ints(self.index)
        assert got[:self.entries] == p.flat, what
        assert got[:self.entries] == ints(index)[:self.entries], what
        assert got[self.entries:] == [FILL] * PAD, what

    def check_read(self, what):
        p = self.p
        self.out.assert_guards(what)
        self.r_out.assert_guards(what)
        assert read_errs(self.errs) == [OK] * p.n, what
        assert ints(self.out_lens) == [len(d) for d in p.decoded], what
        for s, d in enumerate(p.decoded):
            assert self.out.bytes(s, len(d)) == d, (what, s)
        got, errs = ints(self.r_got), read_errs(self.r_errs)
        for r, ((s, off, n), (wbytes, werr)) in enumerate(
                zip(p.step["ranges"], p.ranges)):
            key = (what, r, s, off, n)
            assert (errs[r], werr) == (OK, OK), (key, errs[r])
            assert got[r] == n, key
            assert self.r_out.bytes(r, n) == wbytes == \
                p.decoded[s][off:off + n], key


# the kernel snapmi_last_kernel names after a write or an append (the
# compressor's: both calls end their codec work with launch_compress) per
# configuration of the cctx fixture - csrc/snapmi_route.hpp
KERNEL = {"lanes": "k_match_blocks", "lanes_segmented": "k_match_blocks",
          "lanes_overlap": "k_match_blocks", "both": "k_match_blocks",
          "lanes_spill": "k_match_blocks", "spans_match": "k_match_spans",
          "spans_match_spill": "k_match_spans", "coresident": "k_match_both",
          "coresident_spill": "k_match_both", "spans_sched": "k_compress_spans",
          "product": "k_compress_spans", "dec3": "k_compress_spans",
          "dec2": "k_compress_spans"}


def kernel_of(name):
    return KERNEL[name[len("product-"):] if name.startswith("product-")
                  else name]


# --------------------------------------------------- a. one step at a time
class Chain:
    """The store on the device between two steps: where every stream lies,
    the length tensor and the index the next call is handed."""

    def __init__(self, n):
        self.ptrs = self.lens = self.first = self.index = None
        self.entries = 0
        self.home = [None] * n    # (slab, number in it) of every stream

    def check_inputs(self, p, what):
        """The streams the call read are unchanged, between intact bands."""
        _, streams, _ = p.before
        for slab in {id(h[0]): h[0] for h in self.home if h}.values():
            slab.assert_guards(what)
        for s, h in enumerate(self.home):
            if h:
                assert h[0].bytes(h[1], len(streams[s])) == streams[s], (
                    what, "input", s)

    def state(self):
        """(lengths, bytes, first, entries) as the device holds them."""
        lens = ints(self.lens)
        for slab in {id(h[0]): h[0] for h in self.home}.values():
            slab.fetch()
        return (lens, [h[0].bytes(h[1], n) for h, n in zip(self.home, lens)],
                ints(self.first), ints(self.index)[:self.entries])


def run_chain(ctx, run, kernel, check=True, spills=False, before_call=None):
    """The steps of a played scenario, one synchronize per step; step k + 1
    reads its streams where step k left them - a stream that succeeded in the
    out slab, a kept one in the slab it was already in - and nothing is
    repacked.  spills: the token pool starts again from the hundredth of the
    worst case the configuration gives it (a pool grows behind every call
    that spilled, and the context has served other tests), and some blocks of
    the chain must have been compressed again by k_redo_spilled.  -> the
    device's state behind every step."""
    c, trace, spilled = Chain(run[0].n), [], 0
    if spills:
        ctx.set_option("token_pool_pct", 1)
    for k, p in enumerate(run):
        what = f"step {k} {p.kind}"
        b = Buffers(p, k)
        torch.cuda.synchronize()  # the buffers are filled
        info = []

        def between():
            info.extend(ctx.info("index_streams_" + x)
                        for x in ("pieced", "fallback"))
            if before_call:
                before_call()
        if before_call:
            before_call()
        b.enqueue(ctx, c.ptrs, c.lens, c.first, c.index, c.entries, between)
        ctx.synchronize()
        if p.kind in ("write", "append"):
            assert ctx.last_kernel() == kernel, (what, ctx.last_kernel())
            if spills:
                spilled += ctx.info("token_blocks_spilled")
        if p.kind == "rebuild":
            b.check_rebuild(what, c.first, c.index)
        elif p.kind == "read":
            b.check_read(what)
            assert ctx.info("range_ranges_failed") == 0, what
            # every stream of two blocks and more was decoded by its index
            assert info == [sum(len(e) >= 3 for e in p.before[2]), 0], what
        elif check:
            b.check_outputs(what)
            b.check_oracle(what)
            b.check_sources(what)
            if p.kind != "compress":
                b.check_counters(ctx, what)
        if p.kind != "compress":
            c.check_inputs(p, what)
        if p.kind in ("rebuild", "read"):
            continue
        # the caller's rule, from what the device answered: a stream with a
        # length takes the new bytes, every other one keeps the old
        ok = b.out_lens != 0
        errs = read_errs(b.errs)
        if p.kind == "compress":
            c.ptrs, c.lens = b.out.d_ptrs, b.out_lens
            c.first, c.index, c.entries = b.first, b.index, b.entries
        else:
            c.ptrs = torch.where(ok, b.out.d_ptrs, c.ptrs)
            c.lens = torch.where(ok, b.out_lens, c.lens)
            failed = [s for s in range(p.n) if errs[s][0] != 0]
            if p.kind == "write" or not failed:
                # (a failed write's old entries are in the new index)
                if p.kind == "append":
                    c.first = b.first
                c.index, c.entries = b.index, b.entries
            else:
                # a failed append's new entries are 0: its old ones are kept
                f, nf = ints(c.first), ints(b.first)
                parts = [c.index[f[s]:f[s + 1]] if s in failed
                         else b.index[nf[s]:nf[s + 1]] for s in range(p.n)]
                c.first = u64(S.firsts([x.cpu().tolist() for x in parts]))
                c.index = torch.cat(parts + [filled(PAD)])
                c.entries = c.index.numel() - PAD
        for s, good in enumerate(ok.cpu().tolist()):
            if good:
                c.home[s] = (b.out, s)
        lens, streams, first, index = state = c.state()
        if check:
            data, want, entries = p.after
            assert lens == [len(x) for x in want], what
            assert streams == want, what
            assert first == S.firsts(entries) and index == flat(entries), what
        trace.append(state)
    assert not spills or spilled > 0
    return trace


# The "_spill" configurations whose pool a chain's calls overrun.  Not
# "coresident_spill": a launch of k_match_both keeps a page and a half in hand
# for every lane of three wavefronts on every CU (snapmi_pool.hpp), more than
# the blocks of these calls fill, so nothing spills there at this size; the
# configuration still runs, for what else it sets.
SPILLS = ("lanes_spill", "spans_match_spill")


def on_route(cctx, run, request, **kw):
    name = request.node.callspec.params["cctx"]
    return run_chain(cctx, run, kernel_of(name), spills=name in SPILLS, **kw)


@pytest.mark.parametrize("ctx", ["dec3", "dec2", "product"], indirect=True)
def test_chain_step_by_step(ctx, played, request):
    """SCENARIO_FAIL on the default route, through both decoders and the
    shipped library."""
    run_chain(ctx, played["fail"],
              kernel_of(request.node.callspec.params["ctx"]))


# (The "small_tables*" configurations are left out: k_match_spans_8k takes the
# blocks of at most 8 KiB that the caller counted, and the writes and appends
# hand launch_compress no such count - cnt8 is 0 at the call site in
# snapmi_update.hip, so compress_route never sets `small`.  "spans", "spans_lds",
# "waves*" are the window kernels the ctx parameters above already reach.)
ROUTES = ["product", "lanes", "lanes_segmented", "lanes_overlap", "both",
          "spans_match", "coresident", "spans_sched", "lanes_spill",
          "coresident_spill", "spans_match_spill", "product-lanes",
          "product-coresident_spill"]


@pytest.mark.parametrize("cctx", ROUTES, indirect=True)
def test_chain_step_by_step_on_every_route(cctx, played, request):
    """SCENARIO_FAIL with the compressor forced into every route a write or
    an append can reach: the lane match finder, the token pool and its
    spills, k_encode_tokens, segmented launches, the scratch slots and
    k_compact."""
    on_route(cctx, played["fail"], request)


@pytest.mark.parametrize("cctx", ["lanes_segmented", "lanes_spill",
                                  "product"], indirect=True)
def test_more_blocks_than_a_segment(cctx, played, request):
    """SCENARIO_LONG: an append of 70 new blocks, a write over 135 and an
    append of 71, each call on what the one before it wrote.  In
    "lanes_segmented" every one of them is cut into token-path launches of at
    most 64 blocks, whose slots, tokens and sizes the next segment reuses; in
    "lanes_spill" nearly all of a call's blocks are compressed a second
    time."""
    for p in played["long"]:
        if p.kind in ("write", "append"):
            assert p.counters[0] > S.SEGMENT
    on_route(cctx, played["long"], request)


# --------------------------------------------------- b. enqueue only
ENQUEUE_ROUTES = {
    "default": {},
    "lanes": {"compress_mode": 1, "lane_min_blocks": 1, "lane_coresident": 0},
    "coresident": {"compress_mode": 1, "lane_min_blocks": 1,
                   "lane_coresident": 1, "lane_coresident_min_blocks": 1},
    # a group per stream: the write scratch is reused many times in a chain
    "default-floor": {"write_scratch_bytes": S.W.FLOOR},
}


@pytest.mark.parametrize("library,route", [
    ("test", "default"), ("test", "lanes"), ("test", "coresident"),
    ("product", "default"), ("product", "lanes"), ("product", "coresident"),
    ("test", "default-floor")])
def test_chain_enqueue_only(built, played, library, route):
    """SCENARIO - every step names every stream - enqueued on a fresh context
    on a caller's stream: each call's out slab, length tensor and index
    tensors are the next call's inputs as they are, everything is allocated
    before the first call, and there is one synchronize at the end.  Then
    every intermediate slab, length and index is still what the model says
    of its step: no later call has written to it."""
    import rust_snappy_amd as R_
    run = played["plain"]
    stream = torch.cuda.Stream()
    lib = R_._lib.load_product() if library == "product" else None
    ctx = R_.raw.Context(0, stream=stream.cuda_stream, lib=lib)
    try:
        for name, value in ENQUEUE_ROUTES[route].items():
            ctx.set_option(name, value)
        with torch.cuda.stream(stream):
            bufs = [Buffers(p, k) for k, p in enumerate(run)]
            stream.synchronize()
            ptrs = lens = first = index = None
            entries = 0
            handed = []
            for b in bufs:
                b.enqueue(ctx, ptrs, lens, first, index, entries)
                handed.append((first, index))
                if b.p.kind in ("compress", "write", "append"):
                    ptrs, lens = b.out.d_ptrs, b.out_lens
                    index, entries = b.index, b.entries
                if b.p.kind in ("compress", "append", "rebuild"):
                    # (the rebuilt index is the one the next call gets)
                    first, index = b.first, b.index
            ctx.synchronize()  # the one wait
            for k, b in enumerate(bufs):
                what = f"step {k} {b.p.kind}"
                if b.p.kind == "rebuild":
                    b.check_rebuild(what, *handed[k])
                elif b.p.kind == "read":
                    b.check_read(what)
                else:
                    errs = b.check_outputs(what)
                    assert errs == [OK] * S.N, what
                    b.check_oracle(what)
                    b.check_sources(what)
            assert ctx.info("range_ranges_failed") == 0
    finally:
        ctx.close()


# --------------------------------------------------- c. twice on one context
def twice(ctx, run, kernel, spills=False):
    one = run_chain(ctx, run, kernel, spills=spills)
    # (with the pool as the first pass left it: grown behind its spills)
    two = run_chain(ctx, run, kernel, check=False)
    assert len(one) == len(two)
    for k, (a, b) in enumerate(zip(one, two)):
        assert a == b, f"pass 2 differs behind mutating step {k}"


@pytest.mark.parametrize("ctx", ["dec3"], indirect=True)
def test_chain_twice_gives_the_same_bytes(ctx, played):
    """The chain a second time on a context that has served it once - grown
    scratch, the token pool's statistics and the ratio hint carried over:
    every stream and every entry of the second pass equals the first."""
    twice(ctx, played["fail"], kernel_of("dec3"))


@pytest.mark.parametrize("cctx", ["lanes_spill", "coresident"], indirect=True)
def test_chain_twice_gives_the_same_bytes_on_the_token_path(cctx, played,
                                                            request):
    name = request.node.callspec.params["cctx"]
    twice(cctx, played["fail"], kernel_of(name), spills=name in SPILLS)


# --------------------------------------------------- d. the wrappers
@pytest.mark.parametrize("ctx", ["product"], indirect=True)
def test_chain_through_the_python_wrappers(ctx, played):
    """The first six steps of SCENARIO through batch.compress, batch.append,
    batch.write_ranges, batch.build_index, batch.decompress and
    batch.read_ranges, each handed the StreamBatch and the index pair the
    call before it returned: the wrappers' own merge of kept and new
    streams, several calls deep."""
    from rust_snappy_amd import batch
    run = played["plain"][:6]
    assert [p.kind for p in run] == ["compress", "append", "write", "append",
                                     "rebuild", "read"]
    cur = idx = None
    for k, p in enumerate(run):
        what = f"step {k} {p.kind}"
        data, streams, entries = p.after
        if p.kind == "compress":
            src = batch.StreamBatch.from_bytes(p.step["datas"],
                                               torch.device("cuda"))
            cur, first, index = batch.compress(ctx, src, want_index=True)
            idx = (first, index)
        elif p.kind == "append":
            cur, idx, errs = batch.append(
                ctx, cur, idx, list(enumerate(p.step["appends"])))
            assert [tuple(e) for e in errs] == [OK] * S.N, what
        elif p.kind == "write":
            cur, idx, errs = batch.write_ranges(ctx, cur, idx,
                                                p.step["writes"])
            assert [tuple(e) for e in errs] == [OK] * S.N, what
        elif p.kind == "rebuild":
            first, index, status = batch.build_index(ctx, cur)
            assert status == [1] * S.N, what
            assert ints(first) == ints(idx[0]), what
            assert ints(index) == ints(idx[1]), what
            idx = (first, index)
        else:
            dst, dlens, derrs = batch.decompress(ctx, cur, index=idx)
            for s in range(S.N):
                assert tuple(derrs[s]) == OK, (what, s)
                assert dst.stream_bytes(s, dlens[s]) == data[s], (what, s)
            got, rerrs = batch.read_ranges(ctx, cur, idx, p.step["ranges"])
            assert [tuple(e) for e in rerrs] == [OK] * len(got), what
            assert got == [data[s][o:o + n]
                           for s, o, n in p.step["ranges"]], what
        assert [cur.stream_bytes(s) for s in range(S.N)] == streams, what
        assert ints(idx[0]) == S.firsts(entries), what
        assert ints(idx[1]) == flat(entries), what
