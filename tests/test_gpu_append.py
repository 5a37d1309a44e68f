"""GPU suite: appends to indexed raw streams (snapmi_append_indexed).

A stream that succeeds must be, byte for byte, varint(new length), the old
full blocks' compressed bytes and the oracle's streams of the new blocks - for
the oracle's own streams that is O.compress(old + extra) with
B.expected_index(old + extra) - and a stream that fails has the error
include/snapmi.h names, a buffer nobody wrote to and new entries that are all
0 (appendindex_ref.expect is that contract in Python).  The streams, the
appended bytes and every output sit between guard bands (gpu_buffers.Slab)
that are checked after every call, and the outputs are filled with the guard
byte, so a byte written behind a stream's new length shows as well."""
import ctypes as C
import random

import pytest
import torch

import appendindex_ref as A
import blockindex_ref as B
import oracle_lib as O
from gpu_buffers import GUARD, Slab, read_errs, u64

pytestmark = pytest.mark.gpu

OK = A.OK
U64 = 1 << 64
SLACK = 37  # bytes of capacity behind the length a stream is expected to take
FILL = U64 - 7  # what the index tensors hold before a call


@pytest.fixture(scope="module", autouse=True)
def _gpu(built):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.fixture(scope="module")
def case():
    return A.Case()


class Call:
    """The device side of one call: streams, index, appended bytes and
    outputs in slabs.  appends[i]: the bytes appended to stream i (empty: not
    named)."""

    def __init__(self, case, appends, flat=None, first=None, comps=None,
                 old_lens=None, caps=None, seed=0, index_entries=None):
        self.case, self.appends = case, [bytes(b) for b in appends]
        self.comps = case.comps if comps is None else comps
        self.flat = case.flat if flat is None else flat
        self.first = case.first if first is None else first
        self.old_lens = case.old_lens if old_lens is None else old_lens
        # (the host's copy of first[n]; smaller: the index is cut short)
        self.entries = len(self.flat) if index_entries is None \
            else index_entries
        n = len(self.comps)
        if caps is None:
            # what the model says each stream takes, and a little more
            res, _, _ = self.model([1 << 40] * n)
            caps = [len(r[0]) + SLACK if r[0] is not None else 64
                    for r in res]
        self.caps = caps
        self.src = Slab([len(c) for c in self.comps], seed + 1, self.comps)
        self.in_lens = u64([len(c) for c in self.comps])
        self.d_first = u64(self.first)
        self.d_index = u64(self.flat + [7] * 4)  # (never read: behind it)
        self.asrc = Slab([max(len(b), 1) for b in self.appends], seed + 2,
                         self.appends)
        ptrs = [int(p) for p in self.asrc.d_ptrs.cpu().tolist()]
        self.a_ptrs = [p if b else 0 for p, b in zip(ptrs, self.appends)]
        self.a_lens = [len(b) for b in self.appends]
        self.total = A.new_first(self.old_lens, self.a_lens)[-1]
        self.out = Slab(caps, seed)
        self.out_lens = torch.full((n,), -7, dtype=torch.int64, device="cuda")
        self.errs = torch.full((32 * n,), 0x77, dtype=torch.uint8,
                               device="cuda")
        self.new_first = torch.full((n + 1,), -7, dtype=torch.int64,
                                    device="cuda")
        self.new_index = torch.full((self.total + 4,), -7, dtype=torch.int64,
                                    device="cuda")

    def model(self, caps=None):
        index = self.flat[:self.entries]
        return A.expect(self.comps, index, self.first, self.old_lens,
                        self.appends, self.caps if caps is None else caps,
                        O.compress, A.decode_piece, A.header_error)

    def enqueue(self, ctx):
        from rust_snappy_amd import raw
        raw.append_indexed(
            ctx, self.src.d_ptrs, self.in_lens, self.old_lens, self.d_first,
            self.d_index, self.a_ptrs, self.a_lens, self.out.d_ptrs,
            self.out.d_caps, self.out_lens, self.errs, self.new_first,
            self.new_index, index_entries=self.entries,
            new_index_cap=self.total)

    def untouched(self, what):
        """Nothing the call may write has been written."""
        self.out.assert_guards(what)
        assert bool((self.out.data == GUARD).all()), what
        assert set(self.out_lens.cpu().tolist()) == {-7}, what
        assert bool((self.errs == 0x77).all()), what
        assert set(self.new_first.cpu().tolist()) == {-7}, what
        assert set(self.new_index.cpu().tolist()) == {-7}, what

    def results(self, what):
        for slab in (self.out, self.src, self.asrc):
            slab.assert_guards(what)
        for i, c in enumerate(self.comps):  # the streams are only read
            assert self.src.bytes(i, len(c)) == c, (what, i)
        for i, b in enumerate(self.appends):
            assert self.asrc.bytes(i, len(b)) == b, (what, i)
        lens = self.out_lens.cpu().tolist()
        errs = read_errs(self.errs)
        first = [x & (U64 - 1) for x in self.new_first.cpu().tolist()]
        index = [x & (U64 - 1) for x in self.new_index.cpu().tolist()]
        return lens, errs, first, index

    def check(self, ctx, what):
        lens, errs, first, index = self.results(what)
        want, want_first, want_index = self.model()
        for i, (wbytes, wentries, werr) in enumerate(want):
            key = (what, i)
            print(key, lens[i], errs[i], werr)
            assert errs[i] == werr, key
            n = 0 if wbytes is None else len(wbytes)
            assert lens[i] == n, key
            assert self.out.bytes(i, n) == (wbytes or b""), key
            # exactly [0, new length) is written - nothing for a stream that
            # failed or that nobody names
            rest = self.out.bytes(i, self.caps[i])[n:]
            assert rest == bytes([GUARD]) * len(rest), key
            assert index[want_first[i]:want_first[i + 1]] == wentries, key
        assert first == want_first, what
        assert index[:self.total] == want_index, what
        assert index[self.total:] == [FILL] * 4, what  # the sentinels
        # the counters
        blocks, decoded, ok, failed = A.counters(self.old_lens, self.appends,
                                                 want)
        assert ctx.info("append_blocks") == blocks, what
        assert ctx.info("append_blocks_decoded") == decoded, what
        assert ctx.info("append_streams_ok") == ok, what
        assert ctx.info("append_streams_failed") == failed, what
        return lens, errs, index, want


def run(ctx, case, appends, what, **kw):
    c = Call(case, appends, **kw)
    torch.cuda.synchronize()  # the buffers are filled
    c.enqueue(ctx)
    ctx.synchronize()
    return c, c.check(ctx, what)


def exact(c, res, streams, what):
    """The named streams `streams` are the oracle's stream and index of old
    data followed by appended data."""
    lens, errs, index, want = res
    nf = A.new_first(c.old_lens, c.a_lens)
    for s in streams:
        new = c.case.inputs[s] + c.appends[s]
        stream = O.compress(new)
        assert errs[s] == OK and lens[s] == len(stream), (what, s)
        assert c.out.bytes(s, lens[s]) == stream, (what, s)
        assert index[nf[s]:nf[s + 1]] == B.expected_index(new), (what, s)


# --------------------------------------------------------------- 1. exact
@pytest.mark.parametrize("a", A.APPENDS)
def test_exact_bytes_of_every_length(ctx, case, a):
    """One batch per append size over all old lengths (a == 0: nobody is
    named, and the call still writes lengths, errors and the new index)."""
    extra = A.text(a, 4321)
    c, res = run(ctx, case, [extra] * case.n, f"append {a}", seed=a % 7)
    if a:
        exact(c, res, range(case.n), f"append {a}")
    else:
        lens, errs, index, _ = res
        assert lens == [0] * case.n and errs == [OK] * case.n
        assert index[:c.total] == case.flat


# --------------------------------------------------------------- 2. varint
@pytest.fixture(scope="module")
def growth():
    return A.Case([127, 16383, 2097151])


def test_varint_grows_a_byte(ctx, growth):
    """Old lengths 127, 16 383 and 2 097 151 plus one byte: the varint takes
    a byte more and every entry shifts by one."""
    c, res = run(ctx, growth, [b"!"] * 3, "varint growth")
    exact(c, res, range(3), "varint growth")
    lens, errs, index, want = res
    nf = A.new_first(c.old_lens, c.a_lens)
    for s, old in enumerate(growth.old_lens):
        assert len(B.varint(old + 1)) == len(B.varint(old)) + 1
        kf = A.full(old)
        ne = index[nf[s]:nf[s + 1]]
        assert ne[:kf + 1] == [e + 1 for e in growth.index[s][:kf + 1]], s


# --------------------------------------------------------------- 3. aligned
def test_block_aligned_streams_decode_nothing(ctx):
    aligned = A.Case([0, 65536, 131072])
    c, res = run(ctx, aligned, [A.text(5, 9), A.text(70000, 11), b"z"],
                 "aligned")
    exact(c, res, range(3), "aligned")
    assert ctx.info("append_blocks_decoded") == 0
    assert ctx.info("append_blocks") == 1 + 2 + 1


# --------------------------------------------------------------- 4. not named
def test_streams_nobody_names(ctx, case):
    """Named and not named streams side by side: a stream nobody names keeps
    guard bytes, length 0, kind 0 and its old entries - or zeros, when
    d_index_first does not give it just its entries inside the index."""
    appends = [b""] * case.n
    appends[1] = A.text(300, 5)
    appends[5] = A.text(70000, 6)
    c, res = run(ctx, case, appends, "some named")
    exact(c, res, (1, 5), "some named")
    lens, errs, index, _ = res
    nf = A.new_first(c.old_lens, c.a_lens)
    for s in range(case.n):
        if s not in (1, 5):
            assert (lens[s], errs[s]) == (0, OK)
            assert c.out.bytes(s, c.caps[s]) == bytes([GUARD]) * c.caps[s]
            assert index[nf[s]:nf[s + 1]] == case.index[s]
    # stream 6 one entry short, stream 7 one too many: both get zeros
    first = list(case.first)
    first[7] -= 1
    c, res = run(ctx, case, appends, "hostile first", first=first, seed=2)
    exact(c, res, (1, 5), "hostile first")
    lens, errs, index, _ = res
    for s in (6, 7):
        assert (lens[s], errs[s]) == (0, OK)
        assert index[nf[s]:nf[s + 1]] == [0] * len(case.index[s])
    assert index[nf[4]:nf[5]] == case.index[4]
    # every stream's entries behind the index: zeros, and the named fail
    first = [f + len(case.flat) for f in case.first]
    c, res = run(ctx, case, appends, "first beyond the index", first=first,
                 seed=3)
    lens, errs, index, _ = res
    assert index[:c.total] == [0] * c.total
    assert [errs[s] for s in (1, 5)] == [(101, 1, 0, 0), (101, 5, 0, 0)]
    assert [errs[s] for s in (0, 4, 7)] == [OK] * 3 and lens == [0] * case.n


# --------------------------------------------------------------- 5. failures
S = 7   # the stream of 200 000 bytes: three full blocks and a tail
GOOD = {2: 500, 5: 66000}   # healthy streams beside it: what is appended


def foreign_tail():
    """A stream of one full block and a tail whose first element copies from
    across the block boundary: (stream, entries, announced length)."""
    import foreign
    block0, rest = A.text(65536, 31), A.text(3000, 77)
    body0 = foreign.lit(block0)
    body1 = foreign.copy(100, 64, 2) + foreign.lit(rest)
    hdr = foreign.varint(65536 + 64 + 3000)
    stream = hdr + body0 + body1
    assert len(O.decompress(stream)) == 68600
    return stream, [len(hdr), len(hdr) + len(body0), len(stream)], 68600


def failing(case):
    """name -> (keywords of Call, bytes appended to stream S, its error or
    None: the model's)."""
    idx, n_s = case.index[S], len(case.comps[S])

    def with_comp(c):
        comps = list(case.comps)
        comps[S] = c
        return comps

    def lens(v):
        out = list(case.old_lens)
        out[S] = v
        return out
    out = {}
    bad = b"\xff" * 11 + case.comps[S][11:]
    out["corrupt header"] = (dict(comps=with_comp(bad)), b"a",
                             A.header_error(bad))
    out["h_out_lens above"] = (dict(old_lens=lens(200001)), b"a",
                               (101, S, 200000, 200001))
    out["h_out_lens below"] = (dict(old_lens=lens(199999)), b"a",
                               (101, S, 200000, 199999))
    out["too big"] = (dict(comps=with_comp(B.varint(2**32 - 1)),
                           old_lens=lens(2**32 - 1)), b"a",
                      (A.TOO_BIG, 2**32, 2**32 - 1, 0))
    first = list(case.first)
    first[S + 1] -= 1
    out["wrong entry count"] = (dict(first=first), b"a", (101, S, 0, 0))
    flat, first = case.with_index(S, [idx[0] + 1] + idx[1:])
    out["wrong entry 0"] = (dict(flat=flat, first=first), b"a",
                            (101, S, 0, 0))
    flat, first = case.with_index(S, idx[:-1] + [n_s - 1])
    out["wrong last entry"] = (dict(flat=flat, first=first), b"a",
                               (101, S, 0, 0))
    flat, first = case.with_index(S, idx[:2] + [idx[1]] + idx[3:])
    out["not increasing at block 1"] = (dict(flat=flat, first=first), b"a",
                                        (101, S, 1, 0))
    out["entries outside index_entries"] = (
        dict(index_entries=len(case.flat) - 1), b"a", (101, S, 0, 0))
    c = bytearray(case.comps[S])
    c[idx[3]:idx[3] + 3] = b"\xfe\xff\xff"  # copy-2, 64 bytes, offset 65535
    out["corrupt byte in the tail"] = (dict(comps=with_comp(bytes(c))), b"a",
                                       None)
    stream, entries, dlen = foreign_tail()
    out["foreign tail"] = (
        dict(comps=with_comp(stream), old_lens=lens(dlen),
             flat=case.flat[:case.first[S]] + entries,
             first=case.first[:S + 1] + [case.first[S] + 3]), b"a", None)
    return out


FAILURES = ["corrupt header", "h_out_lens above", "h_out_lens below",
            "too big", "wrong entry count", "wrong entry 0",
            "wrong last entry", "not increasing at block 1",
            "entries outside index_entries", "corrupt byte in the tail",
            "foreign tail"]


@pytest.mark.parametrize("name", FAILURES)
def test_failures(ctx, case, name):
    """A failed stream: exact fields, length 0, not one byte of its buffer
    written, all its new entries 0 - and the healthy streams beside it are
    exact."""
    cases = failing(case)
    assert sorted(cases) == sorted(FAILURES)
    kw, add, err = cases[name]
    appends = [b""] * case.n
    for s, n in GOOD.items():
        appends[s] = A.text(n, 100 + s)
    appends[S] = add
    c, res = run(ctx, case, appends, name, **kw)
    lens, errs, index, want = res
    if err is None:  # the piece's error, from the oracle on varint || piece
        e = c.flat[c.first[S]:c.first[S + 1]]
        room = c.old_lens[S] % 65536
        _, err = A.decode_piece(
            B.varint(room) + c.comps[S][e[-2]:e[-1]], room)
        assert err[0] not in (0, 101)
    assert (lens[S], errs[S]) == (0, err), (name, errs[S])
    assert c.out.bytes(S, c.caps[S]) == bytes([GUARD]) * c.caps[S]
    nf = A.new_first(c.old_lens, c.a_lens)
    assert index[nf[S]:nf[S + 1]] == [0] * (nf[S + 1] - nf[S])
    exact(c, res, GOOD, name)


def test_cap_one_below_and_exact(ctx, case):
    appends = [b""] * case.n
    for s, n in GOOD.items():
        appends[s] = A.text(n, 100 + s)
    appends[S] = A.text(3000, 55)
    res, _, _ = A.expect(case.comps, case.flat, case.first, case.old_lens,
                         appends, [1 << 40] * case.n, O.compress,
                         A.decode_piece, A.header_error)
    need = [len(r[0]) if r[0] is not None else 64 for r in res]
    c, r = run(ctx, case, appends, "exact caps", caps=need)
    exact(c, r, list(GOOD) + [S], "exact caps")
    short = list(need)
    short[S] -= 1
    c, r = run(ctx, case, appends, "cap one below", caps=short, seed=4)
    lens, errs, index, _ = r
    assert (lens[S], errs[S]) == (0, (2, need[S] - 1, need[S], 0))
    assert c.out.bytes(S, short[S]) == bytes([GUARD]) * short[S]
    exact(c, r, GOOD, "cap one below")


# --------------------------------------------------------------- 6. groups
def test_groups_at_the_floor(ctx):
    """Six streams, 200 000 bytes appended to each, with "write_scratch_bytes"
    at its floor: a group per stream (each exceeds the floor alone), the same
    bytes as in one group."""
    six = A.Case(A.OLD_LENS[2:])
    appends = [A.text(200000, 10 + s) for s in range(6)]
    lens = [len(b) for b in appends]
    assert A.groups(six.old_lens, lens, 1 << 30) == [list(range(6))]
    assert A.groups(six.old_lens, lens, A.FLOOR) == [[s] for s in range(6)]
    c, plain = run(ctx, six, appends, "one group")
    exact(c, plain, range(6), "one group")
    ctx.set_option("write_scratch_bytes", A.FLOOR)
    try:
        c, grouped = run(ctx, six, appends, "a group per stream", seed=3)
    finally:
        ctx.set_option("write_scratch_bytes", 1 << 30)
    exact(c, grouped, range(6), "a group per stream")
    assert grouped[:3] == plain[:3]


# --------------------------------------------------------------- 6b. scale
class Streams:
    """Any inputs as a case: the oracle's streams and index of them."""

    def __init__(self, inputs):
        self.inputs = list(inputs)
        self.old_lens = [len(d) for d in self.inputs]
        self.comps = [O.compress(d) for d in self.inputs]
        self.index = [B.expected_index(d) for d in self.inputs]
        self.first = [0]
        for idx in self.index:
            self.first.append(self.first[-1] + len(idx))
        self.flat = [e for idx in self.index for e in idx]
        self.n = len(self.comps)


def test_long_stream_strides(ctx):
    """One stream of 70 full blocks and a tail of 100 bytes, 260 blocks and 5
    bytes appended: more old blocks than the 64 a stride of k_append_plan
    checks, old bytes for several splice jobs of 16 384, more new blocks than
    the 256 a stride of k_append_sizes sums - the first of them rebuilt from
    the tail's room."""
    pattern = bytes(range(256)) * 4
    old = (pattern * (71 * 64))[:70 * 65536 + 100]
    extra = (bytes(reversed(pattern)) * (261 * 64))[:260 * 65536 + 5]
    one = Streams([old])
    e = one.index[0]
    assert len(e) == 72 and e[70] - e[0] > 3 * 16384
    assert A.blocks(len(old), len(extra)) == 261
    assert A.block(len(old), len(extra), 0) == (True, 0, 65436, 65536)
    c, res = run(ctx, one, [extra], "331 blocks")
    exact(c, res, [0], "331 blocks")
    assert ctx.info("append_blocks") == 261
    assert ctx.info("append_blocks_decoded") == 1
    assert ctx.info("append_streams_ok") == 1


def test_more_named_streams_than_one_stride_of_the_job_scan(ctx):
    """1 100 streams of 20 to 120 bytes, 1 to 9 bytes appended to each, in one
    group, so k_append_jobs walks a second stride of its scan - whose first
    stream (the group's 1 025th) has a cap one byte short: it fails, is
    written nothing and has no splice job, and the streams behind it find
    their jobs past its empty place in the list."""
    rng = random.Random(1100)
    n = 1100
    many = Streams([A.text(rng.randrange(20, 121), 977 * i)
                    for i in range(n)])
    appends = [rng.randbytes(rng.randrange(1, 10)) for _ in range(n)]
    assert A.groups(many.old_lens, [len(b) for b in appends],
                    1 << 30) == [list(range(n))]
    res, _, _ = A.expect(many.comps, many.flat, many.first, many.old_lens,
                         appends, [1 << 40] * n, O.compress, A.decode_piece,
                         A.header_error)
    need = [len(r[0]) for r in res]
    caps = [v + SLACK for v in need]
    caps[1024] = need[1024] - 1
    c, r = run(ctx, many, appends, "1 100 streams", caps=caps)
    lens, errs, index, _ = r
    assert (lens[1024], errs[1024]) == (0, (2, need[1024] - 1, need[1024], 0))
    assert c.out.bytes(1024, caps[1024]) == bytes([GUARD]) * caps[1024]
    assert sum(1 for e in errs if e != OK) == 1
    exact(c, r, [s for s in range(n) if s != 1024], "1 100 streams")
    assert ctx.info("append_streams_ok") == n - 1
    assert ctx.info("append_streams_failed") == 1


# --------------------------------------------------------------- 7. refusals
def test_host_checks_enqueue_nothing(ctx, case):
    """A NULL source for a named stream, a wrapping sum, new_index_cap one
    short and a NULL required pointer are SNAPMI_E_ARGUMENT before anything
    is enqueued: every output keeps its fill."""
    from rust_snappy_amd import _lib
    appends = [b""] * case.n
    appends[2], appends[5] = b"abc", A.text(70000, 3)
    c = Call(case, appends, seed=5)
    torch.cuda.synchronize()
    L = _lib.of(ctx)
    n = case.n

    def call(old_lens=None, a_ptrs=None, a_lens=None, cap=None, null=None):
        arg = dict(
            in_ptrs=c.src.d_ptrs.data_ptr(), in_lens=c.in_lens.data_ptr(),
            old_lens=(C.c_uint64 * n)(*(old_lens or c.old_lens)),
            first=c.d_first.data_ptr(), index=c.d_index.data_ptr(),
            a_ptrs=(C.c_uint64 * n)(*(a_ptrs or c.a_ptrs)),
            a_lens=(C.c_uint64 * n)(*(a_lens or c.a_lens)),
            out_ptrs=c.out.d_ptrs.data_ptr(), out_caps=c.out.d_caps.data_ptr(),
            out_lens=c.out_lens.data_ptr(),
            new_first=c.new_first.data_ptr(),
            new_index=c.new_index.data_ptr())
        if null:
            arg[null] = None
        return L.snapmi_append_indexed(
            ctx._h, arg["in_ptrs"], arg["in_lens"], arg["old_lens"], n,
            arg["first"], arg["index"], len(c.flat), arg["a_ptrs"],
            arg["a_lens"], arg["out_ptrs"], arg["out_caps"], arg["out_lens"],
            c.errs.data_ptr(), arg["new_first"], arg["new_index"],
            c.total if cap is None else cap)

    no_src = list(c.a_ptrs)
    no_src[5] = 0
    wraps = list(c.old_lens)
    wraps[2] = U64 - 2
    many = list(c.a_lens)
    many[5] = 65536 * ((1 << 31) - 3)
    refused = {
        "NULL source of a named stream": dict(a_ptrs=no_src),
        "h_out_lens + h_app_len wraps": dict(old_lens=wraps),
        "new_index_cap one short": dict(cap=c.total - 1),
        "new entries at the limit": dict(a_lens=many, cap=U64 - 1),
    }
    for what, kw in refused.items():
        assert call(**kw) == 101, what
        ctx.synchronize()
        c.untouched(what)
    for name in ("in_ptrs", "in_lens", "old_lens", "first", "index",
                 "a_ptrs", "a_lens", "out_ptrs", "out_caps", "out_lens",
                 "new_first", "new_index"):
        assert call(null=name) == 101, name
        ctx.synchronize()
        c.untouched(name + " NULL")
    # ... and the context serves the call itself afterwards
    assert call() == 0
    ctx.synchronize()
    res = c.check(ctx, "after the refusals")
    exact(c, res, (2, 5), "after the refusals")


# --------------------------------------------------------------- 8. ordering
def test_two_appends_back_to_back(ctx, case):
    """Two calls enqueued back to back on one context, the second naming other
    streams of the same batch, one synchronize at the end: the second call's
    lists go through the staging the first one's copy may still be reading."""
    first = [A.text(1000 + 300 * s, s) if s % 2 == 0 else b""
             for s in range(case.n)]
    second = [A.text(66000 + s, 50 + s) if s % 2 else b""
              for s in range(case.n)]
    a, b = Call(case, first, seed=1), Call(case, second, seed=6)
    torch.cuda.synchronize()
    a.enqueue(ctx)
    b.enqueue(ctx)
    ctx.synchronize()  # the one wait
    ra = a.results("first of two")
    rb = b.check(ctx, "second of two")
    exact(b, rb, range(1, case.n, 2), "second of two")
    lens, errs, nfirst, index = ra
    want, want_first, want_index = a.model()
    assert nfirst == want_first and index[:a.total] == want_index
    assert index[a.total:] == [FILL] * 4
    for s in range(case.n):
        n = len(want[s][0]) if want[s][0] is not None else 0
        assert (lens[s], errs[s]) == (n, OK), s
        assert a.out.bytes(s, n) == (want[s][0] or b""), s
        rest = a.out.bytes(s, a.caps[s])[n:]
        assert rest == bytes([GUARD]) * len(rest), s
        if s % 2 == 0:
            assert a.out.bytes(s, n) == O.compress(case.inputs[s] + first[s])


# --------------------------------------------------------------- 9. round trip
def test_round_trip_through_the_indexed_readers(ctx, case):
    """batch.append, then the new streams with the new index through
    snapmi_decompress_batch_indexed and snapmi_decompress_ranges_indexed (a
    range across the seam between old and new bytes): old + extra."""
    from rust_snappy_amd import batch
    appends = [(s, A.text(100 + 33000 * s, 7 * s)) for s in range(case.n)
               if s != 3]
    src = batch.StreamBatch.from_bytes(case.comps, torch.device("cuda"))
    merged, new_idx, errs = batch.append(
        ctx, src, (u64(case.first), u64(case.flat)), appends)
    assert [tuple(e) for e in errs] == [OK] * case.n
    new = list(case.inputs)
    for s, b in appends:
        new[s] = new[s] + b
    flat = [x & (U64 - 1) for x in new_idx[1].cpu().tolist()]
    assert flat == [e for d in new for e in B.expected_index(d)]
    for s in range(case.n):
        assert merged.stream_bytes(s) == O.compress(new[s]), s
    dst, dlens, derrs = batch.decompress(ctx, merged, index=new_idx)
    for s in range(case.n):
        assert derrs[s] == OK and dst.stream_bytes(s, dlens[s]) == new[s], s
    ranges = []
    for s, b in appends:
        old = case.old_lens[s]
        lo = max(old - 70, 0)
        ranges.append((s, lo, min(len(new[s]) - lo, 70 + 66000)))
    ranges.append((3, 0, case.old_lens[3]))
    got, rerrs = batch.read_ranges(ctx, merged, new_idx, ranges)
    assert [tuple(e) for e in rerrs] == [OK] * len(ranges)
    assert got == [new[s][o:o + n] for s, o, n in ranges]
