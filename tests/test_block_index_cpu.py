"""The block index of raw streams on the CPU: the rule and the layout
(csrc/snapmi_blockindex.hpp, compiled for the host as test_host_batch_cpu.py
does with its header) against a few lines of Python, every way the rule can
break, the identity the expected index of the GPU tests rests on, and the
exports and bindings of the three calls."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import blockindex_ref as B
import oracle_lib as O
from conftest import ROOT

LENGTHS = [0, 1, 65535, 65536, 65537, 131072, 3 * 65536 + 5]


@pytest.fixture(scope="module")
def H(tmp_path_factory):
    so = tmp_path_factory.mktemp("blockindex") / "blockindex_host.so"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror",
                           "-shared", "-fPIC",
                           str(ROOT / "tests" / "blockindex_host.cpp"),
                           "-o", str(so)])
    L = C.CDLL(str(so))
    u64, p = C.c_uint64, C.c_void_p
    L.t_block.restype = u64
    L.t_entries.restype = u64
    L.t_entries.argtypes = [u64]
    L.t_header.restype = C.c_uint32
    L.t_header.argtypes = [C.c_char_p, u64, p]
    L.t_indexed.restype = C.c_int
    L.t_indexed.argtypes = [C.c_char_p, u64, u64, p, u64, u64, u64]
    L.t_piece.argtypes = [p, u64, u64, p]
    L.t_find.restype = C.c_uint32
    L.t_find.argtypes = [p, C.c_uint32, u64]
    return L


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def host_indexed(H, stream, cap, index, first, nxt, index_entries):
    idx = np.asarray(list(index) + [0], dtype=np.uint64)
    return bool(H.t_indexed(bytes(stream), len(stream), cap, ptr(idx), first,
                            nxt, index_entries))


def fake_stream(dlen, nbytes):
    """A varint for dlen and nbytes of anything: the rule reads the header
    and the lengths only."""
    return B.varint(dlen) + bytes(nbytes)


def honest_index(dlen, stream):
    """Strictly increasing entries of the right count for `stream`."""
    hdr = len(B.varint(dlen))
    blocks = B.entries(dlen) - 1
    step = (len(stream) - hdr) // blocks
    assert step >= 1
    return [hdr + k * step for k in range(blocks)] + [len(stream)]


def test_entry_count(H):
    assert H.t_block() == B.BLOCK == 65536
    for n in LENGTHS + [2**32 - 1, 2**32]:
        assert H.t_entries(n) == B.entries(n), n
    assert [B.entries(n) for n in LENGTHS] == [1, 2, 2, 2, 3, 3, 5]


def test_header(H):
    cases = [b"", b"\x00", b"\x7f", b"\x80", b"\x80\x01",
             B.varint(2**32 - 1), B.varint(2**32), b"\xff" * 12,
             b"\x80" * 9 + b"\x02", B.varint(3 * 65536 + 5) + b"abc"]
    for s in cases:
        v = C.c_uint64(0)
        h = H.t_header(s, len(s), C.byref(v))
        want = B.header(s)
        assert (h, v.value if h else 0) == want, s
    assert B.header(B.varint(2**32)) == (0, 0)
    assert B.header(B.varint(70000)) == (3, 70000)


def test_verdict_on_honest_indexes(H):
    for dlen in LENGTHS:
        stream = fake_stream(dlen, 1000)
        if dlen == 0:
            idx = [1]
        elif dlen <= 65536:
            idx = [len(B.varint(dlen)), len(stream)]
        else:
            idx = honest_index(dlen, stream)
        assert len(idx) == B.entries(dlen)
        got = host_indexed(H, stream, dlen, idx, 0, len(idx), len(idx))
        assert got == B.indexed(stream, dlen, idx, 0, len(idx), len(idx))
        # two blocks or more: indexed; anything shorter never is
        assert got == (dlen > 65536), dlen
        # ... and the same inside a larger index
        pad = [7, 7, 7]
        big = pad + idx + pad
        assert host_indexed(H, stream, dlen, big, 3, 3 + len(idx),
                            len(big)) == (dlen > 65536)


@pytest.mark.parametrize("dlen", [65537, 131072, 3 * 65536 + 5])
def test_every_way_the_rule_breaks(H, dlen):
    stream = fake_stream(dlen, 1000)
    good = honest_index(dlen, stream)
    n = len(good)

    def both(idx, first=0, nxt=None, total=None, cap=dlen, s=stream):
        nxt = len(idx) if nxt is None else nxt
        total = len(idx) if total is None else total
        a = host_indexed(H, s, cap, idx, first, nxt, total)
        assert a == B.indexed(s, cap, list(idx), first, nxt, total)
        return a

    assert both(good)
    # wrong entry 0
    assert not both([good[0] + 1] + good[1:])
    assert not both([good[0] - 1] + good[1:])
    assert not both([0] + good[1:])
    # a non-increasing pair: equal, and swapped
    for k in range(1, n - 1):
        assert not both(good[:k] + [good[k - 1]] + good[k + 1:])
    if n > 3:
        assert not both(good[:1] + [good[2], good[1]] + good[3:])
    # last entry != in_len
    assert not both(good[:-1] + [good[-1] - 1])
    assert not both(good[:-1] + [good[-1] + 1])
    # one entry too few, one too many
    assert not both(good[:-2] + good[-1:])
    assert not both(good[:-1] + [good[-1] - 1, good[-1]])
    # dlen > cap
    assert not both(good, cap=dlen - 1)
    assert both(good, cap=dlen + 1)
    # a range beyond index_entries, an empty one, a reversed one
    assert not both(good, total=n - 1)
    assert not both(good + [1, 2, 3], first=1, nxt=n + 3, total=n + 2)
    assert not both(good, first=0, nxt=0)
    assert not both(good, first=2, nxt=1)
    # no header, a header alone
    assert not both(good, s=b"\xff" * len(stream))
    assert not both([1, 2, 3], s=B.varint(dlen))
    # all entries equal, garbage
    assert not both([good[0]] * n)
    assert not both([2**64 - 1 - k for k in range(n)])


def test_piece_ranges(H):
    for dlen in [65537, 131072, 3 * 65536 + 5]:
        stream = fake_stream(dlen, 1000)
        e = honest_index(dlen, stream)
        arr = np.asarray(e, dtype=np.uint64)
        out_pos = 0
        for k in range(len(e) - 1):
            got = np.zeros(4, dtype=np.uint64)
            H.t_piece(ptr(arr), dlen, k, ptr(got))
            assert tuple(int(x) for x in got) == B.piece(e, dlen, k)
            in_off, in_len, out_off, out_len = (int(x) for x in got)
            # the pieces tile the input behind the header and the output
            assert in_off == e[k] and in_off + in_len == e[k + 1]
            assert out_off == out_pos and 0 < out_len <= 65536
            out_pos += out_len
        assert out_pos == dlen
    assert B.piece([3, 10, 20, 30], 131073, 2) == (20, 10, 131072, 1)


def test_entry_to_stream_search(H):
    lens = [0, 1, 65537, 0, 3 * 65536 + 5, 65536, 0]
    first = [0]
    for n in lens:
        first.append(first[-1] + B.entries(n))
    arr = np.asarray(first, dtype=np.uint64)
    for s in range(len(lens)):
        for e in range(first[s], first[s + 1]):
            assert H.t_find(ptr(arr), len(lens), e) == s
    # whatever first[] holds the answer is a stream of the batch
    for bad in ([9, 3, 7, 1, 0, 2**63, 5, 4], [0] * 8, [2**64 - 1] * 8):
        arr = np.asarray(bad, dtype=np.uint64)
        for e in (0, 1, 5, 2**40):
            assert H.t_find(ptr(arr), 7, e) < 7


@pytest.mark.parametrize("name", ["alice29.txt", "html_x_4",
                                  "fireworks.jpeg"])
def test_stream_is_header_plus_block_streams(name):
    """What the expected index rests on: a stream is the varint of its length
    and, back to back, the streams of its 64 KiB blocks without their own
    varints - so entry j is the varint's length plus the compressed bytes of
    the blocks in front of block j."""
    data = (O.CORPUS / name).read_bytes()
    assert len(data) > 65536
    stream = O.compress(data)
    blocks = B.block_streams(data)
    assert stream == B.varint(len(data)) + b"".join(blocks)
    e = B.expected_index(data)
    assert len(e) == B.entries(len(data))
    assert e[0] == len(B.varint(len(data))) and e[-1] == len(stream)
    assert all(a < b for a, b in zip(e, e[1:]))
    assert B.indexed(stream, len(data), e, 0, len(e), len(e))
    # every piece decodes on its own to its block of the input
    for k in range(len(e) - 1):
        in_off, in_len, out_off, out_len = B.piece(e, len(data), k)
        piece = B.varint(out_len) + stream[in_off:in_off + in_len]
        assert O.decompress(piece) == data[out_off:out_off + out_len]
    assert B.expected_index(b"") == [1]
    assert B.expected_index(b"a") == [1, len(O.compress(b"a"))]


def test_binding_exposes_the_three_calls(built):
    from rust_snappy_amd import _lib, batch, raw
    L = _lib.load()
    P = _lib.load_product()
    names = {s[0] for s in _lib.SYMBOLS}
    for name in ("snapmi_block_index_entries",
                 "snapmi_compress_batch_indexed",
                 "snapmi_decompress_batch_indexed"):
        assert name in names
        assert hasattr(L, name) and hasattr(P, name)
    # host code: no GPU needed
    for lens in ([], [0], LENGTHS, [2**32 - 1] * 3):
        assert raw.block_index_entries(lens) == sum(B.entries(n)
                                                    for n in lens)
    import inspect
    assert "want_index" in inspect.signature(batch.compress).parameters
    assert "index" in inspect.signature(batch.decompress).parameters
    for f in (raw.compress_batch, raw.decompress_batch):
        assert "index_first" in inspect.signature(f).parameters
