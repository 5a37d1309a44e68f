"""Building the block index of streams that came without one, on the CPU:
bi_build (csrc/snapmi_blockindex.hpp, compiled for the host) against the
sequential walker of indexbuild_ref.py and against the index the oracle's
streams must have (blockindex_ref.expected_index), on libsnappy's streams
where it loads, on every unaligned and corrupt shape of the GPU suite, and
the binding of the new call."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import blockindex_ref as B
import indexbuild_ref as IB
import oracle_lib as O
from conftest import ROOT


@pytest.fixture(scope="module")
def H(tmp_path_factory):
    so = tmp_path_factory.mktemp("indexbuild") / "indexbuild_host.so"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror",
                           "-shared", "-fPIC",
                           str(ROOT / "tests" / "indexbuild_host.cpp"),
                           "-o", str(so)])
    L = C.CDLL(str(so))
    L.t_build.restype = C.c_int
    L.t_build.argtypes = [C.c_char_p, C.c_uint64, C.c_uint64, C.c_void_p]
    L.t_status.restype = C.c_int
    L.t_status.argtypes = [C.c_int]
    return L


@pytest.fixture(scope="module")
def text():
    return (O.CORPUS / "alice29.txt").read_bytes() * 2


def host_build(H, stream, dlen):
    """bi_build between two poisoned entries, which it must leave alone."""
    n = B.entries(dlen)
    e = np.full(n + 2, 0x7777, dtype=np.uint64)
    st = H.t_build(bytes(stream), len(stream), dlen,
                   C.c_void_p(e.ctypes.data + 8))
    assert e[0] == 0x7777 and e[-1] == 0x7777
    return st, [int(v) for v in e[1:-1]]


def both(H, stream, dlen):
    got = host_build(H, stream, dlen)
    assert got == IB.build(stream, dlen), (len(stream), dlen)
    return got


def test_verdict_values(H):
    assert [H.t_status(k) for k in range(4)] == [
        IB.BUILT, IB.UNALIGNED, IB.CORRUPT, IB.MISSIZED] == [1, 2, 3, 4]


def test_oracle_streams_have_the_expected_index(H, text):
    for data in IB.inputs(text):
        st, e = both(H, O.compress(data), len(data))
        assert st == IB.BUILT, len(data)
        assert e == B.expected_index(data), len(data)
    assert [len(B.expected_index(d)) for d in IB.inputs(text)] == [
        1, 2, 2, 2, 2, 3, 3, 5, 4, 3]


def test_libsnappy_streams(H, text):
    if O.libsnappy() is None:
        pytest.skip("libsnappy does not load here")
    for data in IB.inputs(text):
        stream = O.libsnappy_compress(data)
        st, e = both(H, stream, len(data))
        assert st == IB.BUILT, len(data)
        # 64 KiB blocks that stand alone: the built index passes the rule and
        # every piece decodes to its block
        if len(data) > 65536:
            assert B.indexed(stream, len(data), e, 0, len(e), len(e))
        for k in range(len(e) - 1):
            in_off, in_len, out_off, out_len = B.piece(e, len(data), k)
            piece = B.varint(out_len) + stream[in_off:in_off + in_len]
            assert O.decompress(piece) == data[out_off:out_off + out_len]


def test_foreign_aligned(H):
    stream, want = IB.foreign_aligned()
    assert both(H, stream, 68600) == (IB.BUILT, want)


def test_streams_of_at_most_one_block(H):
    # not walked: the header decides
    assert both(H, b"\x00", 0) == (IB.BUILT, [1])
    assert both(H, b"\x00\x00", 0) == (IB.CORRUPT, [0])
    assert both(H, b"", 0) == (IB.CORRUPT, [0])
    junk = B.varint(1000) + b"\xff" * 7
    assert both(H, junk, 1000) == (IB.BUILT, [2, len(junk)])
    assert both(H, B.varint(65536), 65536) == (IB.BUILT, [3, 3])
    assert both(H, b"\xff" * 12, 1000) == (IB.CORRUPT, [0, 0])
    # the announced length is not the caller's
    assert both(H, junk, 1001) == (IB.MISSIZED, [0, 0])
    assert both(H, junk, 70000) == (IB.MISSIZED, [0, 0, 0])
    assert both(H, B.varint(2**32), 5) == (IB.CORRUPT, [0, 0])


def test_unaligned_shapes(H):
    for name, (stream, dlen) in IB.unaligned().items():
        assert O.decompress_len(stream) == dlen
        st, e = both(H, stream, dlen)
        assert (st, e) == (IB.UNALIGNED, [0] * B.entries(dlen)), name


def test_corrupt_shapes(H, text):
    base = O.compress(text[:200000])
    shapes = IB.corrupt(base)
    assert len(shapes) == 7
    for name, (stream, dlen) in shapes.items():
        assert dlen > 65536, name
        st, e = both(H, stream, dlen)
        assert (st, e) == (IB.CORRUPT, [0] * B.entries(dlen)), name
    # (the base itself is fine, and a wrong belief about it is MISSIZED)
    assert both(H, base, 200000)[0] == IB.BUILT
    assert both(H, base, 200001)[0] == IB.MISSIZED


def test_copy_offsets_are_not_looked_at(H):
    """The builder finds boundaries and is no validator: a copy that reaches
    in front of the output changes nothing."""
    import foreign
    import random
    rng = random.Random(3)
    body = (foreign.lit(rng.randbytes(65536)) + foreign.copy(60000, 64, 2)
            + foreign.copy(2**31, 64, 4) + foreign.lit(rng.randbytes(10)))
    stream = foreign.varint(65536 + 128 + 10) + body
    st, e = both(H, stream, 65536 + 138)
    assert st == IB.BUILT and e == [3, 3 + 3 + 65536, len(stream)]


def test_binding_exposes_the_call(built):
    from rust_snappy_amd import _lib, batch, raw
    L, P = _lib.load(), _lib.load_product()
    assert "snapmi_build_block_index" in {s[0] for s in _lib.SYMBOLS}
    assert hasattr(L, "snapmi_build_block_index")
    assert hasattr(P, "snapmi_build_block_index")
    assert callable(raw.build_block_index) and callable(batch.build_index)
    # refused before anything touches a device
    assert L.snapmi_build_block_index(None, None, None, None, None, 0, None,
                                      None, 0, None) == 101
