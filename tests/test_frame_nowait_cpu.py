"""The no-wait framed decode (SNAPMI_FRAME_NO_WAIT of
snapmi_frame_decompress_ex) without a GPU: the flag and the info name where
the sources must carry them, and the rules of csrc/snapmi_framewalk.hpp -
the side-index check, which front decides, when the caller's bound is
exceeded, what pads the chunk table - built for the host
(tests/framenowait_host.cpp) and compared with a restatement in Python."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

import oracle_lib as O
from conftest import ROOT
from test_frame_host_batch_cpu import chunk, error_streams

IDENT = b"\xff\x06\x00\x00sNaPpY"
E_ARGUMENT = 101
INDEX, PARALLEL, WALK, EXCEEDED = 1, 2, 3, 4


def test_flag_is_one_bit_of_its_own():
    header = (ROOT / "include" / "snapmi.h").read_text()
    flags = {}
    for name in ("NO_WAIT", "CONTINUATION", "FINAL"):
        m = re.search(rf"^#define SNAPMI_FRAME_{name} (\d+)u\b", header, re.M)
        assert m, name
        flags[name] = int(m.group(1))
    nw = flags["NO_WAIT"]
    assert nw == 4 and nw & (nw - 1) == 0
    assert nw & (flags["CONTINUATION"] | flags["FINAL"]) == 0


def test_names_in_the_sources():
    from test_options_cpu import options_table
    header = (ROOT / "include" / "snapmi.h").read_text()
    assert '"frame_nowait_front"' in header
    assert options_table().has_info("frame_nowait_front")
    shim = (ROOT / "shim" / "src" / "gpu.rs").read_text()
    assert re.search(r"pub const SNAPMI_FRAME_NO_WAIT: u32 = 4;", shim)
    frame = (ROOT / "rust-snappy_amd" / "csrc" / "snapmi_framedec.hip"
             ).read_text()
    assert "k_frame_nowait_seal" in frame
    from rust_snappy_amd import frame as F
    assert F.NO_WAIT == 4 and callable(F.decompress_nowait)


def test_flagged_path_has_no_wait_in_it():
    """The branch of snapmi_frame_decompress_ex the flag takes: no
    hipStreamSynchronize, no mailbox and no retry loop between its first line
    and its return - nor in frame_front, the launcher of the fronts that the
    branch shares with the retry loop."""
    frame = (ROOT / "rust-snappy_amd" / "csrc" / "snapmi_framedec.hip"
             ).read_text()
    body = frame[frame.index("int snapmi_frame_decompress_ex("):]
    lo = body.index("    if (nowait) {")
    branch = body[lo:body.index("    for (int attempt", lo)]
    assert "return fbd_finish(ctx, b);" in branch
    assert "frame_front(ctx, a, " in branch
    at = frame.index("static int frame_front(")
    front = frame[at:frame.index("\n}\n", at)]
    for name in ("k_frame_index", "k_fw_candidates", "k_frame_walk"):
        assert name in front, name
    for text in (branch, front):
        for word in ("hipStreamSynchronize", "h_mail", "k_post_words",
                     "post_words", "for (", "while (", "continue;"):
            assert word not in text, word
    assert "!nowait && (rc = mailbox(ctx))" in body[:lo]


# ------------------------------------------------------------ the host build
@pytest.fixture(scope="module")
def W(tmp_path_factory):
    so = tmp_path_factory.mktemp("framenowait") / "framenowait_host.so"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-shared",
                           "-fPIC", "-I", str(ROOT / "include"),
                           str(ROOT / "tests" / "framenowait_host.cpp"),
                           "-o", str(so)])
    L = C.CDLL(str(so))
    L.t_flag_nowait.restype = C.c_uint32
    L.t_index_front.restype = C.c_int
    L.t_index_front.argtypes = [C.c_char_p, C.c_uint64, C.c_uint32,
                                C.c_void_p, C.c_uint32, C.c_void_p]
    L.t_nowait.restype = None
    L.t_nowait.argtypes = [C.c_char_p, C.c_uint64, C.c_uint32, C.c_char_p,
                           C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32,
                           C.c_void_p]
    return L


# ------------------------------------------------- the restatement in Python
def py_walk(s, continuation=False):
    """(data chunk header offsets in front of the first header the reader
    rejects, whether there is one).  The stale-buffer rule: a compressed
    payload of fewer than 10 bytes, all >= 0x80, is always an error."""
    r, seen, offs = 0, continuation, []
    while r != len(s):
        if len(s) - r < 4:
            return offs, True
        ty, n = s[r], int.from_bytes(s[r + 1:r + 4], "little")
        if not seen and ty != 0xFF:
            return offs, True
        seen = True
        if n > 76490 or 2 <= ty <= 0x7F:
            return offs, True
        if ty == 0xFF and (n != 6 or s[r + 4:r + 10] != b"sNaPpY"):
            return offs, True
        if ty <= 1:
            if n < 4 or len(s) - r - 4 < 4 or (ty == 1 and n - 4 > 65536):
                return offs, True
        if len(s) - r - 4 < n:
            return offs, True
        if ty == 0 and n - 4 < 10 and all(b >= 0x80
                                          for b in s[r + 8:r + 4 + n]):
            return offs, True
        if ty <= 1:
            offs.append(r)
        r += 4 + n
    return offs, False


def py_index_ok(s, index, n, continuation=False):
    """The index tiles [identifier, len) with plain data chunks."""
    start = 0 if continuation else 10
    if not continuation and s[:10] != IDENT:
        return False
    if n == 0:
        return len(s) == start
    e = [int(x) for x in index[:n + 1]]
    if e[0] != start or e[n] != len(s):
        return False
    for i in range(n):
        r = e[i]
        if r < 0 or r + 8 > len(s):
            return False
        ty, ln = s[r], int.from_bytes(s[r + 1:r + 4], "little")
        if ty > 1 or ln < 4 or ln > 76490 or r + 4 + ln > len(s):
            return False
        if ty == 1 and ln - 4 > 65536:
            return False
        if e[i + 1] != r + 4 + ln:
            return False
        if ty == 0 and ln - 4 < 10 and all(b >= 0x80
                                           for b in s[r + 8:r + 4 + ln]):
            return False
    return True


def py_nowait(s, index, n, parallel=0, parallel_found=0, continuation=False):
    """(front, found, exceeded) of one no-wait decode."""
    first, found, decided = WALK, 0, False
    if index is not None:
        first, found = INDEX, n
        decided = py_index_ok(s, index, n, continuation)
    elif parallel:
        first = PARALLEL
        decided, found = parallel == 2, parallel_found if parallel == 2 else 0
    front = first
    if not decided:
        front, found = WALK, len(py_walk(s, continuation)[0])
    exceeded = found > n
    return (EXCEEDED if exceeded else front), found, exceeded


def run(W, s, index, n, parallel=0, parallel_found=0, continuation=False):
    out = np.zeros(10, dtype=np.uint64)
    idx = None
    if index is not None:
        idx = np.asarray([int(v) & (2**64 - 1) for v in index],
                         dtype=np.uint64)
        assert idx.size == n + 1
    W.t_nowait(bytes(s), len(s), (1 if continuation else 0) | 4, bytes(10),
               idx.ctypes.data_as(C.c_void_p) if idx is not None else None,
               n, parallel, parallel_found, out.ctypes.data_as(C.c_void_p))
    front, exceeded, chunks, pad_lo, found, good, nothing, kind, a, b = (
        int(x) for x in out)
    want = py_nowait(s, index, n, parallel, parallel_found, continuation)
    assert (front, found, bool(exceeded)) == want, (want, out)
    # the table: the stream's chunks, then records that decode to nothing
    assert chunks == pad_lo == (0 if exceeded else found)
    assert good == chunks and good + nothing == n, out
    if exceeded:
        assert (kind, a, b) == (E_ARGUMENT, found, n)
    return front, found


def streams():
    text = (O.CORPUS / "alice29.txt").read_bytes()
    f = O.frame_compress((text * 2)[:200000])            # 4 chunks
    one = O.frame_compress(text[:1000])
    offs = [o for o in py_walk(f)[0]]
    first = offs[1] - offs[0]
    foreign = (f[:10] + bytes([0x80, 3, 0, 0, 1, 2, 3]) + f[10:10 + first]
               + bytes([0xFE, 2, 0, 0, 9, 9]) + f[:10] + f[10 + first:])
    return {"four": f, "one": one, "foreign": foreign, "empty": b"",
            "ident": IDENT}


def test_flag_value_in_the_host_build(W):
    assert W.t_flag_nowait() == 4


def test_index_front_decides_only_what_tiles(W):
    S = streams()
    f = S["four"]
    offs, bad = py_walk(f)
    assert not bad and len(offs) == 4
    exact = offs + [len(f)]
    n = 4
    assert run(W, f, exact, n) == (INDEX, 4)
    assert run(W, f, None, n) == (WALK, 4)
    for more in (1, 5, 1000):
        assert run(W, f, None, n + more) == (WALK, 4)
        # an index padded to a generous bound no longer tiles: the walk
        assert run(W, f, exact + [len(f)] * more, n + more) == (WALK, 4)
    hostile = {
        "beyond": [exact[0], len(f) + 1000] + exact[2:],
        "huge": [exact[0], 2**64 - 8] + exact[2:],
        "equal": [exact[0]] * 5,
        "descending": exact[::-1],
        "last_short": exact[:-1] + [exact[-1] - 1],
        "payload": [exact[0]] + [e + 1 for e in exact[1:-1]] + [exact[-1]],
    }
    for name, idx in hostile.items():
        assert run(W, f, idx, n) == (WALK, 4), name
        good = np.zeros(n, dtype=np.uint8)
        arr = np.asarray([v & (2**64 - 1) for v in idx], dtype=np.uint64)
        assert W.t_index_front(f, len(f), 0, arr.ctypes.data_as(C.c_void_p),
                               n, good.ctypes.data_as(C.c_void_p)) == 0, name
    # the data chunks of a stream with foreign chunks in between
    g = S["foreign"]
    goffs, bad = py_walk(g)
    assert not bad and len(goffs) == 4
    assert run(W, g, goffs + [len(g)], 4) == (WALK, 4)
    assert run(W, g, None, 9) == (WALK, 4)
    # no chunks at all
    assert run(W, b"", [0], 0, continuation=True) == (INDEX, 0)
    assert run(W, b"", [0], 0) == (WALK, 0)       # (no identifier: the walk)
    assert run(W, IDENT, [10], 0) == (INDEX, 0)
    assert run(W, IDENT, None, 0) == (WALK, 0)
    assert run(W, b"", None, 0) == (WALK, 0)


def test_broken_promise(W):
    S = streams()
    f, one = S["four"], S["one"]
    offs = py_walk(f)[0] + [len(f)]
    assert run(W, f, None, 3) == (EXCEEDED, 4)
    assert run(W, f, offs[:4], 3) == (EXCEEDED, 4)
    assert run(W, one, None, 0) == (EXCEEDED, 1)
    assert run(W, one, [10], 0) == (EXCEEDED, 1)
    # the parallel walk counts before it emits: its verdict is the same
    assert run(W, f, None, 3, parallel=2, parallel_found=4) == (EXCEEDED, 4)
    assert run(W, f, None, 4, parallel=2, parallel_found=4) == (PARALLEL, 4)
    assert run(W, f, None, 9, parallel=2, parallel_found=4) == (PARALLEL, 4)
    assert run(W, f, None, 4, parallel=1) == (WALK, 4)
    assert run(W, f, None, 3, parallel=1) == (EXCEEDED, 4)


def test_error_streams_count_the_chunks_in_front(W):
    """Every malformed stream of the host-batch suite: the walk decides, the
    count is that of the chunks in front of the first rejected header, and a
    bound below it is a broken promise whatever else is wrong."""
    for k, s in enumerate(error_streams()):
        offs, bad = py_walk(s)
        n = len(offs)
        assert run(W, s, None, n + 5) == (WALK, n), k
        idx = offs + [len(s)]
        front, found = run(W, s, idx, n)
        assert found == n and front in (INDEX, WALK), k
        if bad:
            assert front == WALK, k
        if n:
            assert run(W, s, None, n - 1) == (EXCEEDED, n), k


def test_continuation_and_short_varint(W):
    S = streams()
    f = S["four"]
    body = f[10:]
    offs = [o - 10 for o in py_walk(f)[0]] + [len(body)]
    assert run(W, body, offs, 4, continuation=True) == (INDEX, 4)
    assert run(W, body, offs, 4) == (WALK, 0)      # StreamHeader, no chunks
    crc = b"\x11\x22\x33\x44"
    s = f + chunk(0, b"\x80" * 6, crc)
    good = py_walk(f)[0]
    assert py_walk(s) == (good, True)
    # listed in the index or not, the short chunk is the walk's to judge
    assert run(W, s, good + [len(f), len(s)], 5) == (WALK, 4)
    assert run(W, s, None, 4) == (WALK, 4)
