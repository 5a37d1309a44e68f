"""tests/tiled_batch.py on CPU tensors: the whole-batch comparison the GPU
suites rely on reports what it must - a wrong byte, a wrong length, an error
record, each with its stream - and nothing else, and the guard check sees a
byte written into any gap."""
import re

import numpy as np
import pytest
import torch

import tiled_batch as TB
from gpu_buffers import BAND, ERR_DT, GUARD

PAYLOADS = [b"", b"a", bytes(range(200)), b"xyz" * 700, bytes(5000),
            bytes(range(256)) * 300]            # (the last: 76 800 bytes)
# what a "codec" makes of payload k: any bytes will do, of other lengths
EXPECTED = [b"\x00", b"\x01a", bytes(reversed(range(150))), b"q" * 33,
            b"", bytes(range(255, -1, -1)) * 40]
CAPS = [len(e) + 40 for e in EXPECTED]


def _image(n=1000, seed=5):
    """A correct result of n streams: (batch, slab, lens, errs)."""
    rng = np.random.default_rng(seed)
    kind = rng.integers(0, len(PAYLOADS), n)
    kind[-1] = 5
    tb = TB.TiledBatch(PAYLOADS, kind, device="cpu")
    slab = tb.outputs(CAPS, seed=seed)
    for i, k in enumerate(kind):
        o = int(slab.offs[i])
        # the over-copy of a block kernel: junk behind the stream's end
        slab.data[o:o + CAPS[k]] = 0x5A
        slab.data[o:o + len(EXPECTED[k])] = torch.from_numpy(
            np.frombuffer(EXPECTED[k], dtype=np.uint8).copy())
    lens = torch.tensor([len(EXPECTED[k]) for k in kind], dtype=torch.int64)
    errs = torch.zeros(32 * n, dtype=torch.uint8)
    return tb, slab, lens, errs


def _check(tb, slab, lens, errs):
    return TB.assert_all(slab.data, slab.d_offs, lens, tb.kind, EXPECTED,
                         errs=errs, what="self-test")


def _failure(tb, slab, lens, errs):
    with pytest.raises(AssertionError) as e:
        _check(tb, slab, lens, errs)
    return str(e.value)


def test_a_tiled_batch_points_every_stream_at_its_payload():
    tb, slab, _, _ = _image(300)
    assert tb.n == 300 and tb.d_in_lens.tolist() == [
        len(PAYLOADS[k]) for k in tb.kind]
    base = tb.data.data_ptr()
    host = tb.data.numpy()
    for i, k in enumerate(tb.kind):
        o = int(tb.d_in_ptrs[i]) - base
        assert o % 16 == 0
        assert host[o:o + len(PAYLOADS[k])].tobytes() == PAYLOADS[k]
    back = tb.reordered(tb.kind[::-1])
    assert back.data.data_ptr() == base
    assert back.d_in_ptrs.tolist() == tb.d_in_ptrs.tolist()[::-1]
    assert back.h_in_lens.tolist() == tb.h_in_lens.tolist()[::-1]
    # the output slab: exact capacities, a band between any two, the start
    # of the slab and its end; every alignment
    assert slab.caps.tolist() == [CAPS[k] for k in tb.kind]
    gap = slab.offs[1:] - (slab.offs[:-1] + slab.caps[:-1])
    assert gap.min() >= BAND and gap.max() < BAND + 16
    assert slab.offs[0] >= BAND
    assert slab.size - (slab.offs[-1] + slab.caps[-1]) >= BAND
    assert len(set((slab.offs % 16).tolist())) == 16
    assert (slab.d_ptrs - slab.data.data_ptr()).tolist() == slab.offs.tolist()


def test_a_correct_image_passes_and_every_stream_is_counted():
    tb, slab, lens, errs = _image()
    assert _check(tb, slab, lens, errs) == tb.n == 1000
    slab.assert_guards("correct")
    # the records as a list of tuples and the tensors as arrays do as well
    assert TB.assert_all(slab.data, slab.offs, lens.numpy(), tb.kind,
                         EXPECTED, errs=[(0, 0, 0, 0)] * tb.n) == tb.n


def test_one_wrong_byte_in_the_last_stream_is_reported():
    tb, slab, lens, errs = _image()
    last = tb.n - 1
    at = len(EXPECTED[5]) - 1                   # its last byte
    slab.data[int(slab.offs[last]) + at] ^= 1
    msg = _failure(tb, slab, lens, errs)
    assert "1 of 1000 streams differ" in msg
    assert re.search(rf"stream {last} kind 5: .*first wrong byte at {at}\b",
                     msg), msg


def test_a_wrong_byte_behind_the_length_is_not_reported():
    tb, slab, lens, errs = _image()
    for i in (0, 17, tb.n - 1):
        k = tb.kind[i]
        assert CAPS[k] > len(EXPECTED[k])
        slab.data[int(slab.offs[i]) + len(EXPECTED[k])] ^= 0xFF
        slab.data[int(slab.offs[i]) + CAPS[k] - 1] ^= 0xFF
    assert _check(tb, slab, lens, errs) == tb.n
    slab.assert_guards("inside the capacities")


def test_a_length_off_by_one_is_reported():
    tb, slab, lens, errs = _image()
    for i, d in ((0, 1), (613, -1)):
        if lens[i] + d < 0:
            d = 1
        lens[i] += d
    msg = _failure(tb, slab, lens, errs)
    assert "2 of 1000 streams differ" in msg
    for i in (0, 613):
        k = int(tb.kind[i])
        assert re.search(rf"stream {i} kind {k}: length {int(lens[i])} "
                         rf"\(expected {len(EXPECTED[k])}\)", msg), msg


def test_an_error_record_is_reported():
    tb, slab, lens, errs = _image()
    rec = np.zeros(tb.n, dtype=ERR_DT)
    rec[998]["kind"] = 2                        # BufferTooSmall
    rec[4]["b"] = 7                             # a field without a kind
    errs = torch.from_numpy(np.frombuffer(rec.tobytes(), dtype=np.uint8)
                            .copy())
    msg = _failure(tb, slab, lens, errs)
    assert "2 of 1000 streams differ" in msg
    assert re.search(r"stream 998 kind \d: .*error kind 2", msg), msg
    assert re.search(r"stream 4 kind \d: .*error kind 0, bytes equal", msg)


def test_the_first_ten_of_many_are_named():
    tb, slab, lens, errs = _image()
    rows = [i for i in range(tb.n) if len(EXPECTED[tb.kind[i]]) > 3][5::7]
    assert len(rows) > 20
    for i in rows:
        slab.data[int(slab.offs[i]) + 2] ^= 0x80
    msg = _failure(tb, slab, lens, errs)
    assert f"{len(rows)} of 1000 streams differ" in msg
    named = [int(m) for m in re.findall(r"^stream (\d+) ", msg, re.M)]
    assert named == rows[:10]
    assert msg.count("first wrong byte at 2") == 10


def test_a_decode_is_checked_against_the_payloads():
    tb, _, _, _ = _image(400)
    slab = tb.outputs([len(p) for p in PAYLOADS], seed=9)
    for i, k in enumerate(tb.kind):
        o = int(slab.offs[i])
        slab.data[o:o + len(PAYLOADS[k])] = torch.from_numpy(
            np.frombuffer(PAYLOADS[k], dtype=np.uint8).copy())
    errs = torch.zeros(32 * tb.n, dtype=torch.uint8)
    assert TB.assert_all(slab.data, slab.d_offs, tb.d_in_lens, tb.kind,
                         PAYLOADS, errs=errs) == 400
    slab.assert_guards("exact capacities")
    # ... or against the inputs where they lie, without a second copy
    inputs = TB.Expected.in_slab(tb.data, tb.payload_offs, tb.payload_lens)
    assert TB.assert_all(slab.data, slab.d_offs, tb.d_in_lens, tb.kind,
                         inputs, errs=errs) == 400
    i = int(np.flatnonzero(tb.kind == 5)[0])
    slab.data[int(slab.offs[i]) + 70000] = 0xEE     # was 70000 % 256 = 0x70
    for expected in (PAYLOADS, inputs, TB.Expected(PAYLOADS)):
        with pytest.raises(AssertionError) as e:
            TB.assert_all(slab.data, slab.d_offs, tb.d_in_lens, tb.kind,
                          expected, errs=errs)
        assert f"stream {i} kind 5" in str(e.value)
        assert "first wrong byte at 70000" in str(e.value)


@pytest.mark.parametrize("where", ["front", "behind_0", "before_last",
                                   "behind_last", "end"])
def test_a_byte_in_any_gap_fails_the_guard_check(where):
    tb, slab, _, _ = _image(200)
    at = {"front": 0,
          "behind_0": int(slab.offs[0] + slab.caps[0]),
          "before_last": int(slab.offs[-1]) - 1,
          "behind_last": int(slab.offs[-1] + slab.caps[-1]),
          "end": slab.size - 1}[where]
    assert int(slab.data[at]) == GUARD
    slab.data[at] = 0
    with pytest.raises(AssertionError) as e:
        slab.assert_guards(where)
    assert e.value.args[0] == (where, 1, at)


def test_gathers_of_a_few_streams_at_a_time_see_the_same(monkeypatch):
    """The comparison and the guard check work through the batch in pieces
    of GATHER_BYTES: with pieces smaller than one stream, as with one piece."""
    monkeypatch.setattr(TB, "GATHER_BYTES", 1000)
    tb, slab, lens, errs = _image()
    assert _check(tb, slab, lens, errs) == tb.n
    slab.assert_guards("in pieces")
    last = tb.n - 1
    slab.data[int(slab.offs[last]) + len(EXPECTED[5]) - 1] ^= 1
    slab.data[int(slab.offs[500]) - 1] = 0
    msg = _failure(tb, slab, lens, errs)
    assert "1 of 1000 streams differ" in msg and f"stream {last} kind 5" in msg
    with pytest.raises(AssertionError) as e:
        slab.assert_guards("in pieces")
    assert e.value.args[0] == ("in pieces", 1, int(slab.offs[500]) - 1)
