"""Batches of many streams tiled from a few distinct payloads, and the
comparison of EVERY stream of such a batch with what it must be, on the
tensors' own device.

A chip-filling batch has a hundred thousand streams; what each must compress
to is known from a few dozen oracle calls, one per payload.  TiledBatch puts
the payloads into device memory once and points the streams at them; OutSlab
is gpu_buffers.Slab's layout - buffers of exactly their capacity between bands
of guard bytes, at every alignment - made and checked without a host image;
assert_all compares all lengths, all error records and all bytes and names
the streams that differ.  Everything here also runs on CPU tensors
(tests/test_tiled_batch_cpu.py)."""
import numpy as np
import torch

from gpu_buffers import BAND, GUARD

ALIGN = 16
# bytes one gather of assert_all / assert_guards compares at a time (its
# indexes take some forty times that)
GATHER_BYTES = 16 << 20


def _tensor(x, device):
    """x (tensor, array or list of integers) as an int64 tensor there."""
    if isinstance(x, torch.Tensor):
        return x.to(device=device, dtype=torch.int64)
    return torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype=np.int64))
                            ).to(device)


class OutSlab:
    """Buffers of exactly caps[i] bytes in one slab, a band of BAND guard
    bytes in front of the first and behind every one, each start shifted by
    0..15 bytes: gpu_buffers.Slab's layout, computed with numpy and filled on
    the device."""

    def __init__(self, caps, device="cuda", seed=0):
        self.caps = np.asarray(caps, dtype=np.int64)
        n = len(self.caps)
        jitter = np.random.default_rng(seed).integers(0, 16, n)
        before = np.concatenate([[0], np.cumsum(self.caps + BAND)[:-1]]) \
            if n else np.zeros(0, dtype=np.int64)
        self.offs = (BAND + np.cumsum(jitter) + before).astype(np.int64)
        end = int(self.offs[-1] + self.caps[-1]) if n else 0
        self.size = end + 2 * BAND
        self.data = torch.full((self.size,), GUARD, dtype=torch.uint8,
                               device=device)
        self.d_offs = torch.from_numpy(self.offs).to(device)
        self.d_ptrs = self.d_offs + self.data.data_ptr()
        self.d_caps = torch.from_numpy(self.caps).to(device)

    def assert_guards(self, what=""):
        """Every byte of the slab outside the buffers is still a guard byte
        (what gpu_buffers.Slab.assert_guards asserts, without a host copy:
        the gaps are gathered on the device)."""
        dev = self.data.device
        ends = np.concatenate([[0], self.offs + self.caps])
        starts = np.concatenate([self.offs, [self.size]])
        g_at = torch.from_numpy(ends).to(dev)
        g_len = torch.from_numpy(starts - ends).to(dev)
        width = int((starts - ends).max())
        col = torch.arange(width, device=dev)
        rows = max(1, GATHER_BYTES // width)
        bad_total, first = 0, None
        for lo in range(0, len(ends), rows):
            at, ln = g_at[lo:lo + rows], g_len[lo:lo + rows]
            idx = (at[:, None] + col).clamp_(max=self.size - 1)
            bad = (self.data[idx] != GUARD) & (col < ln[:, None])
            count = int(bad.sum())
            if count and first is None:
                first = int(idx[bad].min())
            bad_total += count
        assert bad_total == 0, (what, bad_total, first)


class TiledBatch:
    """n streams, stream i being payloads[kind[i]]: the payloads lie in device
    memory once, 16-byte aligned, and d_in_ptrs / d_in_lens point the streams
    at them (inputs are read-only: many streams may share one payload)."""

    def __init__(self, payloads, kind, device="cuda"):
        self.payloads = [bytes(p) for p in payloads]
        self.kind = np.asarray(kind, dtype=np.int64)
        assert self.kind.size == 0 or (
            0 <= self.kind.min() and self.kind.max() < len(self.payloads))
        lens = np.array([len(p) for p in self.payloads], dtype=np.int64)
        room = (np.maximum(lens, 1) + ALIGN - 1) // ALIGN * ALIGN
        at = np.concatenate([[0], np.cumsum(room)[:-1]]).astype(np.int64)
        host = np.zeros(int(room.sum()), dtype=np.uint8)
        for o, p in zip(at, self.payloads):     # (over the payloads, not n)
            host[o:o + len(p)] = np.frombuffer(p, dtype=np.uint8)
        self.device = device
        self.data = torch.from_numpy(host).to(device)
        self.payload_offs, self.payload_lens = at, lens
        self._point()

    def _point(self):
        self.in_lens = self.payload_lens[self.kind]
        self.h_in_lens = torch.from_numpy(self.in_lens.copy())
        self.d_in_lens = self.h_in_lens.to(self.device)
        self.d_in_ptrs = (torch.from_numpy(self.payload_offs[self.kind]).to(self.device)
                          + self.data.data_ptr())

    @property
    def n(self):
        return int(self.kind.size)

    def reordered(self, kind):
        """The same payloads in the same memory, other streams."""
        other = object.__new__(TiledBatch)
        other.__dict__.update(self.__dict__)
        other.kind = np.asarray(kind, dtype=np.int64)
        other._point()
        return other

    def outputs(self, cap_of_kind, seed=0):
        """An OutSlab with a buffer of cap_of_kind[kind[i]] bytes for stream
        i."""
        caps = np.asarray(cap_of_kind, dtype=np.int64)[self.kind]
        return OutSlab(caps, self.device, seed)


def _error_kinds(errs, n, device):
    """The n error records (a uint8 tensor of 32 * n bytes as the batch calls
    fill it, or a list of (kind, a, b, c)) as (kind, a | b | c) tensors."""
    if errs is None:
        return None
    if isinstance(errs, torch.Tensor):
        rec = errs.to(device).contiguous().view(torch.int64).reshape(n, 4)
        kind = rec[:, 0] & 0xFFFFFFFF
        return kind, rec[:, 1] | rec[:, 2] | rec[:, 3]
    rec = _tensor(np.asarray(errs, dtype=np.uint64).view(np.int64)
                  .reshape(n, 4), device)
    return rec[:, 0], rec[:, 1] | rec[:, 2] | rec[:, 3]


class Expected:
    """What the streams of each kind must be, as one array: assert_all takes
    a list of bytes as well; a test that checks many calls against the same
    thousands of expectations makes this once."""

    def __init__(self, streams):
        self.lens = np.array([len(e) for e in streams], dtype=np.int64)
        self.at = np.concatenate([[0], np.cumsum(self.lens)[:-1]]
                                 ).astype(np.int64)
        self.flat = np.frombuffer(b"".join(bytes(e) for e in streams) + b"\0",
                                  dtype=np.uint8)
        self._on = {}

    @classmethod
    def in_slab(cls, data, offs, lens):
        """Expectations that already lie in a tensor - the inputs of a
        compress call, for its decode: lens[k] bytes at data[offs[k]]."""
        self = object.__new__(cls)
        self.lens = np.asarray(lens, dtype=np.int64)
        self.at, self.flat = np.asarray(offs, dtype=np.int64), None
        self._on = {str(data.device): (
            data, torch.from_numpy(self.at.copy()).to(data.device))}
        return self

    def on(self, device):
        """(all the bytes, where each kind's begin) on that device."""
        key = str(device)
        if key not in self._on:
            self._on = {key: (torch.from_numpy(self.flat.copy()).to(device),
                              torch.from_numpy(self.at).to(device))}
        return self._on[key]

    def drop(self):
        """Gives the device copy back (the host's stays)."""
        if self.flat is not None:
            self._on = {}


def assert_all(out_data, out_offs, out_lens, kind, expected, errs=None,
               what=""):
    """Every stream i of a batch call's result - out_lens[i] bytes at
    out_data[out_offs[i]], its error record errs[i] - is expected[kind[i]]
    with no error: all lengths, all records, all bytes, compared on
    out_data's device.  A decode is checked the same way: expected[k] is then
    the payload itself.  Bytes behind a stream's length are not looked at
    (the block kernels over-copy inside a buffer's capacity).  Returns the
    number of streams compared; on failure names how many differ and, for the
    first ten, the stream, its kind, its length and error kind, and the
    offset of its first wrong byte.

    The bytes are compared as one ragged gather, GATHER_BYTES at a time:
    byte j of stream i is out_data[out_offs[i] + j] on one side and byte j
    of its kind on the other, so there is a loop neither over the streams nor
    over the kinds and 30 000 distinct expectations cost what 30 do."""
    dev = out_data.device
    if not isinstance(expected, Expected):
        expected = Expected(expected)
    offs, lens = _tensor(out_offs, dev), _tensor(out_lens, dev)
    h_kind = kind.cpu().numpy() if isinstance(kind, torch.Tensor) \
        else np.asarray(kind, dtype=np.int64)
    kind = _tensor(h_kind, dev)
    n = kind.numel()
    assert offs.numel() == n and lens.numel() == n, (what, n)
    h_want = expected.lens[h_kind]
    want_len = torch.from_numpy(h_want).to(dev)
    bad = lens != want_len
    err = _error_kinds(errs, n, dev)
    if err is not None:
        bad |= (err[0] != 0) | (err[1] != 0)
    assert n == 0 or int((offs + want_len).max()) <= out_data.numel(), \
        (what, "a buffer is smaller than what is expected in it")
    flat, e_at = expected.on(dev)
    e_at = e_at[kind]
    none = 1 << 62
    first_diff = torch.full((n,), none, dtype=torch.int64, device=dev)
    cum = np.concatenate([[0], np.cumsum(h_want)])
    a = 0
    while a < n:
        # streams [a, b): as many as fit into one gather, one at the least
        b = max(int(np.searchsorted(cum, cum[a] + GATHER_BYTES, "right")) - 1,
                a + 1)
        total = int(cum[b] - cum[a])
        if total:
            begin = torch.from_numpy(cum[a:b] - cum[a]).to(dev)
            sid = torch.repeat_interleave(torch.arange(b - a, device=dev),
                                          want_len[a:b], output_size=total)
            pos = torch.arange(total, device=dev) - begin[sid]
            ne = out_data[offs[a:b][sid] + pos] != flat[e_at[a:b][sid] + pos]
            if bool(ne.any()):
                first_diff[a:b].scatter_reduce_(0, sid[ne], pos[ne], "amin")
        a = b
    first_diff[first_diff == none] = -1
    bad |= first_diff >= 0
    count = int(bad.sum())
    if count:
        lines = []
        for i in torch.nonzero(bad).flatten()[:10].tolist():
            lines.append(
                f"stream {i} kind {int(kind[i])}: length {int(lens[i])} "
                f"(expected {int(want_len[i])})"
                + (f", error kind {int(err[0][i])}" if err is not None else "")
                + (f", first wrong byte at {int(first_diff[i])}"
                   if int(first_diff[i]) >= 0 else ", bytes equal"))
        raise AssertionError(
            f"{what}: {count} of {n} streams differ\n" + "\n".join(lines))
    return n
