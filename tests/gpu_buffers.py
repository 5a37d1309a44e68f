"""Device buffers the GPU suites of the batch calls share: a slab of
exact-size buffers between guard bands, the error records and the index
tensors of a call, and the ways an index is made hostile."""
import random

import numpy as np
import torch

GUARD, BAND = 0xA5, 256
ERR_DT = np.dtype([("kind", "<i4"), ("r", "<u4"), ("a", "<u8"), ("b", "<u8"),
                   ("c", "<u8")])


class Slab:
    """Buffers of exactly caps[i] bytes in one slab with a band of 256 guard
    bytes in front of the first and behind every one; the buffers start at
    every alignment."""

    def __init__(self, caps, seed=0, fill=None):
        rng = random.Random(seed)
        self.caps = [int(c) for c in caps]
        offs, pos = [], BAND
        for c in self.caps:
            pos += rng.randrange(16)
            offs.append(pos)
            pos += c + BAND
        self.size = pos + BAND
        self.offs = np.array(offs, dtype=np.int64)
        self.data = torch.from_numpy(self.image(fill)).cuda()
        self.d_ptrs = torch.from_numpy(self.offs).cuda() + self.data.data_ptr()
        self.d_caps = torch.tensor(self.caps, dtype=torch.int64, device="cuda")

    def image(self, fill=None):
        host = np.full(self.size, GUARD, dtype=np.uint8)
        if fill is not None:
            for o, b in zip(self.offs, fill):
                host[o:o + len(b)] = np.frombuffer(bytes(b), dtype=np.uint8)
        return host

    def refill(self, fill=None):
        """The same device memory as a new slab would hold it (on torch's
        current stream)."""
        self.data.copy_(torch.from_numpy(self.image(fill)))

    def fetch(self):
        self.host = self.data.cpu().numpy()
        return self.host

    def bytes(self, i, n):
        o = int(self.offs[i])
        return self.host[o:o + int(n)].tobytes()

    def assert_guards(self, what):
        host = self.fetch()
        inside = np.zeros(self.size + 1, dtype=np.int32)
        np.add.at(inside, self.offs, 1)
        np.add.at(inside, self.offs + np.array(self.caps, dtype=np.int64), -1)
        inside = np.cumsum(inside[:-1]) > 0
        bad = np.flatnonzero(~inside & (host != GUARD))
        assert bad.size == 0, (what, bad.size, int(bad[0]))


def read_errs(t):
    rec = np.frombuffer(t.cpu().numpy().tobytes(), dtype=ERR_DT)
    return [(int(r["kind"]), int(r["a"]), int(r["b"]), int(r["c"]))
            for r in rec]


def u64(values):
    a = np.asarray([int(v) & (2**64 - 1) for v in values], dtype=np.uint64)
    return torch.from_numpy(a.view(np.int64).copy()).cuda()


def hostile(idx, in_len, how, rng, other):
    e = list(idx)
    n = len(e)
    if how == "plus1":
        e[rng.randrange(n)] += 1
    elif how == "minus1":
        e[rng.randrange(n)] -= 1
    elif how == "swapped" and n >= 2:
        a = rng.randrange(n - 1)
        e[a], e[a + 1] = e[a + 1], e[a]
    elif how == "equal":
        e = [e[0]] * n
    elif how == "beyond":
        e[rng.randrange(n)] = in_len + rng.choice([1, 1000, 2**33])
    elif how == "last_short":
        e[-1] -= rng.choice([1, 7])
    elif how == "random":
        e = [rng.getrandbits(64) for _ in range(n)]
    elif how == "other":
        e = list(other)
    elif how == "none":
        e = []
    elif how == "mid_element":
        # (strictly increasing, the right ends: the rule passes)
        e = [e[0]] + [x + 1 for x in e[1:-1]] + [e[-1]]
    return e
