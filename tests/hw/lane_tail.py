"""The tail of the lane match finder's launch, measured: one compress call of
bench.py's workload through the experiment build SNAPMI_PROFILE=3
(`make -C rust-snappy_amd/csrc profile`: libsnapmi_profile3.so), whose lane
wavefronts record the device's 100 MHz clock at the launch's start and end,
when the ticket was first found empty and when every lane went out of work.
Prints idle lanes against time in 1 ms bins, the time the ticket ran out and
the time from "half the lanes idle" to the kernel's end.
usage: python tests/hw/lane_tail.py [gib] [option=value ...]"""
import ctypes as C
import os
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent.parent
os.environ["SNAPMI_LIB"] = str(ROOT / "rust-snappy_amd" /
                               "libsnapmi_profile3.so")
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT / "tests" / "hw"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from lane_tail_ab import compress, round_batch  # noqa: E402
from rust_snappy_amd import _lib, raw  # noqa: E402

gib = float(sys.argv[1]) if len(sys.argv) > 1 and "=" not in sys.argv[1] \
    else 8.0
opts = [a.split("=") for a in sys.argv[1:] if "=" in a]
dev = torch.device("cuda", 0)
ctx = raw.Context(0)
for k, v in opts:
    ctx.set_option(k, int(v))
src, comp, clens = round_batch(dev, gib)
for _ in range(3):
    ms = compress(ctx, src, comp, clens)
L = _lib.load()
L.snapmi_debug_lane_tail.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
L.snapmi_debug_lane_tail.restype = C.c_int64
cap = 3 + (1 << 20)
buf = np.zeros(cap, dtype=np.uint64)
lanes = L.snapmi_debug_lane_tail(ctx._h, buf.ctypes.data, cap)
assert lanes > 0, lanes
start, end, empty = (int(x) for x in buf[:3])
out = np.sort(buf[3:3 + lanes].astype(np.int64))
assert (out > 0).all(), "a lane left no record"
to_ms = lambda t: (t - start) / 1e5  # noqa: E731 - 100 MHz ticks
print(f"# {gib:g} GiB, {ctx.last_kernel()}, {lanes} lanes, options "
      f"{dict(opts) or 'default'}: dominant {ms[0]} ms, codec {ms[1]} ms")
print(f"kernel {to_ms(end):.2f} ms by the device clock; ticket first found "
      f"empty at {to_ms(empty):.2f} ms")
half = int(out[lanes // 2])
for pct in (1, 10, 25, 50, 75, 90, 99, 100):
    t = int(out[min(lanes - 1, max(0, lanes * pct // 100 - 1))])
    print(f"{pct:3d} % of the lanes idle at {to_ms(t):7.2f} ms "
          f"({to_ms(end) - to_ms(t):6.2f} ms before the end)")
print(f"half the lanes idle -> kernel end: {to_ms(end) - to_ms(half):.2f} ms")
print("ms  idle lanes at the end of the bin")
for b in range(int(to_ms(end)) + 1):
    n = int(np.searchsorted(out, start + (b + 1) * 100000, side="right"))
    if n:
        print(f"{b:3d} {n:6d} {'#' * (n * 60 // lanes)}")
ctx.close()
