"""Experiment: per-phase cycle split of k_compress_blocks (profile build)."""
import ctypes as C, os, sys
_R = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ["SNAPMI_LIB"] = os.path.join(_R, "rust-snappy_amd", "libsnapmi_profile.so")
sys.path.insert(0, _R); sys.path.insert(0, os.path.join(_R, 'tests'))
import numpy as np, torch
import oracle_lib as O
import rust_snappy_amd as R
from rust_snappy_amd import batch, _lib
ctx = R.raw.Context(0)
rnd = [d for _, d in O.corpus_round()]
rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 300
sets = {"all": rnd * rounds}
for name, idx in (("html", 0), ("urls", 1), ("txt4", 9), ("jpg", 2), ("pdf", 4)):
    sets[name] = [rnd[idx]] * (rounds * 4)
L = _lib.load()
L.snapmi_debug_profile.argtypes = [C.c_void_p, C.c_void_p]
names = ["top->build", "x load", "hash+lds atomic", "gather", "cmp+ballot+rollback", "literal", "extend", "copy emit", "tail", "-"]
for k, streams in sets.items():
    src = batch.StreamBatch.from_bytes(streams)
    for _ in range(2):
        dst, lens, errs = batch.compress(ctx, src)
    t = ctx.last_timing()
    out = (C.c_uint64 * 16)()
    L.snapmi_debug_profile(ctx._h, out)
    v = list(out)
    tot = sum(v[:9]); nb, nc, nblk = v[10], v[11], v[12]
    ub = sum(len(s) for s in streams)
    print(f"== {k}: {ub/2**30:.2f} GiB, codec {t['codec_ms']:.1f} ms -> {ub/2**30/(t['codec_ms']/1e3):.2f} GiB/s; blocks {nblk}, batches/blk {nb/nblk:.0f}, copies/blk {nc/nblk:.0f}, cycles/blk {tot/nblk/1e6:.2f}M, cycles/batch {tot/nb:.0f}")
    print("   " + "  ".join(f"{names[i]}={v[i]/nb:.0f}" for i in range(9)))
