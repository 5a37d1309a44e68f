"""Options lane_tail_probes / lane_tail_idle_pct against the plain round, in
ONE process on ONE context - the lane tables' placement, which the match
kernel follows by up to 15 %, is then the same for every sample: bench.py's
workload (the 12-stream round tiled to `gib`), compress calls alternating
between lane_tail_probes 0 and each candidate setting, `alternations` times
`calls` calls per side.  dominant_ms (the match kernel) and codec_ms of every
call from snapmi_last_timing, medians and spreads, and per candidate whether
EVERY sample lies below EVERY sample of option 0 taken beside it.
usage: python tests/hw/lane_tail_ab.py [out.json] [gib] [alternations] [calls]
       [depths, comma separated] [idle percentages, comma separated]
"""
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

DEPTHS = (2, 3, 4)
IDLE_PCTS = (25, 40, 50, 60, 75)


def round_batch(dev, gib):
    """bench.py's workload: (source batch, output batch, lengths tensor)."""
    import oracle_lib as O
    from rust_snappy_amd import batch, raw
    rnd = O.corpus_round()
    offs, pos = [], 0
    for _, d in rnd:
        offs.append(pos)
        pos += (len(d) + 15) // 16 * 16
    one = np.zeros(pos, dtype=np.uint8)
    for (_, d), o in zip(rnd, offs):
        one[o:o + len(d)] = np.frombuffer(d, dtype=np.uint8)
    r_lens = np.array([len(d) for _, d in rnd], dtype=np.int64)
    rounds = max(1, int(round(gib * 2**30 / int(r_lens.sum()))))
    data = torch.from_numpy(one).to(dev).repeat(rounds)
    o_all = (np.arange(rounds, dtype=np.int64)[:, None] * pos
             + np.array(offs, dtype=np.int64)[None, :]).reshape(-1)
    src = batch.StreamBatch(data, o_all, np.tile(r_lens, rounds))
    caps = np.array([raw.max_compress_len(int(x)) for x in r_lens],
                    dtype=np.int64)
    comp = batch.StreamBatch.empty(np.tile(caps, rounds), dev)
    clens = torch.zeros(12 * rounds, dtype=torch.int64, device=dev)
    return src, comp, clens


def compress(ctx, src, comp, clens):
    from rust_snappy_amd import raw
    raw.compress_batch(ctx, src.d_ptrs, src.d_lens, comp.d_ptrs, comp.d_lens,
                       clens, None, host_in_lens=src.h_lens)
    t = ctx.last_timing()
    return round(t["dominant_ms"], 3), round(t["codec_ms"], 3)


def _stats(v):
    return {"median": round(statistics.median(v), 3), "min": min(v),
            "max": max(v)}


def main():
    from rust_snappy_amd import raw
    out_path = sys.argv[1] if len(sys.argv) > 1 else None
    gib = float(sys.argv[2]) if len(sys.argv) > 2 else 8.0
    alternations = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    calls = int(sys.argv[4]) if len(sys.argv) > 4 else 5
    depths = [int(x) for x in sys.argv[5].split(",")] if len(sys.argv) > 5 \
        else DEPTHS
    pcts = [int(x) for x in sys.argv[6].split(",")] if len(sys.argv) > 6 \
        else IDLE_PCTS
    dev = torch.device("cuda", 0)
    ctx = raw.Context(0)
    src, comp, clens = round_batch(dev, gib)
    ctx.set_option("lane_tail_probes", 0)
    for _ in range(3):  # places the tables, allocates
        compress(ctx, src, comp, clens)
    want = clens.clone()
    res = {"gib": gib, "alternations": alternations, "calls": calls,
           "kernel": ctx.last_kernel(), "placement": ctx.table_probe_log(),
           "candidates": []}
    for depth in depths:
        for pct in pcts:
            off, on = [], []
            for _ in range(alternations):
                ctx.set_option("lane_tail_probes", 0)
                off += [compress(ctx, src, comp, clens) for _ in range(calls)]
                ctx.set_option("lane_tail_probes", depth)
                ctx.set_option("lane_tail_idle_pct", pct)
                on += [compress(ctx, src, comp, clens) for _ in range(calls)]
                assert torch.equal(clens, want)
            row = {"lane_tail_probes": depth, "lane_tail_idle_pct": pct}
            for k, name in ((0, "dominant_ms"), (1, "codec_ms")):
                a, b = [x[k] for x in off], [x[k] for x in on]
                row[name] = {"off": a, "on": b, "off_stats": _stats(a),
                             "on_stats": _stats(b),
                             "gain_ms": round(statistics.median(a) -
                                              statistics.median(b), 3),
                             "every_on_below_every_off": max(b) < min(a)}
            res["candidates"].append(row)
            d = row["dominant_ms"]
            print(f"probes {depth} idle {pct:2d} %: dominant off "
                  f"{d['off_stats']} on {d['on_stats']} gain {d['gain_ms']} "
                  f"ms clear {d['every_on_below_every_off']}", flush=True)
    wins = [r for r in res["candidates"]
            if r["dominant_ms"]["every_on_below_every_off"]
            and r["codec_ms"]["every_on_below_every_off"]]
    best = max(wins, key=lambda r: r["dominant_ms"]["gain_ms"], default=None)
    res["best"] = best and {k: best[k] for k in ("lane_tail_probes",
                                                 "lane_tail_idle_pct")}
    print("best:", res["best"])
    if out_path:
        Path(out_path).write_text(json.dumps(res, indent=1) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
