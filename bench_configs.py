#!/usr/bin/env python3
"""Secondary benchmarks: BASELINE.json configs 3 and 5 (bench.py is the
headline config 2), the per-file rates of the reference's bench list and the
PCIe-inclusive rate of the host-buffer entry points.  One JSON line per
config on stdout; --only picks one.

  cfg3  FrameEncoder/FrameDecoder (framing + CRC32C kernel) on seeded
        synthetic English-like text, device resident.  Text: tokens of the
        four corpus text files drawn i.i.d. from their unigram distribution
        (torch.multinomial, seed 0x5EED5A4D), single spaces, a newline where a
        token crosses a 73-byte boundary; a period of --period-mib is generated
        on the device and tiled to --gib.
  cfg5  incompressible path: fireworks.jpeg as independent raw streams tiled
        to --gib (literal fast path; the one workload near the HBM roofline).
"""
import argparse
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

GIB = float(1 << 30)


SYNTH_SEED = 0x5EED5A4D53505931
_GAMMA = 0x9E3779B97F4A7C15
_M1, _M2 = 0xBF58476D1CE4E5B9, 0x94D049BB133111EB


def _s64(x):
    """a 64-bit pattern as the int64 torch computes with (wrapping)"""
    x &= (1 << 64) - 1
    return x - (1 << 64) if x >> 63 else x


def _vocabulary():
    """Whitespace-delimited tokens of the four text files of the corpus, in
    byte order, with their counts (the empirical unigram distribution)."""
    import oracle_lib as O
    words = []
    for name in ("alice29.txt", "asyoulik.txt", "lcet10.txt", "plrabn12.txt"):
        words += (O.CORPUS / name).read_bytes().split()
    vocab, counts = np.unique(np.array(words, dtype=object),
                              return_counts=True)
    return [bytes(w) for w in vocab], counts.astype(np.int64)


def synth_text_reference(period_bytes, seed=SYNTH_SEED):
    """The generator of SURVEY 8d, one token at a time on the CPU (small
    periods only: it pins synth_text below).  Token i is drawn with the i-th
    output of splitmix64(seed): r = (z >> 1) mod total count, looked up in
    the cumulative counts of the vocabulary; tokens are joined by single
    spaces; the separator behind the first token that passes column 72 is a
    newline."""
    vocab, counts = _vocabulary()
    cum = np.cumsum(counts)
    total = int(cum[-1])
    out = bytearray()
    state, col = seed, 0
    mask = (1 << 64) - 1
    while len(out) < period_bytes:
        state = (state + _GAMMA) & mask
        z = state
        z = ((z ^ (z >> 30)) * _M1) & mask
        z = ((z ^ (z >> 27)) * _M2) & mask
        z ^= z >> 31
        w = vocab[int(np.searchsorted(cum, (z >> 1) % total, side="right"))]
        out += w
        col += len(w)
        if col > 72:
            out += b"\n"
            col = 0
        else:
            out += b" "
            col += 1
    return bytes(out[:period_bytes])


def synth_text(dev, period_bytes, seed=SYNTH_SEED):
    """synth_text_reference on the device (a period is 10^7..10^8 tokens):
    counter-based splitmix64 in wrapping int64 arithmetic, a search in the
    cumulative counts, byte positions by a prefix sum - and the greedy line
    breaks, which are a chain (line k starts where line k-1 broke): "the line
    that starts at token i ends behind token next(i)" for every i, then the
    orbit of token 0 by pointer doubling."""
    vocab, counts = _vocabulary()
    maxlen = max(len(w) for w in vocab)
    table = np.zeros((len(vocab), maxlen), dtype=np.uint8)
    lens = np.array([len(w) for w in vocab], dtype=np.int64)
    for i, w in enumerate(vocab):
        table[i, :len(w)] = np.frombuffer(w, dtype=np.uint8)
    cum = torch.from_numpy(np.cumsum(counts)).to(dev)
    total = int(cum[-1].item())
    mean_len = float((lens * counts).sum() / counts.sum()) + 1.0
    ntok = int(period_bytes / mean_len * 1.02) + 64
    i = torch.arange(1, ntok + 1, dtype=torch.int64, device=dev)
    z = i * _s64(_GAMMA) + _s64(seed)                   # wraps mod 2^64

    def lsr(x, k):                                      # logical shift right
        return (x >> k) & ((1 << (64 - k)) - 1)
    z = (z ^ lsr(z, 30)) * _s64(_M1)
    z = (z ^ lsr(z, 27)) * _s64(_M2)
    z = z ^ lsr(z, 31)
    ids = torch.searchsorted(cum, lsr(z, 1) % total, right=True)
    del z, i
    d_len = torch.from_numpy(lens).to(dev)[ids]          # token lengths
    ends = torch.cumsum(d_len + 1, 0)                    # behind separator
    starts = ends - d_len - 1
    total_bytes = int(ends[-1].item())
    assert total_bytes >= period_bytes
    # a line that starts at token i (byte starts[i]) breaks behind the first
    # token j whose last byte passes column 72: ends[j] - 1 - starts[i] > 72
    brk = torch.searchsorted(ends, starts + 73, right=True)   # that token j
    nxt = torch.clamp(brk + 1, max=ntok - 1)             # next line's first
    is_start = torch.zeros(ntok, dtype=torch.bool, device=dev)
    is_start[0] = True
    jump = nxt
    while True:                                          # pointer doubling
        idx = is_start.nonzero().squeeze(1)
        before = idx.numel()
        is_start[jump[idx]] = True
        if int(is_start.sum().item()) == before:
            break
        jump = jump[jump]
    del jump
    is_start[-1] = True   # (the clamp's fixed point; behind the period)
    line_first = is_start.nonzero().squeeze(1)
    last_tok = brk[line_first]                           # gets the newline
    last_tok = last_tok[last_tok < ntok]
    out = torch.full((total_bytes,), 32, dtype=torch.uint8, device=dev)
    d_table = torch.from_numpy(table).to(dev)
    for k in range(maxlen):                              # k-th character
        m = d_len > k
        out[starts[m] + k] = d_table[ids[m], k]
    out[ends[last_tok] - 1] = 10
    return out[:period_bytes].contiguous()


def time_it(fn, steps, ctx):
    fn()
    ctx.synchronize()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    ctx.synchronize()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps


def cfg3(args, ctx, dev):
    from rust_snappy_amd import frame
    import oracle_lib as O
    pbytes = min(int(args.period_mib * (1 << 20)),
                 max(1 << 20, int(args.gib * GIB) // 65536 * 65536))
    period = synth_text(dev, pbytes)
    reps = max(1, int(args.gib * GIB / period.numel()))
    data = period.repeat(reps)
    n = data.numel()
    out, flen, index = frame.compress_device(ctx, data, want_index=True)
    # parity: the first 64 MiB (1024 chunks) against the oracle's restatement
    # of write::FrameEncoder, chunk for chunk; the timed decode below checks
    # every period of the round trip against the generator's period
    hn = min(64 << 20, n // 65536 * 65536)
    head = data[:hn].cpu().numpy().tobytes()
    want = O.frame_compress(head)
    k = hn // 65536
    cut = int(index[k].item())
    assert out[:cut].cpu().numpy().tobytes() == want[:cut], "framed bytes differ"
    import ctypes as C
    from rust_snappy_amd import _lib, raw
    L = _lib.load()
    out_len = torch.zeros(1, dtype=torch.int64, device=dev)
    err = torch.zeros(32, dtype=torch.uint8, device=dev)
    cap = frame.frame_max_len(n)

    def enc():
        rc = L.snapmi_frame_compress(ctx._h, C.c_void_p(data.data_ptr()), n,
                                     C.c_void_p(out.data_ptr()), cap,
                                     C.c_void_p(out_len.data_ptr()),
                                     C.c_void_p(index.data_ptr()))
        assert rc == 0

    te = time_it(enc, args.steps, ctx)
    # the input is not needed any more (64 GiB + 75 GiB of output capacity +
    # 64 GiB of decoded output would not leave room for the scratch)
    del data
    torch.cuda.empty_cache()
    back, m = frame.decompress_device(ctx, out, flen, index=index, out_cap=n)
    assert m == n, "frame round trip length"

    def dec():
        rc = L.snapmi_frame_decompress(ctx._h, C.c_void_p(out.data_ptr()),
                                       flen, C.c_void_p(back.data_ptr()), n,
                                       C.c_void_p(out_len.data_ptr()),
                                       C.c_void_p(err.data_ptr()),
                                       C.c_void_p(index.data_ptr()),
                                       index.numel() - 1)
        assert rc == 0

    def dec_walk():  # no side index: the device walks the chunk headers
        rc = L.snapmi_frame_decompress(ctx._h, C.c_void_p(out.data_ptr()),
                                       flen, C.c_void_p(back.data_ptr()), n,
                                       C.c_void_p(out_len.data_ptr()),
                                       C.c_void_p(err.data_ptr()), None, 0)
        assert rc == 0

    tw = time_it(dec_walk, 1, ctx)
    td = time_it(dec, args.steps, ctx)
    # round trip of the timed decode against the generator's period
    per = back[:reps * period.numel()].view(reps, period.numel())
    for r in range(reps):
        assert torch.equal(per[r], period), "frame round trip (timed)"
    types = out[index[:-1]]                  # chunk type bytes
    n_stored = int((types == 1).sum().item())
    return {"config": "cfg3 framed synthetic text (SURVEY 8d generator: "
                      "splitmix64 seed 0x5EED5A4D53505931, unigram tokens of "
                      "the four corpus texts, newline behind the first token "
                      "past column 72; period "
                      f"{period.numel() >> 20} MiB)",
            "gib": round(n / GIB, 3),
            "chunks": index.numel() - 1, "uncompressed_chunks": n_stored,
            "ratio": round(flen / n, 4),
            "frame_encode_gibs": round(n / GIB / te, 2),
            "frame_decode_gibs": round(n / GIB / td, 2),
            "encode_ms": round(te * 1e3, 2), "decode_ms": round(td * 1e3, 2),
            "decode_uses_side_index": True,
            "frame_decode_no_index_gibs": round(n / GIB / tw, 2),
            "decode_no_index_ms": round(tw * 1e3, 2)}


def stream_probe(t, write=True):
    """GB/s of a plain streaming pass over the uint8 tensor `t` - a fill
    (write) or a sum (read) by torch's own kernels: where in the device's
    memory a buffer lies decides 20 % of what streams into it (tests/hw/
    zone_stream.hip: writes run at 4.7 TB/s into the first 64 GiB a process is
    handed and at 5.2-6.3 TB/s behind them, reads at 5.7 / 6.0-6.3)."""
    v = t[:t.numel() // 8 * 8].view(torch.int64)
    for k in range(3):
        if k == 1:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
        if write:
            v.fill_(0)
        else:
            v.sum()
    torch.cuda.synchronize()
    return round(2 * v.numel() * 8 / (time.perf_counter() - t0) / 1e9)


def raw_tiles(ctx, dev, blob, gib, steps, want=None, diag=None,
              back_first=False):
    """`blob` as independent raw streams tiled to `gib`: compress and
    decompress rates, first/last stream checked against `want`.  `diag`: a
    dict for the streaming rates of the buffers where they lie."""
    from rust_snappy_amd import batch, raw
    reps = max(1, int(gib * GIB / max(1, len(blob))))
    stride = (len(blob) + 15) // 16 * 16
    back = None
    if back_first:   # the decoder's output buffer before everything else
        back = batch.StreamBatch.empty(
            np.full(reps, len(blob), dtype=np.int64), dev)
    one = np.zeros(stride, dtype=np.uint8)
    one[:len(blob)] = np.frombuffer(blob, dtype=np.uint8)
    data = torch.from_numpy(one).to(dev).repeat(reps)
    offs = np.arange(reps, dtype=np.int64) * stride
    lens = np.full(reps, len(blob), dtype=np.int64)
    src = batch.StreamBatch(data, offs, lens)
    cap = raw.max_compress_len(len(blob))
    comp = batch.StreamBatch.empty(np.full(reps, cap, dtype=np.int64), dev)
    clens = torch.zeros(reps, dtype=torch.int64, device=dev)
    if back is None:
        back = batch.StreamBatch.empty(lens, dev)
    blens = torch.zeros(reps, dtype=torch.int64, device=dev)

    def enc():
        raw.compress_batch(ctx, src.d_ptrs, src.d_lens, comp.d_ptrs,
                           comp.d_lens, clens, None, host_in_lens=src.h_lens)

    def dec():
        raw.decompress_batch(ctx, comp.d_ptrs, clens, back.d_ptrs,
                             back.d_lens, blens, None)

    if diag is not None:
        diag.update({"write_gbs_into_compressed": stream_probe(comp.data),
                     "write_gbs_into_decoded": stream_probe(back.data),
                     "read_gbs_of_input": stream_probe(data, write=False)})
    enc()
    ctx.synchronize()
    if want is not None:
        assert comp.stream_bytes(0, int(clens[0])) == want
        assert comp.stream_bytes(reps - 1, int(clens[-1])) == want
    te = time_it(enc, steps, ctx)
    td = time_it(dec, steps, ctx)
    assert back.stream_bytes(reps // 2) == blob
    n = reps * len(blob)
    c = int(clens.sum().item())
    return n, c, reps, te, td


def cfg5(args, ctx, dev):
    import oracle_lib as O
    jpg = (O.CORPUS / "fireworks.jpeg").read_bytes()

    def row(n, c, reps, te, td, diag):
        return {"gib": round(n / GIB, 3), "streams": reps,
                "compress_gibs": round(n / GIB / te, 2),
                "decompress_gibs": round(n / GIB / td, 2),
                "compress_hbm_frac": round((n + c) / te / 8e12, 4),
                "decompress_hbm_frac": round((n + c) / td / 8e12, 4),
                "compress_ms": round(te * 1e3, 2),
                "decompress_ms": round(td * 1e3, 2), **diag}
    diag = {"free_gib_before": round(torch.cuda.mem_get_info(dev)[0] / GIB)}
    res = {"config": "cfg5 incompressible (fireworks.jpeg tiles)"}
    res.update(row(*raw_tiles(ctx, dev, jpg, args.gib, args.steps,
                              O.compress(jpg), diag), diag))
    # Round 5 left a riddle: this pure streaming path took 11.8 ms to decode
    # on one box and 14.0 on the next.  It is WHERE the buffers lie (see
    # stream_probe): the same call with every buffer allocated behind a
    # spacer of 96 GiB, and with the decoder's output buffer allocated first
    # (the part of the memory that takes writes slowest) - beside the row above, whose buffers lie wherever the allocator
    # put them after the configs that ran before.
    torch.cuda.empty_cache()
    d2 = {}
    res["decoded_buffer_allocated_first"] = row(
        *raw_tiles(ctx, dev, jpg, args.gib, args.steps, O.compress(jpg), d2,
                   back_first=True), d2)
    torch.cuda.empty_cache()
    need = 3.3 * args.gib + 96 + 8
    if torch.cuda.mem_get_info(dev)[0] / GIB > need:
        spacer = torch.empty(int(96 * GIB), dtype=torch.uint8, device=dev)
        d3 = {}
        res["behind_a_96_gib_spacer"] = row(
            *raw_tiles(ctx, dev, jpg, args.gib, args.steps, O.compress(jpg),
                       d3), d3)
        del spacer
        torch.cuda.empty_cache()
    return res


def files(args, ctx, dev):
    """The 12 inputs of the reference's bench list one at a time
    (bench/src/bench.rs:83-114; README.md:135-158 quotes them per file),
    each tiled to --gib as independent raw streams."""
    import oracle_lib as O
    rows = {}
    for bench_id, blob in O.corpus_round():
        n, c, reps, te, td = raw_tiles(ctx, dev, blob, args.gib, args.steps,
                                       O.compress(blob))
        rows[bench_id] = {"bytes": len(blob), "ratio": round(c / n, 4),
                          "streams": reps,
                          "compress_gibs": round(n / GIB / te, 2),
                          "decompress_gibs": round(n / GIB / td, 2)}
    return {"config": f"per-file rates, each tiled to {args.gib} GiB",
            "files": rows}


def round_tiles(ctx, dev, gib, steps, diag=None):
    """The 12-stream zflat/uflat round tiled to `gib` as independent raw
    streams (bench.py's workload at another size): compress and decompress
    seconds per pass, round 0 compared with the oracle's bytes, the round
    trip with the input.  `diag` (a dict) gets what explains a row from the
    outside: the first compress call on this context at this size on its own
    (it allocates, and places the lane tables), the placement's log, every
    timed call's kernel ms, hipMemGetInfo's free bytes around it all."""
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
    rounds = max(1, int(round(gib * GIB / int(r_lens.sum()))))
    data = torch.from_numpy(one).to(dev).repeat(rounds)
    o_all = (np.arange(rounds, dtype=np.int64)[:, None] * pos
             + np.array(offs, dtype=np.int64)[None, :]).reshape(-1)
    lens = np.tile(r_lens, rounds)
    n = 12 * rounds
    src = batch.StreamBatch(data, o_all, lens)
    caps = np.array([raw.max_compress_len(int(x)) for x in r_lens],
                    dtype=np.int64)
    comp = batch.StreamBatch.empty(np.tile(caps, rounds), dev)
    clens = torch.zeros(n, dtype=torch.int64, device=dev)
    back = batch.StreamBatch.empty(lens, dev)
    blens = torch.zeros(n, dtype=torch.int64, device=dev)

    def enc():
        raw.compress_batch(ctx, src.d_ptrs, src.d_lens, comp.d_ptrs,
                           comp.d_lens, clens, None, host_in_lens=src.h_lens)

    def dec():
        raw.decompress_batch(ctx, comp.d_ptrs, clens, back.d_ptrs,
                             back.d_lens, blens, None)

    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info(dev)[0]
    t0 = time.perf_counter()
    enc()
    ctx.synchronize()
    first_ms = (time.perf_counter() - t0) * 1e3
    cl = clens.cpu().numpy()
    for j, (_, d) in enumerate(rnd):
        assert comp.stream_bytes(j, int(cl[j])) == O.compress(d), j
        k = n - 12 + j
        assert comp.stream_bytes(k, int(cl[k])) == O.compress(d), k
    calls = []

    def enc_logged():
        t0 = time.perf_counter()
        enc()
        ctx.synchronize()
        calls.append(round((time.perf_counter() - t0) * 1e3, 2))
    te = time_it(enc_logged if diag is not None else enc, steps, ctx)
    enc_kernel = ctx.last_kernel()
    td = time_it(dec, steps, ctx)
    if diag is not None:
        diag.update({
            "first_call_ms": round(first_ms, 1),
            "call_ms": calls,            # the warm call, then the timed ones
            "kernel": enc_kernel,        # the compress side's dominant kernel
            "placement": ctx.table_probe_log(),
            "free_gib_before": round(free0 / GIB, 1),
            "free_gib_after": round(torch.cuda.mem_get_info(dev)[0] / GIB, 1)})
    for j, (_, d) in enumerate(rnd):
        assert back.stream_bytes(n - 12 + j) == d, j
    ub = rounds * int(r_lens.sum())
    return ub, int(cl.sum()), n, te, td


def sweep(args, ctx, dev):
    """The batch-size regime the headline hides: bench.py's workload (the
    12-stream round as independent raw streams) at 64 MiB / 256 MiB / 1 GiB /
    4 GiB per call - what an adapter's batch, a host slice or a frame of a
    few hundred MiB pays."""
    from rust_snappy_amd import raw
    rows = {}
    # (a context of its own: its lane tables are made for the first size
    # that needs them, which is not how the other configs meet theirs)
    own = raw.Context(ctx.device)
    for label, gib in (("64MiB", 1 / 16), ("256MiB", 0.25), ("1GiB", 1.0),
                       ("4GiB", 4.0)):
        if gib > args.gib:
            continue
        diag = {}
        ub, cb, n, te, td = round_tiles(own, dev, gib, max(args.steps, 3),
                                        diag)
        rows[label] = {"gib": round(ub / GIB, 4), "streams": n,
                       "compress_gibs": round(ub / GIB / te, 2),
                       "decompress_gibs": round(ub / GIB / td, 2),
                       "compress_ms": round(te * 1e3, 3),
                       "decompress_ms": round(td * 1e3, 3), **diag}
    own.close()
    torch.cuda.empty_cache()
    return {"config": "bench.py's workload (12-stream round, independent raw "
                      "streams, device resident) by batch size", "sizes": rows}


def budget(args, ctx, dev):
    """What the headline's memory setting buys: bench.py's workload at --gib
    with the lane tables allowed 75 % (bench.py), 33 % (the library's
    default) and 15 % of the free device memory - compress GiB/s, the bytes
    the tables hold afterwards and the most that was held while a placement
    was chosen (snapmi_table_probe_log)."""
    from rust_snappy_amd import _lib, raw
    rows = {}
    for pct in (75, 33, 15):
        c = raw.Context(ctx.device)
        c.set_option("lane_table_budget_pct", pct)
        free0 = torch.cuda.mem_get_info(dev)[0]
        diag = {}
        ub, cb, n, te, td = round_tiles(c, dev, args.gib, max(args.steps, 3),
                                        diag)
        log = c.table_probe_log()
        held = None
        if "held at most" in log:
            held = int(log.split("held at most")[1].split()[0])
        torch.cuda.empty_cache()
        free1 = torch.cuda.mem_get_info(dev)[0]
        rows[f"pct{pct}"] = {"compress_gibs": round(ub / GIB / te, 2),
                             "compress_ms": round(te * 1e3, 2),
                             "context_bytes": int(free0 - free1),
                             "token_scratch_bytes":
                                 c.info("token_scratch_bytes"),
                             "input_bytes": int(ub),
                             "held_at_most_during_placement": held,
                             "first_call_ms": diag["first_call_ms"],
                             "call_ms": diag["call_ms"],
                             "placement": diag["placement"]}
        c.close()
        torch.cuda.empty_cache()
    # ... and the explicit opt-in: snapmi_ctx_prepare(TOP_OF_MEMORY) before
    # the first batch (holds the whole device for a moment, include/snapmi.h).
    # NOTE what this row is: the call is made for a process that asks FIRST;
    # here it is the fourth context of a process that has allocated and freed
    # hundreds of GB, where "the far end" is wherever the allocator's free
    # lists say (the device reuses what was freed last): the row shows the
    # call's cost and that it works, not its best case
    # (profiles/r6_budget_chunks.txt: 71.6-71.8 GiB/s in a fresh process)
    c = raw.Context(ctx.device)
    rounds = max(1, int(round(args.gib * GIB / 2928571)))
    free0 = torch.cuda.mem_get_info(dev)[0]
    t0 = time.perf_counter()
    c.prepare(50 * rounds, top_of_memory=True)     # 50 blocks per round
    prep_ms = (time.perf_counter() - t0) * 1e3
    diag = {}
    ub, cb, n, te, td = round_tiles(c, dev, args.gib, max(args.steps, 3), diag)
    torch.cuda.empty_cache()
    free1 = torch.cuda.mem_get_info(dev)[0]
    rows["prepared_top_of_memory"] = {
        "compress_gibs": round(ub / GIB / te, 2),
        "compress_ms": round(te * 1e3, 2),
        "context_bytes": int(free0 - free1),
        "prepare_ms": round(prep_ms, 1),
        "first_call_ms": diag["first_call_ms"], "call_ms": diag["call_ms"],
        "placement": diag["placement"]}
    c.close()
    torch.cuda.empty_cache()
    # ... and the token scratch: the pool at 100 % of the worst case (no
    # block can spill; round 5's layout in pages), and the block list matched
    # and encoded in two equal launches (lane_segment_blocks) - what the
    # context holds against what it costs
    for seg in (1 << 20, 98304):
        c = raw.Context(ctx.device)
        c.set_option("lane_table_budget_pct", 75)
        c.set_option("lane_segment_blocks", seg)
        if seg == 1 << 20:
            c.set_option("token_pool_pct", 100)
        free0 = torch.cuda.mem_get_info(dev)[0]
        diag = {}
        ub, cb, n, te, td = round_tiles(c, dev, args.gib, max(args.steps, 3),
                                        diag)
        torch.cuda.empty_cache()
        free1 = torch.cuda.mem_get_info(dev)[0]
        launches = -(-50 * rounds // seg)
        rows["token_pool_100_pct" if seg == 1 << 20 else
             f"segments_of_at_most_{seg}_blocks"] = {
            "launches": launches,
            "compress_gibs": round(ub / GIB / te, 2),
            "compress_ms": round(te * 1e3, 2),
            "context_bytes": int(free0 - free1),
            "token_scratch_bytes": c.info("token_scratch_bytes"),
            "blocks_spilled": c.info("token_blocks_spilled"),
            "input_bytes": int(ub), "call_ms": diag["call_ms"]}
        c.close()
        torch.cuda.empty_cache()
    return {"config": f"lane_table_budget_pct 75 / 33 / 15 at {args.gib:g} "
                      "GiB of bench.py's workload, snapmi_ctx_prepare("
                      "SNAPMI_PREPARE_TOP_OF_MEMORY), token_pool_pct 100, "
                      "and the batch in two launches (lane_segment_blocks)",
            "budgets": rows}


def tiny(args, ctx, dev):
    """The tiny-stream regime on its own: zflat03 (the first 200 bytes of
    fireworks.jpeg, bench/src/bench.rs:91) tiled to --gib = 10.7 M streams
    at 2 GiB; beside it the first 200 bytes of alice29.txt (tiny streams
    that do compress: literals and copies in every lane) and its first
    400 / 1 000 / 2 000 / 4 096 bytes."""
    import oracle_lib as O
    res = None
    for bench_id, blob in O.corpus_round():
        if len(blob) == 200:
            n, c, reps, te, td = raw_tiles(ctx, dev, blob, args.gib,
                                           args.steps, O.compress(blob))
            res = {"config": f"{bench_id} tiled to {args.gib} GiB",
                   "streams": reps, "ratio": round(c / n, 4),
                   "compress_gibs": round(n / GIB / te, 2),
                   "decompress_gibs": round(n / GIB / td, 2),
                   "compress_ms": round(te * 1e3, 2),
                   "decompress_ms": round(td * 1e3, 2)}
    # (400 .. 2 000 bytes: the three classes of k_compress_small; 4 KiB: a
    # one-block stream of the block kernels)
    for key, size in (("text_200", 200), ("text_400", 400),
                      ("text_1k", 1000), ("text_2k", 2000),
                      ("text_4k", 4096)):
        text = (O.CORPUS / "alice29.txt").read_bytes()[:size]
        n, c, reps, te, td = raw_tiles(ctx, dev, text, args.gib, args.steps,
                                       O.compress(text))
        res[key] = {"ratio": round(c / n, 4),
                    "compress_gibs": round(n / GIB / te, 2),
                    "decompress_gibs": round(n / GIB / td, 2)}
    return res


def seam(args, ctx, dev):
    """The reference-side view of the native seam (snappy-cpp/src/lib.rs:13-88,
    the `cpp` group of bench/src/bench.rs:117-153): tests/seam_consumer.c - a C
    program against snappy-c.h, linked with -lsnappy - built once against a
    directory whose libsnappy.so is a symlink to libsnapmi.so and once against
    Google's libsnappy 1.1.8, one call per file, 1 and 16 callers at once.
    MB/s of uncompressed bytes, [compress, uncompress]; args.gib = milliseconds
    per file, direction and thread count."""
    import oracle_lib as O
    import os
    import subprocess
    import tempfile
    hdr = "/opt/conda/include"
    if not os.path.exists(f"{hdr}/snappy-c.h"):
        return {"error": "no snappy-c.h in this image"}
    ms = max(20.0, float(args.gib))
    with tempfile.TemporaryDirectory() as d:
        lib = ROOT / "rust-snappy_amd" / "libsnapmi.so"
        os.symlink(lib, f"{d}/libsnappy.so")
        ins = f"{d}/in"
        os.mkdir(ins)
        for name, data in O.corpus_round():
            open(f"{ins}/{name}.in", "wb").write(data)
            open(f"{ins}/{name}.snappy", "wb").write(O.compress(data))
        src = str(ROOT / "tests" / "seam_consumer.c")
        builds = {"snapmi": [f"-L{d}", f"-Wl,-rpath,{d}",
                             f"-Wl,-rpath,{lib.parent}"]}
        if os.path.exists("/opt/conda/lib/libsnappy.so"):
            builds["libsnappy_1_1_8"] = ["-L/opt/conda/lib",
                                         "-Wl,-rpath,/opt/conda/lib"]
        res = {"config": "one call per bench input through snappy-c.h "
                         "(tests/seam_consumer.c, -lsnappy)",
               "unit": "MB/s uncompressed [compress, uncompress]",
               "ms_per_leg": ms}
        for key, flags in builds.items():
            exe = f"{d}/consumer_{key}"
            subprocess.check_call(["gcc", "-O2", "-I", hdr, "-o", exe, src]
                                  + flags + ["-lsnappy", "-lpthread"])
            p = subprocess.run([exe, "check", ins], capture_output=True,
                               text=True, timeout=120)
            if p.returncode != 0:
                return {"error": f"{key}: check failed: "
                                 + (p.stdout + p.stderr)[-200:]}
            rows = {}
            for threads in (1, 16):
                p = subprocess.run([exe, "bench", ins, str(threads), str(ms)],
                                   capture_output=True, text=True,
                                   timeout=300)
                if p.returncode != 0:
                    return {"error": f"{key}: bench with {threads} callers: "
                                     + (p.stdout + p.stderr)[-200:]}
                for line in p.stdout.splitlines():
                    name, n, t, c, u = line.split()
                    rows.setdefault(name, {})[f"callers_{t}"] = [
                        float(c), float(u)]
            res[key] = rows
        return res


def _host_corpus(gib):
    """The corpus round tiled into pinned host memory (snapmi_host_alloc)."""
    import oracle_lib as O
    from rust_snappy_amd import frame
    blob = b"".join(d for _, d in O.corpus_round())
    reps = max(1, int(gib * GIB / len(blob)))
    n = reps * len(blob)
    h_in = frame.HostBuffer(n)
    h_in.array.reshape(reps, len(blob))[:] = np.frombuffer(blob, dtype=np.uint8)
    return blob, n, h_in


def pcie(args, ctx, dev):
    """Host to host through the frame layer: snapmi_frame_encode_host and
    snapmi_frame_decode_host on pinned host buffers - what a host-side
    FrameEncoder / FrameDecoder pays per batch (slices in flight on three
    streams: copy in, kernels, copy out).  bench.py's `value` is device
    resident; this is never it."""
    import ctypes as C
    import oracle_lib as O
    from rust_snappy_amd import _lib, frame
    L = _lib.load()
    blob, n, h_in = _host_corpus(min(args.gib, 4.0))
    nch = (n + 65535) // 65536
    lens = np.full(nch, 65536, dtype=np.uint32)
    lens[-1] = n - (nch - 1) * 65536
    h_out = frame.HostBuffer(10 + n + 8 * nch)
    h_back = frame.HostBuffer(nch * 65536)
    flen = 0

    def enc():
        nonlocal flen
        flen = frame.encode_host_into(ctx, h_in.view, lens, h_out)

    def dec():
        stale = (C.c_uint8 * 10)()
        written, consumed = C.c_size_t(0), C.c_size_t(0)
        err = _lib.SnapmiError()
        rc = L.snapmi_frame_decode_host(
            ctx._h, C.c_void_p(h_out.ptr), flen, 2, stale,
            C.c_void_p(h_back.ptr), h_back.nbytes, C.byref(written),
            C.byref(consumed), C.byref(err))
        assert rc == 0 and written.value == n and consumed.value == flen, \
            (rc, written.value, consumed.value)

    te = time_it(enc, args.steps, ctx)
    td = time_it(dec, args.steps, ctx)
    assert bool((h_back.array[:n] == h_in.array).all()), "host round trip"
    head = O.frame_compress(bytes(h_in.view[:1 << 20]))
    assert bytes(h_out.view[:len(head)]) == head, "framed bytes vs the oracle"
    res = {"config": "host to host through snapmi_frame_encode_host / "
                     "_decode_host (pinned memory; slices pipelined over "
                     "copy-in, kernels, copy-out)",
           "gib": round(n / GIB, 3), "ratio": round(flen / n, 4),
           "frame_encode_gibs": round(n / GIB / te, 2),
           "frame_decode_gibs": round(n / GIB / td, 2),
           "encode_ms": round(te * 1e3, 2), "decode_ms": round(td * 1e3, 2)}
    for b in (h_in, h_out, h_back):
        b.close()
    return res


def adapters(args, ctx, dev):
    """The streaming adapters the north star keeps: FrameEncoder.write_all of
    one large host buffer (rust-snappy_amd/frame.py, the mirror of
    snap::write::FrameEncoder), FrameDecoder.read_to_end of the result (Python
    bytes) and FrameDecoder.readinto of it (the caller's pinned buffer)."""
    import io
    import oracle_lib as O
    from rust_snappy_amd import frame
    blob, n, h_in = _host_corpus(min(args.gib, 4.0))

    class Sink:
        def __init__(self):
            self.n, self.head = 0, bytearray()

        def write(self, b):
            if len(self.head) < (2 << 20):
                self.head += b[:2 << 20]
            self.n += len(b)
            return len(b)

    # one encoder, written to repeatedly (its pinned staging buffer is made
    # by the first large write, like a Vec that has grown)
    sink = Sink()
    enc = frame.FrameEncoder(sink, ctx)
    enc.write_all(h_in.view[:64 << 20])
    enc.flush()
    enc.DIRECT_MAX = 4 << 30    # one device call for the whole write
    enc.write_all(h_in.view)                    # staging grows here
    enc.flush()
    head0 = bytes(sink.head)
    best = None
    for _ in range(max(2, args.steps)):
        t0 = time.perf_counter()
        enc.write_all(h_in.view)
        enc.flush()
        t = time.perf_counter() - t0
        best = t if best is None or t < best else best
    sink = Sink()
    enc2 = frame.FrameEncoder(sink, ctx)
    enc2.write_all(h_in.view[:4 << 20])
    enc2.flush()
    want = O.frame_compress(bytes(h_in.view[:1 << 20]))
    assert bytes(sink.head[:len(want)]) == want, "adapter bytes vs the oracle"
    # decoder adapter on a smaller stream (it hands out Python bytes)
    m = min(n, 1 << 30)
    sink = io.BytesIO()
    enc = frame.FrameEncoder(sink, ctx)
    enc.write_all(h_in.view[:m])
    enc.flush()
    framed = sink.getvalue()
    # read_to_end: everything into one bytearray (the reference's Vec<u8>).
    # Its ceiling is the host's, not the device's: every byte of the result
    # is written once into memory the process has never touched - timed here
    # as a plain copy of the same size into a fresh bytearray
    t0 = time.perf_counter()
    fresh = bytearray(h_in.view[:m])
    t_fresh = time.perf_counter() - t0
    del fresh
    td = None
    for _ in range(2):
        dec = frame.FrameDecoder(io.BytesIO(framed), ctx)
        t0 = time.perf_counter()
        back = dec.read_to_end()
        t = time.perf_counter() - t0
        td = t if td is None or t < td else td
        assert len(back) == m and back[:1 << 20] == h_in.view[:1 << 20] and \
            back[m - (1 << 20):] == h_in.view[m - (1 << 20):m], \
            "adapter round trip"
        del back
        dec.close()

    def readinto_all(reader):
        """io::Read::read as the reference has it - into the caller's
        buffer (pinned, with room for a batch: the bytes come straight from
        the device call)"""
        dec = frame.FrameDecoder(reader, ctx)
        t0 = time.perf_counter()
        pos = 0
        while True:
            k = dec.readinto(h_back.view[pos:])
            if k == 0:
                break
            pos += k
        t = time.perf_counter() - t0
        assert pos == m and bytes(h_back.view[:1 << 20]) == bytes(
            h_in.view[:1 << 20]) and bytes(
            h_back.view[m - (1 << 20):m]) == bytes(
            h_in.view[m - (1 << 20):m]), "readinto round trip"
        dec.close()
        return t

    h_back = frame.HostBuffer(m + (256 << 20))
    # ... from Python bytes (io.BytesIO lends its buffer: no host copy, but
    # the copy to the device reads pageable memory) and from pinned memory
    # (HostReader: both ends pinned - what the device call itself does)
    ti = min(readinto_all(io.BytesIO(framed)) for _ in range(2))
    h_fr = frame.HostBuffer(len(framed))
    h_fr.view[:] = framed
    tp = min(readinto_all(frame.HostReader(h_fr.view)) for _ in range(2))
    h_fr.close()
    h_back.close()
    h_in.close()
    return {"config": "Python streaming adapters over the host-buffer calls: "
                      "FrameEncoder.write_all of one pinned buffer (no copy "
                      "on the Python side), FrameDecoder.read_to_end (one "
                      "bytearray), FrameDecoder.readinto a pinned buffer "
                      "from io.BytesIO and from a pinned HostReader",
            "gib": round(n / GIB, 3), "framed_bytes": sink_n(sink, framed),
            "frame_encoder_write_all_gibs": round(n / GIB / best, 2),
            "frame_decoder_read_to_end_gibs": round(m / GIB / td, 2),
            "fresh_bytearray_copy_gibs": round(m / GIB / t_fresh, 2),
            "frame_decoder_readinto_pinned_gibs": round(m / GIB / ti, 2),
            "frame_decoder_readinto_pinned_from_pinned_gibs": round(
                m / GIB / tp, 2),
            "decoder_gib": round(m / GIB, 3)}


def sink_n(sink, framed):
    return len(framed)


def stream(args, ctx, dev):
    """ONE raw stream of --gib (the 12 corpus files repeated): compressed as
    one Encoder::compress call (blocks in parallel), decoded by
    snapmi_decompress_stream (many wavefronts) and, for comparison, 1/16 of
    it as a batch of one stream: through snapmi_decompress_batch as it is
    (the long stream gets its pieces) and with batch_long_streams 0 (a
    single wavefront)."""
    import oracle_lib as O
    from rust_snappy_amd import batch, raw
    blob = b"".join(d for _, d in O.corpus_round())
    reps = max(1, int(min(args.gib, 3.0) * GIB / len(blob)))  # < 2^32 * 6/7
    one = torch.frombuffer(bytearray(blob), dtype=torch.uint8).to(dev)
    data = one.repeat(reps)
    n = data.numel()
    src = batch.StreamBatch(data, np.array([0], dtype=np.int64),
                            np.array([n], dtype=np.int64))
    comp = batch.StreamBatch.empty(
        np.array([raw.max_compress_len(n)], dtype=np.int64), dev)
    clen = torch.zeros(1, dtype=torch.int64, device=dev)
    raw.compress_batch(ctx, src.d_ptrs, src.d_lens, comp.d_ptrs, comp.d_lens,
                       clen, None, host_in_lens=src.h_lens)
    ctx.synchronize()
    c = int(clen.item())
    back = torch.empty(n, dtype=torch.uint8, device=dev)
    out_len = torch.zeros(1, dtype=torch.int64, device=dev)
    err = torch.zeros(32, dtype=torch.uint8, device=dev)

    def dec():
        raw.decompress_stream(ctx, comp.data, c, back, out_len, err)

    td = time_it(dec, args.steps, ctx)
    assert raw.stream_decode_path(ctx) == 0
    assert int(out_len.item()) == n
    per = back.view(reps, len(blob))
    for r in range(0, reps, max(1, reps // 16)):
        assert torch.equal(per[r], one), "stream round trip"
    # a single wavefront on 1/16 of it
    m = (reps // 16 or 1) * len(blob)
    src1 = batch.StreamBatch(data, np.array([0], dtype=np.int64),
                             np.array([m], dtype=np.int64))
    raw.compress_batch(ctx, src1.d_ptrs, src1.d_lens, comp.d_ptrs,
                       comp.d_lens, clen, None, host_in_lens=src1.h_lens)
    ctx.synchronize()
    cap1 = torch.tensor([m], dtype=torch.int64, device=dev)
    optr = torch.tensor([back.data_ptr()], dtype=torch.int64, device=dev)

    def dec1():
        raw.decompress_batch(ctx, comp.d_ptrs, clen, optr, cap1, out_len, None)

    tb = time_it(dec1, 2, ctx)    # the batch call: the stream gets its pieces
    ctx.set_option("batch_long_streams", 0)
    try:
        t1 = time_it(dec1, 1, ctx)   # ... and a wavefront to itself
    finally:
        ctx.set_option("batch_long_streams", 1)
    return {"config": "one raw stream, device resident",
            "gib": round(n / GIB, 3), "ratio": round(c / n, 4),
            "decompress_stream_gibs": round(n / GIB / td, 2),
            "decompress_stream_ms": round(td * 1e3, 2),
            "batch_of_one_gibs": round(m / GIB / tb, 2),
            "one_wavefront_gibs": round(m / GIB / t1, 3),
            "one_wavefront_gib": round(m / GIB, 3)}


def cfg4(args, ctx, dev):
    """BASELINE config 4: the framed text stream of cfg3 sharded over the
    ranks of a torch.distributed job (launch with torch.distributed.run;
    world 1 works too).  Rank r frames periods [r*P/N, (r+1)*P/N) of the
    stream - a contiguous range of 64 KiB chunks, no exchange during compute -
    and the framed parts are gathered on rank 0 (shard.gatherv: sizes first,
    then grouped point-to-point into the root's buffer).  Parts after the
    first drop their 10-byte stream identifier, so the gathered bytes are the
    single-stream framing."""
    import os
    import torch.distributed as dist
    from rust_snappy_amd import frame, shard
    import oracle_lib as O
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    if world > 1 and not dist.is_initialized():
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if os.environ.get("SNAPMI_OVERSUBSCRIBE") == "1":
            dist.init_process_group("gloo")  # N ranks on one GPU: proof run
        else:
            dist.init_process_group("nccl", device_id=dev)
    pbytes = min(int(args.period_mib * (1 << 20)),
                 max(1 << 20, int(args.gib * GIB / world) // 65536 * 65536))
    period = synth_text(dev, pbytes)
    assert period.numel() % 65536 == 0
    periods = max(world, int(args.gib * GIB / period.numel()))
    lo, hi = periods * rank // world, periods * (rank + 1) // world
    data = period.repeat(hi - lo)
    n = data.numel()

    def sync():
        ctx.synchronize()
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()

    out, flen, _ = frame.compress_device(ctx, data)          # warm-up
    sync()
    t0 = time.perf_counter()
    out, flen, _ = frame.compress_device(ctx, data)
    sync()
    t_enc = time.perf_counter() - t0
    part = out[:flen] if rank == 0 else out[10:flen]
    del data
    if world > 1:
        # communicator and point-to-point channels are set up by the first
        # exchange: keep that out of the timed gather
        shard.gatherv(part[:1 << 20], dst=0)
        sync()
    t0 = time.perf_counter()
    whole = shard.gatherv(part, dst=0) if world > 1 else part
    sync()
    t_gather = time.perf_counter() - t0
    seen = [rank]
    if world > 1:
        seen = [None] * world
        dist.all_gather_object(seen, rank)
    res = None
    if rank == 0:
        # the head of the gathered stream against the oracle, chunk for chunk
        head = period[:1 << 20].cpu().numpy().tobytes()
        want = O.frame_compress(head)
        got = whole[:len(want)].cpu().numpy().tobytes()
        parity_ok = got == want  # (raised after the last barrier: a rank
        total = periods * period.numel()  # must not leave the others waiting)
        res = {"config": "cfg4 framed synthetic text sharded by chunk range",
               "n_gpus": world, "gib": round(total / GIB, 3),
               "framed_bytes": int(whole.numel()),
               "frame_encode_gibs_no_gather": round(total / GIB / t_enc, 2),
               "frame_encode_gibs_with_gather": round(
                   total / GIB / (t_enc + t_gather), 2),
               "encode_ms": round(t_enc * 1e3, 2),
               "gather_ms": round(t_gather * 1e3, 2),
               "gathered_bytes_from_peers": int(whole.numel() - part.numel()),
               # root ingress: 7 xGMI links x 153 GB/s
               "gather_gbs": (round((whole.numel() - part.numel()) / t_gather
                                    / 1e9, 1) if world > 1 else None),
               "gather_bound_gbs": 1071.0,
               "ranks_seen": sorted(seen)}
    if world > 1:
        dist.barrier()
    if rank == 0:
        assert parity_ok, "gathered framed bytes differ from the oracle's"
    return res


def frames_batch(args, ctx, dev):
    """Many framed streams per call (frame.compress_many_ptrs /
    decompress_many_ptrs: snapmi_frame_compress_batch / _decompress_batch)
    against a loop of one-stream calls over the same streams
    (snapmi_frame_compress / snapmi_frame_decompress) and against the raw
    batch calls over the same inputs (the floor: no headers, no CRC, no
    walk).  Two sets: 4 096 streams of 16 KiB of corpus text, and 512 streams
    of 100 B .. 1 MiB (log-uniform) of the same text.  All three are timed in
    this process on the same context."""
    import random
    import oracle_lib as O
    from rust_snappy_amd import _lib, batch, frame, raw
    text = b"".join((O.CORPUS / n).read_bytes()
                    for n in ("alice29.txt", "asyoulik.txt", "lcet10.txt",
                              "plrabn12.txt")) * 2
    rng = random.Random(0x5EED)

    def piece(n):
        o = rng.randrange(len(text) - n)
        return text[o:o + n]
    sets = {"text_4096x16k": [piece(16384) for _ in range(4096)],
            "mixed_512_100b_1m": [piece(int(100 * (10486 ** rng.random())))
                                  for _ in range(512)]}
    L = _lib.of(ctx)
    res = {"config": "frames_batch: n framed streams per call vs n one-stream "
                     "calls vs the raw batch floor",
           "steps": args.steps}
    for key, datas in sets.items():
        n = len(datas)
        nbytes = sum(len(d) for d in datas)
        src = batch.StreamBatch.from_bytes(datas, dev)
        fout = batch.StreamBatch.empty(
            [frame.frame_max_len(len(d)) for d in datas], dev)
        flens = torch.zeros(n, dtype=torch.int64, device=dev)
        ferrs = torch.zeros(32 * n, dtype=torch.uint8, device=dev)

        def f_enc():
            frame.compress_many_ptrs(ctx, src.d_ptrs, src.d_lens, fout.d_ptrs,
                                     fout.d_lens, flens, ferrs,
                                     host_in_lens=src.h_lens)
        f_enc()
        ctx.synchronize()
        fl = flens.cpu().numpy()
        assert all(e[0] == 0 for e in batch.read_errors(ferrs))
        for i in (0, n // 2, n - 1):
            assert fout.stream_bytes(i, fl[i]) == O.frame_compress(datas[i])
        framed = batch.StreamBatch(fout.data, fout.offsets, fl)
        back = batch.StreamBatch.empty([len(d) for d in datas], dev)
        blens = torch.zeros(n, dtype=torch.int64, device=dev)
        berrs = torch.zeros(32 * n, dtype=torch.uint8, device=dev)

        def f_dec():
            frame.decompress_many_ptrs(ctx, framed.d_ptrs, framed.d_lens,
                                       back.d_ptrs, back.d_lens, blens, berrs)
        f_dec()
        ctx.synchronize()
        assert all(e[0] == 0 for e in batch.read_errors(berrs))
        for i in (0, n // 2, n - 1):
            assert back.stream_bytes(i, blens[i]) == datas[i]
        # the loop of one-stream calls (addresses prepared beforehand)
        in_a = [src.data.data_ptr() + int(o) for o in src.offsets]
        fo_a = [fout.data.data_ptr() + int(o) for o in fout.offsets]
        bo_a = [back.data.data_ptr() + int(o) for o in back.offsets]
        lens_in = [len(d) for d in datas]
        caps = [int(c) for c in fout.lens]
        flen_l = [int(x) for x in fl]
        one_len = torch.zeros(n, dtype=torch.int64, device=dev)
        one_err = torch.zeros(32 * n, dtype=torch.uint8, device=dev)
        la, ea = one_len.data_ptr(), one_err.data_ptr()
        s_out = batch.StreamBatch.empty(caps, dev)
        so_a = [s_out.data.data_ptr() + int(o) for o in s_out.offsets]

        def s_enc():
            for i in range(n):
                L.snapmi_frame_compress(ctx._h, in_a[i], lens_in[i], so_a[i],
                                        caps[i], la + 8 * i, None)

        def s_dec():
            for i in range(n):
                L.snapmi_frame_decompress(ctx._h, fo_a[i], flen_l[i], bo_a[i],
                                          lens_in[i], la + 8 * i,
                                          ea + 32 * i, None, 0)
        s_enc()
        ctx.synchronize()
        assert s_out.stream_bytes(n - 1, int(one_len[n - 1])) == \
            fout.stream_bytes(n - 1, fl[n - 1])
        # the raw floor
        rout = batch.StreamBatch.empty(
            [raw.max_compress_len(len(d)) for d in datas], dev)
        rlens = torch.zeros(n, dtype=torch.int64, device=dev)
        rback = batch.StreamBatch.empty(lens_in, dev)
        rblens = torch.zeros(n, dtype=torch.int64, device=dev)

        def r_enc():
            raw.compress_batch(ctx, src.d_ptrs, src.d_lens, rout.d_ptrs,
                               rout.d_lens, rlens, None,
                               host_in_lens=src.h_lens)

        def r_dec():
            raw.decompress_batch(ctx, rout.d_ptrs, rlens, rback.d_ptrs,
                                 rback.d_lens, rblens, None)
        r_enc()
        ctx.synchronize()
        t = {}
        for name, fn in (("batch_enc", f_enc), ("batch_dec", f_dec),
                         ("single_enc", s_enc), ("single_dec", s_dec),
                         ("raw_enc", r_enc), ("raw_dec", r_dec)):
            t[name] = time_it(fn, args.steps, ctx)
        assert back.stream_bytes(n - 1, blens[n - 1]) == datas[n - 1]
        assert rback.stream_bytes(n - 1) == datas[n - 1]
        res[key] = {
            "streams": n, "bytes": nbytes,
            "ms": {k: round(v * 1e3, 3) for k, v in t.items()},
            "batch_gibs": {"compress": round(nbytes / GIB / t["batch_enc"], 2),
                           "decompress": round(nbytes / GIB / t["batch_dec"],
                                               2)},
            "batch_over_single_loop_speedup": {
                "compress": round(t["single_enc"] / t["batch_enc"], 1),
                "decompress": round(t["single_dec"] / t["batch_dec"], 1)},
            "batch_over_raw_floor": {
                "compress": round(t["batch_enc"] / t["raw_enc"], 2),
                "decompress": round(t["batch_dec"] / t["raw_dec"], 2)},
            "single_call_us": {
                "compress": round(t["single_enc"] / n * 1e6, 1),
                "decompress": round(t["single_dec"] / n * 1e6, 1)}}
    return res


def raw_index(args, ctx, dev):
    """The block index of raw streams (snapmi_compress_batch_indexed /
    snapmi_decompress_batch_indexed) on frames_batch's two device-resident
    sets and on 256 streams of 1 MiB of the same text: decode with the index
    compress wrote against snapmi_decompress_batch with batch_long_streams 1
    and 0, compress with and without the index - all in this process on one
    context, five alternating repeats of --steps calls each (medians, and the
    spread max - min over the repeats).  Writes profiles/raw_index.json."""
    import random
    import statistics
    import oracle_lib as O
    from rust_snappy_amd import batch, raw
    text = b"".join((O.CORPUS / n).read_bytes()
                    for n in ("alice29.txt", "asyoulik.txt", "lcet10.txt",
                              "plrabn12.txt")) * 2
    rng = random.Random(0x5EED)

    def piece(n):
        o = rng.randrange(len(text) - n)
        return text[o:o + n]
    sets = {"text_4096x16k": [piece(16384) for _ in range(4096)],
            "mixed_512_100b_1m": [piece(int(100 * (10486 ** rng.random())))
                                  for _ in range(512)],
            "text_256x1m": [piece(1 << 20) for _ in range(256)]}
    repeats = 5
    res = {"config": "raw_index: decode with the block index vs "
                     "snapmi_decompress_batch (batch_long_streams 1 / 0), "
                     "compress with / without the index",
           "steps": args.steps, "repeats": repeats}
    for key, datas in sets.items():
        n = len(datas)
        nbytes = sum(len(d) for d in datas)
        src = batch.StreamBatch.from_bytes(datas, dev)
        out = batch.StreamBatch.empty(
            [raw.max_compress_len(len(d)) for d in datas], dev)
        clens = torch.zeros(n, dtype=torch.int64, device=dev)
        entries = raw.block_index_entries([len(d) for d in datas])
        first = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        index = torch.zeros(entries, dtype=torch.int64, device=dev)
        back = batch.StreamBatch.empty([len(d) for d in datas], dev)
        blens = torch.zeros(n, dtype=torch.int64, device=dev)
        berrs = torch.zeros(32 * n, dtype=torch.uint8, device=dev)

        def enc_plain():
            raw.compress_batch(ctx, src.d_ptrs, src.d_lens, out.d_ptrs,
                               out.d_lens, clens, None,
                               host_in_lens=src.h_lens)

        def enc_indexed():
            raw.compress_batch(ctx, src.d_ptrs, src.d_lens, out.d_ptrs,
                               out.d_lens, clens, None,
                               host_in_lens=src.h_lens, index_first=first,
                               index=index, index_cap=entries)

        def dec_indexed():
            raw.decompress_batch(ctx, out.d_ptrs, clens, back.d_ptrs,
                                 back.d_lens, blens, berrs,
                                 index_first=first, index=index,
                                 index_entries=entries)

        def dec_plain(long_streams):
            def run():
                raw.decompress_batch(ctx, out.d_ptrs, clens, back.d_ptrs,
                                     back.d_lens, blens, berrs)

            def timed():
                ctx.set_option("batch_long_streams", long_streams)
                try:
                    return time_it(run, args.steps, ctx)
                finally:
                    ctx.set_option("batch_long_streams", 1)
            return timed
        enc_indexed()
        ctx.synchronize()
        for i in (0, n // 2, n - 1):
            assert out.stream_bytes(i, int(clens[i])) == O.compress(datas[i])
        blens.zero_()
        back.data.zero_()
        dec_indexed()
        pieced = ctx.info("index_streams_pieced")
        fallback = ctx.info("index_streams_fallback")
        assert all(e[0] == 0 for e in batch.read_errors(berrs))
        for i in (0, n // 2, n - 1):
            assert back.stream_bytes(i, int(blens[i])) == datas[i]
        timers = {"dec_indexed": lambda: time_it(dec_indexed, args.steps, ctx),
                  "dec_long_streams_1": dec_plain(1),
                  "dec_long_streams_0": dec_plain(0),
                  "enc_indexed": lambda: time_it(enc_indexed, args.steps, ctx),
                  "enc_plain": lambda: time_it(enc_plain, args.steps, ctx)}
        t = {k: [] for k in timers}
        for _ in range(repeats):
            for k, fn in timers.items():
                t[k].append(fn() * 1e3)
        med = {k: statistics.median(v) for k, v in t.items()}
        spread = {k: max(v) - min(v) for k, v in t.items()}

        def not_slower(a, b):
            return med[a] <= med[b] + max(spread[a], spread[b])
        res[key] = {
            "streams": n, "bytes": nbytes, "index_entries": entries,
            "index_streams_pieced": pieced,
            "index_streams_fallback": fallback,
            "ms_median": {k: round(v, 4) for k, v in med.items()},
            "ms_spread": {k: round(v, 4) for k, v in spread.items()},
            "ms_repeats": {k: [round(x, 4) for x in v] for k, v in t.items()},
            "dec_indexed_gibs": round(nbytes / GIB / (med["dec_indexed"] / 1e3),
                                      1),
            "dec_indexed_over_long_streams_1": round(
                med["dec_indexed"] / med["dec_long_streams_1"], 3),
            "dec_indexed_over_long_streams_0": round(
                med["dec_indexed"] / med["dec_long_streams_0"], 3),
            "enc_indexed_over_plain": round(
                med["enc_indexed"] / med["enc_plain"], 3),
            "dec_indexed_not_slower_than_both_within_spread":
                not_slower("dec_indexed", "dec_long_streams_1")
                and not_slower("dec_indexed", "dec_long_streams_0")}
    (ROOT / "profiles" / "raw_index.json").write_text(json.dumps(res) + "\n")
    return res


def raw_index_build(args, ctx, dev):
    """Building the block index of streams that came without one
    (snapmi_build_block_index) on raw_index's 256 streams of 1 MiB of text
    and its mixed set of 512 streams of 100 B .. 1 MiB, compressed WITHOUT an
    index: the build, snapmi_decompress_batch with batch_long_streams 1 (the
    yardstick: the same scan plus the piece decode) and 0, and the indexed
    decode through the built index - all in this process on one context, five
    alternating repeats of --steps calls each (medians, and the spread max -
    min over the repeats) - and build / (unindexed - indexed), the decodes
    after which building has paid for itself.  The text set again with every
    stream's last byte cut off (all CORRUPT: the scan gives up on every one
    and the walker walks it to its end - the worst a batch can do to the
    build).  With the test build of the library also the walker alone
    (index_build_route 1).
    Writes profiles/raw_index_build.json."""
    import random
    import statistics
    import oracle_lib as O
    from rust_snappy_amd import _lib, batch, raw
    text = b"".join((O.CORPUS / n).read_bytes()
                    for n in ("alice29.txt", "asyoulik.txt", "lcet10.txt",
                              "plrabn12.txt")) * 2
    rng = random.Random(0x5EED)

    def piece(n):
        o = rng.randrange(len(text) - n)
        return text[o:o + n]
    sets = {"text_256x1m": [piece(1 << 20) for _ in range(256)],
            "mixed_512_100b_1m": [piece(int(100 * (10486 ** rng.random())))
                                  for _ in range(512)]}
    has_test = hasattr(_lib.of(ctx), "snapmi_ctx_set_test_option")
    repeats = 5
    res = {"config": "raw_index_build: snapmi_build_block_index vs "
                     "snapmi_decompress_batch (batch_long_streams 1 / 0) and "
                     "the indexed decode through the built index",
           "steps": args.steps, "repeats": repeats, "test_build": has_test}
    for key, datas in sets.items():
        n = len(datas)
        nbytes = sum(len(d) for d in datas)
        src = batch.StreamBatch.from_bytes(datas, dev)
        comp, clens, errs = batch.compress(ctx, src)   # no index
        assert all(e[0] == 0 for e in errs)
        comp = batch.StreamBatch(comp.data, comp.offsets, clens)
        h_in = [int(x) for x in clens]
        h_out = [len(d) for d in datas]
        entries = raw.block_index_entries(h_out)
        first = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        index = torch.zeros(entries, dtype=torch.int64, device=dev)
        status = torch.zeros(n, dtype=torch.uint8, device=dev)
        back = batch.StreamBatch.empty(h_out, dev)
        blens = torch.zeros(n, dtype=torch.int64, device=dev)
        berrs = torch.zeros(32 * n, dtype=torch.uint8, device=dev)

        def build(src=comp, h_in=h_in):
            raw.build_block_index(ctx, src.d_ptrs, src.d_lens, h_in, h_out,
                                  first, index, status, index_cap=entries)

        def dec_indexed():
            raw.decompress_batch(ctx, comp.d_ptrs, comp.d_lens, back.d_ptrs,
                                 back.d_lens, blens, berrs,
                                 index_first=first, index=index,
                                 index_entries=entries)

        def dec_plain(long_streams):
            def run():
                raw.decompress_batch(ctx, comp.d_ptrs, comp.d_lens,
                                     back.d_ptrs, back.d_lens, blens, berrs)

            def timed():
                ctx.set_option("batch_long_streams", long_streams)
                try:
                    return time_it(run, args.steps, ctx)
                finally:
                    ctx.set_option("batch_long_streams", 1)
            return timed
        # the built index is what compress would have written
        _, want_first, want_index = batch.compress(ctx, src, want_index=True)
        build()
        ctx.synchronize()
        assert torch.equal(first, want_first) and torch.equal(index, want_index)
        assert bool((status == 1).all())
        walked = ctx.info("index_build_walked")
        dec_indexed()
        pieced = ctx.info("index_streams_pieced")
        assert all(e[0] == 0 for e in batch.read_errors(berrs))
        for i in (0, n // 2, n - 1):
            assert back.stream_bytes(i, int(blens[i])) == datas[i]
        timers = {"build": lambda: time_it(build, args.steps, ctx),
                  "dec_long_streams_1": dec_plain(1),
                  "dec_long_streams_0": dec_plain(0),
                  "dec_indexed": lambda: time_it(dec_indexed, args.steps, ctx)}
        extra = {}
        if key == "text_256x1m":
            # every stream cut by a byte: CORRUPT, by the walker, to its end
            cut = batch.StreamBatch(comp.data, comp.offsets,
                                    [x - 1 for x in h_in])
            cut_in = [x - 1 for x in h_in]

            def build_cut():
                build(cut, cut_in)
            build_cut()
            ctx.synchronize()
            extra["cut_walked"] = ctx.info("index_build_walked")
            assert ctx.info("index_build_corrupt") == n
            timers["build_all_corrupt"] = lambda: time_it(build_cut,
                                                          args.steps, ctx)
            if has_test:
                def walker_alone():
                    ctx.set_test_option("index_build_route", 1)
                    try:
                        return time_it(build, args.steps, ctx)
                    finally:
                        ctx.set_test_option("index_build_route", 0)
                timers["walker_alone"] = walker_alone
        t = {k: [] for k in timers}
        for _ in range(repeats):
            for k, fn in timers.items():
                t[k].append(fn() * 1e3)
        build()   # (the last timed build may have been the cut one)
        ctx.synchronize()
        assert torch.equal(index, want_index)
        med = {k: statistics.median(v) for k, v in t.items()}
        gain1 = med["dec_long_streams_1"] - med["dec_indexed"]
        gain0 = med["dec_long_streams_0"] - med["dec_indexed"]
        res[key] = {
            "streams": n, "bytes": nbytes, "compressed_bytes": sum(h_in),
            "index_entries": entries, "index_build_walked": walked,
            "index_streams_pieced": pieced, **extra,
            "ms_median": {k: round(v, 4) for k, v in med.items()},
            "ms_spread": {k: round(max(v) - min(v), 4) for k, v in t.items()},
            "ms_repeats": {k: [round(x, 4) for x in v] for k, v in t.items()},
            "build_over_dec_long_streams_1": round(
                med["build"] / med["dec_long_streams_1"], 3),
            "decodes_to_pay_vs_long_streams_1":
                round(med["build"] / gain1, 2) if gain1 > 0 else None,
            "decodes_to_pay_vs_long_streams_0":
                round(med["build"] / gain0, 2) if gain0 > 0 else None}
    (ROOT / "profiles" / "raw_index_build.json").write_text(
        json.dumps(res) + "\n")
    return res


def raw_ranges(args, ctx, dev):
    """Range reads through the block index
    (snapmi_decompress_ranges_indexed) on 256 streams of 1 MiB of text with
    the index compress wrote: one 4 KiB range per stream, one aligned 64 KiB
    block per stream, every stream whole as one range - each against
    snapmi_decompress_batch_indexed of the same streams (slicing its output
    is free) - and, to say where a small read's time goes, one lone 4 KiB
    range and 256 empty ranges; in this process on one context, five
    alternating repeats of
    --steps calls each (medians, and the spread max - min over the repeats).
    Writes profiles/raw_ranges.json (--sets 4k,...: only these shapes, for a
    kernel trace; nothing is written)."""
    import random
    import statistics
    import oracle_lib as O
    from rust_snappy_amd import batch, raw
    text = b"".join((O.CORPUS / n).read_bytes()
                    for n in ("alice29.txt", "asyoulik.txt", "lcet10.txt",
                              "plrabn12.txt")) * 2
    rng = random.Random(0x5EED)
    n, size = 256, 1 << 20
    datas = []
    for _ in range(n):
        o = rng.randrange(len(text) - size)
        datas.append(text[o:o + size])
    src = batch.StreamBatch.from_bytes(datas, dev)
    comp, first, index = batch.compress(ctx, src, want_index=True)
    entries = index.numel()
    back = batch.StreamBatch.empty([size] * n, dev)
    blens = torch.zeros(n, dtype=torch.int64, device=dev)
    berrs = torch.zeros(32 * n, dtype=torch.uint8, device=dev)

    def dec_indexed():
        raw.decompress_batch(ctx, comp.d_ptrs, comp.d_lens, back.d_ptrs,
                             back.d_lens, blens, berrs, index_first=first,
                             index=index, index_entries=entries)
    shapes = {
        "4k": [(i, rng.randrange(size - 4096), 4096) for i in range(n)],
        "block_64k": [(i, 65536 * rng.randrange(16), 65536)
                      for i in range(n)],
        "whole": [(i, 0, size) for i in range(n)],
        # what a call costs whatever it reads: ONE 4 KiB range (one piece on
        # one wavefront behind the call's chain of launches), and 256 empty
        # ranges (the scan and the plan alone: nothing is decoded)
        "one_4k": [(n // 2, 300000, 4096)],
        "none": [(i, 0, 0) for i in range(n)]}
    if args.sets:  # (for a kernel trace of one shape; no record is written)
        shapes = {k: v for k, v in shapes.items()
                  if k in args.sets.split(",")}
    repeats = 5
    res = {"config": "raw_ranges: range reads through the block index vs "
                     "snapmi_decompress_batch_indexed of the same 256 "
                     "streams of 1 MiB of text",
           "steps": args.steps, "repeats": repeats, "streams": n,
           "bytes": n * size, "index_entries": entries}
    timers = {}
    if not args.sets:
        timers["dec_indexed"] = lambda: time_it(dec_indexed, args.steps, ctx)
    for key, ranges in shapes.items():
        offs, lens = [r[1] for r in ranges], [r[2] for r in ranges]
        dst = batch.StreamBatch.empty(lens, dev)
        d_stream = torch.tensor([r[0] for r in ranges],
                                dtype=torch.int32).to(dev)
        d_off = torch.tensor(offs, dtype=torch.int64).to(dev)
        d_len = torch.tensor(lens, dtype=torch.int64).to(dev)
        m = len(ranges)
        got = torch.zeros(m, dtype=torch.int64, device=dev)
        errs = torch.zeros(32 * m, dtype=torch.uint8, device=dev)

        def read(d_stream=d_stream, d_off=d_off, d_len=d_len, offs=offs,
                 lens=lens, dst=dst, got=got, errs=errs):
            raw.decompress_ranges_indexed(
                ctx, comp.d_ptrs, comp.d_lens, first, index, d_stream, d_off,
                d_len, offs, lens, dst.d_ptrs, got, errs,
                index_entries=entries)
        read()
        ctx.synchronize()
        assert all(e[0] == 0 for e in batch.read_errors(errs))
        assert got.cpu().tolist() == lens
        for r in (0, m // 2, m - 1):
            s, o, ln = ranges[r]
            assert dst.stream_bytes(r, ln) == datas[s][o:o + ln]
        res[key] = {"pieces": ctx.info("range_pieces"),
                    "bytes": sum(lens)}
        timers["ranges_" + key] = (lambda read=read:
                                   time_it(read, args.steps, ctx))
    t = {k: [] for k in timers}
    for _ in range(repeats):
        for k, fn in timers.items():
            t[k].append(fn() * 1e3)
    med = {k: statistics.median(v) for k, v in t.items()}
    res["ms_median"] = {k: round(v, 4) for k, v in med.items()}
    res["ms_spread"] = {k: round(max(v) - min(v), 4) for k, v in t.items()}
    res["ms_repeats"] = {k: [round(x, 4) for x in v] for k, v in t.items()}
    if not args.sets:
        for key in shapes:
            res[key]["over_dec_indexed"] = round(
                med["ranges_" + key] / med["dec_indexed"], 3)
        (ROOT / "profiles" / "raw_ranges.json").write_text(
            json.dumps(res) + "\n")
    return res


def raw_writes(args, ctx, dev):
    """Range writes through the block index (snapmi_write_ranges_indexed) on
    256 streams of 1 MiB of text with the index compress wrote: one 4 KiB
    write per stream, one aligned 64 KiB block per stream, sixteen 4 KiB
    writes per stream (every block touched) - each beside the whole-stream
    way to the same edit: snapmi_decompress_batch_indexed of the streams, a
    device copy of the new bytes into the output, and
    snapmi_compress_batch_indexed of the result; in this process on one
    context, five alternating repeats of --steps calls each (medians, and the
    spread max - min over the repeats).  Writes profiles/raw_writes.json
    (--sets 4k,16x4k:write,...: only these shapes, only that way - for a
    kernel trace; nothing is written)."""
    import random
    import statistics
    import oracle_lib as O
    from rust_snappy_amd import batch, raw
    text = b"".join((O.CORPUS / n).read_bytes()
                    for n in ("alice29.txt", "asyoulik.txt", "lcet10.txt",
                              "plrabn12.txt")) * 2
    rng = random.Random(0x5EED)
    n, size = 256, 1 << 20
    datas = []
    for _ in range(n):
        o = rng.randrange(len(text) - size)
        datas.append(text[o:o + size])
    src = batch.StreamBatch.from_bytes(datas, dev)
    comp, first, index = batch.compress(ctx, src, want_index=True)
    entries = index.numel()
    h_size = torch.full((n,), size, dtype=torch.int64)
    # the whole-stream way's buffers: the decoded streams, the streams
    # compressed again, their index
    back = batch.StreamBatch.empty([size] * n, dev)
    blens = torch.zeros(n, dtype=torch.int64, device=dev)
    berrs = torch.zeros(32 * n, dtype=torch.uint8, device=dev)
    cap = raw.max_compress_len(size)
    again = batch.StreamBatch.empty([cap] * n, dev)
    alens = torch.zeros(n, dtype=torch.int64, device=dev)
    afirst = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    aindex = torch.zeros(entries, dtype=torch.int64, device=dev)
    # the write way's buffers
    out = batch.StreamBatch.empty([cap] * n, dev)
    olens = torch.zeros(n, dtype=torch.int64, device=dev)
    oerrs = torch.zeros(32 * n, dtype=torch.uint8, device=dev)
    oindex = torch.zeros(entries, dtype=torch.int64, device=dev)
    shapes = {
        "4k": [(i, rng.randrange(size - 4096), 4096) for i in range(n)],
        "block_64k": [(i, 65536 * rng.randrange(16), 65536)
                      for i in range(n)],
        "16x4k": [(i, 65536 * k + rng.randrange(65536 - 4096), 4096)
                  for i in range(n) for k in range(16)]}
    # (--sets 4k:write / 4k:whole - for a kernel trace of one way to one
    # shape; no record is written)
    ways = ("write", "whole")
    if args.sets:
        picked = [x.partition(":") for x in args.sets.split(",")]
        shapes = {k: v for k, v in shapes.items()
                  if k in [x[0] for x in picked]}
        ways = tuple(w for w in ways
                     if any(x[2] in ("", w) for x in picked))
    repeats = 5
    res = {"config": "raw_writes: range writes through the block index vs "
                     "decode whole + copy + compress whole of the same 256 "
                     "streams of 1 MiB of text",
           "steps": args.steps, "repeats": repeats, "streams": n,
           "bytes": n * size, "index_entries": entries}
    timers = {}
    for key, writes in shapes.items():
        m = len(writes)
        # new bytes: text from elsewhere, one slab, a source per write
        news = []
        for _, _, ln in writes:
            o = rng.randrange(len(text) - ln)
            news.append(text[o:o + ln])
        wsrc = batch.StreamBatch.from_bytes(news, dev)
        w_stream = [w[0] for w in writes]
        w_off, w_len = [w[1] for w in writes], [w[2] for w in writes]
        w_ptrs = [int(p) for p in wsrc.d_ptrs.cpu().tolist()]
        # (the whole-stream way's copy: one index_copy_ of all new bytes)
        new_flat = torch.from_numpy(
            np.frombuffer(b"".join(news), dtype=np.uint8).copy()).to(dev)
        new_at = torch.cat([torch.arange(ln, dtype=torch.int64)
                            + (int(back.offsets[s]) + o)
                            for s, o, ln in writes]).to(dev)
        side = torch.cuda.ExternalStream(ctx.stream) if ctx.stream \
            else torch.cuda.default_stream(dev)

        def write(w_stream=w_stream, w_off=w_off, w_len=w_len,
                  w_ptrs=w_ptrs):
            raw.write_ranges_indexed(
                ctx, comp.d_ptrs, comp.d_lens, first, index, w_stream, w_off,
                w_len, w_ptrs, out.d_ptrs, out.d_lens, olens, oerrs, oindex,
                index_entries=entries)

        def whole(new_flat=new_flat, new_at=new_at):
            raw.decompress_batch(ctx, comp.d_ptrs, comp.d_lens, back.d_ptrs,
                                 back.d_lens, blens, berrs, index_first=first,
                                 index=index, index_entries=entries)
            with torch.cuda.stream(side):  # (the context's stream)
                back.data.index_copy_(0, new_at, new_flat)
            raw.compress_batch(ctx, back.d_ptrs, back.d_lens, again.d_ptrs,
                               again.d_lens, alens, None, host_in_lens=h_size,
                               index_first=afirst, index=aindex,
                               index_cap=entries)
        write()
        whole()
        ctx.synchronize()
        torch.cuda.synchronize()
        assert all(e[0] == 0 for e in batch.read_errors(oerrs))
        # both ways give the same streams and the same index
        assert torch.equal(olens, alens) and torch.equal(oindex, aindex)
        for i in (0, n // 2, n - 1):
            assert out.stream_bytes(i, int(olens[i])) == \
                again.stream_bytes(i, int(alens[i]))
        res[key] = {"writes": m, "bytes": sum(w_len),
                    "write_blocks": ctx.info("write_blocks"),
                    "write_blocks_decoded": ctx.info("write_blocks_decoded")}
        if "write" in ways:
            timers["write_" + key] = (lambda write=write:
                                      time_it(write, args.steps, ctx))
        if "whole" in ways:
            timers["whole_" + key] = (lambda whole=whole:
                                      time_it(whole, args.steps, ctx))
    t = {k: [] for k in timers}
    for _ in range(repeats):
        for k, fn in timers.items():
            t[k].append(fn() * 1e3)
    med = {k: statistics.median(v) for k, v in t.items()}
    res["ms_median"] = {k: round(v, 4) for k, v in med.items()}
    res["ms_spread"] = {k: round(max(v) - min(v), 4) for k, v in t.items()}
    res["ms_repeats"] = {k: [round(x, 4) for x in v] for k, v in t.items()}
    if not args.sets:
        for key in shapes:
            res[key]["over_whole"] = round(
                med["write_" + key] / med["whole_" + key], 3)
        (ROOT / "profiles" / "raw_writes.json").write_text(
            json.dumps(res) + "\n")
    return res


def raw_appends(args, ctx, dev):
    """Appends through the block index (snapmi_append_indexed) on the 256
    streams of 1 MiB of text of raw_writes, with the index compress wrote:
    4 KiB per stream (the streams are block-aligned: no tail is decoded), the
    same with the streams cut to 1 MiB - 1000 bytes (every tail is decoded),
    64 KiB per stream, 1 MiB per stream - each beside the whole-stream way to
    the same result: snapmi_decompress_batch_indexed of the streams, a device
    copy of the new bytes behind them, and snapmi_compress_batch_indexed of
    the concatenation; in this process on one context, five alternating
    repeats of --steps calls each (medians, and the spread max - min over the
    repeats).  Writes profiles/raw_appends.json (--sets 4k,1m:append,...: only
    these shapes, only that way - for a kernel trace; nothing is written)."""
    import random
    import statistics
    import oracle_lib as O
    from rust_snappy_amd import batch, raw
    text = b"".join((O.CORPUS / n).read_bytes()
                    for n in ("alice29.txt", "asyoulik.txt", "lcet10.txt",
                              "plrabn12.txt")) * 2
    rng = random.Random(0x5EED)
    n, size = 256, 1 << 20
    datas = []
    for _ in range(n):
        o = rng.randrange(len(text) - size)
        datas.append(text[o:o + size])
    # shape: (old length of every stream, bytes appended to each)
    shapes = {"4k": (size, 4096), "4k_tail": (size - 1000, 4096),
              "64k": (size, 65536), "1m": (size, size)}
    ways = ("append", "whole")
    if args.sets:
        picked = [x.partition(":") for x in args.sets.split(",")]
        shapes = {k: v for k, v in shapes.items()
                  if k in [x[0] for x in picked]}
        ways = tuple(w for w in ways
                     if any(x[2] in ("", w) for x in picked))
    repeats = 5
    res = {"config": "raw_appends: appends through the block index vs decode "
                     "whole + copy + compress whole of the same 256 streams "
                     "of 1 MiB of text",
           "steps": args.steps, "repeats": repeats, "streams": n}
    side = torch.cuda.ExternalStream(ctx.stream) if ctx.stream \
        else torch.cuda.default_stream(dev)
    timers, olds = {}, {}
    for key, (old, add) in shapes.items():
        if old not in olds:
            src = batch.StreamBatch.from_bytes([d[:old] for d in datas], dev)
            olds[old] = batch.compress(ctx, src, want_index=True)
        comp, first, index = olds[old]
        entries = index.numel()
        new_len = old + add
        h_old = [old] * n
        news = []
        for _ in range(n):
            o = rng.randrange(len(text) - add)
            news.append(text[o:o + add])
        asrc = batch.StreamBatch.from_bytes(news, dev)
        a_ptrs = [int(p) for p in asrc.d_ptrs.cpu().tolist()]
        a_lens = [add] * n
        new_entries = raw.block_index_entries([new_len] * n)
        cap = raw.max_compress_len(new_len)
        # the append way's buffers
        out = batch.StreamBatch.empty([cap] * n, dev)
        olens = torch.zeros(n, dtype=torch.int64, device=dev)
        oerrs = torch.zeros(32 * n, dtype=torch.uint8, device=dev)
        ofirst = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        oindex = torch.zeros(new_entries, dtype=torch.int64, device=dev)
        # the whole-stream way's buffers: the decoded streams with room for
        # the new bytes, the concatenations compressed, their index
        back = batch.StreamBatch.empty([new_len] * n, dev)
        blens = torch.zeros(n, dtype=torch.int64, device=dev)
        berrs = torch.zeros(32 * n, dtype=torch.uint8, device=dev)
        again = batch.StreamBatch.empty([cap] * n, dev)
        alens = torch.zeros(n, dtype=torch.int64, device=dev)
        afirst = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        aindex = torch.zeros(new_entries, dtype=torch.int64, device=dev)
        h_new = torch.full((n,), new_len, dtype=torch.int64)
        # (the whole-stream way's copy: one strided copy of all new bytes -
        # the streams of `back` lie a fixed stride apart)
        new_rows = torch.from_numpy(
            np.frombuffer(b"".join(news), dtype=np.uint8).copy()).to(
                dev).view(n, add)
        stride = int(back.offsets[1])
        assert list(back.offsets) == [i * stride for i in range(n)]
        behind = back.data[:n * stride].view(n, stride)[:, old:new_len]

        def append(comp=comp, first=first, index=index, entries=entries,
                   h_old=h_old, a_ptrs=a_ptrs, a_lens=a_lens, out=out,
                   olens=olens, oerrs=oerrs, ofirst=ofirst, oindex=oindex,
                   new_entries=new_entries):
            raw.append_indexed(
                ctx, comp.d_ptrs, comp.d_lens, h_old, first, index, a_ptrs,
                a_lens, out.d_ptrs, out.d_lens, olens, oerrs, ofirst, oindex,
                index_entries=entries, new_index_cap=new_entries)

        def whole(comp=comp, first=first, index=index, entries=entries,
                  back=back, blens=blens, berrs=berrs, again=again,
                  alens=alens, afirst=afirst, aindex=aindex, h_new=h_new,
                  new_rows=new_rows, behind=behind, new_entries=new_entries):
            raw.decompress_batch(ctx, comp.d_ptrs, comp.d_lens, back.d_ptrs,
                                 back.d_lens, blens, berrs, index_first=first,
                                 index=index, index_entries=entries)
            with torch.cuda.stream(side):  # (the context's stream)
                behind.copy_(new_rows)
            raw.compress_batch(ctx, back.d_ptrs, back.d_lens, again.d_ptrs,
                               again.d_lens, alens, None, host_in_lens=h_new,
                               index_first=afirst, index=aindex,
                               index_cap=new_entries)
        append()
        whole()
        ctx.synchronize()
        torch.cuda.synchronize()
        assert all(e[0] == 0 for e in batch.read_errors(oerrs))
        # both ways give the same streams and the same index
        assert torch.equal(olens, alens) and torch.equal(oindex, aindex)
        assert torch.equal(ofirst, afirst)
        for i in (0, n // 2, n - 1):
            assert out.stream_bytes(i, int(olens[i])) == \
                again.stream_bytes(i, int(alens[i]))
        res[key] = {"old_bytes": old, "appended_bytes": add,
                    "append_blocks": ctx.info("append_blocks"),
                    "append_blocks_decoded":
                        ctx.info("append_blocks_decoded")}
        if "append" in ways:
            timers["append_" + key] = (lambda append=append:
                                       time_it(append, args.steps, ctx))
        if "whole" in ways:
            timers["whole_" + key] = (lambda whole=whole:
                                      time_it(whole, args.steps, ctx))
    t = {k: [] for k in timers}
    for _ in range(repeats):
        for k, fn in timers.items():
            t[k].append(fn() * 1e3)
    med = {k: statistics.median(v) for k, v in t.items()}
    res["ms_median"] = {k: round(v, 4) for k, v in med.items()}
    res["ms_spread"] = {k: round(max(v) - min(v), 4) for k, v in t.items()}
    res["ms_repeats"] = {k: [round(x, 4) for x in v] for k, v in t.items()}
    if not args.sets:
        for key in shapes:
            res[key]["over_whole"] = round(
                med["append_" + key] / med["whole_" + key], 3)
        (ROOT / "profiles" / "raw_appends.json").write_text(
            json.dumps(res) + "\n")
    return res


class HostArena:
    """buffers of the given sizes, 64 bytes apart at least, in one
    pageable array or one snapmi_host_alloc allocation"""

    def __init__(self, sizes, pinned):
        sizes = np.asarray(sizes, dtype=np.uint64)
        step = (sizes + np.uint64(127)) // np.uint64(64) * np.uint64(64)
        self.offs = np.concatenate(([0], np.cumsum(step)[:-1])).astype(
            np.uint64)
        total = int(step.sum()) + 64
        from rust_snappy_amd import frame
        self.host = frame.HostBuffer(total) if pinned else None
        self.arr = self.host.array if pinned \
            else np.zeros(total, dtype=np.uint8)
        self.arr[:] = 0
        self.ptrs = self.offs + np.uint64(self.arr.ctypes.data)
        self.sizes = sizes

    def fill(self, datas):
        for o, d in zip(self.offs, datas):
            self.arr[int(o):int(o) + len(d)] = np.frombuffer(
                d, dtype=np.uint8)

    def bytes(self, i, n):
        o = int(self.offs[i])
        return self.arr[o:o + int(n)].tobytes()

    def close(self):
        if self.host is not None:
            self.arr = None
            self.host.close()


def host_batch(args, ctx, dev):
    """Many raw streams in HOST memory per call (snapmi_compress_batch_host /
    snapmi_decompress_batch_host) from pageable and from pinned buffers,
    against a loop of snapmi_raw_compress / snapmi_raw_decompress over the
    same buffers (timed on the first `loop_streams` streams and scaled), the
    device-resident batch calls on the same data (the kernel floor) and the
    host-to-host rate of `pcie` (the link floor).  Three sets: 4 096 streams
    of 16 KiB of corpus text, 65 536 of 4 KiB, 512 of 100 B .. 1 MiB
    (log-uniform).  Then the sweeps the defaults were chosen from: the slice
    size, and - with the test build (SNAPMI_TESTING=1) - the direct-copy
    threshold and where k_hb_pack stores."""
    import random
    import oracle_lib as O
    from rust_snappy_amd import _lib, batch, frame, raw
    text = b"".join((O.CORPUS / n).read_bytes()
                    for n in ("alice29.txt", "asyoulik.txt", "lcet10.txt",
                              "plrabn12.txt")) * 2
    rng = random.Random(0x5EED)

    def piece(n):
        o = rng.randrange(len(text) - n)
        return text[o:o + n]
    sets = {"text_4096x16k": [piece(16384) for _ in range(4096)],
            "text_65536x4k": [piece(4096) for _ in range(65536)],
            "mixed_512_100b_1m": [piece(int(100 * (10486 ** rng.random())))
                                  for _ in range(512)]}
    L = _lib.of(ctx)
    has_test = hasattr(L, "snapmi_ctx_set_test_option")

    Arena = HostArena

    def measure(datas, pinned, steps):
        n = len(datas)
        lens = np.array([len(d) for d in datas], dtype=np.uint64)
        caps = np.array([raw.max_compress_len(len(d)) for d in datas],
                        dtype=np.uint64)
        src, comp, back = Arena(lens, pinned), Arena(caps, pinned), \
            Arena(lens, pinned)
        src.fill(datas)
        state = {}

        def enc():
            state["clens"], state["errs"] = raw.batch_host(
                ctx, True, src.ptrs, lens, comp.ptrs, caps)
        enc()
        assert not state["errs"]["kind"].any()
        clens = state["clens"]
        for i in (0, n // 2, n - 1):
            assert comp.bytes(i, clens[i]) == O.compress(datas[i])
        info = {k: ctx.info("host_batch_" + k)
                for k in ("slices", "h2d_bytes", "d2h_bytes")}

        def dec():
            state["blens"], state["errs"] = raw.batch_host(
                ctx, False, comp.ptrs, clens, back.ptrs, lens)
        dec()
        assert not state["errs"]["kind"].any()
        assert np.array_equal(state["blens"], lens)
        assert np.array_equal(back.arr, src.arr), "host batch round trip"
        out = {"compress_ms": time_it(enc, steps, ctx) * 1e3,
               "decompress_ms": time_it(dec, steps, ctx) * 1e3,
               "compress_info": info, "compressed_bytes": int(clens.sum())}
        keep = (src, comp, back, lens, caps, clens)
        return out, keep

    def loop_of_scalar_calls(keep, k):
        src, comp, back, lens, caps, clens = keep
        w, err = C.c_size_t(0), _lib.SnapmiError()
        a = [(int(src.ptrs[i]), int(lens[i]), int(comp.ptrs[i]), int(caps[i]),
              int(clens[i]), int(back.ptrs[i])) for i in range(k)]

        def s_enc():
            for sp, sl, cp, cc, _, _ in a:
                L.snapmi_raw_compress(ctx._h, C.c_char_p(sp), sl, cp, cc,
                                      C.byref(w), C.byref(err))

        def s_dec():
            for sp, sl, cp, cc, cl, bp in a:
                L.snapmi_raw_decompress(ctx._h, C.c_char_p(cp), cl, bp, sl,
                                        C.byref(w), C.byref(err))
        return time_it(s_enc, 1, ctx), time_it(s_dec, 1, ctx)

    import ctypes as C
    res = {"config": "host_batch: n raw streams in host memory per call vs a "
                     "loop of scalar calls, the device-resident batch and "
                     "the link", "steps": args.steps,
           "defaults": {"host_batch_slice": 16 << 20,
                        "host_batch_direct_min": 1 << 20,
                        "host_batch_pack_to_host": 1}}
    try:
        gib = args.gib
        args.gib = 0.5
        link = pcie(args, ctx, dev)
        args.gib = gib
        res["link_floor_pcie"] = {k: link[k] for k in (
            "gib", "frame_encode_gibs", "frame_decode_gibs")}
    except Exception as e:  # noqa: BLE001 - reported, not hidden
        res["link_floor_pcie"] = {"error": f"{type(e).__name__}: {e}"[:200]}
    for key, datas in sets.items():
        n = len(datas)
        nbytes = sum(len(d) for d in datas)
        row = {"streams": n, "bytes": nbytes}
        for pinned in (False, True):
            out, keep = measure(datas, pinned, args.steps)
            name = "pinned" if pinned else "pageable"
            row[name] = {
                "compress_ms": round(out["compress_ms"], 3),
                "decompress_ms": round(out["decompress_ms"], 3),
                "compress_gibs": round(nbytes / GIB / out["compress_ms"] * 1e3,
                                       2),
                "decompress_gibs": round(
                    nbytes / GIB / out["decompress_ms"] * 1e3, 2)}
            row["compressed_bytes"] = out["compressed_bytes"]
            row["compress_info"] = out["compress_info"]
            if not pinned:
                k = min(n, 1024)
                te, td = loop_of_scalar_calls(keep, k)
                row["scalar_loop"] = {
                    "loop_streams": k,
                    "call_us": {"compress": round(te / k * 1e6, 1),
                                "decompress": round(td / k * 1e6, 1)},
                    "ms_for_all": {"compress": round(te / k * n * 1e3, 1),
                                   "decompress": round(td / k * n * 1e3, 1)}}
                row["host_batch_over_scalar_loop_speedup"] = {
                    "compress": round(te / k * n * 1e3 / out["compress_ms"], 1),
                    "decompress": round(
                        td / k * n * 1e3 / out["decompress_ms"], 1)}
            for a in keep[:3]:
                a.close()
        # the kernel floor: the same streams, device resident
        src = batch.StreamBatch.from_bytes(datas, dev)
        rout = batch.StreamBatch.empty(
            [raw.max_compress_len(len(d)) for d in datas], dev)
        rlens = torch.zeros(n, dtype=torch.int64, device=dev)
        rback = batch.StreamBatch.empty([len(d) for d in datas], dev)
        rblens = torch.zeros(n, dtype=torch.int64, device=dev)

        def r_enc():
            raw.compress_batch(ctx, src.d_ptrs, src.d_lens, rout.d_ptrs,
                               rout.d_lens, rlens, None,
                               host_in_lens=src.h_lens)

        def r_dec():
            raw.decompress_batch(ctx, rout.d_ptrs, rlens, rback.d_ptrs,
                                 rback.d_lens, rblens, None)
        r_enc()
        ctx.synchronize()
        te, td = time_it(r_enc, args.steps, ctx), time_it(r_dec, args.steps,
                                                          ctx)
        assert rback.stream_bytes(n - 1) == datas[n - 1]
        row["device_resident_batch"] = {
            "compress_ms": round(te * 1e3, 3),
            "decompress_ms": round(td * 1e3, 3),
            "compress_gibs": round(nbytes / GIB / te, 2),
            "decompress_gibs": round(nbytes / GIB / td, 2)}
        del src, rout, rback
        res[key] = row

    # the sweeps behind the defaults (pinned buffers; two steps each)
    def sweep(datas, pinned, setter, values):
        out = {}
        for v in values:
            setter(v)
            m, keep = measure(datas, pinned, 2)
            out[str(v)] = {"compress_ms": round(m["compress_ms"], 3),
                           "decompress_ms": round(m["decompress_ms"], 3)}
            for a in keep[:3]:
                a.close()
        return out
    sw = {}
    for key in ("text_4096x16k", "text_65536x4k"):
        sw["host_batch_slice/" + key] = sweep(
            sets[key], True, lambda v: ctx.set_option("host_batch_slice", v),
            [1 << 20, 4 << 20, 16 << 20, 64 << 20])
    ctx.set_option("host_batch_slice", 16 << 20)
    if has_test:
        for pinned in (False, True):
            sw["host_batch_direct_min/mixed_512_100b_1m/" +
               ("pinned" if pinned else "pageable")] = sweep(
                sets["mixed_512_100b_1m"], pinned,
                lambda v: ctx.set_test_option("host_batch_direct_min", v),
                [64 << 10, 256 << 10, 1 << 20, 1 << 40])
        ctx.set_test_option("host_batch_direct_min", 1 << 20)
        for key in ("text_4096x16k", "text_65536x4k"):
            sw["host_batch_pack_to_host/" + key] = sweep(
                sets[key], True,
                lambda v: ctx.set_test_option("host_batch_pack_to_host", v),
                [0, 1])
        ctx.set_test_option("host_batch_pack_to_host", 1)
    else:
        sw["host_batch_direct_min"] = sw["host_batch_pack_to_host"] = \
            "test options: run with SNAPMI_TESTING=1"
    res["sweeps"] = sw
    return res


def frames_host_batch(args, ctx, dev):
    """Many FRAMED streams in HOST memory per call
    (snapmi_frame_compress_batch_host / snapmi_frame_decompress_batch_host)
    from pageable and from pinned buffers, against a loop of
    snapmi_frame_encode_host / snapmi_frame_decode_host one-stream calls over
    the same buffers (timed on the first streams and scaled), the raw host
    batch calls on the same payload, and - with the test build
    (SNAPMI_TESTING=1) - the decode from the host's chunk list against the
    device's walk (host_batch_listed 1 / 0, three repeats each: their spread
    is the noise the difference is read against).  The sets of host_batch
    and 64 streams of 16 MiB (256 chunks each), where the walk matters."""
    import ctypes as C
    import random
    import oracle_lib as O
    from rust_snappy_amd import _lib, frame, raw
    text = b"".join((O.CORPUS / n).read_bytes()
                    for n in ("alice29.txt", "asyoulik.txt", "lcet10.txt",
                              "plrabn12.txt")) * 2
    rng = random.Random(0x5EED)

    def piece(n):
        o = rng.randrange(len(text) - n)
        return text[o:o + n]

    def long_piece(n):
        return b"".join(piece(1 << 20) for _ in range(n >> 20))
    sets = {"text_4096x16k": [piece(16384) for _ in range(4096)],
            "text_65536x4k": [piece(4096) for _ in range(65536)],
            "mixed_512_100b_1m": [piece(int(100 * (10486 ** rng.random())))
                                  for _ in range(512)],
            "text_64x16m": [long_piece(16 << 20) for _ in range(64)]}
    only = getattr(args, "sets", "")
    L = _lib.of(ctx)
    has_test = hasattr(L, "snapmi_ctx_set_test_option")
    res = {"config": "frames_host_batch: n framed streams in host memory per "
                     "call vs a loop of one-stream host calls, the raw host "
                     "batch, and listed vs walked decode",
           "steps": args.steps}
    for key, datas in sets.items():
        if only and key not in only.split(","):
            continue
        n = len(datas)
        nbytes = sum(len(d) for d in datas)
        row = {"streams": n, "bytes": nbytes}
        lens = np.array([len(d) for d in datas], dtype=np.uint64)
        fcaps = np.array([frame.frame_max_len(len(d)) for d in datas],
                         dtype=np.uint64)
        rcaps = np.array([raw.max_compress_len(len(d)) for d in datas],
                         dtype=np.uint64)
        for pinned in (False, True):
            src, comp, back = HostArena(lens, pinned), \
                HostArena(fcaps, pinned), HostArena(lens, pinned)
            src.fill(datas)
            st = {}

            def enc():
                st["clens"], st["errs"] = frame.batch_host(
                    ctx, True, src.ptrs, lens, comp.ptrs, fcaps)
            enc()
            assert not st["errs"]["kind"].any()
            clens = st["clens"]
            for i in (0, n - 1):
                if len(datas[i]) <= 1 << 20:
                    assert comp.bytes(i, clens[i]) == O.frame_compress(datas[i])

            def dec():
                st["blens"], st["errs"] = frame.batch_host(
                    ctx, False, comp.ptrs, clens, back.ptrs, lens)
            dec()
            assert not st["errs"]["kind"].any()
            assert np.array_equal(st["blens"], lens)
            assert np.array_equal(back.arr, src.arr), "round trip"
            info = {k: ctx.info("host_batch_" + k)
                    for k in ("slices", "listed_slices", "h2d_bytes",
                              "d2h_bytes")}
            out = {"compress_ms": round(time_it(enc, args.steps, ctx) * 1e3, 3),
                   "decompress_ms": round(time_it(dec, args.steps, ctx) * 1e3,
                                          3),
                   "decompress_info": info}
            if has_test:
                rep = {}
                for listed in (1, 0, 1, 0, 1, 0):
                    ctx.set_test_option("host_batch_listed", listed)
                    rep.setdefault(str(listed), []).append(
                        round(time_it(dec, args.steps, ctx) * 1e3, 3))
                ctx.set_test_option("host_batch_listed", 1)
                noise = max(max(v) - min(v) for v in rep.values())
                out["decompress_ms_by_host_batch_listed"] = rep
                out["listed_noise_ms"] = round(noise, 3)
                out["walked_minus_listed_ms"] = round(
                    sorted(rep["0"])[1] - sorted(rep["1"])[1], 3)
            # the raw host batch on the same payload
            rcomp = HostArena(rcaps, pinned)

            def r_enc():
                st["rlens"], st["errs"] = raw.batch_host(
                    ctx, True, src.ptrs, lens, rcomp.ptrs, rcaps)
            r_enc()
            rlens = st["rlens"]

            def r_dec():
                raw.batch_host(ctx, False, rcomp.ptrs, rlens, back.ptrs, lens)
            if int(lens.max()) <= 0xFFFFFFFF:
                out["raw_host_batch_ms"] = {
                    "compress": round(time_it(r_enc, args.steps, ctx) * 1e3, 3),
                    "decompress": round(time_it(r_dec, args.steps, ctx) * 1e3,
                                        3)}
            if not pinned:
                # a loop of one-stream calls, on the first streams
                k = min(n, 256)
                w, got, err = C.c_size_t(0), C.c_size_t(0), _lib.SnapmiError()
                chunk_lens = [np.array(
                    [min(65536, len(d) - o) for o in range(0, len(d), 65536)],
                    dtype=np.uint32) for d in datas[:k]]

                # (the one-stream decoder wants room for whole chunks)
                back1 = HostArena(np.maximum(lens[:k], 65536), False)

                def s_enc():
                    for i in range(k):
                        L.snapmi_frame_encode_host(
                            ctx._h, C.c_void_p(int(src.ptrs[i])),
                            chunk_lens[i].ctypes.data_as(C.c_void_p),
                            len(chunk_lens[i]), 0,
                            C.c_void_p(int(comp.ptrs[i])), int(fcaps[i]),
                            C.byref(w))

                def s_dec():
                    for i in range(k):
                        L.snapmi_frame_decode_host(
                            ctx._h, C.c_void_p(int(comp.ptrs[i])),
                            int(clens[i]), 2, None,
                            C.c_void_p(int(back1.ptrs[i])),
                            int(back1.sizes[i]), C.byref(w), C.byref(got),
                            C.byref(err))
                te, td = time_it(s_enc, 1, ctx), time_it(s_dec, 1, ctx)
                out["one_stream_loop"] = {
                    "loop_streams": k,
                    "ms_for_all": {"compress": round(te / k * n * 1e3, 1),
                                   "decompress": round(td / k * n * 1e3, 1)},
                    "speedup": {
                        "compress": round(te / k * n * 1e3 / out["compress_ms"],
                                          1),
                        "decompress": round(
                            td / k * n * 1e3 / out["decompress_ms"], 1)}}
            row["pinned" if pinned else "pageable"] = out
            for a in (src, comp, back, rcomp):
                a.close()
        res[key] = row
    return res


def crc(args, ctx, dev):
    """Masked CRC32C on the device (snapmi_crc32c_masked_batch) over random
    bytes: 16 384 buffers of 64 KiB (one wavefront a buffer: the route of the
    frame codec's chunks), the same 1 GiB as one buffer and as 16 buffers of
    64 MiB (cut into segments that the whole device shares), and 512 buffers
    of 100 B .. 4 MiB mixed.  Five alternating repeats of 20 calls each
    (medians, and the spread max - min over the repeats); beside each shape
    the CPU codec's rate on the same bytes.  With SNAPMI_PARENT_LIB=<another
    build of libsnapmi.so> the first shape - all that an older build can do -
    is timed through that build as well, in this process, in turn with this
    one: the yardstick.  Writes profiles/crc_long.json."""
    import os
    import random
    import statistics
    import oracle_lib as O
    from rust_snappy_amd import _lib, frame, raw
    steps, repeats = 20, 5
    rng = random.Random(0x5EED)
    torch.manual_seed(0x5EED)
    gib = torch.randint(0, 256, (1 << 30,), dtype=torch.uint8, device=dev)
    mixed_lens = [int(100 * (41943.04 ** rng.random())) for _ in range(512)]
    mixed_offs = np.concatenate([[0], np.cumsum(mixed_lens)]).astype(np.int64)
    assert int(mixed_offs[-1]) <= gib.numel()
    base = gib.data_ptr()
    shapes = {
        "short_16384x64k": ([base + (i << 16) for i in range(16384)],
                            [1 << 16] * 16384),
        "one_1g": ([base], [1 << 30]),
        "long_16x64m": ([base + (i << 26) for i in range(16)], [1 << 26] * 16),
        "mixed_512_100b_4m": ([base + int(o) for o in mixed_offs[:-1]],
                              mixed_lens),
    }
    host = gib.cpu().numpy()
    parent = None
    if os.environ.get("SNAPMI_PARENT_LIB"):
        parent = raw.Context(ctx.device, lib=_lib._open(
            Path(os.environ["SNAPMI_PARENT_LIB"])))
    res = {"config": "crc: snapmi_crc32c_masked_batch, random bytes",
           "steps": steps, "repeats": repeats,
           "segment_bytes": frame.CRC_SEGMENT}
    try:
        for key, (ptrs, lens) in shapes.items():
            n, nbytes = len(lens), sum(lens)
            d_ptrs = torch.tensor(ptrs, dtype=torch.int64, device=dev)
            d_lens = torch.tensor(lens, dtype=torch.int64, device=dev)
            out = torch.zeros(n, dtype=torch.int32, device=dev)
            torch.cuda.synchronize()

            def run(c):
                return lambda: frame.crc32c_masked_ptrs(c, d_ptrs, d_lens, out)
            run(ctx)()
            ctx.synchronize()
            got = [int(v) & 0xFFFFFFFF for v in out.cpu().tolist()]
            # the CPU codec on the same bytes: its rate, and the check (every
            # buffer of the long shapes, a sample of the others)
            sample = range(n) if n <= 16 else random.Random(1).sample(
                range(n), 64)
            t0, cpu_bytes = time.perf_counter(), 0
            for i in sample:
                o = ptrs[i] - base
                assert got[i] == O.crc32c_masked(host[o:o + lens[i]]), (key, i)
                cpu_bytes += lens[i]
            cpu_s = time.perf_counter() - t0
            timers = {"this": lambda: time_it(run(ctx), steps, ctx)}
            if parent is not None and key == "short_16384x64k":
                timers["parent"] = lambda: time_it(run(parent), steps, parent)
            t = {k: [] for k in timers}
            for _ in range(repeats):
                for k, fn in timers.items():
                    t[k].append(fn() * 1e3)
            med = {k: statistics.median(v) for k, v in t.items()}
            res[key] = {
                "buffers": n, "bytes": nbytes,
                "ms_median": {k: round(v, 4) for k, v in med.items()},
                "ms_spread": {k: round(max(v) - min(v), 4)
                              for k, v in t.items()},
                "ms_repeats": {k: [round(x, 4) for x in v]
                               for k, v in t.items()},
                "gibs": {k: round(nbytes / GIB / (v / 1e3), 1)
                         for k, v in med.items()},
                "cpu_codec_gibs": round(cpu_bytes / GIB / cpu_s, 3)}
    finally:
        if parent is not None:
            parent.close()
    (ROOT / "profiles" / "crc_long.json").write_text(json.dumps(res) + "\n")
    return res


def frame_nowait(args, ctx, dev):
    """snapmi_frame_decompress_ex with SNAPMI_FRAME_NO_WAIT against the call
    without the flag, on this build and - with SNAPMI_PARENT_LIB=<the parent
    commit's libsnapmi.so> - on the parent's, in this process, in turn:
    (a) 4 096 framed streams of 16 KiB of text, decoded by a loop of
    one-stream calls with one wait at the end; (b) one 1 GiB framed text
    stream, with its index and without (bound exact); (c) the same without
    an index under a bound of four times the count, beside the scratch the
    context then holds.  Five alternating repeats (medians, and the spread
    max - min over the repeats).  Writes profiles/frame_nowait.json."""
    import ctypes as C
    import os
    import statistics
    from rust_snappy_amd import _lib, frame, raw
    repeats = 5
    V = C.c_void_p
    parent = None
    if os.environ.get("SNAPMI_PARENT_LIB"):
        parent = raw.Context(ctx.device, lib=_lib._open(
            Path(os.environ["SNAPMI_PARENT_LIB"])))
    res = {"config": "frame_nowait: SNAPMI_FRAME_NO_WAIT against the "
                     "unflagged call, synthetic text", "repeats": repeats,
           "parent": parent is not None}

    def timed(timers):
        t = {k: [] for k in timers}
        for _ in range(repeats):
            for k, fn in timers.items():
                t[k].append(fn() * 1e3)
        med = {k: statistics.median(v) for k, v in t.items()}
        return med, {
            "ms_median": {k: round(v, 3) for k, v in med.items()},
            "ms_spread": {k: round(max(v) - min(v), 3) for k, v in t.items()},
            "ms_repeats": {k: [round(x, 3) for x in v] for k, v in t.items()}}

    def decode(c, d_in, n_in, out, cap, out_len, err, idx, n_chunks, flags):
        rc = c._L.snapmi_frame_decompress_ex(c._h, d_in, n_in, out, cap,
                                             out_len, err, idx, n_chunks,
                                             flags, None)
        if rc:
            raw._raise(c, rc)

    try:
        # (a) many small streams, one call each
        n, piece = 4096, 16 << 10
        text = synth_text(dev, n * piece)
        cap = frame.frame_max_len(piece)
        mid = torch.zeros(n * cap, dtype=torch.uint8, device=dev)
        ar = torch.arange(n, dtype=torch.int64, device=dev)
        in_ptrs = text.data_ptr() + ar * piece
        in_lens = torch.full((n,), piece, dtype=torch.int64, device=dev)
        mid_ptrs = mid.data_ptr() + ar * cap
        mid_lens = torch.zeros(n, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        frame.compress_many_ptrs(ctx, in_ptrs, in_lens, mid_ptrs, None,
                                 mid_lens, None, host_in_lens=in_lens.cpu())
        ctx.synchronize()
        flens = mid_lens.cpu().tolist()
        index = torch.tensor([[10, f] for f in flens], dtype=torch.int64,
                             device=dev)
        out = torch.zeros(n * piece, dtype=torch.uint8, device=dev)
        out_lens = torch.zeros(n, dtype=torch.int64, device=dev)
        errs = torch.zeros(n * 32, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        argv = [(V(mid.data_ptr() + i * cap), flens[i],
                 V(out.data_ptr() + i * piece), piece,
                 V(out_lens.data_ptr() + 8 * i), V(errs.data_ptr() + 32 * i),
                 V(index.data_ptr() + 16 * i), 1) for i in range(n)]

        def loop(c, flags):
            def run():
                out_lens.zero_()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for a in argv:
                    decode(c, *a, flags)
                c.synchronize()
                return time.perf_counter() - t0
            run()
            assert out_lens.cpu().tolist() == [piece] * n
            assert not errs.any().item() and torch.equal(out, text)
            return run
        timers = {"flagged": loop(ctx, 4), "unflagged": loop(ctx, 0)}
        if parent is not None:
            timers["parent"] = loop(parent, 0)
        med, rec = timed(timers)
        rec.update(streams=n, stream_bytes=piece,
                   us_per_call={k: round(v * 1e3 / n, 2)
                                for k, v in med.items()})
        if parent is not None:
            rec["flagged_over_parent"] = round(med["flagged"] / med["parent"],
                                               4)
        res["a_4096x16k"] = rec
        del text, mid, out, argv
        torch.cuda.empty_cache()

        # (b), (c) one long stream
        nbytes = 1 << 30
        text = synth_text(dev, nbytes)
        framed, flen, index = frame.compress_device(ctx, text,
                                                    want_index=True)
        chunks = index.numel() - 1
        out = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
        out_len = torch.zeros(1, dtype=torch.int64, device=dev)
        err = torch.zeros(32, dtype=torch.uint8, device=dev)
        wide = raw.Context(ctx.device, lib=ctx._L)   # (c): its own scratch
        torch.cuda.synchronize()

        def one(c, idx, bound, flags):
            a = (V(framed.data_ptr()), flen, V(out.data_ptr()), nbytes,
                 V(out_len.data_ptr()), V(err.data_ptr()),
                 V(index.data_ptr()) if idx else None, bound, flags)

            def run():
                out_len.zero_()
                out[:4096].zero_()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(3):
                    decode(c, *a)
                c.synchronize()
                return (time.perf_counter() - t0) / 3
            run()
            assert int(out_len.item()) == nbytes and not err.any().item()
            assert torch.equal(out, text)
            return run
        timers = {"flagged_index": one(ctx, True, chunks, 4),
                  "flagged_bound": one(ctx, False, chunks, 4),
                  "unflagged_index": one(ctx, True, chunks, 0),
                  "unflagged_walk": one(ctx, False, 0, 0)}
        scratch_exact = ctx.info("scratch_bytes")
        timers["flagged_bound_x4"] = one(wide, False, 4 * chunks, 4)
        scratch_wide = wide.info("scratch_bytes")
        tight = raw.Context(ctx.device, lib=ctx._L)
        one(tight, False, chunks, 4)
        scratch_tight = tight.info("scratch_bytes")
        tight.close()
        if parent is not None:
            timers["parent_index"] = one(parent, True, chunks, 0)
            timers["parent_walk"] = one(parent, False, 0, 0)
        med, rec = timed(timers)
        rec.update(bytes=nbytes, framed_bytes=flen, chunks=chunks,
                   gibs={k: round(nbytes / GIB / (v / 1e3), 1)
                         for k, v in med.items()},
                   scratch_bytes={"bound_exact": scratch_tight,
                                  "bound_x4": scratch_wide,
                                  "bench_context": scratch_exact,
                                  "per_extra_chunk": round(
                                      (scratch_wide - scratch_tight)
                                      / (3 * chunks), 1)})
        res["b_c_one_1g"] = rec
        wide.close()
    finally:
        if parent is not None:
            parent.close()
    (ROOT / "profiles" / "frame_nowait.json").write_text(
        json.dumps(res) + "\n")
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=8.0)
    ap.add_argument("--period-mib", type=float, default=1024.0,
                    help="period of the synthetic text (SURVEY 8d: 1 GiB)")
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--only", default="")
    ap.add_argument("--sets", default="",
                    help="frames_host_batch: only these data sets (a,b,...); "
                         "raw_ranges, raw_writes, raw_appends: only these "
                         "shapes, nothing "
                         "recorded")
    ap.add_argument("--plan", default="",
                    help="name:gib,... - run these configs at these sizes, "
                         "one JSON line each with a \"name\" key; a config "
                         "that fails prints {\"name\", \"error\"} and the "
                         "rest still run (bench.py's extras)")
    ap.add_argument("--option", action="append", default=[],
                    help="name=value: snapmi_ctx_set_option on the context "
                         "(experiments: --option tiny_stream_kernel=0)")
    args = ap.parse_args()
    import __graft_entry__ as g
    g.build()
    from rust_snappy_amd import raw
    import os
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if os.environ.get("SNAPMI_OVERSUBSCRIBE") == "1":
        local = 0  # bench.py --oversubscribe: every rank drives cuda:0
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    ctx = raw.Context(local)      # the library's defaults (extras.budget)
    for item in args.option:
        name, value = item.split("=")
        ctx.set_option(name, int(value))
    table = {"cfg3": cfg3, "cfg5": cfg5, "files": files, "pcie": pcie,
             "adapters": adapters, "stream": stream, "cfg4": cfg4,
             "tiny": tiny, "sweep": sweep, "budget": budget, "seam": seam,
             "frames_batch": frames_batch, "host_batch": host_batch,
             "frames_host_batch": frames_host_batch, "raw_index": raw_index,
             "raw_ranges": raw_ranges, "raw_index_build": raw_index_build,
             "raw_writes": raw_writes, "raw_appends": raw_appends,
             "crc": crc, "frame_nowait": frame_nowait}
    if args.plan:
        for item in args.plan.split(","):
            name, gib = item.split(":")
            args.gib = float(gib)
            t0 = time.perf_counter()
            try:
                res = table[name](args, ctx, dev)
            except Exception as e:  # noqa: BLE001 - reported, not hidden
                res = {"error": f"{type(e).__name__}: {e}"[:300]}
            torch.cuda.empty_cache()
            if res is not None:
                res["name"] = name
                res["wall_s"] = round(time.perf_counter() - t0, 1)
                print(json.dumps(res), flush=True)
        return
    for name, fn in (("cfg3", cfg3), ("cfg5", cfg5), ("files", files),
                     ("pcie", pcie), ("adapters", adapters),
                     ("stream", stream), ("cfg4", cfg4),
                     ("frames_batch", frames_batch),
                     ("host_batch", host_batch),
                     ("frames_host_batch", frames_host_batch),
                     ("raw_index", raw_index),
                     ("raw_ranges", raw_ranges),
                     ("raw_index_build", raw_index_build),
                     ("raw_writes", raw_writes),
                     ("raw_appends", raw_appends),
                     ("crc", crc),
                     ("frame_nowait", frame_nowait)):
        if args.only != name and (args.only or name in ("cfg4",
                                                         "frames_batch",
                                                         "host_batch",
                                                         "frames_host_batch",
                                                         "raw_index",
                                                         "raw_ranges",
                                                         "raw_index_build",
                                                         "raw_writes",
                                                         "raw_appends",
                                                         "crc",
                                                         "frame_nowait")):
            continue  # cfg4 (the multi-rank config), *_batch: on request
        res = fn(args, ctx, dev)
        if res is not None:
            print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
