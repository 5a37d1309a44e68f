#!/usr/bin/env python3
"""bench.py -- BASELINE.json's headline metric on MI355X.

Workload (BASELINE.json configs[1], SURVEY.md 8d "cfg2"): the 12-stream
zflat/uflat round of the reference's bench (bench/src/bench.rs:83-114), tiled
to 8 GiB per GPU as independent raw streams.  One step = one compress pass
and one decompress pass of the raw block codec over the whole batch, inputs
and outputs resident in HBM.  value = uncompressed bytes through both
directions / time, whole job, GiB/s.

  python bench.py [--gpus N] [--steps K] [--warmup W] [--gib G]
                  [--dump-outputs DIR] [--full]
  python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N

A plain run does what the headline needs and nothing else: it sets up (the
first compress and decompress call of the context, untimed), warms up, times
the K steps, writes the outputs of the last step if asked and prints the
line.  `--full` adds everything else the benchmark measures or checks: the
parity gate against the oracle's bytes before and after the timed steps,
roofline.traffic from two PMC child runs, the `extras` and the CPU baseline
(each of them can be left out again with --no-verify / --no-pmc /
--no-extras / --no-cpu).

Multi-GPU: streams are independent, so each rank compresses its own shard;
no data-path collective (scaling = weak: G GiB per GPU).  `--gpus N` without
a torch.distributed environment re-executes itself under
torch.distributed.run with N ranks (one per GPU, 127.0.0.1 rendezvous); it
fails loudly when fewer than N devices are visible or when WORLD_SIZE
disagrees with N.  With --full, after the timed region the line gets
`extras`: BASELINE configs 3 and 5 at full size and the per-file rates
(N = 1), and config 4 - the framed stream sharded by chunk range over the
ranks with the RCCL gather of the framed parts (any N).
"""
import argparse
import hashlib
import json
import os
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

GIB = float(1 << 30)
HBM_PEAK_GBS = 8000.0  # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def build_round():
    """The 12 bench inputs laid out back to back (16-byte aligned)."""
    import kats
    import oracle_lib  # only for the corpus file list (no oracle compute)
    rnd = oracle_lib.corpus_round()
    offs, pos = [], 0
    for _, d in rnd:
        offs.append(pos)
        pos += (max(len(d), 1) + 15) // 16 * 16
    host = np.zeros(pos, dtype=np.uint8)
    for (_, d), o in zip(rnd, offs):
        host[o:o + len(d)] = np.frombuffer(d, dtype=np.uint8)
    lens = [len(d) for _, d in rnd]
    shas = [kats.CORPUS_SHA256[b] for b, _ in rnd]
    return rnd, host, np.array(offs, dtype=np.int64), np.array(
        lens, dtype=np.int64), shas


def source_sha16():
    """sha256[:16] over the sources a bench line is a measurement OF: the
    kernels and the C ABI (rust-snappy_amd/csrc, include), the Python
    mirror, this file and bench_configs.py - in sorted order, path and bytes.
    The GPU box has no .git; this is how a line under profiles/ says which
    code it is of (tests/test_bench_spawn_cpu.py compares the committed final
    line with the tree)."""
    import hashlib
    h = hashlib.sha256()
    files = []
    for pat in ("rust-snappy_amd/csrc/*", "include/*.h",
                "rust-snappy_amd/*.py"):
        files += sorted(ROOT.glob(pat))
    files += [ROOT / "bench.py", ROOT / "bench_configs.py"]
    for f in files:
        if f.is_file() and f.suffix in (".hip", ".hpp", ".h", ".py", ".map",
                                        "") and f.name != "__pycache__":
            h.update(str(f.relative_to(ROOT)).encode())
            h.update(f.read_bytes())
    return h.hexdigest()[:16]


DUMP_MAX_STREAMS = 1 << 16   # per-stream lengths / errors kept in a dump


def dump_outputs(out_dir, comp, comp_lens, comp_errs, back, back_lens,
                 back_errs, n_files):
    """--dump-outputs: what the last timed step handed back to its caller,
    as .npy files (float32 / float64) under `out_dir`, so that two builds
    can be compared output for output.  Per stream: the compressed and the
    decompressed length and both error records (kind, a, b, c) - for every
    stream, or a seeded sample of DUMP_MAX_STREAMS of them in larger
    batches.  Bytes: the compressed and the decompressed bytes of one stream
    per bench input, each from a seeded choice of round, back to back
    (about 18 MB as float32).  The seeds are fixed, so the same arguments
    dump the same streams."""
    out = Path(out_dir)
    out.mkdir(parents=True, exist_ok=True)
    n = len(comp.lens)
    rng = np.random.default_rng(20240601)
    if n <= DUMP_MAX_STREAMS:
        idx = np.arange(n, dtype=np.int64)
    else:
        idx = np.sort(rng.choice(n, DUMP_MAX_STREAMS, replace=False))
    cl = comp_lens.cpu().numpy()
    bl = back_lens.cpu().numpy()

    def records(errs):
        rec = np.frombuffer(errs.cpu().numpy().tobytes(), dtype=np.dtype(
            [("kind", "<i4"), ("r", "<u4"), ("a", "<u8"), ("b", "<u8"),
             ("c", "<u8")]))[idx]
        return np.stack([rec[f].astype(np.float64)
                         for f in ("kind", "a", "b", "c")], axis=1)

    rounds = n // n_files
    picks = (rng.integers(0, rounds, n_files) * n_files
             + np.arange(n_files)).astype(np.int64)
    arrays = {
        "stream_index": idx.astype(np.float64),
        "compressed_len": cl[idx].astype(np.float64),
        "decompressed_len": bl[idx].astype(np.float64),
        "compress_error": records(comp_errs),
        "decompress_error": records(back_errs),
        "bytes_stream_index": picks.astype(np.float64),
        "compressed_bytes": np.frombuffer(b"".join(
            comp.stream_bytes(i, cl[i]) for i in picks),
            dtype=np.uint8).astype(np.float32),
        "decompressed_bytes": np.frombuffer(b"".join(
            back.stream_bytes(i, bl[i]) for i in picks),
            dtype=np.uint8).astype(np.float32),
    }
    total = sum(a.nbytes for a in arrays.values())
    assert total <= 64 << 20, f"--dump-outputs: {total} bytes over 64 MiB"
    for name, a in arrays.items():
        np.save(out / f"{name}.npy", a)
    return {"bytes": total, "streams": int(idx.size),
            "byte_streams": int(picks.size)}


def usable_cores():
    """CPUs this process can actually use: the scheduler affinity mask capped
    by the cgroup CPU quota (os.cpu_count() is the machine's, not ours)."""
    info = {"os_cpu_count": os.cpu_count() or 1}
    try:
        info["affinity"] = len(os.sched_getaffinity(0))
    except AttributeError:
        info["affinity"] = info["os_cpu_count"]
    quota = None
    for path in ("/sys/fs/cgroup/cpu.max",                       # cgroup v2
                 "/sys/fs/cgroup/cpu/cpu.cfs_quota_us"):          # cgroup v1
        try:
            text = Path(path).read_text().split()
        except OSError:
            continue
        if path.endswith("cpu.max"):
            info["cgroup_cpu_max"] = " ".join(text)
            if text and text[0] != "max":
                quota = float(text[0]) / float(text[1])
        else:
            q = float(text[0])
            if q > 0:
                per = float(Path(
                    "/sys/fs/cgroup/cpu/cpu.cfs_period_us").read_text())
                info["cgroup_cpu_max"] = f"{int(q)} {int(per)}"
                quota = q / per
        break
    cores = info["affinity"]
    if quota is not None:
        cores = max(1, min(cores, int(quota + 0.999)))
    info["usable"] = cores
    return cores, info


def native_oracle():
    """oracle/snappy_oracle.c compiled -O3 -march=native for THIS host into a
    temporary directory (the in-tree liboracle.so is built without
    -march=native because it travels between machines).  Falls back to the
    in-tree library if gcc is missing."""
    import ctypes as C
    import subprocess
    import tempfile
    import oracle_lib as O
    src = O.ORACLE_DIR / "snappy_oracle.c"
    fast = O.ORACLE_DIR / "snappy_port_fast.c"
    try:
        out = Path(tempfile.mkdtemp(prefix="snapo_native_")) / "liboracle.so"
        subprocess.check_call(
            ["gcc", "-O3", "-march=native", "-std=gnu11", "-fPIC", "-shared",
             "-I", str(O.ORACLE_DIR), "-o", str(out), str(src), str(fast),
             "-lpthread"],
            stderr=subprocess.DEVNULL)
        return C.CDLL(str(out)), "-O3 -march=native"
    except (OSError, subprocess.CalledProcessError):
        return O.lib(), "-O3 (in-tree build; gcc -march=native failed)"


def cpu_baseline(rnd, seconds=2.0):
    """The CPU path timed beside the GPU, on a bounded sample: the
    12-stream round, repeated by every thread for `seconds` per leg.  Codecs:
      port_fast  oracle/snappy_port_fast.c - the restatement of the reference
                 WITH its fast paths (16-byte blind copies, tag table, the
                 three copy strategies, src/decompress.rs:170-183,233-343,
                 src/compress.rs:440-453): what `value` quotes (kind 'port').
                 The reference's README (:135-158) shows Rust within a few
                 percent of C++ snappy either way, and so is this, file by
                 file (`per_file`);
      libsnappy  Google libsnappy 1.1.8, what the reference's own bench
                 compares against (bench/src/bench.rs:117-153);
      oracle     oracle/snappy_oracle.c, the parity checker - plain loops, no
                 fast paths: listed so that nobody takes the checker's speed
                 for the reference's (round 5's `value` did).
    Legs: {all usable cores, 1 thread (the README's is a 1-thread table)} x
    {compress, decompress}; threads pinned, buffers allocated before the
    clock, gcc -O3 -march=native."""
    import ctypes as C
    import oracle_lib as O
    cores, host = usable_cores()
    L, flags = native_oracle()
    datas = [d for _, d in rnd]
    comps = [O.compress(d) for d in datas]
    L.snapo_bench_ext.restype = C.c_double

    def leg(direction, threads, fns, secs, ds=datas, cs=comps):
        n = len(ds)
        PP = C.c_char_p * n
        SZ = C.c_size_t * n
        L.snapo_bench_ext.argtypes = [PP, SZ, PP, SZ, C.c_int, C.c_int,
                                      C.c_int, C.c_double,
                                      C.POINTER(C.c_uint64), C.c_void_p,
                                      C.c_void_p, C.c_int]
        rounds = C.c_uint64(0)
        t0 = time.perf_counter()
        bps = L.snapo_bench_ext(
            PP(*ds), SZ(*[len(d) for d in ds]), PP(*cs),
            SZ(*[len(c) for c in cs]), n, direction, threads, secs,
            C.byref(rounds), fns[0] if fns else None,
            fns[1] if fns else None, 1)
        return bps / GIB, rounds.value, time.perf_counter() - t0

    def codec(fns):
        ca, da = leg(0, cores, fns, seconds), leg(1, cores, fns, seconds)
        c1, d1 = leg(0, 1, fns, seconds), leg(1, 1, fns, seconds)
        return {"all_cores": {"threads": cores,
                              "compress_gibs": round(ca[0], 4),
                              "decompress_gibs": round(da[0], 4)},
                "one_thread": {"compress_gibs": round(c1[0], 4),
                               "decompress_gibs": round(d1[0], 4)}}, ca, da

    fast_fns = (C.cast(L.snapf_compress, C.c_void_p),
                C.cast(L.snapf_uncompress, C.c_void_p))
    fast, ca, da = codec(fast_fns)
    c, d = ca[0], da[0]
    out = {
        "value": round(2.0 / (1.0 / c + 1.0 / d), 4), "unit": "GiB/s",
        "cores": cores, "kind": "port",
        "compress_gibs": round(c, 4), "decompress_gibs": round(d, 4),
        "sample": (f"12-stream zflat/uflat round (2928571 B) x {ca[1]} "
                   f"(compress, {ca[2]:.1f}s) / x {da[1]} (decompress, "
                   f"{da[2]:.1f}s) on {cores} pinned pthreads, "
                   f"oracle/snappy_port_fast.c (the reference's algorithm "
                   f"with its fast paths) {flags}; every leg {seconds:g} s"),
        "host": host, "port_fast": fast,
        "oracle_plain_loops": codec(None)[0],
    }
    S = O.libsnappy()
    if S is not None:
        ext = (C.cast(S.snappy_compress, C.c_void_p),
               C.cast(S.snappy_uncompress, C.c_void_p))
        out["libsnappy_1_1_8"] = codec(ext)[0]
        # file by file, one thread, MB/s like README.md:135-158: the port
        # beside the library (0.25 s per cell)
        rows = {}
        for (name, dd), cc in zip(rnd, comps):
            cell = {}
            for tag, fns in (("port_fast", fast_fns), ("libsnappy", ext)):
                cell[tag] = [round(leg(k, 1, fns, 0.25, [dd], [cc])[0]
                                   * GIB / 1e6) for k in (0, 1)]
            cell["ratio"] = [round(cell["port_fast"][k]
                                   / max(cell["libsnappy"][k], 1), 2)
                             for k in (0, 1)]
            rows[name] = cell
        out["per_file_mbs_compress_decompress"] = rows
    return out


def measure_traffic(args, kernels):
    """HBM bytes per launch of `kernels` from the PMC counters of THIS
    command: two child runs of one step each under rocprofv3 (separate
    --pmc FETCH_SIZE / WRITE_SIZE passes with --kernel-trace only, as
    MI355X_MICROARCH.md prescribes; FETCH_SIZE x2 for wide reads).  Returns
    {kernel: bytes} or raises."""
    import importlib.util
    import shutil
    import subprocess
    import tempfile
    spec = importlib.util.spec_from_file_location(
        "pmc_traffic", ROOT / "profiles" / "pmc_traffic.py")
    pt = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(pt)
    rp = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    vals = {}
    tmp = tempfile.mkdtemp(prefix="snapmi_pmc_", dir="/tmp")
    try:
        for counter in ("FETCH_SIZE", "WRITE_SIZE"):
            out = os.path.join(tmp, counter)
            cmd = [rp, "--kernel-trace", "--pmc", counter, "--output-format",
                   "csv", "-d", out, "-o", "p", "--", sys.executable,
                   str(Path(__file__).resolve()), "--steps", "1", "--warmup",
                   "0", "--gib", f"{args.gib:g}"]
            env = dict(os.environ, TMPDIR="/tmp")
            p = subprocess.run(cmd, cwd="/tmp", env=env, capture_output=True,
                               text=True, timeout=240)
            csvs = list(Path(out).rglob("*counter_collection.csv"))
            if p.returncode != 0 or not csvs:
                raise RuntimeError(f"rocprofv3 --pmc {counter}: exit "
                                   f"{p.returncode} {p.stderr.strip()[-200:]}")
            vals[counter] = pt.per_kernel(str(csvs[0]), counter)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    res = {}
    for k in kernels:
        f, w = vals["FETCH_SIZE"].get(k), vals["WRITE_SIZE"].get(k)
        if f is None or w is None:
            raise RuntimeError(f"no counters for {k}")
        res[k] = int(round((2 * f + w) * 1024))   # counters are KB
    return res


def run_extras(args, local_rank, dev, rank, world):
    """BASELINE configs beside the headline one, for the driver's record:
    cfg3 (framed text, 64 GiB), cfg5 (incompressible, 32 GiB), the 12
    per-file rates, one long raw stream, cfg4 at N = 1, the PCIe-inclusive
    host-to-host rate of the frame entry points and the streams of 200 ..
    4 096 bytes (the lane-per-stream kernels) - in a child
    process (bench_configs.py --plan), so that nothing they do can take the
    headline line down; at N > 1 cfg4 only (the framed stream sharded over
    the ranks, gathered on rank 0), one child per rank with a process group
    of their own.  Each config is parity-checked inside bench_configs.py; a
    failure is recorded."""
    import subprocess
    out = {}
    if world == 1:
        g3 = args.extras_gib or 64.0
        g5 = args.extras_gib or 32.0
        plan = (f"sweep:4,cfg3:{g3:g},cfg5:{g5:g},files:2,stream:2,cfg4:8,"
                "pcie:4,adapters:4,tiny:1,budget:8,seam:100")
        cmd = [sys.executable, str(ROOT / "bench_configs.py"), "--plan", plan]
        try:
            p = subprocess.run(cmd, capture_output=True, text=True,
                               timeout=540)
            for ln in p.stdout.splitlines():
                if ln.startswith("{"):
                    rec = json.loads(ln)
                    out[rec.pop("name", f"cfg{len(out)}")] = rec
            if p.returncode != 0:
                out["error"] = (f"bench_configs.py exit {p.returncode}: "
                                + p.stderr.strip()[-300:])
        except subprocess.TimeoutExpired:
            out["error"] = "bench_configs.py --plan timed out (540 s)"
        return out
    # N > 1: every rank starts one child (bench_configs.py --plan cfg4) and
    # the children form a process group of their own on a fresh port.  The
    # sharded encode + gather has never met a multi-GPU box in this repo's
    # own runs; in a child with a time limit, whatever goes wrong there is a
    # recorded error and not a lost headline line.
    over = os.environ.get("SNAPMI_OVERSUBSCRIBE") == "1"
    res = with_deadline(
        lambda: rank_children(
            [sys.executable, str(ROOT / "bench_configs.py"), "--plan",
             f"cfg4:{(1 if over else 8) * world}"]
            + (["--period-mib", "64"] if over else []),
            rank, local_rank, world, 300), 420,
        {"error": f"rank {rank}: cfg4 children: no answer within 420 s "
                  "(the rendezvous of the child group, or a rank that is "
                  "gone)"})
    if res is not None:
        out["cfg4"] = res
    return out if rank == 0 else None


def with_deadline(fn, seconds, on_timeout):
    """fn() on a helper thread; its result, or `on_timeout` when it has not
    come back in time (a collective that waits for a rank that is gone must
    not take the headline line with it: the thread is left behind, the
    process exits through os._exit at the end of main in that case)."""
    import threading
    box = {}

    def run():
        try:
            box["v"] = fn()
        except Exception as e:  # noqa: BLE001 - recorded, not hidden
            box["v"] = {"error": f"{type(e).__name__}: {e}"[:300]}

    th = threading.Thread(target=run, daemon=True)
    th.start()
    th.join(seconds)
    if th.is_alive():
        box["hung"] = True
        return dict(on_timeout, hung=True)
    return box.get("v")


def rank_children(cmd, rank, local_rank, world, limit_s):
    """Every rank of this process group runs `cmd` as a child; the children
    rendezvous on a fresh port that rank 0 picks and broadcasts.  Returns the
    last JSON line of this rank's child (None if it printed none), or an
    {"error"} record - after limit_s the child is killed."""
    import subprocess
    import torch.distributed as dist
    port = [0]
    if rank == 0:
        import socket
        with socket.socket() as sk:
            sk.bind(("127.0.0.1", 0))
            port[0] = sk.getsockname()[1]
    dist.broadcast_object_list(port, src=0)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port[0]),
               RANK=str(rank), LOCAL_RANK=str(local_rank),
               WORLD_SIZE=str(world))
    for k in list(env):
        if k.startswith("TORCHELASTIC_"):
            env.pop(k)  # the child group has a TCP store of its own
    t0 = time.perf_counter()
    res = None
    child = subprocess.Popen(cmd, env=env, stdout=subprocess.PIPE,
                             stderr=subprocess.PIPE, text=True)
    try:
        so, se = child.communicate(timeout=limit_s)
        for ln in so.splitlines():
            if ln.startswith("{"):
                res = json.loads(ln)
                res.pop("name", None)
        if child.returncode != 0:
            res = {"error": (f"rank {rank} child exit {child.returncode}: "
                             + se.strip()[-300:])}
    except subprocess.TimeoutExpired:
        child.kill()
        child.communicate()
        res = {"error": f"rank {rank} child timed out ({limit_s} s)"}
    if rank == 0 and res is None:
        res = {"error": "no record from rank 0's child"}
    if res is not None:
        res["wall_s"] = round(time.perf_counter() - t0, 1)
    return res


# what plumbing_check's children do: a process group of their own (gloo),
# one all_reduce, one JSON line from rank 0
_CHILD_STUB = (
    "import os, json, torch, torch.distributed as dist\n"
    "dist.init_process_group('gloo')\n"
    "t = torch.tensor([1.0 + dist.get_rank()])\n"
    "dist.all_reduce(t)\n"
    "if dist.get_rank() == 0:\n"
    "    print(json.dumps({'name': 'stub', 'sum': t.item(),\n"
    "                      'port': os.environ['MASTER_PORT']}))\n"
    "dist.destroy_process_group()\n")


def maybe_spawn(args):
    """`python bench.py --gpus N` with N > 1 and no torch.distributed
    environment: run the N ranks ourselves (the driver's own launch line,
    one rank per GPU, rendezvous on 127.0.0.1) and return the exit code;
    None when this process is a rank (or N == 1) and should carry on."""
    if args.gpus <= 1 or "WORLD_SIZE" in os.environ:
        return None
    if not args.plumbing_check and not args.oversubscribe:
        have = torch.cuda.device_count() if torch.cuda.is_available() else 0
        if have < args.gpus:
            sys.exit(f"bench.py: --gpus {args.gpus} but {have} GPU(s) visible "
                     f"(no CPU fallback, no oversubscription)")
    import socket
    import subprocess
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
           f"--nproc-per-node={args.gpus}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), str(Path(__file__).resolve())] + \
        sys.argv[1:]
    log(f"[bench] --gpus {args.gpus}: spawning {args.gpus} ranks: "
        + " ".join(cmd[1:8]) + " ...")
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get(
        "HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    if args.oversubscribe:
        env["SNAPMI_OVERSUBSCRIBE"] = "1"
    return subprocess.call(cmd, env=env)


def plumbing_check(rank, world):
    """The rank plumbing of the real run without a GPU: process group (gloo),
    barrier, MAX-reduce of a per-rank time, gather of the ranks seen, one
    JSON line from rank 0 marked invalid."""
    import torch.distributed as dist
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("gloo")
        dist.barrier()
        t = torch.tensor([1.0 + rank], dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        seen = [None] * world
        dist.all_gather_object(seen, rank)
        # the N > 1 extras: a child per rank, a process group of their own
        child = rank_children([sys.executable, "-c", _CHILD_STUB], rank,
                              int(os.environ.get("LOCAL_RANK", "0")), world,
                              120)
        dist.barrier()
        dist.destroy_process_group()
    else:
        t, seen, child = torch.tensor([1.0]), [0], None
    if rank == 0:
        print(json.dumps({"metric": "plumbing check", "n_gpus": world,
                          "ranks_seen": sorted(seen),
                          "max_over_ranks": float(t[0]),
                          "children": child,
                          "INVALID": "plumbing check, no GPU work"}),
              flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--gib", type=float, default=8.0,
                    help="uncompressed GiB per GPU (BASELINE cfg2: 8)")
    ap.add_argument("--full", action="store_true",
                    help="besides the headline: the parity gate, "
                         "roofline.traffic from PMC child runs, the extra "
                         "configs and the CPU baseline (a plain run does "
                         "none of them)")
    ap.add_argument("--no-cpu", action="store_true",
                    help="with --full: skip the cpu_baseline leg")
    ap.add_argument("--no-verify", action="store_true",
                    help="experiment builds only: skip the parity gate of "
                         "--full (the JSON line is then marked invalid)")
    ap.add_argument("--no-extras", action="store_true",
                    help="with --full: skip the extra configs "
                         "(cfg3/cfg4/cfg5/per-file)")
    ap.add_argument("--extras-gib", type=float, default=None,
                    help="size of the cfg3 / cfg5 extras (default: BASELINE's "
                         "64 and 32 GiB)")
    ap.add_argument("--no-pmc", action="store_true",
                    help="with --full: do not measure roofline.traffic (two "
                         "child runs of one step each under rocprofv3 --pmc "
                         "FETCH_SIZE / WRITE_SIZE); the committed profile is "
                         "quoted instead, as in a plain run, and the line "
                         "says traffic_measured: false")
    ap.add_argument("--oversubscribe", action="store_true",
                    help="proof run of the N > 1 code on ONE GPU: all ranks "
                         "drive cuda:0, collectives over gloo; the JSON line "
                         "is marked INVALID (it is no scaling number)")
    ap.add_argument("--plumbing-check", action="store_true",
                    help="no GPU work: only the --gpus N launch plumbing over "
                         "gloo (what tests/test_bench_spawn_cpu.py runs)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last step "
                         "computed (lengths, error records, a seeded sample "
                         "of the compressed and decompressed bytes) as "
                         "DIR/<name>.npy, 64 MiB at most (rank 0)")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be at least 1 and --warmup at least 0")

    spawned = maybe_spawn(args)
    if spawned is not None:
        sys.exit(spawned)
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        sys.exit(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}: "
                 f"launch N ranks for --gpus N (or let bench.py do it)")
    if args.plumbing_check:
        return plumbing_check(rank, world)
    assert torch.cuda.is_available(), "bench.py needs a GPU (no CPU fallback)"
    # --oversubscribe: the real rank code, N ranks on cuda:0, gloo instead of
    # RCCL (which refuses two ranks on one device) - proves the N > 1 path
    # before a multi-GPU box runs it; never a measurement
    over = args.oversubscribe or os.environ.get("SNAPMI_OVERSUBSCRIBE") == "1"
    if over:
        os.environ["SNAPMI_OVERSUBSCRIBE"] = "1"
        local_rank = 0
    if torch.cuda.device_count() <= local_rank or (
            not over and torch.cuda.device_count() < world):
        # EVERY rank sees this (the same count on one node) and leaves at
        # once: no rank is left waiting in a rendezvous for one that is gone
        msg = (f"--gpus {world}: {torch.cuda.device_count()} device(s) "
               f"visible to rank {rank} (wants cuda:{local_rank}; one device "
               f"per rank, no oversubscription)")
        log("[bench] " + msg)
        if rank == 0:
            print(json.dumps({
                "metric": "GiB/s uncompressed (compress + decompress) on "
                          "zflat/uflat corpus", "value": None,
                "unit": "GiB/s", "n_gpus": world, "steps": args.steps,
                "warmup": args.warmup, "higher_is_better": True,
                "scaling": "weak", "error": msg}), flush=True)
        sys.exit(2)
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    cdev = torch.device("cpu") if over else dev  # where collectives run
    if world > 1:
        import datetime
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        try:
            if over:
                dist.init_process_group(
                    "gloo", timeout=datetime.timedelta(seconds=600))
            else:
                dist.init_process_group(
                    "nccl", device_id=dev,
                    timeout=datetime.timedelta(seconds=600))
                # the first collective is where RCCL really comes up
                # (communicator, xGMI rings): fail here, with a record,
                # rather than in the middle of the timed region
                probe = torch.ones(1, device=dev)
                dist.all_reduce(probe)
                torch.cuda.synchronize()
                assert int(probe.item()) == world, probe
        except Exception as e:  # noqa: BLE001 - recorded, not hidden
            # no process group: every rank says why (rank 0 on stdout, as the
            # one JSON line the driver reads) and leaves with an error code
            msg = f"rank {rank}: process group: {type(e).__name__}: {e}"[:400]
            log("[bench] " + msg)
            if rank == 0:
                print(json.dumps({
                    "metric": "GiB/s uncompressed (compress + decompress) on "
                              "zflat/uflat corpus", "value": None,
                    "unit": "GiB/s", "n_gpus": world, "steps": args.steps,
                    "warmup": args.warmup, "higher_is_better": True,
                    "scaling": "weak", "error": msg}), flush=True)
            sys.exit(3)

    import __graft_entry__ as g
    g.build()
    import rust_snappy_amd as R
    from rust_snappy_amd import batch, raw

    rnd, host_round, r_offs, r_lens, shas = build_round()
    round_stride = int(host_round.size)
    round_ubytes = int(r_lens.sum())
    rounds = int(np.ceil(args.gib * GIB / round_ubytes))
    n = 12 * rounds
    ubytes = rounds * round_ubytes
    if rank == 0:
        log(f"[bench] {rounds} rounds x 12 streams = {n} streams, "
            f"{ubytes / GIB:.3f} GiB uncompressed per GPU, world={world}")

    # ---- inputs resident in HBM, tiled on the device --------------------
    # (the library's defaults throughout: the lane tables within a third of
    # the free memory.  Rounds 2-3 quoted the headline at 75 %; measured in
    # round 4 - extras.budget - 75, 33 and 15 % give the same rate)
    ctx = raw.Context(local_rank)
    d_round = torch.from_numpy(host_round).to(dev)
    data = d_round.repeat(rounds)
    offs = (np.arange(rounds, dtype=np.int64)[:, None] * round_stride
            + r_offs[None, :]).reshape(-1)
    lens = np.tile(r_lens, rounds)
    src = batch.StreamBatch(data, offs, lens)
    caps = np.array([raw.max_compress_len(int(x)) for x in r_lens],
                    dtype=np.int64)
    comp = batch.StreamBatch.empty(np.tile(caps, rounds), dev)
    comp_lens = torch.zeros(n, dtype=torch.int64, device=dev)
    comp_errs = torch.zeros(32 * n, dtype=torch.uint8, device=dev)
    back = batch.StreamBatch.empty(lens, dev)
    back_lens = torch.zeros(n, dtype=torch.int64, device=dev)
    back_errs = torch.zeros(32 * n, dtype=torch.uint8, device=dev)

    def do_compress():
        raw.compress_batch(ctx, src.d_ptrs, src.d_lens, comp.d_ptrs,
                           comp.d_lens, comp_lens, comp_errs,
                           host_in_lens=src.h_lens)
        return ctx.last_timing()  # waits for this batch's last event

    def do_decompress():
        raw.decompress_batch(ctx, comp.d_ptrs, comp_lens, back.d_ptrs,
                             back.d_lens, back_lens, back_errs)
        return ctx.last_timing()

    # ---- the first call of the context, untimed -------------------------
    # (the first compress call of the context on its own: it allocates the
    # scratch and places the lane tables - the line carries what it took and
    # the device's free memory around it, so that a record explains itself)
    torch.cuda.synchronize()
    free_before_first = torch.cuda.mem_get_info(dev)[0]
    t_first = time.perf_counter()
    do_compress()
    ctx.synchronize()
    first_call_ms = (time.perf_counter() - t_first) * 1e3
    free_after_first = torch.cuda.mem_get_info(dev)[0]
    do_decompress()
    ctx.synchronize()
    cl = comp_lens.cpu().numpy()
    c_stride = int(comp.offsets[12]) if rounds > 1 else 0
    per = back.data[:rounds * round_stride].view(rounds, round_stride)
    gate = args.full and not args.no_verify

    def kinds(t):
        return np.frombuffer(t.cpu().numpy().tobytes(),
                             dtype="<i4").reshape(n, 8)[:, 0]

    # ---- --full: parity gate before any number is reported --------------
    if args.full:
        assert (kinds(comp_errs) == 0).all(), "compress reported errors"
    if gate:
        assert (kinds(back_errs) == 0).all(), "decompress reported errors"
        for j in range(12):  # round 0 vs sha256
            got = comp.stream_bytes(j, cl[j])
            n_in, n_out, sha = shas[j]
            assert len(got) == n_out and \
                hashlib.sha256(got).hexdigest() == sha, \
                f"compressed bytes of stream {j} differ from the oracle's"
        assert (cl.reshape(rounds, 12) == cl[:12][None, :]).all()
        if rounds > 1:  # every round equals round 0
            perc = comp.data[:rounds * c_stride].view(rounds, c_stride)
            for j in range(12):
                o, m = int(comp.offsets[j]), int(cl[j])
                assert bool((perc[:, o:o + m] == perc[0:1, o:o + m]).all()), j
        for j in range(12):  # round trip == input
            o, m = int(r_offs[j]), int(r_lens[j])
            assert bool((per[:, o:o + m] == d_round[None, o:o + m]).all()), \
                f"round trip of stream {j} differs from the input"
    cbytes = int(cl.sum())
    ratio = cbytes / ubytes
    if rank == 0:
        log(f"[bench] {'parity ok; ' if gate else ''}compressed "
            f"{cbytes / GIB:.3f} GiB (ratio {ratio:.4f})")

    # ---- timed region ----------------------------------------------------
    def barrier():
        if world > 1:
            torch.distributed.barrier()
        ctx.synchronize()
        torch.cuda.synchronize()

    for _ in range(args.warmup):
        do_compress()
        do_decompress()
    barrier()
    k_comp_ms, k_dec_ms, t_comp, t_dec, compact_ms, plan_ms = [], [], 0.0, \
        0.0, [], []
    k_dom_ms = []
    w_comp, w_dec = [], []   # wall ms of every timed call (incl. its wait)
    comp_kernel, dec_kernel = "k_match_both", "k_decompress_streams3"
    t0 = time.perf_counter()
    for _ in range(args.steps):
        ta = time.perf_counter()
        tm = do_compress()
        comp_kernel = ctx.last_kernel()
        tb = time.perf_counter()
        td = do_decompress()
        dec_kernel = ctx.last_kernel()
        tc = time.perf_counter()
        k_comp_ms.append(tm["codec_ms"])
        k_dom_ms.append(tm["dominant_ms"])
        compact_ms.append(tm["compact_ms"])
        plan_ms.append(tm["plan_ms"])
        k_dec_ms.append(td["codec_ms"])
        t_comp += tb - ta
        t_dec += tc - tb
        w_comp.append((tb - ta) * 1e3)
        w_dec.append((tc - tb) * 1e3)
    barrier()
    elapsed = time.perf_counter() - t0
    # ---- the same gate AFTER the timed steps: what the last step left in
    # `comp` and `back` is still the oracle's bytes and the input
    verified_after = False
    placement_log = None
    if gate:
        cl2 = comp_lens.cpu().numpy()
        assert (cl2 == cl).all(), "compressed lengths changed during the run"
        assert (kinds(comp_errs) == 0).all() and (kinds(back_errs) == 0).all()
        for j in range(12):
            got = comp.stream_bytes(j, cl2[j])
            assert hashlib.sha256(got).hexdigest() == shas[j][2], \
                f"after the timed steps: stream {j} differs from the oracle's"
        if rounds > 1:
            perc = comp.data[:rounds * c_stride].view(rounds, c_stride)
            for r in {rounds // 2, rounds - 1}:
                for j in range(12):
                    o, m = int(comp.offsets[j]), int(cl2[j])
                    assert bool((perc[r, o:o + m] == perc[0, o:o + m]).all())
        for r in {0, rounds // 2, rounds - 1}:
            for j in range(12):
                o, m = int(r_offs[j]), int(r_lens[j])
                assert bool((per[r, o:o + m] == d_round[o:o + m]).all()), \
                    f"after the timed steps: round trip of stream {j}"
        verified_after = True
    dumped = None
    if args.dump_outputs and rank == 0:
        dumped = dump_outputs(args.dump_outputs, comp, comp_lens, comp_errs,
                              back, back_lens, back_errs, len(rnd))
        log(f"[bench] outputs of the last timed step in "
            f"{args.dump_outputs}: {dumped}")
    context_holds = None
    if rank == 0:
        placement_log = ctx.table_probe_log()
        log(f"[bench] lane-table placement: {placement_log}")
        # what the context holds behind the timed steps (snapmi_ctx_get_info:
        # the library's own count, compress and decompress scratch together)
        context_holds = {
            "scratch_bytes": ctx.info("scratch_bytes"),
            "token_scratch_bytes": ctx.info("token_scratch_bytes"),
            "token_scratch_over_input": round(
                ctx.info("token_scratch_bytes") / ubytes, 4),
            "token_pool_pct_now": ctx.info("token_pool_pct_now"),
            "token_blocks_spilled_last_launch":
                ctx.info("token_blocks_spilled")}
        log(f"[bench] the context holds: {context_holds}")
        log("[bench] compress kernel ms per step: "
            + " ".join(f"{x:.1f}/{y:.1f}" for x, y in zip(k_dom_ms, k_comp_ms))
            + " | decompress: " + " ".join(f"{x:.1f}" for x in k_dec_ms))
    per_rank = [[float(np.mean(k_dom_ms)), float(np.mean(k_comp_ms)),
                 float(np.mean(k_dec_ms)), elapsed / args.steps * 1e3]]
    # which physical device this rank drove (the N ranks of a real run must
    # have N different ones)
    props = torch.cuda.get_device_properties(dev)
    my_dev = str(getattr(props, "uuid", None) or
                 (getattr(props, "pci_domain_id", 0),
                  getattr(props, "pci_bus_id", local_rank),
                  getattr(props, "pci_device_id", 0)))
    coll_error = None
    if world > 1:
        try:
            t = torch.tensor([elapsed, t_comp, t_dec], dtype=torch.float64,
                             device=cdev)
            torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
            elapsed, t_comp, t_dec = t.tolist()
            mine = torch.tensor(per_rank[0], dtype=torch.float64, device=cdev)
            allr = [torch.zeros_like(mine) for _ in range(world)]
            torch.distributed.all_gather(allr, mine)
            per_rank = [x.tolist() for x in allr]
            seen = [None] * world
            torch.distributed.all_gather_object(seen, (rank, my_dev))
            ranks_seen = [r for r, _ in seen]
            devices_seen = [d for _, d in seen]
        except Exception as e:  # noqa: BLE001 - the line still gets printed
            coll_error = f"collective after the timed region: " \
                         f"{type(e).__name__}: {e}"[:300]
            log(f"[bench] rank {rank}: {coll_error}")
            ranks_seen, devices_seen = [rank], [my_dev]
    else:
        ranks_seen, devices_seen = [0], [my_dev]
    if world > 1 and not over and coll_error is None and \
            len(set(devices_seen)) != world:
        coll_error = (f"{world} ranks drove {len(set(devices_seen))} distinct "
                      f"device(s): {devices_seen}")

    # ---- extra configs (never part of `value`) ---------------------------
    extras = None
    if gate and not args.no_extras:
        # the extras need the memory (cfg3: 64 GiB in, 64 GiB framed, 64 GiB
        # decoded): drop the headline buffers and the context's scratch
        # (87 GB of lane tables); the extras run on a context of their own
        del src, comp, back, data, per, d_round
        ctx.close()
        torch.cuda.empty_cache()
        try:
            extras = run_extras(args, local_rank, dev, rank, world)
        except Exception as e:  # noqa: BLE001 - recorded, not hidden
            extras = {"error": f"{type(e).__name__}: {e}"[:300]}

    if rank == 0:
        K = args.steps
        total_u = ubytes * world
        value = 2.0 * total_u * K / elapsed / GIB
        comp_gibs = total_u * K / t_comp / GIB
        dec_gibs = total_u * K / t_dec / GIB
        # roofline of the dominant kernel (k_match_both: the lane kernel and
        # the window kernel on every CU; k_match_blocks below 6 GiB): algorithmic
        # bytes per launch = U read + C written ((1+rho) B per
        # uncompressed byte), over the HIP-event duration of that launch.
        kc = float(np.mean(k_comp_ms)) * 1e-3   # all compress-side kernels
        kdom = float(np.mean(k_dom_ms)) * 1e-3  # the dominant kernel alone
        kd = float(np.mean(k_dec_ms)) * 1e-3
        alg = ubytes + cbytes
        # k_match_blocks reads the input (U) and writes 8-byte tokens, the
        # encoder kernel writes C; the algorithmic bytes of the compress
        # direction (U + C) are charged to the dominant kernel's duration
        ach = alg / kdom / 1e9
        ach_d = alg / kd / 1e9
        # (the library says which kernels these were: snapmi_last_kernel)
        dom_name, dec_name = comp_kernel, dec_kernel
        # roofline.traffic: measured by this command (two PMC child runs) -
        # or, if that is switched off or fails, quoted from the committed
        # profile of the same workload and labelled as such
        traffic = traffic_d = None
        traffic_measured, traffic_note = False, None
        if gate and world == 1 and not args.no_pmc:
            try:
                # (the headline context's 87 GB of tables are still held:
                # the child runs need that memory)
                ctx.close()
                torch.cuda.empty_cache()
                m = measure_traffic(args, [dom_name, dec_name])
                traffic, traffic_d = m[dom_name], m[dec_name]
                traffic_measured = True
                traffic_note = ("this command: child runs of one step under "
                                "rocprofv3 --kernel-trace --pmc FETCH_SIZE / "
                                "--pmc WRITE_SIZE (separate passes), "
                                "FETCH_SIZE x2 + WRITE_SIZE, per launch")
            except Exception as e:  # noqa: BLE001 - recorded, not hidden
                traffic_note = f"PMC passes failed ({type(e).__name__}: {e})"[
                    :200]
        if not traffic_measured:
            pmc_name = None
            for cand in ("r6_pmc_traffic.json", "r5_pmc_traffic.json",
                         "r4_pmc_traffic.json",
                         "r3_pmc_traffic.json"):
                if (ROOT / "profiles" / cand).exists():
                    pmc_name = cand
                    break
            if pmc_name and abs(args.gib - 8.0) < 1e-9:
                pj = json.loads((ROOT / "profiles" / pmc_name).read_text())[
                    "kernels"]
                if dom_name in pj:
                    traffic = pj[dom_name]["traffic_bytes_fetch_x2"]
                if dec_name in pj:
                    traffic_d = pj[dec_name]["traffic_bytes_fetch_x2"]
            traffic_note = ((traffic_note + "; " if traffic_note else "")
                            + f"quoted from profiles/{pmc_name} (a committed "
                            "profile of the same workload, NOT this run)")
        line = {
            "metric": "GiB/s uncompressed (compress + decompress) on "
                      "zflat/uflat corpus",
            "value": round(value, 3), "unit": "GiB/s", "n_gpus": world,
            "steps": K, "warmup": args.warmup,
            "ms_per_step": round(elapsed / K * 1e3, 3),
            "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": "u8",
            "data": "synthetic (the reference's 12 bench inputs, committed "
                    "under tests/golden/corpus, tiled on the device)",
            "config": {
                "workload": (f"raw block codec, 12-stream zflat/uflat round "
                             f"tiled x{rounds} = {ubytes / GIB:.3f} GiB per "
                             f"GPU ({n} independent raw streams), compress "
                             f"then decompress, HBM-resident"),
                "streams_per_gpu": n, "ratio": round(ratio, 4),
                "lane_table_budget_pct": 33,
                "parallelism": f"shard-by-stream x{world}"},
            "compress_gibs": round(comp_gibs, 3),
            "decompress_gibs": round(dec_gibs, 3),
            "roofline": {
                "kernel": dom_name, "bound": "hbm",
                "achieved": round(ach, 2), "peak": HBM_PEAK_GBS,
                "unit": "GB/s", "frac": round(ach / HBM_PEAK_GBS, 5),
                "traffic": traffic,
                "traffic_measured": traffic_measured,
                "traffic_source": traffic_note,
                "alg_bytes_per_launch": alg,
                "avg_launch_ms": round(kdom * 1e3, 3),
                # which bytes: the algorithmic bytes of the compress
                # DIRECTION, U read + C written.  This kernel
                # reads U and writes tokens; C is written by k_encode_tokens
                # behind it - so the same bytes over the whole compress side:
                "bytes_counted": "U + C of the compress direction; C is "
                                 "written by k_encode_tokens behind this "
                                 "kernel (whole_side: both kernels' time)",
                "whole_side": {
                    "kernels": f"{dom_name} + k_scan_sizes + k_encode_tokens",
                    "avg_ms": round(kc * 1e3, 3),
                    "achieved": round(alg / kc / 1e9, 2),
                    "frac": round(alg / kc / 1e9 / HBM_PEAK_GBS, 5)}},
            "source_sha16": source_sha16(),
            "git_sha": os.environ.get("SNAPMI_GIT_SHA"),
            "placement": placement_log,
            "context_holds": context_holds,
            "first_compress_call_ms": round(first_call_ms, 1),
            "free_gib_around_first_call": [
                round(free_before_first / GIB, 1),
                round(free_after_first / GIB, 1)],
            "step_wall_ms": {"compress": [round(x, 2) for x in w_comp],
                             "decompress": [round(x, 2) for x in w_dec]},
            "roofline_decompress": {
                "kernel": dec_name, "bound": "hbm",
                "achieved": round(ach_d, 2), "peak": HBM_PEAK_GBS,
                "unit": "GB/s", "frac": round(ach_d / HBM_PEAK_GBS, 5),
                "traffic": traffic_d, "traffic_measured": traffic_measured,
                "alg_bytes_per_launch": alg,
                "avg_launch_ms": round(kd * 1e3, 3)},
            # median and min over the timed steps (HIP events)
            "kernel_ms_median": {
                "compress": round(float(np.median(k_comp_ms)), 3),
                "decompress": round(float(np.median(k_dec_ms)), 3)},
            "kernel_ms_min": {
                "compress": round(float(np.min(k_comp_ms)), 3),
                "decompress": round(float(np.min(k_dec_ms)), 3)},
            "kernel_ms": {"plan": round(float(np.mean(plan_ms)), 3),
                          "compress": round(kc * 1e3, 3),
                          "compress_dominant": round(kdom * 1e3, 3),
                          "compact": round(float(np.mean(compact_ms)), 3),
                          "decompress": round(kd * 1e3, 3)},
        }
        # per rank: [dominant compress kernel, all compress kernels,
        # decompress kernel, wall per step] in ms (HIP events / host clock)
        line["per_rank_ms"] = [[round(v, 3) for v in r] for r in per_rank]
        line["ranks_seen"] = sorted(ranks_seen)
        line["devices_seen"] = len(set(devices_seen))
        line["verified_after_timed_steps"] = verified_after
        if dumped is not None:
            line["dumped_outputs"] = dumped
        if coll_error is not None:
            line["error"] = coll_error
        if extras is not None:
            line["extras"] = extras
        if args.no_verify:
            line["INVALID"] = "experiment build, parity gate skipped"
        if over:
            line["INVALID"] = (f"oversubscribed: {world} ranks on one GPU over "
                               "gloo - a proof of the N > 1 code, not a "
                               "measurement")
        if args.full and world == 1 and not args.no_cpu:
            line["cpu_baseline"] = cpu_baseline(rnd)
        print(json.dumps(line), flush=True)
    if world > 1:
        hung = isinstance(extras, dict) and any(
            isinstance(v, dict) and v.get("hung") for v in extras.values())
        if hung or coll_error is not None:
            # a collective is stuck or failed: leave without waiting for it
            sys.stdout.flush()
            os._exit(4 if rank == 0 else 5)
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
