#!/usr/bin/env python3
"""bench.py -- KV blocks/s fetch+decompress on MI355X, against the HBM roofline.

    python bench.py --gpus N --steps K --warmup W
    (N > 1: python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...)

A "step" is one pass of the hot path over one batch: fetch + decompress every
4 KiB KV block of one Llama-3-8B-shaped sequence (BASELINE.json configs[1]:
32 layers, 8 KV heads, D=128, fp16, T=4096 -> 131 072 blocks = 512 MiB) from the
local-HBM pool into a contiguous fp16 destination, through the drop-in library's
C ABI (speckv_ext_fetch_range; one kernel launch).  The pool is populated (and
compressed on the GPU) before the timed region, so inputs are resident in HBM.

With N ranks the blocks shard naturally: every rank owns the pool of its own
sequence and decodes it locally -- no data-path collective, weak scaling.  Rank 0
prints ONE JSON line; `value` is whole-job blocks/s.

`roofline`     : the dominant kernel (k_fetch_decompress), algorithmic bytes per
                 launch / average launch duration from HIP events recorded on the
                 launch stream inside the timed region, vs 8 TB/s HBM3E.
`cpu_baseline` : the reference's own FPGACacheEngine::decompress (oracle/_ref,
                 kind "reference") or our C restatement (kind "port") timed on
                 this host's cores on a bounded sample of the same workload.

A plain run sets up, ramps the clocks, runs the W warm-up and K timed steps and
prints the line.  `--full` adds everything else: the as-called and sustained
variants, the parity spot check, the extras, `cpu_baseline` and, at N > 1, the
remote-pool (`xgmi`) phase.  `--dump-outputs DIR` writes a fixed sample of the
last timed step's destination (see dump_outputs()).
"""
import argparse
import json
import os
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBPS = 8000.0          # MI355X HBM3E spec peak (MI355X_MICROARCH.md)
EXTRAS_RAMP_MS = 25.0           # untimed clock ramp before each secondary measurement (see ramp())
PAGE = 4096
BLOCK_ELEMS = 2048
SCHEME_NAMES = {0: "fp16", 1: "int8", 2: "int8_delta_rle"}
# the arithmetic type of the path: int8 RLE records are expanded, prefix-summed in int8, dequantised in fp32
# (float(q) / 127.0f * scale, cache_engine.cpp:272-284) and rounded ONCE to the fp16 destination
DTYPE_LABEL = "fp32 (int8 records -> fp16)"


def set_tuning(key, value):
    """speckv_ext_set_tuning on the loaded library (the library reads its environment only once)."""
    import ctypes as C
    import cxl_speckv_amd as pkg
    lib = pkg.load_library()
    lib.speckv_ext_set_tuning.argtypes = [C.c_char_p, C.c_longlong]
    lib.speckv_ext_set_tuning.restype = C.c_int
    lib.speckv_ext_set_tuning(key.encode(), int(value))


def pmc_traffic(scheme, quant):
    """HBM bytes per launch of the dominant kernel from the committed rocprofv3
    --pmc passes of this same command (profiles/*_pmc.json, corrected as
    MI355X_MICROARCH.md prescribes).  PMC cannot be read from inside the run, so
    this is the profile's number, labelled with its source; None if absent."""
    import glob
    key = f"k_fetch_decompress<{scheme}, {quant}, false"
    for fn in sorted(glob.glob(os.path.join(ROOT, "profiles", "r[0-9][0-9]*_pmc.json")), reverse=True):
        try:
            d = next((v for k, v in json.load(open(fn))["pmc"].items() if k.startswith(key)), None)
        except Exception:
            d = None
        if d and d.get("hbm_traffic_bytes_per_launch"):
            return int(d["hbm_traffic_bytes_per_launch"]), os.path.relpath(fn, ROOT)
    return None, None


def parse_args():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--scheme", type=int, default=2, help="0 fp16, 1 int8, 2 int8+delta+rle (reference codec)")
    ap.add_argument("--quant", type=int, default=0, help="0 REF_EXACT (parity mode), 1 INTENT")
    ap.add_argument("--tokens", type=int, default=4096)
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-extras", action="store_true")
    ap.add_argument("--cpu-seconds", type=float, default=10.0)
    ap.add_argument("--ramp-ms", type=float, default=60.0, help="untimed clock ramp before the 'ramped' variant and the extras")
    ap.add_argument("--sustain-s", type=float, default=1.0, help="length of the 'sustained' variant")
    ap.add_argument("--no-variants", action="store_true", help="only the as-called figure (profiling runs)")
    ap.add_argument("--full", action="store_true",
                    help="everything beside the headline: the as-called and sustained variants, the parity spot check, the extras, "
                         "the CPU baseline and, at N > 1, the remote-pool phase (a plain run does only what `value` needs)")
    ap.add_argument("--dump-outputs", metavar="DIR",
                    help="after the timed steps, write a fixed sample of the last step's fp16 destination as DIR/<name>.npy (float32)")
    ap.add_argument("--xgmi-child", action="store_true", help=argparse.SUPPRESS)   # internal: see run_xgmi_children()
    return ap.parse_args()


# --------------------------------------------------------------------------
# CPU baseline (checker code, used here ONLY as the thing timed beside the GPU)
# --------------------------------------------------------------------------
def host_cpu_info():
    """(model string, physical cores, logical CPUs) of this host from /proc/cpuinfo (BASELINE.md section 3 asks for both)."""
    model, cores = None, set()
    try:
        phys = core = None
        for line in open("/proc/cpuinfo"):
            k, _, v = line.partition(":")
            k, v = k.strip(), v.strip()
            if k == "model name" and model is None: model = v
            elif k == "physical id": phys = v
            elif k == "core id": core = v
            elif not k and phys is not None:
                cores.add((phys, core)); phys = core = None
        if phys is not None: cores.add((phys, core))
    except OSError:
        pass
    return model or "unknown", len(cores) or None, os.cpu_count() or 1


def cpu_baseline(seconds, sample_blocks=None, seed=2001):
    """The CPU path timed beside the GPU figure, on this host's cores, on a bounded sample of the same workload.
    `kind: "reference"`: the reference's own FPGACacheEngine::decompress (oracle/_ref, compiled from /root/reference in the
    development container; present on the GPU box as a prebuilt .so).  `port`: our C restatement of it (oracle/), always
    timed and printed beside the reference figure (the restatement is what is guaranteed to travel)."""
    import ctypes as C
    from oracle.bindings import Oracle, Reference, have_reference, _ptr, f32p, u8p, u16p, u32p
    n_threads = os.cpu_count() or 1
    if sample_blocks is None:
        # >= 128 blocks per thread and call, so the ctypes call (GIL released) dominates the Python loop
        sample_blocks = max(8192, 128 * n_threads)
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((sample_blocks, BLOCK_ELEMS)).astype(np.float16)
    orc = Oracle()
    scales, lens, recs = orc.compress_blocks_f16(x, 2, 0)
    legs = 4 if have_reference() else 2
    leg_s = max(1.0, 2.0 * seconds / legs)           # the whole baseline stays at ~2 x seconds of wall time

    def port_work(lo, hi, out):
        y = np.empty((hi - lo, BLOCK_ELEMS), np.uint16)
        t0 = time.perf_counter(); done = 0
        while time.perf_counter() - t0 < leg_s:
            orc.lib.orc_decompress_blocks_f16(_ptr(recs[lo:hi], u8p), recs.shape[1], _ptr(lens[lo:hi], u32p), _ptr(scales[lo:hi], f32p),
                                              hi - lo, BLOCK_ELEMS, 2, 0, _ptr(y, u16p), 1)
            done += hi - lo
        out.append((done, time.perf_counter() - t0))

    def timed(work):
        # 1 thread (the reference is single-threaded behind one mutex) ...
        one = []
        work(0, min(1024, sample_blocks), one)
        v1 = one[0][0] / one[0][1]
        # ... and all host cores, one engine per thread over disjoint blocks
        outs, threads = [], []
        per = sample_blocks // n_threads
        for t in range(n_threads):
            th = threading.Thread(target=work, args=(t * per, (t + 1) * per, outs))
            th.start(); threads.append(th)
        for th in threads:
            th.join()
        return round(sum(d for d, _ in outs) / max(e for _, e in outs), 1), round(v1, 1)

    pv, pv1 = timed(port_work)
    cpu_model, physical, logical = host_cpu_info()
    host = {"cpu_model": cpu_model, "physical_cores": physical, "logical_cpus": logical,
            "cores_note": "`cores` = the threads that ran (one per logical CPU); physical_cores from /proc/cpuinfo"}
    port = {"value": pv, "value_1thread": pv1, "unit": "blocks/s", "cores": n_threads,
            "what": "oracle/speckv_oracle.c (C restatement), INT8_DELTA_RLE decompress to fp16 -- through a bit-by-bit software float -> half "
                    "conversion per element (no F16C intrinsics in a C99 checker), which is most of its distance to the reference's fp32 output"}
    sample = (f"{sample_blocks} N(0,1) fp16 blocks (seed {seed}), INT8_DELTA_RLE decompress, looped ~{leg_s:.0f}s per leg; "
              f"1 thread and {n_threads} threads (one engine each)")
    if not have_reference():
        return {"value": pv, "unit": "blocks/s", "cores": n_threads, "kind": "port", "value_1thread": pv1, "sample": sample, "port": port, **host}
    ref = Reference()
    L = ref.lib
    x32 = x.astype(np.float32)
    rrecs = np.zeros((sample_blocks, 2 * BLOCK_ELEMS), np.uint8)
    rlens = np.zeros(sample_blocks, np.uint32)
    rscales = np.zeros(sample_blocks, np.float32)
    L.ref_engine_compress_blocks(ref.engine, _ptr(x32, f32p), sample_blocks, BLOCK_ELEMS, _ptr(rscales, f32p),
                                 _ptr(rrecs, u8p), 2 * BLOCK_ELEMS, _ptr(rlens, u32p))

    def ref_work(lo, hi, out):
        eng = L.ref_engine_new()          # one engine per thread, disjoint blocks
        y = np.empty((hi - lo, BLOCK_ELEMS), np.float32)
        t0 = time.perf_counter(); done = 0
        while time.perf_counter() - t0 < leg_s:
            L.ref_engine_decompress_blocks(eng, _ptr(rrecs[lo:hi], u8p), 2 * BLOCK_ELEMS, _ptr(rlens[lo:hi], u32p),
                                           _ptr(rscales[lo:hi], f32p), hi - lo, _ptr(y, f32p), BLOCK_ELEMS)
            done += hi - lo
        out.append((done, time.perf_counter() - t0))
        L.ref_engine_delete(eng)

    rv, rv1 = timed(ref_work)
    return {"value": rv, "unit": "blocks/s", "cores": n_threads, "kind": "reference", "value_1thread": rv1,
            "sample": sample + "; reference = FPGACacheEngine::decompress to fp32", "port": port, **host}


# --------------------------------------------------------------------------
# clock ramp: an idle MI355X sits at 648 MHz sclk and needs ~8 ms (about 40 launches of the 180 us kernel) of
# continuous work before the shader clock settles: measured per-step durations 181-190 us for the first 40 steps,
# 171 us from then on (profiles/tools/step_trend.py).  Every timed region below is therefore preceded by an UNTIMED run of
# the same step for ramp_ms of wall time, in addition to the W warm-up steps of the contract.
# --------------------------------------------------------------------------
def ramp(fn, sync, ramp_ms):
    if ramp_ms <= 0:
        return 0
    t0 = time.perf_counter()
    n = 0
    while (time.perf_counter() - t0) * 1e3 < ramp_ms:
        for _ in range(8):
            fn()
        sync()
        n += 8
    return n


# --------------------------------------------------------------------------
# timing contract (shared with tests/test_multirank_cpu.py, which runs it under gloo)
# --------------------------------------------------------------------------
def run_timed(step, steps, warmup, sync, dist=None, warm=None, reduce_device="cpu"):
    """W untimed warmup steps, then EXACTLY `steps` timed steps bracketed by a
    barrier + device sync on both sides; returns the MAX elapsed over ranks."""
    import torch
    for _ in range(warmup):
        (warm or (lambda: step(0)))()
    if dist is not None:
        dist.barrier()
    sync()
    t0 = time.perf_counter()
    for i in range(steps):
        step(i)
    sync()
    if dist is not None:
        dist.barrier()
    elapsed = time.perf_counter() - t0
    if dist is not None:
        t = torch.tensor([elapsed], dtype=torch.float64, device=reduce_device)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    return elapsed


def whole_job_rate(world, units_per_rank, steps, elapsed):
    """Units all ranks processed / max-over-ranks time (weak scaling: per-rank work fixed)."""
    return world * units_per_rank * steps / elapsed


DUMP_ROWS = 4096                # 4096 blocks x 2048 fp32 = 32 MiB, under the 64 MB a dump may take


def dump_rows(n_blocks):
    """The blocks --dump-outputs writes: a fixed, seeded sample (the same for every run of the same shape), first and last included."""
    if n_blocks <= DUMP_ROWS:
        return np.arange(n_blocks)
    rows = np.random.default_rng(4242).choice(np.arange(1, n_blocks - 1), size=DUMP_ROWS - 2, replace=False)
    return np.concatenate(([0], np.sort(rows), [n_blocks - 1]))


def dump_outputs(out_dir, name, dst, n_blocks):
    """What a caller of the timed path receives: the fp16 destination of the last timed step, as float32 (exact)."""
    import torch
    os.makedirs(out_dir, exist_ok=True)
    torch.cuda.synchronize()
    rows = torch.from_numpy(dump_rows(n_blocks)).to(dst.device)
    np.save(os.path.join(out_dir, f"{name}.npy"), dst.index_select(0, rows).float().cpu().numpy())


def spawn_own_ranks(args):
    """`python bench.py --gpus N` with N > 1 and no launcher around it: start the N ranks ourselves, one per GPU, as a
    CHILD `python -m torch.distributed.run` of this same script with the same arguments, pass its output through (rank 0
    prints the one JSON line) and leave with its exit code.  Called before torch is imported or anything touches the
    GPU: this process never initialises HIP, and nothing is exec'ed."""
    import socket
    import subprocess
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")       # dmabuf IPC: RCCL / peer mappings across processes
    env.setdefault("OMP_NUM_THREADS", "1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    return subprocess.call(cmd, env=env)


def host_dry_run(args, world, rank):
    """SPECKV_BENCH_HOST_DRY_RUN=1 (tests/test_multirank_cpu.py, no GPU in the container): the ranks go through the same
    launcher, rendezvous, timing contract and rank-0 line as a real run, with a host-side sleep in place of the step.  The
    line says so (`dry_run`); it is never a measurement."""
    import torch.distributed as dist
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    dist.init_process_group(backend="gloo")
    elapsed = run_timed(lambda i: time.sleep(0.002), args.steps, args.warmup, lambda: None, dist)
    n_blocks = args.tokens * args.layers * 8 * 128 * 2 * 2 // PAGE
    if rank == 0:
        print(json.dumps({"metric": "KV blocks/s fetch+decompress", "value": round(whole_job_rate(world, n_blocks, args.steps, elapsed), 1),
                          "unit": "blocks/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
                          "ms_per_step": round(elapsed / args.steps * 1e3, 4), "dry_run": "host sleep in place of the step: not a measurement"}),
              flush=True)
    dist.barrier()
    dist.destroy_process_group()
    return 0


def main():
    args = parse_args()
    if args.xgmi_child:
        return xgmi_child_main(args)
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(spawn_own_ranks(args))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    if world != args.gpus:                                   # never a 1-GPU line labelled as N, or the reverse
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
    if os.environ.get("SPECKV_BENCH_HOST_DRY_RUN") == "1":
        return host_dry_run(args, world, rank)
    import torch
    import cxl_speckv_amd as pkg

    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    # test hook (one-GPU boxes): SPECKV_BENCH_SINGLE_GPU_TEST=1 runs every rank on GPU 0
    # with gloo so the N>1 control flow can be exercised without a second GPU
    single_gpu_test = os.environ.get("SPECKV_BENCH_SINGLE_GPU_TEST") == "1"
    xgmi_wanted = args.full and world > 1 and os.environ.get("SPECKV_BENCH_XGMI", "1") != "0"
    xgmi_early = single_gpu_test and xgmi_wanted
    if xgmi_early:
        # every rank and every remote-pool child on the one GPU: the children run FIRST, before any rank opens the GPU, so
        # that N ranks and N children never hold it at the same time (at N = 8 that would be 16 processes on one GPU)
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group(backend="gloo")
        x_early = run_xgmi_children(args, torch, dist, rank, world, "cpu")
    assert torch.cuda.is_available(), "bench.py needs the MI355X (no CPU fallback for the data path)"
    if single_gpu_test:
        local_rank = 0
    torch.cuda.set_device(local_rank)
    dist = None
    red_dev = "cuda"
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if single_gpu_test:
            if not dist.is_initialized():
                dist.init_process_group(backend="gloo")
            red_dev = "cpu"
        else:
            dist.init_process_group(backend="nccl", device_id=torch.device("cuda", local_rank))

    # Everything after the main measurement is guarded by a watchdog: if a later phase wedges (the remote phase runs
    # on hardware the development pool does not have) the line collected so far is printed WITH a marker and the
    # process exits non-zero -- a hang is never reported as a clean run.
    state = {"out": None, "phase": "setup", "emitted": False}
    lock = threading.Lock()

    def emit():
        with lock:
            if rank == 0 and state["out"] is not None and not state["emitted"]:
                state["emitted"] = True
                print(json.dumps(state["out"]), flush=True)

    def bail():
        if state["out"] is not None:
            state["out"]["watchdog_fired"] = {"phase": state["phase"],
                                              "after_s": float(os.environ.get("SPECKV_BENCH_WATCHDOG_S", "420"))}
            if state["phase"].startswith("xgmi"):
                state["out"].setdefault("xgmi", {})["skipped"] = "watchdog"
        emit()
        os._exit(3)                      # never restart / re-exec a process that has touched the GPU

    dog = threading.Timer(float(os.environ.get("SPECKV_BENCH_WATCHDOG_S", "420")), bail)
    dog.daemon = True
    dog.start()

    T, Lyr, H, D, bpe = args.tokens, args.layers, 8, 128, 2
    kv = pkg.CxlSpeckvKVAllocator(pkg.library_path(), f"hip:{local_rank}")
    lib = kv.lib
    lib.set_compression_scheme(args.scheme)
    lib.set_quant_mode(args.quant)
    handle = kv.allocate(T, Lyr, H, D, bpe)
    n_blocks = T * Lyr * H * D * bpe * 2 // PAGE
    # a dedicated HIP stream: the kernels are launched on it and the HIP events
    # that time them are recorded on it (the NULL stream means "engine stream"
    # to the library)
    stream = torch.cuda.Stream()
    sp = stream.cuda_stream
    assert sp != 0

    # synthetic KV: N(0,1) fp16 in the shim layout [req][layer][kind][pos][head][D]
    g = torch.Generator(device="cuda"); g.manual_seed(2001 + rank)
    src = torch.randn((n_blocks, BLOCK_ELEMS), generator=g, device="cuda", dtype=torch.float32).to(torch.float16)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    lib.write(handle, 0, src.data_ptr(), src.numel() * 2, on_device=True)      # compress into the pool
    compress_s = time.perf_counter() - t0
    dst = torch.empty((n_blocks, BLOCK_ELEMS), dtype=torch.float16, device="cuda")

    # every step is ONE launch of the dominant kernel; the count lets profiles/summarize_r04.py find the timed launches
    # of each variant in the rocprofv3 per-dispatch trace of this same process (0-based, in dispatch order, counted over
    # the launches of this template instance only)
    launches = [0]

    def step():
        lib.fetch_range(handle, 0, n_blocks, dst.data_ptr(), False, sp)
        launches[0] += 1

    # HIP events on the launch stream bracket the timed region; the dominant
    # kernel's average launch duration is that interval / K (one launch per step)
    def timed_region(steps, warmup):
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

        def timed_step(i):
            if i == 0:
                ev0.record(stream)
            step()
            if i == steps - 1:
                ev1.record(stream)
        first = launches[0] + warmup
        elapsed = run_timed(timed_step, steps, warmup, torch.cuda.synchronize, dist, warm=lambda: step(), reduce_device=red_dev)
        assert launches[0] == first + steps
        return elapsed, ev0.elapsed_time(ev1) / steps, [first, first + steps - 1]

    def alg():
        # c_i + 4 + 4096 per block; the record lengths are read back after the timed regions (it is a
        # device-to-host copy of the page table: not something to put between pool setup and the first timed step)
        return lib.stats().compressed_bytes + n_blocks * (4 + PAGE)

    def figure(elapsed, kern_ms, steps, span):
        return {"blocks_per_s": round(whole_job_rate(world, n_blocks, steps, elapsed), 1),
                "ms_per_step": round(elapsed / steps * 1e3, 4), "avg_launch_ms": round(kern_ms, 4), "steps": steps,
                "frac_hbm": round(alg_bytes / (kern_ms * 1e-3) / 1e9 / HBM_PEAK_GBPS, 4), "launches": span}

    # Three figures of the same step ("harden the headline"):
    #   as_called  W warm-up steps, then exactly K timed steps, first thing after pool setup (an idle MI355X sits at
    #              648 MHz and needs ~8 ms of work to reach its clocks; W = 5 steps are 0.9 ms)
    #   ramped     the same W + K after ramp_ms of untimed launches of the same step: the contract's timed region at
    #              steady clocks -- this is `value` (as in round 1, so rounds compare)
    #   sustained  at least sustain_s seconds of back-to-back launches
    # A plain run measures only the figure that is `value`; the other two are --full.
    state["phase"] = "main"
    torch.cuda.synchronize()
    variants = {}
    if args.full or args.no_variants:
        e1, k1, s1 = timed_region(args.steps, args.warmup)
        note = "--warmup steps only, straight after pool setup (cold clocks)"
        variants["as_called"] = (e1, k1, args.steps, s1), dict(note=note + ("; this is `value` (--no-variants)" if args.no_variants else ""))
    if args.no_variants:
        elapsed, kern_ms = e1, k1
    else:
        ramp_steps = ramp(step, torch.cuda.synchronize, args.ramp_ms)
        elapsed, kern_ms, s2 = timed_region(args.steps, args.warmup)
        variants["ramped"] = (elapsed, kern_ms, args.steps, s2), dict(untimed_ramp_ms=args.ramp_ms, untimed_ramp_steps=ramp_steps,
                                                                     note="same W + K steps after an untimed clock ramp; this is `value`")
        if args.full:
            n_sus = max(args.steps, int(1.03 * args.sustain_s / max(kern_ms * 1e-3, 1e-6)) + 1)    # a little over: steps may run faster than the ramped figure
            e3, k3, s3 = timed_region(n_sus, 0)
            variants["sustained"] = (e3, k3, n_sus, s3), dict(seconds=round(e3, 3), note=f">= {args.sustain_s} s of back-to-back launches")
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, "fetch_decompress_fp16" + (f"_rank{rank}" if world > 1 else ""), dst, n_blocks)
    alg_bytes = alg()
    variants = {k: dict(figure(*fig), **extra) for k, (fig, extra) in variants.items()}

    # parity spot check without any checker code in the loop: the reference's own vectors (tests/golden/
    # codec_vectors.npz: inputs, RLE bytes, scale bits and fp32 outputs recorded from the reference) go through
    # the same engine entry points the timed step uses, plus the size-independent properties of the timed data
    # (every record length positive, logical ids as the reference computes them).
    parity = None
    if args.full and rank == 0 and args.scheme == 2 and args.quant == 0:
        gold = np.load(os.path.join(ROOT, "tests", "golden", "codec_vectors.npz"))
        names = [k[:-2] for k in gold.files if k.endswith(".x") and gold[k].size == BLOCK_ELEMS]
        x16 = np.stack([gold[f"{nm}.x"] for nm in names]).astype(np.float16)
        hg = lib.alloc(len(names) * PAGE)
        lib.write(hg, 0, x16.ctypes.data, x16.nbytes, False)
        yg = torch.empty((len(names), BLOCK_ELEMS), dtype=torch.float32, device="cuda")
        lib.fetch_range(hg, 0, len(names), yg.data_ptr(), True, sp)
        torch.cuda.synchronize()
        got = yg.cpu().numpy()
        parity = True
        for j, nm in enumerate(names):
            info = lib.translate(hg, j * PAGE)
            parity = parity and info.rec_bytes == gold[f"{nm}.rle"].size
            parity = parity and np.float32(info.scale).tobytes() == gold[f"{nm}.scale"][0].tobytes()
            parity = parity and got[j].view(np.uint32).tobytes() == gold[f"{nm}.y"].view(np.uint32).tobytes()
            parity = parity and info.phys_page_id == 0x4000000000 + (hg << 20) + (j << 12)
        lib.free(hg)
        for pg in (0, n_blocks // 2, n_blocks - 1):
            info = lib.translate(handle, pg * PAGE)
            parity = parity and 2 <= info.rec_bytes <= 2 * BLOCK_ELEMS and info.phys_page_id == 0x4000000000 + (handle << 20) + (pg << 12)
        parity = bool(parity)

    if rank == 0:
        achieved = alg_bytes / (kern_ms * 1e-3) / 1e9
        traffic, traffic_src = (pmc_traffic(args.scheme, args.quant)
                                if (T, Lyr) == (4096, 32) else (None, None))
        state["out"] = {
            "metric": "KV blocks/s fetch+decompress",
            "value": round(whole_job_rate(world, n_blocks, args.steps, elapsed), 1),
            "unit": "blocks/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(elapsed / args.steps * 1e3, 4),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": DTYPE_LABEL,
            "data": "synthetic",
            "config": {
                "workload": f"BASELINE configs[1]: 1xMI355X local-HBM pool, Llama-3-8B-shaped KV ({Lyr} layers, 8 KV heads, "
                            f"D=128, fp16, T={T}) = {n_blocks} x 4 KiB blocks per GPU, fetch+decompress all blocks per step",
                "scheme": SCHEME_NAMES[args.scheme],
                "quantiser": "REF_EXACT" if args.quant == 0 else "INTENT",
                "blocks_per_gpu": n_blocks,
                "parallelism": f"blocks sharded over {world} rank(s), no data-path collective",
            },
            "roofline": {
                "bound": "hbm",
                "kernel": "k_fetch_decompress",
                "achieved": round(achieved, 1),
                "peak": HBM_PEAK_GBPS,
                "unit": "GB/s",
                "frac": round(achieved / HBM_PEAK_GBPS, 4),
                "traffic": traffic,
                "traffic_source": traffic_src,
                "algorithmic_bytes_per_launch": int(alg_bytes),
                "avg_launch_ms": round(kern_ms, 4),
                **({"frac_as_called": variants["as_called"]["frac_hbm"],
                    "avg_launch_ms_as_called": variants["as_called"]["avg_launch_ms"]} if "as_called" in variants else {}),
                "launches": {"kernel_instance": f"k_fetch_decompress<{args.scheme}, {args.quant}, false, 0>",
                             **{k: v["launches"] for k, v in variants.items()},
                             "note": "0-based indices of this instance's dispatches in this process, in dispatch order: "
                                     "profiles/summarize_r04.py averages the same dispatches in the rocprofv3 kernel trace"},
                "bytes_per_block": round(alg_bytes / n_blocks, 1),
                "timed_region": "W warm-up steps then exactly K steps, preceded by an untimed clock ramp (variants.ramped); "
                                "the cold as-called figure and a >= 1 s sustained one are in `variants` with --full",
            },
            "variants": variants,
            "compress_s_untimed": round(compress_s, 4),
        }
        if args.full:
            state["out"].update(parity_spot_check=parity, extras={})
    out = state["out"]
    extras_wanted = args.full and not args.no_extras

    if rank == 0 and world == 1 and extras_wanted:           # secondary measurements: single-GPU runs only
        state["phase"] = "extras"
        with torch.cuda.stream(stream):
            extras = run_extras(torch, pkg, lib, src, dst, n_blocks, sp)
        extras.update(run_engine_extras(torch, kv, handle, n_blocks, T, Lyr))
        out["extras"] = extras

    kv.close()
    if rank == 0 and world == 1 and extras_wanted:
        state["phase"] = "extras:flush_cfg4"
        out["extras"].update(flush_cfg4_extra(torch, pkg))
        state["phase"] = "extras:striped_attention"
        out["extras"].update(striped_attention_extra(torch, pkg))
    if xgmi_wanted:
        state["phase"] = "xgmi"
        del src, dst
        torch.cuda.empty_cache()
        x = x_early if xgmi_early else run_xgmi_children(args, torch, dist, rank, world, red_dev)   # rank 0 alone gets the object
        if rank == 0 and out is not None:
            out["xgmi"] = x
            rx = roofline_xgmi_from(x, world)
            out["roofline_xgmi"] = rx
            if rx and rx.get("frac") is not None and "skipped" not in rx:
                # north_star's second fraction, beside the HBM one, in the object the driver reads
                out["roofline"]["xgmi"] = {"frac": rx["frac"], "achieved": rx["achieved"], "peak": rx["peak_nominal_per_direction"],
                                           "unit": "GB/s", "links": rx["links"], "layout": rx["layout"], "engine": rx["engine"]}
                if os.environ.get("SPECKV_BENCH_SINGLE_GPU_TEST") == "1":
                    out["roofline"]["xgmi"]["one_gpu_dry_run"] = "every 'peer' is the same GPU: no link was crossed, the fraction means nothing"
                # `value` at N > 1 is replica weak scaling of the LOCAL path (every rank decodes its own pool); north_star's
                # remote fetch is a different figure and stands beside it at the top level so that nobody mistakes one for the other
                out["north_star_fields"] = {"xgmi_remote_fetch_at_N_gpus": "value_remote_fetch_GBps_inbound (and roofline.xgmi.frac: target >= 0.60)",
                                            "hbm_local_decompress": "roofline.frac (target >= 0.70)",
                                            "not_a_north_star_figure": "value at N > 1 (replica weak scaling of the local path)"}
                out["value_remote_fetch_blocks_per_s"] = rx.get("blocks_per_s")
                out["value_remote_fetch_GBps_inbound"] = rx["achieved"]
                out["value_note"] = ("`value` = blocks/s of the local fetch+decompress path summed over ranks (replicas, no exchange: linear by "
                                     "construction); value_remote_fetch_* = 1 compute GPU fetching from its N-1 pool GPUs over xGMI "
                                     f"({rx['layout']}, {rx['engine']}); roofline.xgmi.frac is that figure over links x 153.6 GB/s")
    if rank == 0 and world == 1 and args.full and not args.no_cpu_baseline:   # rank 0 at N=1 only (bench contract)
        state["phase"] = "cpu_baseline"
        try:
            out["cpu_baseline"] = cpu_baseline(args.cpu_seconds)
        except Exception as e:                                  # the checker must never cost the result
            out["cpu_baseline"] = {"error": repr(e)}
    elif rank == 0 and world > 1 and args.full:
        out["cpu_baseline"] = None                              # measured by the N=1 run
    dog.cancel()
    emit()
    if dist:
        dist.barrier()
        dist.destroy_process_group()


# --------------------------------------------------------------------------
# Remote-pool (xGMI) phase.  It runs on hardware the development pool does not have, so it is isolated: every rank starts
# a CHILD process (a fresh interpreter, never an exec of this one) that does the whole phase with its own process group
# (file-store rendezvous) and the rank-0 child prints the `xgmi` object on its stdout.  A crash or hang there costs the
# `xgmi` object -- reported as {"failed": ...} with the child's last stderr lines -- and never the scaling line.
# --------------------------------------------------------------------------
def run_xgmi_children(args, torch, dist, rank, world, red_dev):
    import subprocess
    import tempfile
    t = torch.tensor([os.getpid() if rank == 0 else 0], dtype=torch.int64, device=red_dev)
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    store = os.path.join(tempfile.gettempdir(), f"speckv_xgmi_{os.environ.get('MASTER_PORT', '0')}_{int(t.item())}")
    limit = float(os.environ.get("SPECKV_XGMI_TIMEOUT_S", "240"))
    env = dict(os.environ, SPECKV_XGMI_STORE=store)
    cmd = [sys.executable, os.path.abspath(__file__), "--xgmi-child", "--gpus", str(args.gpus), "--steps", str(args.steps),
           "--warmup", str(args.warmup), "--scheme", str(args.scheme), "--quant", str(args.quant), "--tokens", str(args.tokens),
           "--layers", str(args.layers), "--ramp-ms", str(args.ramp_ms)]
    errf = tempfile.TemporaryFile(mode="w+")
    res = None
    try:
        proc = subprocess.Popen(cmd, env=env, stdout=subprocess.PIPE, stderr=errf, text=True)
        try:
            so, _ = proc.communicate(timeout=limit)
            rc = proc.returncode
        except subprocess.TimeoutExpired:
            proc.kill()                                          # exactly the child this rank started
            so, _ = proc.communicate()
            rc = "timeout"
        if rank == 0:
            for line in reversed((so or "").splitlines()):
                at = line.find('{"')
                if at >= 0:
                    try:
                        res = json.loads(line[at:])
                        break
                    except ValueError:
                        pass
            if res is None or rc != 0:
                errf.seek(0)
                tail = errf.read()[-1500:]
                res = dict(res or {}, failed=f"child of rank 0 ended with {rc!r} after at most {limit:.0f} s", stderr_tail=tail)
    except Exception as e:
        res = {"failed": repr(e)}
    finally:
        errf.close()
    dist.barrier()
    if rank == 0:
        try:
            os.remove(store)
        except OSError:
            pass
    return res


def xgmi_child_main(args):
    import torch
    import torch.distributed as dist
    import cxl_speckv_amd as pkg
    world, rank, local_rank = int(os.environ["WORLD_SIZE"]), int(os.environ["RANK"]), int(os.environ.get("LOCAL_RANK", "0"))
    single_gpu_test = os.environ.get("SPECKV_BENCH_SINGLE_GPU_TEST") == "1"
    if single_gpu_test:
        local_rank = 0
    torch.cuda.set_device(local_rank)
    init = "file://" + os.environ["SPECKV_XGMI_STORE"]
    if single_gpu_test:
        dist.init_process_group(backend="gloo", init_method=init, rank=rank, world_size=world)
        red_dev = "cpu"
    else:
        dist.init_process_group(backend="nccl", init_method=init, rank=rank, world_size=world, device_id=torch.device("cuda", local_rank))
        red_dev = "cuda"
    n_blocks = args.tokens * args.layers * 8 * 128 * 2 * 2 // PAGE
    g = torch.Generator(device="cuda"); g.manual_seed(2001 + rank)
    src = torch.randn((n_blocks, BLOCK_ELEMS), generator=g, device="cuda", dtype=torch.float32).to(torch.float16)
    dst = torch.empty((n_blocks, BLOCK_ELEMS), dtype=torch.float16, device="cuda")
    stream = torch.cuda.Stream()
    x = xgmi_phase(args, torch, pkg, dist, rank, local_rank, world, src, dst, stream, red_dev, single_gpu_test, None)
    if rank == 0:
        print(json.dumps(x), flush=True)
    dist.barrier()
    dist.destroy_process_group()


XGMI_LINK_GBPS = 153.6          # nominal per link (task statement: 7 links x ~153 GB/s per GPU)
XGMI_MODES = ("cfg3", "cfg4", "symmetric")


def pool_devices_for(mode, rank, world):
    """Which GPUs hold the pool of `rank` in each remote-fetch mode (None = this rank only idles at the barriers).
      cfg3      BASELINE configs[2]: rank 0 computes, the pool lives entirely on GPU 1
      cfg4      BASELINE configs[3]: rank 0 computes, pool striped page % (N-1) over ALL other GPUs
      symmetric every rank computes, its pool striped over its N-1 peers (each GPU is compute and 1/(N-1) of N-1 pools)
    Pure function of (mode, rank, world): tests/test_multirank_cpu.py cross-checks it between ranks under gloo."""
    others = [d for d in range(world) if d != rank]
    if mode == "symmetric":
        return others
    if rank != 0 or not others:
        return None
    if mode == "cfg3":
        return others[:1]
    if mode == "cfg4":
        return others
    raise ValueError(mode)


MALL_BYTES = 256 << 20           # Infinity Cache per GPU (MI355X_MICROARCH.md): SURVEY 8(d) wants the remote set >= 10x this per pool GPU


def xgmi_sets_for(n_pool_gpus, set_bytes, single_gpu_test):
    """How many copies of the 8B-shaped set (one allocation each) the remote working set holds, so that every pool GPU
    keeps at least 10 x MALL of records.  SPECKV_XGMI_SETS overrides; the one-GPU dry run keeps 2."""
    env = os.environ.get("SPECKV_XGMI_SETS")
    if env:
        return max(1, int(env))
    if single_gpu_test:
        return 2
    return max(1, -(-21 * MALL_BYTES * n_pool_gpus // (2 * max(set_bytes, 1))))      # 10.5x: records are a little smaller than their 4 KiB pages


def xgmi_mode_plan(mode, rank, world, set_bytes, single_gpu_test, device_count):
    """What `rank` does in remote-fetch mode `mode` -- a pure function of its arguments, so that the branch a real 8-GPU node
    takes can be asserted on a machine without one (tests/test_multirank_cpu.py runs it for every rank of world 8 with
    device_count = 8): which GPUs hold its pool, the SPECKV_POOL_DEVICES value it opens the engine with, how many allocations of
    the 8B-shaped set make the remote working set (>= 10 x the Infinity Cache per pool GPU), the per-peer copy streams the copy
    engine will use (one per pool GPU), and a pessimistic wall-time estimate of the mode (every byte at 40 GB/s per link:
    one compressing write of the set + 10 timed passes x 2 engines x {records, fp16 pages})."""
    pools = pool_devices_for(mode, rank, world)
    links = len(pool_devices_for(mode, 0, world))
    n_sets = xgmi_sets_for(links, set_bytes, single_gpu_test)
    plan = {"active": pools is not None, "pools": pools, "links": links, "n_sets": n_sets, "error": None,
            "working_set_bytes": n_sets * set_bytes, "working_set_bytes_per_pool_gpu": n_sets * set_bytes // max(links, 1),
            "peer_streams": len(pools) if pools else 0, "pool_devices_env": None}
    if pools is not None:
        if not single_gpu_test and device_count < world:
            plan["error"] = f"only {device_count} devices visible to this rank"
        else:
            plan["pool_devices_env"] = ",".join(str(d) for d in ([0] * len(pools) if single_gpu_test else pools))
    passes = 1 + 10 * 2 * 2
    plan["expected_wall_s_at_40GBps_per_link"] = round(plan["working_set_bytes"] * passes / (40e9 * max(links, 1)) + 20.0, 1)
    return plan


def xgmi_phase(args, torch, pkg, dist, rank, local_rank, world, src, dst, stream, red_dev="cuda", single_gpu_test=False, state=None):
    """Remote fetch over xGMI in the three shapes of pool_devices_for(), each with both fetch engines: the fused
    peer-load + decompress kernel (engine 1) and the copy engines (engine 2: one hipMemcpyPeerAsync per pool GPU and
    chunk on per-peer streams into local staging, local decompress), a speculative-prefetch leg (BASELINE configs[2]
    verbatim: look-ahead depth 4 per (sequence, layer), device-side flush, pages fetched into the L2 ring over the
    link), plus a raw peer-copy calibration of the same links.  Inbound GB/s is per compute GPU; fractions are given
    against the nominal link figure under BOTH readings of it (153.6 GB/s per link counted per direction, or as the
    sum of both directions = 76.8 inbound) and against the raw copy measured here."""
    def all_ok(flag):
        t = torch.tensor([1 if flag else 0], dtype=torch.int32, device=red_dev)
        dist.all_reduce(t, op=dist.ReduceOp.MIN)
        return bool(t.item())

    def max_over_ranks(v):
        t = torch.tensor([float(v)], dtype=torch.float64, device=red_dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return float(t.item())

    n_blocks = src.shape[0]
    sp = stream.cuda_stream
    steps = max(1, min(args.steps, 10))
    result = {"link_nominal_GBps": XGMI_LINK_GBPS,
              "accounting": "frac_nominal_per_direction = inbound / (links x 153.6); frac_nominal_bidirectional = inbound / "
                            "(links x 76.8) if 153.6 is the sum of both directions; frac_of_raw_copy = inbound / the raw "
                            "hipMemcpy rate measured on the same links in the same phase.  inbound = record bytes (what the "
                            "decoder needs) per second; the copy engines move whole record SLOTS: their actual link bytes are "
                            "reported beside it (copy_engine_link_bytes_per_pass, link_GBps_actual)"}
    for mode in XGMI_MODES:
        if state is not None:
            state["phase"] = f"xgmi:{mode}"
        if mode == "cfg4" and world == 2:
            result[mode] = {"same_as": "cfg3", "note": "with 2 GPUs the striped pool has one peer"}
            continue
        plan = xgmi_mode_plan(mode, rank, world, n_blocks * PAGE, single_gpu_test, torch.cuda.device_count())
        pools, active, links, n_sets = plan["pools"], plan["active"], plan["links"], plan["n_sets"]
        info = {"compute_ranks": world if mode == "symmetric" else 1, "pool_gpus_per_compute_gpu": links, "links": links,
                "expected_wall_s_at_40GBps_per_link": plan["expected_wall_s_at_40GBps_per_link"]}
        kv2, err, rec_bytes, handles = None, None, 0, []
        try:
            if active:
                if plan["error"]:
                    raise RuntimeError(plan["error"])
                os.environ["SPECKV_POOL_DEVICES"] = plan["pool_devices_env"]
                kv2 = pkg.CxlSpeckvKVAllocator(pkg.library_path(), f"hip:{local_rank}")
                lib = kv2.lib
                lib.set_compression_scheme(args.scheme)
                lib.set_quant_mode(args.quant)
                # the remote working set: n_sets allocations of the 8B-shaped set (same synthetic KV in each: bytes are what
                # count), sized so that every pool GPU holds >= 10 x its Infinity Cache
                for i in range(n_sets):
                    h = kv2.allocate(args.tokens, args.layers, 8, 128, 2)
                    lib.write(h, 0, src.data_ptr(), src.numel() * 2, on_device=True)   # compress straight into peer HBM
                    handles.append(h)
                rec_bytes = lib.stats().compressed_bytes
        except Exception as e:
            err = repr(e)
        finally:
            os.environ.pop("SPECKV_POOL_DEVICES", None)
        if not all_ok(err is None):
            if kv2 is not None:
                kv2.close()
            info["skipped"] = err or "another rank could not open its peer pool"
            result[mode] = info
            continue
        per_pool = max_over_ranks(rec_bytes) / max(links, 1)
        info["working_set"] = {"allocations": n_sets, "record_bytes_per_compute_gpu": int(max_over_ranks(rec_bytes)),
                               "record_MiB_per_pool_gpu": round(per_pool / 2**20, 1), "x_infinity_cache": round(per_pool / MALL_BYTES, 2),
                               "meets_10x_infinity_cache": bool(per_pool >= 10 * MALL_BYTES),
                               "note": "SURVEY 8(d): the remote set should exceed the pool GPU's 256 MiB Infinity Cache by >= 10x"
                                       + ("; the one-GPU dry run keeps it small on purpose" if single_gpu_test else "")}
        # raw calibration: one large device-to-device copy from EVERY pool GPU of this rank at once, each on its own stream
        raw, raw_err = None, None
        try:
            if active:
                nbytes = 128 << 20
                me = 0 if single_gpu_test else local_rank
                bufs = []
                for d in ([0] * len(pools) if single_gpu_test else pools):
                    bufs.append((torch.empty(nbytes, dtype=torch.uint8, device=f"cuda:{d}"),
                                 torch.empty(nbytes, dtype=torch.uint8, device=f"cuda:{me}"), torch.cuda.Stream(device=me)))
                for r_, l_, s_ in bufs:
                    with torch.cuda.stream(s_):
                        l_.copy_(r_, non_blocking=True)
                torch.cuda.synchronize()
        except Exception as e:
            raw_err = repr(e)
        ok = all_ok(raw_err is None)
        dist.barrier()
        if ok and active:
            t0 = time.perf_counter()
            for _ in range(4):
                for r_, l_, s_ in bufs:
                    with torch.cuda.stream(s_):
                        l_.copy_(r_, non_blocking=True)
            torch.cuda.synchronize()
            raw = 4 * len(bufs) * nbytes / (time.perf_counter() - t0) / 1e9
            del bufs
        if not ok:
            info["raw_copy_skipped"] = raw_err or "failed on another rank"
        all_ok(True)
        rawm = max_over_ranks(raw or 0.0)

        def rates(gbps):
            e = {"frac_nominal_per_direction": round(gbps / (XGMI_LINK_GBPS * links), 4),
                 "frac_nominal_bidirectional": round(gbps / (XGMI_LINK_GBPS / 2 * links), 4)}
            if rawm > 0:
                e["frac_of_raw_copy"] = round(gbps / rawm, 4)
            return e

        for engine, ename in ((1, "fused_peer_load_kernel"), (2, "copy_engines_then_local_decompress")):
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            eerr = None

            def fetch():
                for h in handles:                       # one pass = every allocation of the working set
                    lib.fetch_range(h, 0, n_blocks, dst.data_ptr(), False, sp, engine=engine)

            def tstep(i):
                if not active:
                    return
                if i == 0:
                    ev0.record(stream)
                fetch()
                if i == steps - 1:
                    ev1.record(stream)
            ce0 = 0
            try:
                if active:
                    fetch(); torch.cuda.synchronize()
                    ramp(fetch, torch.cuda.synchronize, min(args.ramp_ms, 30.0))
                    ce0 = lib.stats().copy_engine_bytes
            except Exception as e:
                eerr = repr(e)
            if not all_ok(eerr is None):
                info[ename] = {"skipped": eerr or "failed on another rank"}
                continue
            elapsed = run_timed(tstep, steps, 1 if active else 0, torch.cuda.synchronize, dist,
                                warm=(fetch if active else (lambda: None)), reduce_device=red_dev)
            ms = ev0.elapsed_time(ev1) / steps if active else 0.0
            ms = max_over_ranks(ms)
            rb = max_over_ranks(rec_bytes)
            gbps = rb / (ms * 1e-3) / 1e9
            e = {"inbound_GBps_per_compute_gpu": round(gbps, 1), "ms_per_pass": round(ms, 4),
                 "blocks_per_s_whole_job": round(info["compute_ranks"] * n_blocks * len(handles or [0] * n_sets) * steps / elapsed, 1),
                 "link_bytes_per_pass": int(rb)}
            e.update(rates(gbps))
            if engine == 2:
                # what the copy engines really moved (whole record slots, speckv_ext_stats.copy_engine_bytes); warm-up pass included in the count
                moved = max_over_ranks((lib.stats().copy_engine_bytes - ce0) / (steps + 1) if active else 0.0)
                e["copy_engine_link_bytes_per_pass"] = int(moved)
                e["link_GBps_actual"] = round(moved / (ms * 1e-3) / 1e9, 1)
                e["slot_overhead"] = round(moved / rb, 4) if rb else None
            info[ename] = e
        # the two fetch engines must deliver the same bytes: the last allocation of the working set through each, compared
        # bit for bit on the device
        cmp_ok, cmp_err = None, None
        try:
            if active and handles:
                h = handles[-1]
                dst.zero_(); torch.cuda.synchronize()          # (the fill runs on torch's stream, the fetch on ours)
                lib.fetch_range(h, 0, n_blocks, dst.data_ptr(), False, sp, engine=2); torch.cuda.synchronize()
                step_b = min(n_blocks, 16384)
                first = torch.empty((step_b, BLOCK_ELEMS), dtype=torch.float16, device=dst.device)
                cmp_ok = True
                for b0 in range(0, n_blocks, step_b):
                    nb = min(step_b, n_blocks - b0)
                    first.zero_(); torch.cuda.synchronize()
                    lib.fetch_range(h, b0, nb, first.data_ptr(), False, sp, engine=1); torch.cuda.synchronize()
                    cmp_ok = cmp_ok and torch.equal(first[:nb].view(torch.int16), dst[b0:b0 + nb].view(torch.int16))
                cmp_ok = bool(cmp_ok and dst.view(torch.int16).count_nonzero().item() > dst.numel() // 2)     # and it is data, not two zeroed buffers
                del first
        except Exception as e:
            cmp_err = repr(e)
        cmp_all = all_ok(cmp_err is None and cmp_ok is not False)
        info["engines_bit_identical"] = bool(cmp_all) if cmp_err is None else {"skipped": cmp_err}
        info["engines_compared"] = f"all {n_blocks} blocks of one allocation, fused peer-load kernel vs copy engines + local decompress, int16 views compared on the device"
        if rawm > 0:
            info["raw_peer_copy_GBps"] = round(rawm, 1)
            info["raw_copy_note"] = f"{links} concurrent 128 MiB device-to-device copies, one per pool GPU, into the compute GPU"
        # BASELINE configs[2] verbatim: speculative prefetch, look-ahead depth 4 per (sequence, layer), over the link.  One
        # decode step = one request per layer of every allocation of the working set; the device-side flush resolves them,
        # dedupes, assigns ring slots and fetches the pages (fused peer-load + decompress, list form) into the L2 ring.
        pf, pferr = None, None
        try:
            if active:
                L_ = args.layers
                reqs = np.repeat(np.arange(len(handles), dtype=np.uint32), L_)
                layers = np.tile(np.arange(L_, dtype=np.uint16), len(handles))
                depth = np.full(reqs.size, 4, np.uint32)
                for i, h in enumerate(handles):
                    lib.bind_request(i, h, 0)
                n_steps = 64
                stride_pos = max(8, (args.tokens - 16) // n_steps // 2 * 2)       # fresh pages every step

                def decode_step(j, count):
                    pos = np.full(reqs.size, (j * stride_pos) % (args.tokens - 8), np.uint32)
                    lib.prefetch_batch(reqs, layers, pos, depth)
                    return lib.prefetch_flush(want_count=count)
                pages0 = decode_step(0, True); lib.sync()
                # latency: submit -> every page of the step landed
                lat, pages = [], 0
                for j in range(1, 17):
                    t0 = time.perf_counter()
                    pages += decode_step(j, True)
                    lib.sync()
                    lat.append(time.perf_counter() - t0)
                # throughput: the steps submitted back to back (the queue of flushes the engine keeps in flight)
                torch.cuda.synchronize()
                st0 = lib.stats().total_prefetches
                t0 = time.perf_counter()
                for j in range(17, 17 + n_steps - 17):
                    decode_step(j, False)
                lib.sync()
                dt = time.perf_counter() - t0
                moved_pages = lib.stats().total_prefetches - st0
                page_rec = rec_bytes / max(n_blocks * len(handles), 1)
                gb = moved_pages * page_rec / dt / 1e9
                pf = {"depth_k": 4, "requests_per_step": int(reqs.size), "pages_per_step": round(pages / 16, 1), "first_step_pages": int(pages0),
                      "ms_submit_to_landed": round(float(np.median(lat)) * 1e3, 4),
                      "pipelined": {"steps": n_steps - 17, "pages": int(moved_pages), "ms_per_step": round(dt / max(n_steps - 17, 1) * 1e3, 4),
                                    "inbound_GBps_per_compute_gpu": round(gb, 2), **rates(gb)},
                      "note": "speckv_ext_prefetch_batch + device-side flush; pages decoded into the compute GPU's L2 ring"}
        except Exception as e:
            pferr = repr(e)
        all_ok(True)
        if rank == 0:
            info["speculative_prefetch_depth4"] = pf if pf is not None else {"skipped": pferr or "rank 0 idle"}
        # the uncompressed variant (fp16 pages: 4096 B per block over the link), fused kernel
        f16 = None
        ferr = None
        try:
            if active:
                lib.set_compression_scheme(0)
                h16 = lib.alloc(n_blocks * PAGE)
                lib.write(h16, 0, src.data_ptr(), src.numel() * 2, on_device=True)
                f0, f1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                lib.fetch_range(h16, 0, n_blocks, dst.data_ptr(), False, sp); torch.cuda.synchronize()
                f0.record(stream)
                for _ in range(5):
                    lib.fetch_range(h16, 0, n_blocks, dst.data_ptr(), False, sp)
                f1.record(stream); torch.cuda.synchronize()
                ms16 = f0.elapsed_time(f1) / 5
                f16 = {"inbound_GBps_per_compute_gpu": round(n_blocks * PAGE / (ms16 * 1e-3) / 1e9, 1),
                       "blocks_per_s_per_compute_gpu": round(n_blocks / (ms16 * 1e-3), 1), "engine": "auto"}
                lib.free(h16)
        except Exception as e:
            ferr = repr(e)
        all_ok(True)
        if rank == 0:
            info["fp16_pages"] = f16 if f16 is not None else {"skipped": ferr or "rank 0 idle"}
        if kv2 is not None:
            kv2.close()
        result[mode] = info
    # the collective alternative for the symmetric layout: every rank contributes a shard of compressed
    # records and RCCL all-gathers them over xGMI; the path uses it only if it beats the engines above
    if not single_gpu_test and dist.get_backend() == "nccl":
        if state is not None:
            state["phase"] = "xgmi:rccl"
        try:
            shard = torch.empty(64 << 20, dtype=torch.uint8, device=f"cuda:{local_rank}")
            gathered = torch.empty(world * shard.numel(), dtype=torch.uint8, device=f"cuda:{local_rank}")
            dist.all_gather_into_tensor(gathered, shard); torch.cuda.synchronize()
            dist.barrier()
            g0, g1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            g0.record()
            for _ in range(5):
                dist.all_gather_into_tensor(gathered, shard)
            g1.record(); torch.cuda.synchronize()
            ag_ms = g0.elapsed_time(g1) / 5
            result["rccl_allgather"] = {"shard_MiB": 64, "ms": round(ag_ms, 3),
                                        "inbound_GBps_per_gpu": round((world - 1) * shard.numel() / (ag_ms * 1e-3) / 1e9, 1),
                                        "note": "torch.distributed all_gather_into_tensor (RCCL) of one 64 MiB shard per rank"}
            del shard, gathered
        except Exception as e:
            result["rccl_allgather"] = {"skipped": repr(e)}
    return result


def roofline_xgmi_from(x, world):
    """The remote-fetch roofline of the rank-0 line: BASELINE.json's "achieved xGMI GB/s vs roofline" -- the 1 + (N-1) pool
    layout (cfg4; cfg3 at N = 2), best of the two fetch engines, with the link count and BOTH accountings of the nominal
    figure, the raw-copy ratio and the speculative-prefetch leg.  None when the phase produced nothing usable."""
    if not isinstance(x, dict):
        return None
    mode = "cfg4" if isinstance(x.get("cfg4"), dict) and "same_as" not in x["cfg4"] else "cfg3"
    m = x.get(mode)
    if not isinstance(m, dict):
        return None
    best, best_name = None, None
    for name in ("fused_peer_load_kernel", "copy_engines_then_local_decompress"):
        e = m.get(name)
        if isinstance(e, dict) and "inbound_GBps_per_compute_gpu" in e and (best is None or e["inbound_GBps_per_compute_gpu"] > best["inbound_GBps_per_compute_gpu"]):
            best, best_name = e, name
    if best is None:
        return {"bound": "xgmi", "layout": mode, "skipped": m.get("skipped") or "no engine produced a figure"}
    links = m.get("links", m.get("pool_gpus_per_compute_gpu"))
    out = {"bound": "xgmi", "layout": f"{mode}: 1 compute GPU + {links} pool GPU(s)", "engine": best_name, "links": links,
           "achieved": best["inbound_GBps_per_compute_gpu"], "unit": "GB/s", "blocks_per_s": best.get("blocks_per_s_whole_job"),
           "engines_bit_identical": m.get("engines_bit_identical"),
           "peak_nominal_per_direction": round(XGMI_LINK_GBPS * links, 1), "frac": best.get("frac_nominal_per_direction"),
           "peak_nominal_bidirectional": round(XGMI_LINK_GBPS / 2 * links, 1), "frac_bidirectional_reading": best.get("frac_nominal_bidirectional"),
           "raw_peer_copy_GBps": m.get("raw_peer_copy_GBps"), "frac_of_raw_copy": best.get("frac_of_raw_copy"),
           "link_bytes_per_pass": best.get("link_bytes_per_pass"), "copy_engine_link_bytes_per_pass": (m.get("copy_engines_then_local_decompress") or {}).get("copy_engine_link_bytes_per_pass"),
           "working_set": m.get("working_set"), "speculative_prefetch_depth4": m.get("speculative_prefetch_depth4"),
           "engines": {n: (m.get(n) or {}).get("inbound_GBps_per_compute_gpu") for n in ("fused_peer_load_kernel", "copy_engines_then_local_decompress")},
           "note": "frac = achieved / (links x 153.6 GB/s); north_star target >= 0.60 at 8 GPUs"}
    if world > 1 and os.environ.get("SPECKV_BENCH_SINGLE_GPU_TEST") == "1":
        out["note"] += "; ONE-GPU DRY RUN: every 'peer' is the same GPU, no link was crossed -- control flow only"
    return out


def fp8_scores_extra(torch, kv, T, Lyr):
    """BASELINE configs[4] (int4/fp8 path, 70B-shaped KV: 80 layers, 8 kv heads, D=128, 32k context): the fused
    dequant-matvec -- softmax(q.K^T).V of every layer of one sequence straight from FP8 records on the fp8 matrix cores,
    8 query rows per kv head (GQA).  Bytes = the K and V records read; fp16 K / V are never materialised.
    (The scores-only operator speckv_ext_qk_scores_fp8 is a diagnostic -- its fp32 score stores bound it -- and is no longer
    benched here: VERDICT r3 weak #12.)"""
    lib = kv.lib
    try:
        lib.set_compression_scheme(4)
        h = lib.alloc(T * Lyr * 8 * 128 * 2 * 2)
        lib.set_layout(h, T, Lyr, 8, 128, 2)
        n_pages = T * Lyr * 8 * 128 * 2 * 2 // PAGE
        g = torch.Generator(device="cuda"); g.manual_seed(2005)
        chunk = 65536
        for p0 in range(0, n_pages, chunk):
            x = torch.randn((min(chunk, n_pages - p0), BLOCK_ELEMS), generator=g, device="cuda", dtype=torch.float32).to(torch.float16)
            lib.write(h, p0 * PAGE, x.data_ptr(), x.numel() * 2, True)
        q = torch.randn((Lyr, 8, 8, 128), generator=g, device="cuda", dtype=torch.float32).to(torch.float16)
        s = torch.cuda.Stream()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        reps = 5
        k_bytes = Lyr * (T // 2) * 2048
        o = torch.empty((Lyr, 8, 8, 128), dtype=torch.float32, device="cuda")

        def attend():
            lib.attend_fp8(h, 0, Lyr, q.data_ptr(), 8, 0, T, 0.08838834764831845, o.data_ptr(), None, s.cuda_stream)
        attend(); torch.cuda.synchronize()
        ramp(attend, torch.cuda.synchronize, EXTRAS_RAMP_MS)
        a.record(s)
        for _ in range(reps):
            attend()
        b.record(s); torch.cuda.synchronize()
        ams = a.elapsed_time(b) / reps
        lib.free(h)
        return {"fp8_fused_attention": {"layers": Lyr, "positions": T, "query_rows_per_kv_head": 8, "pool_GiB_fp8": round(n_pages * 2048 / 2**30, 2),
                                        "ms_all_layers": round(ams, 4), "KV_record_GBps": round(2 * k_bytes / (ams * 1e-3) / 1e9, 1),
                                        "frac_hbm": round(2 * k_bytes / (ams * 1e-3) / 1e9 / HBM_PEAK_GBPS, 4),
                                        "note": "softmax(q.K^T).V of all layers: quantise + attend + combine launches; bytes = K and V records"}}
    except Exception as e:
        return {"fp8_fused_attention": {"error": repr(e)}}
    finally:
        lib.set_compression_scheme(2)


def int4_attention_extra(torch, kv, T, Lyr, scheme=3):
    """BASELINE configs[4], the 4:1 formats: the whole decode attention of every layer of one 70B-shaped
    sequence at 32k context straight from INT4_G32 records (scheme 3: 1152 B per 4 KiB page, dequantised on the vector ALUs)
    or MXFP4 records (scheme 5: 1088 B, q.K^T on the block-scaled matrix instruction)."""
    lib = kv.lib
    name = "int4_fused_attention" if scheme == 3 else "mxfp4_fused_attention"
    rec = 1152 if scheme == 3 else 1088
    try:
        lib.set_compression_scheme(scheme)
        h = lib.alloc(T * Lyr * 8 * 128 * 2 * 2)
        lib.set_layout(h, T, Lyr, 8, 128, 2)
        n_pages = T * Lyr * 8 * 128 * 2 * 2 // PAGE
        g = torch.Generator(device="cuda"); g.manual_seed(2005)
        chunk = 65536
        for p0 in range(0, n_pages, chunk):
            x = torch.randn((min(chunk, n_pages - p0), BLOCK_ELEMS), generator=g, device="cuda", dtype=torch.float32).to(torch.float16)
            lib.write(h, p0 * PAGE, x.data_ptr(), x.numel() * 2, True)
        q = torch.randn((Lyr, 8, 8, 128), generator=g, device="cuda", dtype=torch.float32).to(torch.float16)
        o = torch.empty((Lyr, 8, 8, 128), dtype=torch.float32, device="cuda")
        s = torch.cuda.Stream()
        fn = lib.attend_int4 if scheme == 3 else lib.attend_mx4
        def attend():
            fn(h, 0, Lyr, q.data_ptr(), 8, 0, T, 0.08838834764831845, o.data_ptr(), None, s.cuda_stream)
        attend(); torch.cuda.synchronize()
        ramp(attend, torch.cuda.synchronize, EXTRAS_RAMP_MS)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        reps = 5
        a.record(s)
        for _ in range(reps):
            attend()
        b.record(s); torch.cuda.synchronize()
        ms = a.elapsed_time(b) / reps
        rec_bytes = n_pages * rec
        lib.free(h)
        return {name: {"layers": Lyr, "positions": T, "query_rows_per_kv_head": 8, "record_bytes": rec, "ratio_to_fp16": round(PAGE / rec, 2),
                       "pool_GiB": round(rec_bytes / 2**30, 2), "ms_all_layers": round(ms, 4),
                       "KV_record_GBps": round(rec_bytes / (ms * 1e-3) / 1e9, 1),
                       "frac_hbm": round(rec_bytes / (ms * 1e-3) / 1e9 / HBM_PEAK_GBPS, 4),
                       "fp16_equivalent_GBps": round(n_pages * PAGE / (ms * 1e-3) / 1e9, 1),
                       "note": "softmax(q.K^T).V of all layers from " + ("INT4_G32" if scheme == 3 else "MXFP4") + " records: attend + combine launches"}}
    except Exception as e:
        return {name: {"error": repr(e)}}
    finally:
        lib.set_compression_scheme(2)


def ragged_batch_extra(torch, kv, scheme=4, n_seq=256, lo=1024, hi=16384, tail=False):
    """One decode step's attention of ONE layer for a batch whose members DIFFER in length (uniform in lo .. hi positions, seeded): what a serving
    batch looks like.  The engine dispatches such a batch by length (AttendArgs::order) and cuts members far over a CU's share into pieces
    (ring_rule.hpp ragged_tiles_per_piece); `as_given` is the same call in the caller's order, whole sequences."""
    import numpy as np
    lib = kv.lib
    name = {4: "fp8", 3: "int4_g32", 5: "mxfp4"}[scheme] + (f"_{n_seq}_sequences_one_in_16_at_{hi}_others_{lo}_to_{hi // 8}" if tail else f"_{n_seq}_sequences_{lo}_to_{hi}")
    rec = {4: 2048, 3: 1152, 5: 1088}[scheme]
    handles = []
    try:
        lib.set_compression_scheme(scheme)
        lens = [int(v) * 32 for v in np.random.default_rng(7).integers(lo // 32, hi // 32 + 1, n_seq)]
        if tail:                                                         # a heavy tail: one member in 16 at `hi`, the others uniform in lo .. hi / 8
            lens = [hi if i % 16 == 5 else int(v) * 32 for i, v in enumerate(np.random.default_rng(7).integers(lo // 32, max(lo // 32 + 1, hi // 256 + 1), n_seq))]
        g = torch.Generator(device="cuda"); g.manual_seed(2004)
        n_pages = hi * 8 * 128 * 2 * 2 // PAGE
        x = torch.randn((n_pages, BLOCK_ELEMS), generator=g, device="cuda", dtype=torch.float32).to(torch.float16)
        for _ in range(n_seq):
            h = lib.alloc(n_pages * PAGE)
            lib.set_layout(h, hi, 1, 8, 128, 2)
            lib.write(h, 0, x.data_ptr(), x.numel() * 2, True)
            handles.append(h)
        q = torch.randn((n_seq, 8, 8, 128), generator=g, device="cuda", dtype=torch.float32).to(torch.float16)
        o = torch.empty((n_seq, 8, 8, 128), dtype=torch.float32, device="cuda")
        lse = torch.empty((n_seq, 8, 8), dtype=torch.float32, device="cuda")
        s = torch.cuda.Stream()
        plan_bytes = lib.attend_plan_bytes(n_seq)
        d_plan = torch.empty(plan_bytes, dtype=torch.uint8, device="cuda")
        out = {"sequences": n_seq, "positions": f"{lo}..{hi} (mean {sum(lens) // n_seq})"}
        plans = []
        for key, given in (("planned", 0), ("planned_as_given", 1)):
            set_tuning("attend_order_as_given", given)
            d_plan = torch.empty(plan_bytes, dtype=torch.uint8, device="cuda"); plans.append(d_plan)      # (a buffer each: a plan's first batch fixes its launch geometry)
            lib.attend_batch_plan(handles, lens, hi, d_plan.data_ptr(), plan_bytes, s.cuda_stream)
            def step():
                lib.attend_planned(scheme, d_plan.data_ptr(), n_seq, 0, q.data_ptr(), 8, hi, 0.08838834764831845, o.data_ptr(), lse.data_ptr(), s.cuda_stream)
            step(); torch.cuda.synchronize()
            ramp(step, torch.cuda.synchronize, EXTRAS_RAMP_MS)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(s)
            for _ in range(10):
                step()
            b.record(s); torch.cuda.synchronize()
            ms = a.elapsed_time(b) / 10
            out[key + "_ms_per_layer"] = round(ms, 4)
            out[key + "_frac_hbm"] = round(sum(lens) * rec / (ms * 1e-3) / 1e9 / HBM_PEAK_GBPS, 4)
        return {name: out}
    except Exception as e:                                               # noqa: BLE001
        return {name: {"error": repr(e)}}
    finally:
        try: set_tuning("attend_order_as_given", 0)
        except Exception: pass                                           # noqa: BLE001
        for h in handles:
            try: lib.free(h)
            except Exception: pass                                       # noqa: BLE001


def batch_attention_extra(torch, kv, n_seq=256, T=8192, scheme=4):
    """BASELINE configs[3] shape on one GPU: one decode step's attention of ONE layer for a batch of 256 sequences at
    8k context (8 kv heads x 128, 8 query rows per kv head), FP8 (scheme 4) or INT4 (3) records, one launch pair for the
    whole batch."""
    lib = kv.lib
    handles = []
    name = {4: "fp8_attention_batch_decode_step", 3: "int4_attention_batch_decode_step", 5: "mxfp4_attention_batch_decode_step"}[scheme]
    if (n_seq, T) != (256, 8192):
        name += f"_{n_seq}x{T}"
    rec = {4: 2048, 3: 1152, 5: 1088}[scheme]
    try:
        lib.set_compression_scheme(scheme)
        g = torch.Generator(device="cuda"); g.manual_seed(2004)
        n_pages = T * 8 * 128 * 2 * 2 // PAGE
        x = torch.randn((n_pages, BLOCK_ELEMS), generator=g, device="cuda", dtype=torch.float32).to(torch.float16)
        for _ in range(n_seq):
            h = lib.alloc(n_pages * PAGE)
            lib.set_layout(h, T, 1, 8, 128, 2)
            lib.write(h, 0, x.data_ptr(), x.numel() * 2, True)       # same synthetic KV in every sequence: bytes are what count
            handles.append(h)
        q = torch.randn((n_seq, 8, 8, 128), generator=g, device="cuda", dtype=torch.float32).to(torch.float16)
        o = torch.empty((n_seq, 8, 8, 128), dtype=torch.float32, device="cuda")
        s = torch.cuda.Stream()
        lens = [T] * n_seq
        fn = {4: lib.attend_fp8_batch, 3: lib.attend_int4_batch, 5: lib.attend_mx4_batch}[scheme]
        def step():
            fn(handles, 0, q.data_ptr(), 8, lens, 0.08838834764831845, o.data_ptr(), None, s.cuda_stream)
        step(); torch.cuda.synchronize()
        ramp(step, torch.cuda.synchronize, EXTRAS_RAMP_MS)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        reps = 10
        a.record(s)
        for _ in range(reps):
            step()
        b.record(s); torch.cuda.synchronize()
        ms = a.elapsed_time(b) / reps
        rec_bytes = n_seq * n_pages * rec
        # the same launches in the PLANNED form (what the connector's decode loop and a HIP graph use: descriptors planned once per
        # step, the per-layer call is kernel launches only -- no handle look-ups, no descriptor staging on the way)
        plan_bytes = lib.attend_plan_bytes(n_seq)
        d_plan = torch.empty(plan_bytes, dtype=torch.uint8, device="cuda")
        lse = torch.empty((n_seq, 8, 8), dtype=torch.float32, device="cuda")
        lib.attend_batch_plan(handles, lens, T, d_plan.data_ptr(), plan_bytes, s.cuda_stream)
        def pstep():
            lib.attend_planned(scheme, d_plan.data_ptr(), n_seq, 0, q.data_ptr(), 8, T, 0.08838834764831845, o.data_ptr(), lse.data_ptr(), s.cuda_stream)
        pstep(); torch.cuda.synchronize()
        ramp(pstep, torch.cuda.synchronize, EXTRAS_RAMP_MS)
        a.record(s)
        for _ in range(reps):
            pstep()
        b.record(s); torch.cuda.synchronize()
        pms = a.elapsed_time(b) / reps
        return {name: {"sequences": n_seq, "context": T, "layers_per_call": 1,
                       "ms_per_layer": round(ms, 4), "KV_record_GBps": round(rec_bytes / (ms * 1e-3) / 1e9, 1),
                       "frac_hbm": round(rec_bytes / (ms * 1e-3) / 1e9 / HBM_PEAK_GBPS, 4),
                       "planned_ms_per_layer": round(pms, 4), "planned_frac_hbm": round(rec_bytes / (pms * 1e-3) / 1e9 / HBM_PEAK_GBPS, 4),
                       "note": f"speckv_ext_attend_{ {4: 'fp8', 3: 'int4', 5: 'mx4'}[scheme] }_batch: {n_seq} sequences x {T} context, one layer, one launch pair; "
                               "planned_*: the same launches through speckv_ext_attend_batch_plan + _planned (kernel launches only per call)"}}
    except Exception as e:
        return {name: {"error": repr(e)}}
    finally:
        for h in handles:
            try: lib.free(h)
            except Exception: pass
        lib.set_compression_scheme(2)


def connector_append_extra(torch, kv, n_seq=256, Lyr=80, T=64):
    """SURVEY 8f row N2 at the BASELINE configs[3] batch: one decode step's append for 256 sequences x 80 layers through
    the vLLM-shaped connector.  Every other step completes a position pair per sequence: 160 pages per sequence, ONE
    compress launch for the batch (speckv_ext_write_strided_batch); the other steps only park the rows in the tail."""
    from cxl_speckv_amd.kv_connector import SpeckvKVConnector
    conn = None
    try:
        conn = SpeckvKVConnector(kv.lib, num_layers=Lyr, max_tokens=T, scheme="fp8")
        ids = list(range(n_seq))
        for r in ids:
            conn.add_request(r)
        g = torch.Generator(device="cuda"); g.manual_seed(2005)
        k = torch.randn((n_seq, Lyr, 8, 128), generator=g, device="cuda", dtype=torch.float32).to(torch.float16)
        v = torch.randn((n_seq, Lyr, 8, 128), generator=g, device="cuda", dtype=torch.float32).to(torch.float16)
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            t_pair, t_tail, dev_pair = [], [], []
            for step in range(12):
                torch.cuda.synchronize()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0 = time.perf_counter()
                a.record(s)
                keep = conn.append(ids, k, v, stream=s)
                b.record(s)
                host = (time.perf_counter() - t0) * 1e3
                torch.cuda.synchronize()
                if step >= 2:
                    (t_pair if step % 2 else t_tail).append(host)
                    if step % 2: dev_pair.append(a.elapsed_time(b))
                del keep
        pages = n_seq * 2 * Lyr
        return {"connector_append_step": {"sequences": n_seq, "layers": Lyr, "pages_per_pair_step": pages,
                                          "host_ms_pair_step": round(min(t_pair), 3), "host_ms_tail_step": round(min(t_tail), 3),
                                          "device_ms_pair_step": round(min(dev_pair), 3),
                                          "note": "append of one decode step for the whole batch: gather + one speckv_ext_write_strided_batch launch "
                                                  "(fp8 pool); device time includes the torch gathers that build the page images"}}
    except Exception as e:
        return {"connector_append_step": {"error": repr(e)}}
    finally:
        if conn is not None:
            for r in list(conn.requests):
                try: conn.free_request(r)
                except Exception: pass
        kv.lib.set_compression_scheme(2)


def connector_decode_extra(torch, kv, n_seq=256, Lyr=8, ctx=2048, T=4096, scheme="fp8", tail=False):
    """SURVEY 8f row N2 end to end: decode steps of a 256-sequence batch through the vLLM-shaped connector -- per step
    one look-ahead flush (begin_step), one fused attention call per layer for the whole batch, one batched append.  Only the
    KV side of a decode step (no model): what the drop-in costs per generated token at this batch and context."""
    from cxl_speckv_amd.kv_connector import SpeckvKVConnector
    conn = None
    try:
        conn = SpeckvKVConnector(kv.lib, num_layers=Lyr, max_tokens=T, scheme=scheme)
        name = ("connector_decode_step" if scheme == "fp8" else f"connector_decode_step_{scheme}") + ("_heavy_tail" if tail else "")
        rec_per_pos = {"fp8": 1024, "int4": 576, "mxfp4": 544}[scheme]
        ids = list(range(n_seq))
        g = torch.Generator(device="cuda"); g.manual_seed(2006)
        kp = torch.randn((Lyr, ctx, 8, 128), generator=g, device="cuda", dtype=torch.float32).to(torch.float16)
        vp = torch.randn((Lyr, ctx, 8, 128), generator=g, device="cuda", dtype=torch.float32).to(torch.float16)
        # tail: the prompts differ in length -- one request in 16 has ctx positions, the others ctx / 32 .. ctx / 8 (seeded): what a serving batch looks like
        import numpy as np
        lens = [ctx] * n_seq if not tail else [ctx if i % 16 == 5 else int(v) * 32 for i, v in enumerate(np.random.default_rng(11).integers(ctx // 1024, ctx // 256 + 1, n_seq))]
        held = []
        for r in ids:
            conn.add_request(r)
            held.append(conn.write_prefill(r, kp[:, :lens[r]], vp[:, :lens[r]]))      # the same synthetic prompt KV (a prefix of it) in every sequence
        torch.cuda.synchronize()                               # (the launches read the tensors they were given: held until they have run)
        del kp, vp, held
        q = torch.randn((n_seq, 8, 8, 128), generator=g, device="cuda", dtype=torch.float32).to(torch.float16)
        k = torch.randn((n_seq, Lyr, 8, 128), generator=g, device="cuda", dtype=torch.float32).to(torch.float16)
        v = torch.randn((n_seq, Lyr, 8, 128), generator=g, device="cuda", dtype=torch.float32).to(torch.float16)
        s = torch.cuda.Stream()
        times, times_all = [], []
        qall = q[None].expand(Lyr, -1, -1, -1, -1).contiguous()
        with torch.cuda.stream(s):
            for step in range(16):
                all_layers = step >= 8                              # steps 8..15: the layers' attention as ONE library call (attend_layers)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                conn.begin_step(ids, depth_k=0)
                if all_layers:
                    out = conn.attend_layers(0, Lyr, ids, qall, 0.08838834764831845, stream=s)
                else:
                    for layer in range(Lyr):
                        out = conn.attend(layer, ids, q, 0.08838834764831845, stream=s)
                keep = conn.append(ids, k, v, stream=s)
                torch.cuda.synchronize()
                (times_all if all_layers else times).append((time.perf_counter() - t0) * 1e3)
                del keep, out
        # the median of the steps (even and odd steps alternate -- tail fold / pair append -- so of six steps the mean of the middle two): one stalled step of
        # 11 ms (seen once, in both FP8 loops of one process, never again) no longer doubles the figure; fastest and slowest stand beside it
        def med(v):
            v = sorted(v); n = len(v)
            return v[n // 2] if n % 2 else 0.5 * (v[n // 2 - 1] + v[n // 2])
        ms_all = med(times_all[2:])
        ms = med(times[2:])
        rec_bytes = Lyr * 2 * sum(lens) * rec_per_pos            # record bytes read per step (K and V; FP8 1 KiB per position and kind, MXFP4 544 B)
        return {name: {"sequences": n_seq, "layers": Lyr, "context": ctx if not tail else f"one in 16 at {ctx}, the others {ctx // 32}..{ctx // 8} (mean {sum(lens) // n_seq})", "ms_per_step": round(ms, 3),
                                          "ms_fastest_step": round(min(times[2:]), 3), "ms_slowest_step": round(max(times[2:]), 3),
                                          "ms_per_step_layers_in_one_call": round(ms_all, 3), "frac_hbm_layers_in_one_call": round(rec_bytes / (ms_all * 1e-3) / 1e9 / HBM_PEAK_GBPS, 4),
                                          "tokens_per_s_kv_side": round(n_seq / (ms * 1e-3), 1),
                                          "KV_record_GBps": round(rec_bytes / (ms * 1e-3) / 1e9, 1),
                                          "frac_hbm": round(rec_bytes / (ms * 1e-3) / 1e9 / HBM_PEAK_GBPS, 4),
                                          "note": "begin_step (a no-op for fused pools since round 6) + one batch attention call per layer (the tail position goes along in the call) + batched "
                                                  "append (which plans the next step), wall time per step incl. the torch glue (median of the steps); ms_per_step_layers_in_one_call: the same step with the "
                                                  "layers' attention as ONE call (SpeckvKVConnector.attend_layers: for callers that have several layers' query rows at once; over an "
                                                  "MXFP4 pool one launch); " + scheme + " pool"}}
    except Exception as e:
        return {("connector_decode_step" if scheme == "fp8" else f"connector_decode_step_{scheme}") + ("_heavy_tail" if tail else ""): {"error": repr(e)}}
    finally:
        if conn is not None:
            for r in list(conn.requests):
                try: conn.free_request(r)
                except Exception: pass
        kv.lib.set_compression_scheme(2)


def kv_accuracy_extra(torch, kv):
    """What the pool formats cost in attention accuracy on KV-like data (outlier channels, RoPE pairs, heavy-tailed V; peaky / decode-like /
    flat softmax) against float64 attention over the original fp16 K / V with the unquantised query: cxl-speckv_amd/kv_accuracy.py."""
    try:
        from cxl_speckv_amd.kv_accuracy import kv_format_accuracy
        acc = kv_format_accuracy(kv)
        acc["note"] = ("relative L2 error / cosine of the fused attention's output rows, top-1 agreement of the attention weights; format_rel_l2 = the "
                       "format alone (float64 over the dequantised K / V, exact query), kernel_rel_l2 = what the kernel adds (query quantisation, f16 weights); "
                       "'+kscale' = per-channel power-of-two pre-scale of K folded into the query (SpeckvKVConnector.set_k_channel_scale)")
        return {"kv_format_accuracy": acc}
    except Exception as e:                                               # noqa: BLE001
        return {"kv_format_accuracy": {"error": repr(e)}}


def footprint_extra(torch, kv, T, Lyr, seed, seconds=0.4):
    """The hot path at another footprint: one sequence of T positions x Lyr layers (8 kv heads x 128), INT8_DELTA_RLE,
    reference quantiser, one launch per pass, timed over >= `seconds` of back-to-back passes after a clock ramp."""
    lib = kv.lib
    lib.set_compression_scheme(2)
    n_pages = T * Lyr * 8 * 128 * 2 * 2 // PAGE
    h = lib.alloc(n_pages * PAGE)
    try:
        g = torch.Generator(device="cuda"); g.manual_seed(seed)
        chunk = 65536
        for p0 in range(0, n_pages, chunk):
            x = torch.randn((min(chunk, n_pages - p0), BLOCK_ELEMS), generator=g, device="cuda", dtype=torch.float32).to(torch.float16)
            lib.write(h, p0 * PAGE, x.data_ptr(), x.numel() * 2, True)
        del x
        dst = torch.empty((n_pages, BLOCK_ELEMS), dtype=torch.float16, device="cuda")
        s = torch.cuda.Stream()
        def step():
            lib.fetch_range(h, 0, n_pages, dst.data_ptr(), False, s.cuda_stream)
        step(); torch.cuda.synchronize()
        ramp(step, torch.cuda.synchronize, EXTRAS_RAMP_MS)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(s); step(); b.record(s); torch.cuda.synchronize()
        reps = max(5, int(seconds / max(a.elapsed_time(b) * 1e-3, 1e-6)))
        a.record(s)
        for _ in range(reps):
            step()
        b.record(s); torch.cuda.synchronize()
        ms = a.elapsed_time(b) / reps
        info = lib.translate(h, 0)
        alg = n_pages * (4080 + 4 + PAGE)            # N(0,1) blocks: 4080 record bytes on average (measured on the main workload)
        del dst
        return {"blocks": n_pages, "pool_plus_destination_GiB": round(n_pages * (4096 + PAGE) / 2**30, 2), "ms": round(ms, 4), "passes": reps,
                "blocks_per_s": round(n_pages / (ms * 1e-3), 1),
                "frac_hbm": round(alg / (ms * 1e-3) / 1e9 / HBM_PEAK_GBPS, 4),
                "note": "T=%d x %d layers, one launch per pass; first record %d B" % (T, Lyr, info.rec_bytes)}
    finally:
        lib.free(h)


def seq70b_extra(torch, kv):
    """SURVEY 8(d) footprints beside the main workload (cfg1, 1.0 GiB of pool + destination): 4 x cfg1 and one
    Llama-3-70B-shaped sequence at 8k context (BASELINE configs[3] shape per sequence, 655 360 blocks)."""
    out = {}
    for key, T, Lyr, seed in (("fetch_decompress_4x_cfg1_footprint", 16384, 32, 2003),
                              ("fetch_decompress_70b_shaped_sequence", 8192, 80, 2004)):
        try:
            out[key] = footprint_extra(torch, kv, T, Lyr, seed)
        except Exception as e:
            out[key] = {"error": repr(e)}
    return out


def flush_cfg4_extra(torch, pkg, n_seq=256, Lyr=80, T=128):
    """BASELINE configs[3] call count: one decode step of 256 sequences x 80 layers = 20 480 look-ahead requests, one
    allocation per sequence (request ids bound to handles), drained by ONE device-side flush.  Sequences are kept short
    (T positions) so 256 of them fit beside the other extras; the records are never written (they decode to zeros), the
    work per request is the same."""
    os.environ["SPECKV_L2_MB"] = "2048"
    try:
        kv = pkg.CxlSpeckvKVAllocator(pkg.library_path(), f"hip:{torch.cuda.current_device()}")
    finally:
        del os.environ["SPECKV_L2_MB"]
    try:
        lib = kv.lib
        lib.set_compression_scheme(2)
        hs = []
        for s_ in range(n_seq):
            h = lib.alloc(2 * T * Lyr * 8 * 128 * 2)
            lib.set_layout(h, T, Lyr, 8, 128, 2)
            lib.bind_request(s_, h, 0)
            hs.append(h)
        rng = np.random.default_rng(11)
        n_req = n_seq * Lyr
        reqs = np.repeat(np.arange(n_seq, dtype=np.uint32), Lyr)
        layers = np.tile(np.arange(Lyr, dtype=np.uint16), n_seq)
        depth = np.full(n_req, 4, np.uint32)
        ms, sub, enq, pipe, pages = [], [], [], [], []
        for rep in range(6):
            pos = np.full(n_req, 8 * rep, np.uint32)
            before = int(lib.stats().total_prefetches)
            t0 = time.perf_counter()
            lib.prefetch_batch(reqs, layers, pos, depth)
            enq.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            if rep % 2:
                lib.prefetch_flush(want_count=False)            # submit only
                t1 = time.perf_counter()
                sub.append((t1 - t0) * 1e3)
            else:
                lib.prefetch_flush(want_count=True)             # waits for the lookup / dedupe / slot kernels, not for the data
                pipe.append((time.perf_counter() - t0) * 1e3)
            lib.sync()
            ms.append((time.perf_counter() - t0) * 1e3)
            pages.append(int(lib.stats().total_prefetches) - before)
        return {"prefetch_flush_cfg4_step": {"requests": n_req, "sequences": n_seq, "layers": Lyr, "pages_issued": pages[-1],
                                             "ms": round(min(ms[1:]), 3), "submit_ms": round(min(sub), 3), "first_call_ms": round(ms[0], 3),
                                             "enqueue_ms": round(min(enq[1:]), 3), "until_slots_assigned_ms": round(min(pipe[1:]), 3),
                                             "dropped": int(lib.stats().prefetch_dropped),
                                             "note": "one flush for the whole batch's decode step: 256 allocations, request ids bound to handles"}}
    except Exception as e:
        return {"prefetch_flush_cfg4_step": {"error": repr(e)}}
    finally:
        kv.close()


def predictor_extra(torch, lib):
    """Token predictor (reference LSTMPredictor::predict_top_k: 13.5 ms per call on one CPU
    core; paper claim < 10 us on the FPGA): latency of one top-4 prediction
    and of a 256-request batch, random weights of the reference's shape (32000 x 64 / x 128)."""
    try:
        g = torch.Generator(device="cuda"); g.manual_seed(9)
        emb = (torch.rand((32000, 64), generator=g, device="cuda") - 0.5) * 0.1
        wout = (torch.rand((32000, 128), generator=g, device="cuda") - 0.5) * 0.1
        lib.predictor_load(emb.data_ptr(), wout.data_ptr(), 32000, True)
        out = {}
        s = torch.cuda.Stream()
        for n in (1, 256):
            hist = torch.randint(0, 32000, (n, 16), generator=g, device="cuda", dtype=torch.int32)
            tok = torch.empty((n, 4), dtype=torch.int32, device="cuda"); conf = torch.empty((n, 4), dtype=torch.float32, device="cuda")
            lib.predict_batch(n, hist.data_ptr(), 4, tok.data_ptr(), conf.data_ptr(), s.cuda_stream); torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            reps = 20
            a.record(s)
            for _ in range(reps):
                lib.predict_batch(n, hist.data_ptr(), 4, tok.data_ptr(), conf.data_ptr(), s.cuda_stream)
            b.record(s); torch.cuda.synchronize()
            out[f"batch_{n}_us"] = round(a.elapsed_time(b) / reps * 1e3, 2)
        out["reference_cpu_ms_per_call"] = 13.5
        return {"token_predictor_top4": out}
    except Exception as e:
        return {"token_predictor_top4": {"error": repr(e)}}


def tensor_codec_extra(torch, lib, n=131072 * 256):
    """FPGACacheEngine::compress / ::decompress with the reference's own call shape (cache_engine.cpp:40-116): ONE tensor of n
    elements, one scale, one delta chain, one run-length stream (speckv_ext_codec_compress_tensor / _decompress_tensor).
    n = 32 Mi fp16 elements (256 RTL tiles of 1024 x 128), N(0,1)."""
    raw = lib.lib
    try:
        g = torch.Generator(device="cuda"); g.manual_seed(2001)
        x = torch.randn(n, generator=g, device="cuda", dtype=torch.float32).to(torch.float16)
        ws_bytes = int(raw.speckv_ext_codec_tensor_workspace_bytes(n))
        ws = torch.empty(ws_bytes + 256, dtype=torch.uint8, device="cuda")
        wsp = (ws.data_ptr() + 255) & ~255
        rle = torch.empty(2 * n + 32, dtype=torch.uint8, device="cuda")
        meta = torch.zeros(4, dtype=torch.int64, device="cuda")
        y = torch.empty(n, dtype=torch.float16, device="cuda")
        s = torch.cuda.Stream()

        def enc():
            assert raw.speckv_ext_codec_compress_tensor(x.data_ptr(), n, 0, rle.data_ptr(), meta.data_ptr(), meta.data_ptr() + 8, wsp, ws_bytes, 0, s.cuda_stream) == 0
        enc(); torch.cuda.synchronize()
        size = int(meta[0].item())
        scale = float(meta[1:2].view(torch.float32)[0].item())
        dws_bytes = int(raw.speckv_ext_codec_tensor_decode_workspace_bytes(size))
        dws = torch.empty(dws_bytes + 256, dtype=torch.uint8, device="cuda")
        dwsp = (dws.data_ptr() + 255) & ~255

        def dec():
            assert raw.speckv_ext_codec_decompress_tensor(rle.data_ptr(), size, scale, y.data_ptr(), n, 0, meta.data_ptr() + 16, dwsp, dws_bytes, 0, s.cuda_stream) == 0
        out = {"elements": n, "compressed_bytes": size}
        for name, fn, byt in (("compress", enc, 2 * n + size), ("decompress", dec, size + 2 * n)):
            fn(); torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(s)
            for _ in range(5):
                fn()
            b.record(s); torch.cuda.synchronize()
            ms = a.elapsed_time(b) / 5
            out[name] = {"ms": round(ms, 4), "algorithmic_GBps": round(byt / (ms * 1e-3) / 1e9, 1), "frac_hbm": round(byt / (ms * 1e-3) / 1e9 / HBM_PEAK_GBPS, 4)}
        if n <= 64 * 2**20:                                              # the reference's own types at the boundary: float in, float out
            x32 = x.to(torch.float32); y32 = torch.empty(n, dtype=torch.float32, device="cuda")

            def enc32():
                assert raw.speckv_ext_codec_compress_tensor(x32.data_ptr(), n, 1, rle.data_ptr(), meta.data_ptr(), meta.data_ptr() + 8, wsp, ws_bytes, 0, s.cuda_stream) == 0

            def dec32():
                assert raw.speckv_ext_codec_decompress_tensor(rle.data_ptr(), size, scale, y32.data_ptr(), n, 1, meta.data_ptr() + 16, dwsp, dws_bytes, 0, s.cuda_stream) == 0
            for name, fn, byt in (("compress_fp32_source", enc32, 4 * n + size), ("decompress_fp32_output", dec32, size + 4 * n)):
                fn(); torch.cuda.synchronize()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(s)
                for _ in range(5):
                    fn()
                b.record(s); torch.cuda.synchronize()
                ms = a.elapsed_time(b) / 5
                out[name] = {"ms": round(ms, 4), "frac_hbm": round(byt / (ms * 1e-3) / 1e9 / HBM_PEAK_GBPS, 4)}
            del x32, y32
        out["note"] = ("any n, exact.  Compress: an abs-max pass, then ONE pass that encodes whole fp16 tiles by the block encoder's "
                       "8-elements-per-lane path and places them in the stream by look-back across workgroups (two reads of the source, one "
                       "write of the stream); decompress: ONE pass (a chunk of 2048 pairs per wave, one byte scattered per run, look-back across "
                       "workgroups hidden behind the values).  The pool itself stores KV per 4 KiB block (the headline path)")
        return {"tensor_codec_whole_tensor" if n == 131072 * 256 else f"tensor_codec_whole_tensor_{n * 2 // 2**20}MiB": out}
    except Exception as e:
        return {"tensor_codec_whole_tensor": {"error": repr(e)}}


def tensor_codec_batch_extra(torch, lib, n_tensors=4096, n=131072):
    """The reference's codec at the reference's own call size (VERDICT r5 missing #4): FPGACacheEngine::compress(data, n) is called per KV
    tile -- 1024 x 128 = 131 072 elements, hardware/rtl/kv_compress.v:5-11 -- so the shape is MANY tensors of that size, not one giant
    one.  speckv_ext_codec_compress_tensors / _decompress_tensors: one workgroup per tensor, one launch each way; fp32 in and out as
    the reference takes and returns them, and the fp16 forms beside."""
    import ctypes as C
    try:
        raw = lib.lib
        raw.speckv_ext_codec_tensors_workspace_bytes.argtypes = [C.c_uint32, C.c_uint64]; raw.speckv_ext_codec_tensors_workspace_bytes.restype = C.c_size_t
        raw.speckv_ext_codec_compress_tensors.argtypes = [C.c_uint32, C.c_void_p, C.c_uint64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
        raw.speckv_ext_codec_decompress_tensors.argtypes = [C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
        ws_bytes = int(raw.speckv_ext_codec_tensors_workspace_bytes(n_tensors, n))
        ws = torch.empty(ws_bytes + 256, dtype=torch.uint8, device="cuda")
        wsp = (ws.data_ptr() + 255) & ~255
        g = torch.Generator(device="cuda"); g.manual_seed(2007)
        x32 = torch.randn((n_tensors, n), generator=g, device="cuda", dtype=torch.float32)
        x32 *= torch.rand((n_tensors, 1), generator=g, device="cuda") * 4 + 0.25          # every tensor its own scale
        x16 = x32.to(torch.float16)
        cap = 2 * n + 16
        rle = torch.empty((n_tensors, cap), dtype=torch.uint8, device="cuda")
        y32 = torch.empty((n_tensors, n), dtype=torch.float32, device="cuda")
        sizes = torch.zeros(n_tensors, dtype=torch.int64, device="cuda")
        scales = torch.zeros(n_tensors, dtype=torch.float32, device="cuda")
        nout = torch.zeros(n_tensors, dtype=torch.int64, device="cuda")
        s = torch.cuda.Stream()

        def descs(data, esz):
            d = np.zeros((n_tensors, 4), np.uint64)
            d[:, 0] = data.data_ptr() + np.arange(n_tensors, dtype=np.uint64) * np.uint64(n * esz)
            d[:, 1] = n
            d[:, 2] = rle.data_ptr() + np.arange(n_tensors, dtype=np.uint64) * np.uint64(cap)
            d[:, 3] = cap
            return torch.from_numpy(d.view(np.int64)).cuda()
        out = {"tensors": n_tensors, "elements_each": n}
        for tag, src, esz, f32 in (("fp32", x32, 4, 1), ("fp16", x16, 2, 0)):
            dst = y32 if f32 else y32.view(torch.float16)[:, :n]
            if not f32:
                dst = torch.empty((n_tensors, n), dtype=torch.float16, device="cuda")
            dc, dd = descs(src, esz), descs(dst, esz)
            enc = lambda: raw.speckv_ext_codec_compress_tensors(n_tensors, dc.data_ptr(), n, f32, sizes.data_ptr(), scales.data_ptr(), wsp, ws_bytes, 0, s.cuda_stream)
            dec = lambda: raw.speckv_ext_codec_decompress_tensors(n_tensors, dd.data_ptr(), n, sizes.data_ptr(), scales.data_ptr(), f32, nout.data_ptr(), wsp, ws_bytes, 0, s.cuda_stream)
            assert enc() == 0 and dec() == 0
            torch.cuda.synchronize()
            comp = int(sizes.sum().item())
            assert int(nout.min().item()) == n and int(nout.max().item()) == n
            # (REF_EXACT reproduces the reference's double scaling and int8 wrap, cache_engine.cpp:190-192: its round trip is not close
            #  to the input by design; what the streams must be is pinned per tensor in tests/test_gpu_codec.py)
            for name, fn, byt in (("compress", enc, esz * n * n_tensors + comp), ("decompress", dec, comp + esz * n * n_tensors)):
                ramp(lambda: fn(), torch.cuda.synchronize, EXTRAS_RAMP_MS)
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(s)
                for _ in range(5):
                    fn()
                b.record(s); torch.cuda.synchronize()
                ms = a.elapsed_time(b) / 5
                out[f"{name}_{tag}"] = {"ms": round(ms, 4), "tensors_per_s": round(n_tensors / (ms * 1e-3), 1), "algorithmic_GBps": round(byt / (ms * 1e-3) / 1e9, 1),
                                        "frac_hbm": round(byt / (ms * 1e-3) / 1e9 / HBM_PEAK_GBPS, 4)}
            out[f"compressed_bytes_{tag}"] = comp
            del dc, dd
        out["note"] = ("four workgroups per tensor (16 tiles each): max|x| by a rendezvous of the tensor's workgroups, the chains by look-back over the tensor's own "
                       "status words, the second read of the source out of the L2 / Infinity Cache; algorithmic bytes = source once + stream (compress), stream + output (decompress)")
        return {"tensor_codec_batched_131072": out}
    except Exception as e:                                               # noqa: BLE001
        return {"tensor_codec_batched_131072": {"error": repr(e)}}


def compaction_extra(torch, kv, n_pages=131072):
    """speckv_ext_compact on the structured data SURVEY 8(d) names (a third runs of 32, a third zeros, a third N(0,1)):
    pool bytes before / after, i.e. the capacity the reference's scheme really buys once records are packed."""
    lib = kv.lib
    try:
        lib.set_compression_scheme(2)
        g = torch.Generator(device="cuda"); g.manual_seed(2006)
        x = torch.randn((n_pages, BLOCK_ELEMS), generator=g, device="cuda", dtype=torch.float32).to(torch.float16)
        x[0::3] = x[0::3, :64].repeat_interleave(32, dim=1)
        x[1::3] = 0
        h = lib.alloc(n_pages * PAGE)
        lib.write(h, 0, x.data_ptr(), x.numel() * 2, True)
        t0 = time.perf_counter()
        before, after = lib.compact(h)
        ms = (time.perf_counter() - t0) * 1e3
        lib.free(h)
        return {"compaction_structured_third_each": {"pages": n_pages, "pool_bytes_before": before, "pool_bytes_after": after,
                                                     "capacity_ratio_vs_slots": round(before / max(after, 1), 3),
                                                     "capacity_ratio_vs_fp16": round(n_pages * PAGE / max(after, 1), 3), "ms": round(ms, 2),
                                                     "note": "records packed back to back (128-byte aligned), slots returned to the pool"}}
    except Exception as e:
        return {"compaction_structured_third_each": {"error": repr(e)}}
    finally:
        lib.set_compression_scheme(2)


def lstm_cell_extra(torch, lib):
    """The real LSTM cell of the predictor (speckv_ext_predictor_load_lstm, 2 layers, 64 -> 128, vocab 32000)."""
    try:
        g = torch.Generator(device="cuda"); g.manual_seed(10)
        rnd = lambda *s_: (torch.rand(s_, generator=g, device="cuda") - 0.5) * 0.2
        emb, wout, bout = rnd(32000, 64), rnd(32000, 128), rnd(32000)
        w_ih, w_hh, b_ih, b_hh = [rnd(512, 64), rnd(512, 128)], [rnd(512, 128), rnd(512, 128)], [rnd(512), rnd(512)], [rnd(512), rnd(512)]
        lib.predictor_load_lstm(emb.data_ptr(), 32000, [t.data_ptr() for t in w_ih], [t.data_ptr() for t in w_hh],
                                [t.data_ptr() for t in b_ih], [t.data_ptr() for t in b_hh], wout.data_ptr(), bout.data_ptr(), True)
        out = {}
        s = torch.cuda.Stream()
        for n in (1, 256):
            hist = torch.randint(0, 32000, (n, 16), generator=g, device="cuda", dtype=torch.int32)
            tok = torch.empty((n, 4), dtype=torch.int32, device="cuda"); conf = torch.empty((n, 4), dtype=torch.float32, device="cuda")
            lib.predict_batch(n, hist.data_ptr(), 4, tok.data_ptr(), conf.data_ptr(), s.cuda_stream); torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(s)
            for _ in range(20):
                lib.predict_batch(n, hist.data_ptr(), 4, tok.data_ptr(), conf.data_ptr(), s.cuda_stream)
            b.record(s); torch.cuda.synchronize()
            out[f"batch_{n}_us"] = round(a.elapsed_time(b) / 20 * 1e3, 2)
        return {"token_predictor_real_lstm_top4": out}
    except Exception as e:
        return {"token_predictor_real_lstm_top4": {"error": repr(e)}}


def striped_attention_extra(torch, pkg, T=32768, Lyr=80):
    """The fused attention over a pool striped across 7 pools (the 1 + 7 layout of BASELINE configs[3], here 7 same-GPU
    pools): the striped form computes its record addresses; the table form (what an allocation with migrated pages, or a
    range whose last tile would leave its region, takes; SPECKV_ATTEND_GENERAL forces it) reads them from the page table one
    tile ahead.  (The per-wave page-table kernels of rounds 1-3 are retired: INT4 has none left, FP8 keeps one for layouts
    without a scale table.)"""
    out = {}
    mx4 = lambda torch_, kv_, T_, L_: int4_attention_extra(torch_, kv_, T_, L_, scheme=5)
    for scheme, name, fn in ((3, "int4", int4_attention_extra), (4, "fp8", fp8_scores_extra), (5, "mxfp4", mx4)):
        for label, general in (("computed_addresses", 0), ("table_form", 1)):
            os.environ["SPECKV_POOL_DEVICES"] = "0,0,0,0,0,0,0"
            if general:
                set_tuning("attend_general", str(general))
            try:
                kv = pkg.CxlSpeckvKVAllocator(pkg.library_path(), f"hip:{torch.cuda.current_device()}")
                try:
                    r = fn(torch, kv, T, Lyr)
                    r = r.get("int4_fused_attention") or r.get("fp8_fused_attention") or r.get("mxfp4_fused_attention") or r
                    out[f"{name}_{label}"] = {k: r.get(k) for k in ("ms_all_layers", "frac_hbm", "error") if k in r}
                finally:
                    kv.close()
            except Exception as e:
                out[f"{name}_{label}"] = {"error": repr(e)}
            finally:
                os.environ.pop("SPECKV_POOL_DEVICES", None)
                set_tuning("attend_general", 0)
    # ... and BASELINE configs[3]'s decode step itself over that layout: 256 sequences x 8k, every sequence striped over the 7 pools
    for scheme, name in ((4, "fp8"), (5, "mxfp4")):
        os.environ["SPECKV_POOL_DEVICES"] = "0,0,0,0,0,0,0"
        try:
            kv = pkg.CxlSpeckvKVAllocator(pkg.library_path(), f"hip:{torch.cuda.current_device()}")
            try:
                r = list(batch_attention_extra(torch, kv, scheme=scheme).values())[0]
                out[f"{name}_batch_256x8k"] = {k: r.get(k) for k in ("ms_per_layer", "frac_hbm", "error") if k in r}
            finally:
                kv.close()
        except Exception as e:
            out[f"{name}_batch_256x8k"] = {"error": repr(e)}
        finally:
            os.environ.pop("SPECKV_POOL_DEVICES", None)
    return {"fused_attention_striped_x7": out}


def run_engine_extras(torch, kv, handle, n_blocks, T, Lyr):
    """Latency / rate of the non-bulk entry points (C ABI calls, not kernels alone)."""
    lib = kv.lib
    ex = {}
    rng = np.random.default_rng(7)
    # SURVEY 8d access pattern (ii): the same blocks fetched in a seeded uniform-random page permutation
    try:
        perm = torch.from_numpy(np.random.default_rng(2001).permutation(n_blocks).astype(np.int32)).cuda()
        out = torch.empty((n_blocks, BLOCK_ELEMS), dtype=torch.float16, device="cuda")
        st_ = torch.cuda.Stream()
        def gather():
            lib.fetch_list(handle, perm.data_ptr(), n_blocks, out.data_ptr(), False, st_.cuda_stream)
        gather(); torch.cuda.synchronize()
        ramp(gather, torch.cuda.synchronize, EXTRAS_RAMP_MS)
        a_, b_ = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a_.record(st_)
        for _ in range(10):
            gather()
        b_.record(st_); torch.cuda.synchronize()
        ms = a_.elapsed_time(b_) / 10
        rec_total = lib.stats().compressed_bytes
        ex["fetch_random_permutation"] = {"blocks_per_s": round(n_blocks / (ms * 1e-3), 1), "ms": round(ms, 4),
                                          "frac_hbm": round((rec_total + n_blocks * (PAGE + 4 + 12)) / (ms * 1e-3) / 1e9 / HBM_PEAK_GBPS, 4),
                                          "note": "speckv_ext_fetch_list over a seeded permutation of all pages (page list + 8 B destination per block read too)"}
        del out, perm
    except Exception as e:
        ex["fetch_random_permutation"] = {"error": repr(e)}
    # speckv_access: miss = synchronous fetch of one page; hit = page-table lookup only
    offs = [int(p) * PAGE for p in rng.integers(0, n_blocks, 200)]
    t0 = time.perf_counter()
    for o in offs:
        lib.access(handle, o, 256)
    miss_us = (time.perf_counter() - t0) / len(offs) * 1e6
    t0 = time.perf_counter()
    for o in offs[:5]:
        for _ in range(2):
            lib.access(handle, o, 256)
    hit_us = (time.perf_counter() - t0) / 10 * 1e6
    ex["speckv_access_us"] = {"miss_sync_fetch": round(miss_us, 2), "hit": round(hit_us, 2),
                              "reference_emulated_us": "2.2-2.8 (SURVEY 3.1, no data moved)"}
    # one decode step of a 256-sequence batch worth of look-ahead requests against ONE allocation; the first flush of a
    # process also pays scratch allocation and first-launch costs, so it is reported apart.  The flush runs on the
    # device (candidates, dedupe, ring slots, fetch): `submit_ms` is what the caller's thread pays, `ms` includes
    # waiting for the fetched pages.
    n_req = 256 * Lyr
    reqs = np.zeros(n_req, np.uint32)
    layers = (np.arange(n_req) % Lyr).astype(np.uint16)
    depth = np.full(n_req, 4, np.uint32)
    flush_ms, submit_ms, enq_ms, issued_n = [], [], [], []
    for rep in range(5):
        pos = rng.integers(0, T - 8, n_req).astype(np.uint32)
        t0 = time.perf_counter()
        lib.prefetch_batch(reqs, layers, pos, depth)
        enq_ms.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        lib.prefetch_flush(want_count=False)
        t1 = time.perf_counter()
        lib.sync()
        flush_ms.append((time.perf_counter() - t0) * 1e3)
        submit_ms.append((t1 - t0) * 1e3)
        issued_n.append(int(lib.stats().total_prefetches))
    ex["prefetch_flush"] = {"requests": n_req, "pages_issued": issued_n[-1] - issued_n[-2], "ms": round(min(flush_ms[1:]), 3),
                            "submit_ms": round(min(submit_ms[1:]), 3), "enqueue_ms": round(min(enq_ms[1:]), 3),
                            "first_call_ms": round(flush_ms[0], 3), "requests_per_s": round(n_req / (min(flush_ms[1:]) * 1e-3), 1),
                            "note": "device-side flush (candidates + dedupe + ring slots + fetch launch) + sync, steady state; no host round trip"}
    # the reference's own call pattern: a flush every num_layers requests -- 32 requests, one workgroup runs the whole pipeline
    try:
        n_small = min(32, int(Lyr))
        s_req = np.zeros(n_small, np.uint32); s_lay = (np.arange(n_small) % Lyr).astype(np.uint16); s_dep = np.full(n_small, 4, np.uint32)
        sub_us, land_us = [], []
        for rep in range(24):
            pos = np.full(n_small, int(rng.integers(0, T - 8)), np.uint32)
            lib.prefetch_batch(s_req, s_lay, pos, s_dep)
            t0 = time.perf_counter()
            lib.prefetch_flush(want_count=False)
            t1 = time.perf_counter()
            lib.sync()
            land_us.append((time.perf_counter() - t0) * 1e6); sub_us.append((t1 - t0) * 1e6)
        ex["prefetch_flush_small"] = {"requests": n_small, "submit_us": round(float(np.median(sub_us[4:])), 1), "until_landed_us": round(float(np.median(land_us[4:])), 1),
                                      "note": "one speckv_prefetch-sized flush (requests = layers of the shape, look-ahead 4): upload, k_flush_small, fetch launch, sync"}
    except Exception as e:                                               # noqa: BLE001
        ex["prefetch_flush_small"] = {"error": repr(e)}
    ex.update(seq70b_extra(torch, kv))
    ex.update(fp8_scores_extra(torch, kv, 32768, 80))
    ex.update({k + "_8k_context": v for k, v in fp8_scores_extra(torch, kv, 8192, 80).items()})      # the same 80 layers at 8k (the split count by CU balance: round 6)
    ex.update(int4_attention_extra(torch, kv, 32768, 80))
    ex.update(int4_attention_extra(torch, kv, 32768, 80, scheme=5))      # the same on MXFP4 records (block-scaled matrix instruction)
    ex.update(batch_attention_extra(torch, kv))      # BASELINE configs[4] shape: 70B-shaped KV @ 32k context
    ex.update(batch_attention_extra(torch, kv, scheme=3))
    ex.update(batch_attention_extra(torch, kv, scheme=5))
    for sch in (4, 3, 5):                                                 # short contexts: 256 x 1k and 256 x 2k, batch and planned forms
        for T_short in (1024, 2048):
            ex.update(batch_attention_extra(torch, kv, T=T_short, scheme=sch))
    # batches that do not fill whole rounds of the CUs (round 6: the pieces per sequence by ring_rule.hpp balanced_tiles_per_piece; the merge of few rows
    # by a workgroup per row) and the 70B-shaped sequence at 4k context (the fixed grid below 28k, the stream form above)
    off = {}
    try:
        for sch, nm in ((4, "fp8"), (3, "int4_g32"), (5, "mxfp4")):
            for n_off in (32, 160, 300):
                r = list(batch_attention_extra(torch, kv, n_seq=n_off, scheme=sch).values())[0]
                off[f"{nm}_{n_off}x8k"] = {k: r.get(k) for k in ("ms_per_layer", "frac_hbm", "planned_ms_per_layer", "planned_frac_hbm", "error") if k in r}
            r = (fp8_scores_extra(torch, kv, 4096, 80) if sch == 4 else int4_attention_extra(torch, kv, 4096, 80, scheme=sch))
            r = next(v for k, v in r.items() if "fused_attention" in k)
            off[f"{nm}_one_sequence_80_layers_4k"] = {k: r.get(k) for k in ("ms_all_layers", "frac_hbm", "error") if k in r}
        off.update(ragged_batch_extra(torch, kv, scheme=4))            # members of different lengths: dispatched by length (round 6)
        off.update(ragged_batch_extra(torch, kv, scheme=5, n_seq=512))
        off.update(ragged_batch_extra(torch, kv, scheme=4, hi=32768, tail=True))      # ... with a heavy tail: pieces of a CU's share, the grid rows first
    except Exception as e:                                               # noqa: BLE001
        off["error"] = repr(e)
    ex["attention_off_round_sizes"] = dict(off, note="256 x 8k / 32k x 80 layers are the figures above; here: 32, 160 and 300 sequences x 8k (one layer per call, batch and planned "
                                                      "entries) and one sequence x 80 layers x 4k; fraction of 8 TB/s in record bytes")
    ex.update(connector_append_extra(torch, kv))
    ex.update(connector_decode_extra(torch, kv))
    ex.update(connector_decode_extra(torch, kv, scheme="mxfp4"))      # the same decode step over an MXFP4 pool (half the record bytes of FP8)
    ex.update(connector_decode_extra(torch, kv, ctx=16384, T=16384 + 64, scheme="fp8", tail=True))      # prompts of very different lengths (round 6: pieces, dispatch order)
    ex.update(kv_accuracy_extra(torch, kv))
    ex.update(predictor_extra(torch, lib))
    ex.update(lstm_cell_extra(torch, lib))
    ex.update(compaction_extra(torch, kv))
    ex.update(tensor_codec_batch_extra(torch, lib))                    # the reference's call size: 4096 tensors of 131 072 elements, one launch each way
    ex.update(tensor_codec_extra(torch, lib))
    ex.update(tensor_codec_extra(torch, lib, n=1280 * 2**20))          # a 2.5 GiB source: ten times the Infinity Cache
    return ex


def run_extras(torch, pkg, lib, src, dst, n_blocks, sp):
    """Secondary measurements through the raw codec operators (same kernels):
    every scheme's decode, and the compress side.  Not part of `value`."""
    raw = lib.lib
    ex = {}
    recs = torch.empty((n_blocks, PAGE), dtype=torch.uint8, device="cuda")
    lens = torch.empty(n_blocks, dtype=torch.int32, device="cuda")
    scales = torch.empty(n_blocks, dtype=torch.float32, device="cuda")
    try:
        dst32 = torch.empty((n_blocks, BLOCK_ELEMS), dtype=torch.float32, device="cuda")
    except Exception:                                                    # noqa: BLE001  (no room beside the other buffers: the figure is skipped)
        dst32 = None

    def timed(fn, reps=10):
        fn(); torch.cuda.synchronize()
        ramp(fn, torch.cuda.synchronize, EXTRAS_RAMP_MS)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); [fn() for _ in range(reps)]; b.record(); torch.cuda.synchronize()
        return a.elapsed_time(b) / reps

    for scheme, mode, name in ((0, 0, "fp16_copy"), (1, 0, "int8_ref_exact"), (2, 0, "rle_ref_exact"), (2, 1, "rle_intent"),
                               (3, 0, "int4_g32"), (4, 0, "fp8_e4m3"), (5, 0, "mxfp4")):
        stride = {1: 2048, 3: 1152, 4: 2048, 5: 1152}.get(scheme, PAGE)
        enc = lambda: raw.speckv_ext_codec_compress(src.data_ptr(), n_blocks, recs.data_ptr(), stride, lens.data_ptr(), scales.data_ptr(), scheme, mode, sp)
        dec = lambda: raw.speckv_ext_codec_decompress(recs.data_ptr(), stride, lens.data_ptr(), scales.data_ptr(), n_blocks, dst.data_ptr(), 0, scheme, mode, sp)
        enc_ms = timed(enc)
        dec_ms = timed(dec)
        comp = int(lens.to(torch.int64).sum().item())
        dec_bytes = comp + n_blocks * ((0 if scheme in (3, 5) else 4) + PAGE)
        enc_bytes = n_blocks * PAGE + comp + n_blocks * 8
        # the same blocks decoded to fp32, the reference's own output type (FPGACacheEngine::decompress returns floats): 8 KiB written per block
        if dst32 is not None:
            dec32 = lambda: raw.speckv_ext_codec_decompress(recs.data_ptr(), stride, lens.data_ptr(), scales.data_ptr(), n_blocks, dst32.data_ptr(), 1, scheme, mode, sp)
            dec32_ms = timed(dec32)
        ex[name] = {
            "decompress_blocks_per_s": round(n_blocks / (dec_ms * 1e-3), 1),
            "decompress_GBps": round(dec_bytes / (dec_ms * 1e-3) / 1e9, 1),
            "decompress_frac_hbm": round(dec_bytes / (dec_ms * 1e-3) / 1e9 / HBM_PEAK_GBPS, 4),
            "compress_blocks_per_s": round(n_blocks / (enc_ms * 1e-3), 1),
            "compress_GBps": round(enc_bytes / (enc_ms * 1e-3) / 1e9, 1),
            "record_bytes_per_block": round(comp / n_blocks, 1),
        }
        if dst32 is not None:
            ex[name]["decompress_fp32_out_frac_hbm"] = round((dec_bytes + n_blocks * PAGE) / (dec32_ms * 1e-3) / 1e9 / HBM_PEAK_GBPS, 4)
    del dst32
    # SURVEY 8d structured sets that exercise the RLE stage itself: all-zero blocks (one run per 255 elements) and
    # piecewise-constant blocks (runs of 32), INT8_DELTA_RLE, reference quantiser
    g = torch.Generator(device="cuda"); g.manual_seed(77)
    pw = torch.randn((n_blocks, BLOCK_ELEMS // 32), generator=g, device="cuda").repeat_interleave(32, dim=1).to(torch.float16)
    # ... and blocks of LONG runs (equal values for 200 .. 900 elements: every run is split at 255, cache_engine.cpp:224): the fast
    # encoder's SPLIT form (round 4; the element-wise loop took 745 us per 131 072 such blocks)
    m = n_blocks * BLOCK_ELEMS // 200 + 1
    long_runs = torch.repeat_interleave(torch.randn(m, generator=g, device="cuda"), torch.randint(200, 900, (m,), generator=g, device="cuda"))
    long_runs = long_runs[:n_blocks * BLOCK_ELEMS].to(torch.float16).reshape(n_blocks, BLOCK_ELEMS).contiguous()
    for name, data in (("rle_all_zero_blocks", torch.zeros_like(src)), ("rle_piecewise_runs_of_32", pw), ("rle_long_runs_200_900", long_runs)):
        enc = lambda: raw.speckv_ext_codec_compress(data.data_ptr(), n_blocks, recs.data_ptr(), PAGE, lens.data_ptr(), scales.data_ptr(), 2, 0, sp)
        dec = lambda: raw.speckv_ext_codec_decompress(recs.data_ptr(), PAGE, lens.data_ptr(), scales.data_ptr(), n_blocks, dst.data_ptr(), 0, 2, 0, sp)
        # the same with SPECKV_CODEC_HINT_STRUCTURED (0x100): the decoder instantiation for data known to compress
        dec_hint = lambda: raw.speckv_ext_codec_decompress(recs.data_ptr(), PAGE, lens.data_ptr(), scales.data_ptr(), n_blocks, dst.data_ptr(), 0, 2, 0x100, sp)
        enc_ms = timed(enc)
        dec_ms = timed(dec)
        hint_ms = timed(dec_hint)
        comp = int(lens.to(torch.int64).sum().item())
        dec_bytes = comp + n_blocks * (4 + PAGE)
        # ... and through the ENGINE with no hint from anybody: speckv_ext_fetch_range over an allocation that was written with this
        # data -- the compress kernel's own record-length samples pick the flat-run decoder
        eng_ms = None
        try:
            lib.set_compression_scheme(2)
            he = lib.alloc(n_blocks * PAGE)
            lib.write(he, 0, data.data_ptr(), data.numel() * 2, True)
            eng_ms = timed(lambda: lib.fetch_range(he, 0, n_blocks, dst.data_ptr(), False, sp))
            lib.free(he)
        except Exception as e:
            eng_ms = None
        ex[name] = {"decompress_blocks_per_s": round(n_blocks / (dec_ms * 1e-3), 1),
                    "decompress_GBps": round(dec_bytes / (dec_ms * 1e-3) / 1e9, 1),
                    "decompress_frac_hbm": round(dec_bytes / (dec_ms * 1e-3) / 1e9 / HBM_PEAK_GBPS, 4),
                    "decompress_frac_hbm_structured_hint": round(dec_bytes / (hint_ms * 1e-3) / 1e9 / HBM_PEAK_GBPS, 4),
                    "engine_fetch_range_frac_hbm_no_hint_given": round(dec_bytes / (eng_ms * 1e-3) / 1e9 / HBM_PEAK_GBPS, 4) if eng_ms else None,
                    "compress_blocks_per_s": round(n_blocks / (enc_ms * 1e-3), 1),
                    "record_bytes_per_block": round(comp / n_blocks, 1)}
    return ex


if __name__ == "__main__":
    main()
