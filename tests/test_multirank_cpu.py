"""-m "not gpu": the N>1 contract of bench.py under gloo, world size 2, on CPU.

The path shards by blocks with no data-path collective (DESIGN.md sect. 6); what
the ranks share is the timing protocol: barrier + sync on both sides of exactly K
steps, MAX over ranks, whole-job rate = units of all ranks / that time."""
import os
import socket
import sys
import time

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, out_dir):
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import bench
    calls = []

    def step(i):
        calls.append(i)
        time.sleep(0.02 * (rank + 1))          # rank 1 is the slow one

    elapsed = bench.run_timed(step, steps=5, warmup=2, sync=lambda: None, dist=dist,
                              warm=lambda: calls.append("w"))
    rate = bench.whole_job_rate(world, 1000, 5, elapsed)
    # every rank owns its own shard: disjoint seeds / pools, identical sizes
    torch.save({"rank": rank, "elapsed": elapsed, "rate": rate, "calls": calls}, os.path.join(out_dir, f"r{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


def test_timing_protocol_world2(tmp_path):
    world = 2
    mp.spawn(_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    r = [torch.load(os.path.join(tmp_path, f"r{i}.pt")) for i in range(world)]
    for x in r:
        assert x["calls"] == ["w", "w", 0, 1, 2, 3, 4]          # W warmups, exactly K timed steps
    assert r[0]["elapsed"] == r[1]["elapsed"]                   # MAX over ranks is what everyone reports
    assert r[0]["elapsed"] >= 5 * 0.04 * 0.95                   # bounded below by the slow rank
    assert r[0]["rate"] == pytest.approx(2 * 1000 * 5 / r[0]["elapsed"])


def _placement_worker(rank, world, port, out_dir):
    """Each rank opens the page-table engine ("/dev/null": no GPU needed) with the pool list bench.py would give it and
    the ranks cross-check page -> pool placement, logical ids and shard sizes."""
    import ctypes as C
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import bench
    import cxl_speckv_amd as pkg
    PAGE = 4096
    res = {}
    # --- BASELINE configs[3] shape: 8 GPUs, rank 0 computes, pool striped over GPUs 1..7.  Both gloo ranks build the
    # same engine state and each verifies its own half of the page range.
    pools = bench.pool_devices_for("cfg4", 0, 8)
    assert pools == [1, 2, 3, 4, 5, 6, 7] and bench.pool_devices_for("cfg4", 3, 8) is None
    assert bench.pool_devices_for("cfg3", 0, 8) == [1] and bench.pool_devices_for("cfg3", 1, 8) is None
    os.environ["SPECKV_POOL_DEVICES"] = ",".join(map(str, pools))
    lib = pkg.SpeckvLib(pkg.library_path(), "/dev/null")
    os.environ.pop("SPECKV_POOL_DEVICES")
    raw = lib.lib
    raw.speckv_ext_pool_shard_pages.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32]
    raw.speckv_ext_pool_shard_pages.restype = C.c_uint64
    n_pages = 655360                                    # one 70B-shaped sequence at 8k context
    h = lib.alloc(n_pages * PAGE)
    lo, hi = rank * n_pages // world, (rank + 1) * n_pages // world
    count = [0] * 8
    sample = {}
    for p in list(range(lo, hi, 997)) + [lo, hi - 1]:
        info = lib.translate(h, p * PAGE)
        assert info.pool_device == pools[p % 7], (p, info.pool_device)
        sample[p] = (info.pool_device, info.virt_page_id, info.phys_page_id)
    for p in range(lo, hi):                             # exact per-pool page counts of this rank's half (arithmetic rule)
        count[pools[p % 7]] += 1
    shard = [raw.speckv_ext_pool_shard_pages(n_pages, 7, k) for k in range(7)]
    res["cfg4"] = {"count": count, "shard": shard, "sample": sample, "handle": h}
    lib.free(h)
    lib.finalize()
    # --- symmetric mode at the real world size: every rank's pool lives on its peers
    mine = bench.pool_devices_for("symmetric", rank, world)
    os.environ["SPECKV_POOL_DEVICES"] = ",".join(map(str, mine))
    lib = pkg.SpeckvLib(pkg.library_path(), "/dev/null")
    os.environ.pop("SPECKV_POOL_DEVICES")
    h = lib.alloc(64 * PAGE)
    res["symmetric"] = {"pools": mine, "devices": sorted({lib.translate(h, p * PAGE).pool_device for p in range(64)})}
    lib.finalize()
    gathered = [None] * world
    dist.all_gather_object(gathered, res)
    torch.save(gathered, os.path.join(out_dir, f"p{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


def test_page_to_pool_striping_world2(tmp_path):
    """pages striped page % n_pool over the pool GPUs.  Fails if the striping rule, the shard sizes or the
    rank -> pool-GPU lists of bench.py's remote modes break."""
    world = 2
    mp.spawn(_placement_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    views = [torch.load(os.path.join(tmp_path, f"p{i}.pt"), weights_only=False) for i in range(world)]
    assert views[0] == views[1]                                    # every rank gathered the same picture
    g = views[0]
    n_pages = 655360
    total = [g[0]["cfg4"]["count"][d] + g[1]["cfg4"]["count"][d] for d in range(8)]
    assert total[0] == 0 and sum(total) == n_pages                 # the compute GPU holds no pool pages
    assert g[0]["cfg4"]["shard"] == g[1]["cfg4"]["shard"] == [total[d] for d in range(1, 8)]
    assert max(total[1:]) - min(total[1:]) <= 1                    # balanced over the 7 links
    for r in range(world):
        for p, (dev, virt, phys) in g[r]["cfg4"]["sample"].items():
            h = g[r]["cfg4"]["handle"]
            assert dev == 1 + p % 7
            assert virt == (h << 32) | (p << 12) and phys == 0x4000000000 + (h << 20) + (p << 12)
    # the halves are disjoint and meet
    assert max(g[0]["cfg4"]["sample"]) + 1 == min(g[1]["cfg4"]["sample"])
    for r in range(world):
        assert r not in g[r]["symmetric"]["pools"] and g[r]["symmetric"]["devices"] == g[r]["symmetric"]["pools"]
    assert sorted(g[0]["symmetric"]["pools"] + g[1]["symmetric"]["pools"]) == [0, 1]


def test_remote_mode_pool_lists():
    sys.path.insert(0, ROOT)
    import bench
    for world in (2, 4, 8):
        sym = [bench.pool_devices_for("symmetric", r, world) for r in range(world)]
        for r in range(world):
            assert r not in sym[r] and len(sym[r]) == world - 1
        # every GPU serves as a pool of every other GPU exactly once
        assert all(sum(1 for r in range(world) if d in sym[r]) == world - 1 for d in range(world))
        assert bench.pool_devices_for("cfg3", 0, world) == [1]
        assert bench.pool_devices_for("cfg4", 0, world) == list(range(1, world))
        assert all(bench.pool_devices_for(m, r, world) is None for m in ("cfg3", "cfg4") for r in range(1, world))


def test_remote_working_set_rule_and_roofline_object():
    """the remote working set must exceed the pool GPU's 256 MiB Infinity Cache by >= 10x, and the rank-0 line
    carries the remote roofline as a first-class object (pure functions of bench.py, no GPU needed)."""
    sys.path.insert(0, ROOT)
    import bench
    set_bytes = 131072 * 4096                                   # the 8B-shaped set, 512 MiB of fp16
    for links in (1, 3, 7):
        n = bench.xgmi_sets_for(links, set_bytes, False)
        per_pool = n * set_bytes * (4080 / 4096) / links        # INT8_DELTA_RLE records of N(0,1) data
        assert per_pool >= 10 * bench.MALL_BYTES and (n - 1) * set_bytes / links < 10.6 * bench.MALL_BYTES
    assert bench.xgmi_sets_for(7, set_bytes, True) == 2         # the one-GPU dry run stays small
    eng = lambda g: {"inbound_GBps_per_compute_gpu": g, "link_bytes_per_pass": 10, "frac_nominal_per_direction": g / (7 * 153.6),
                     "frac_nominal_bidirectional": g / (7 * 76.8), "frac_of_raw_copy": 0.9}
    x = {"cfg3": {"links": 1, "fused_peer_load_kernel": eng(50.0), "copy_engines_then_local_decompress": eng(60.0)},
         "cfg4": {"links": 7, "fused_peer_load_kernel": eng(700.0), "raw_peer_copy_GBps": 800.0,
                  "copy_engines_then_local_decompress": dict(eng(650.0), copy_engine_link_bytes_per_pass=11),
                  "working_set": {"meets_10x_infinity_cache": True}, "speculative_prefetch_depth4": {"depth_k": 4}}}
    r = bench.roofline_xgmi_from(x, 8)
    assert r["layout"].startswith("cfg4") and r["engine"] == "fused_peer_load_kernel" and r["achieved"] == 700.0 and r["links"] == 7
    assert abs(r["frac"] - 700.0 / (7 * 153.6)) < 1e-9 and r["peak_nominal_per_direction"] == round(7 * 153.6, 1)
    assert r["copy_engine_link_bytes_per_pass"] == 11 and r["speculative_prefetch_depth4"]["depth_k"] == 4
    # two GPUs: cfg4 collapses into cfg3 and the object reports that layout; a failed phase yields no object
    r2 = bench.roofline_xgmi_from({"cfg3": x["cfg3"], "cfg4": {"same_as": "cfg3"}}, 2)
    assert r2["layout"].startswith("cfg3") and r2["engine"] == "copy_engines_then_local_decompress" and r2["links"] == 1
    assert bench.roofline_xgmi_from({"failed": "child died"}, 8) is None
    assert bench.roofline_xgmi_from({"cfg4": {"links": 7, "skipped": "no peer access"}}, 8)["skipped"] == "no peer access"


def test_single_rank_needs_no_process_group():
    sys.path.insert(0, ROOT)
    import bench
    n = []
    e = bench.run_timed(lambda i: n.append(i), steps=3, warmup=1, sync=lambda: None)
    assert n == [0, 0, 1, 2] and e > 0
    assert bench.whole_job_rate(1, 131072, 3, 0.5) == 131072 * 3 / 0.5


def test_bench_gpus_2_starts_its_own_ranks():
    """`python bench.py --gpus 2` with no launcher around it must come back with ONE line that says
    n_gpus == 2.  bench.py starts `python -m torch.distributed.run` as a child BEFORE importing torch or touching the GPU;
    SPECKV_BENCH_HOST_DRY_RUN=1 replaces the step with a host sleep (no GPU in this container), everything else -- launcher,
    rendezvous on 127.0.0.1, barrier + MAX-over-ranks timing, rank-0 line, exit code -- is the real control flow."""
    import json
    import subprocess
    env = dict(os.environ, SPECKV_BENCH_HOST_DRY_RUN="1")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "6", "--warmup", "2"],
                       env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout                              # rank 0 only
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["steps"] == 6 and d["warmup"] == 2 and "dry_run" in d
    assert d["ms_per_step"] >= 2.0                                # six 2 ms host steps were really timed
    assert abs(d["value"] - 2 * 131072 / (d["ms_per_step"] * 1e-3)) / d["value"] < 0.01     # whole-job: both ranks' units
    # a launcher that disagrees with --gpus is an error, not a silently relabelled 1-GPU line
    env2 = dict(env, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0")
    p2 = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0"],
                        env=env2, capture_output=True, text=True, timeout=300)
    assert p2.returncode != 0 and "WORLD_SIZE" in (p2.stderr + p2.stdout)


def test_committed_bench_line_has_the_contract_fields():
    """The bench line committed with the round's profile (profiles/r06f_bench.json = stdout of `python bench.py` on the
    MI355X box) carries every field of the driver's contract, with the tier's meaning: metric and config from
    BASELINE.json, roofline and cpu_baseline objects, no model keys; `value` is the W + K region at steady clocks (ramped), the cold
    as-called figure and a sustained one stand beside it."""
    import json
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    d = json.load(open(os.path.join(root, "profiles", "r06f_bench.json")))
    base = json.load(open(os.path.join(root, "BASELINE.json")))
    assert d["metric"] in base["metric"] and d["unit"] == "blocks/s"
    for k in ("value", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config"):
        assert k in d, k
    assert d["higher_is_better"] is True and d["scaling"] == "weak" and d["vs_baseline"] is None and d["data"] == "synthetic"
    assert d["dtype"].startswith("fp32") and "workload" in d["config"] and "model" not in d["config"]
    assert "configs[1]" in d["config"]["workload"]
    r = d["roofline"]
    assert r["bound"] == "hbm" and r["unit"] == "GB/s" and r["peak"] == 8000.0
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-3 and 0.5 < r["frac"] < 1.0
    # round 4: the cold figure stands in the roofline object too, and every variant names its dispatches (profiles/summarize_r04.py)
    assert r["frac_as_called"] == d["variants"]["as_called"]["frac_hbm"] and r["launches"]["kernel_instance"].startswith("k_fetch_decompress<2, 0, false")
    assert r["launches"]["as_called"] == [d["warmup"], d["warmup"] + d["steps"] - 1] and r["launches"]["ramped"][1] - r["launches"]["ramped"][0] == d["steps"] - 1
    assert r["traffic"] is None or 0.95 < r["traffic"] / r["algorithmic_bytes_per_launch"] < 1.2
    assert abs(d["value"] - 131072 * d["n_gpus"] / (d["ms_per_step"] * 1e-3)) / d["value"] < 0.01
    v = d["variants"]
    assert set(v) == {"as_called", "ramped", "sustained"}
    assert v["ramped"]["blocks_per_s"] == d["value"] and v["ramped"]["frac_hbm"] == r["frac"]
    assert v["as_called"]["frac_hbm"] <= v["ramped"]["frac_hbm"] + 0.02          # cold clocks never beat steady ones by much
    assert v["sustained"]["seconds"] >= 0.98 and v["sustained"]["steps"] > 1000
    assert "watchdog_fired" not in d
    c = d["cpu_baseline"]
    assert c["unit"] == "blocks/s" and c["kind"] in ("reference", "port") and c["cores"] >= 1 and c["value"] > 0 and c["sample"]
    assert c["port"]["value"] > 0 and c["port"]["cores"] == c["cores"]           # the C restatement is timed beside the compiled reference
    assert d["parity_spot_check"] is True
    f = d["extras"]["prefetch_flush"]
    assert f["requests"] == 8192 and f["pages_issued"] > 10000 and f["submit_ms"] < 0.1 and f["ms"] < 0.2
    # the 2-rank run on one GPU shows the three remote shapes with both engines
    d2 = json.load(open(os.path.join(root, "profiles", "r06f_bench_2ranks_one_gpu.json")))       # started by bench.py itself: `python bench.py --gpus 2`
    assert d2["n_gpus"] == 2
    x = d2["xgmi"]
    assert set(x) >= {"cfg3", "cfg4", "symmetric", "accounting"}
    for mode in ("cfg3", "symmetric"):
        assert {"fused_peer_load_kernel", "copy_engines_then_local_decompress", "raw_peer_copy_GBps"} <= set(x[mode])
    # ... and the 8-rank run on one GPU executes the 1 + 7 layout for real (7-way striping, D = 7 in the fetch kernel), with
    # the prefetch-flush leg of configs[2], the working-set statement, the copy engines' actual link bytes, and the top-level
    # remote roofline object of the rank-0 line
    d8 = json.load(open(os.path.join(root, "profiles", "r06f_bench_8ranks_one_gpu.json")))
    assert d8["n_gpus"] == 8 and "watchdog_fired" not in d8
    x8 = d8["xgmi"]
    for mode in ("cfg3", "cfg4", "symmetric"):
        m = x8[mode]
        assert "same_as" not in m and "skipped" not in m, (mode, m)
        assert m["links"] == (1 if mode == "cfg3" else 7)
        for eng in ("fused_peer_load_kernel", "copy_engines_then_local_decompress"):
            assert m[eng]["inbound_GBps_per_compute_gpu"] > 0 and m[eng]["link_bytes_per_pass"] > 0
        ce = m["copy_engines_then_local_decompress"]
        assert ce["copy_engine_link_bytes_per_pass"] >= ce["link_bytes_per_pass"] and 1.0 <= ce["slot_overhead"] < 1.05
        ws = m["working_set"]
        assert ws["allocations"] >= 1 and "meets_10x_infinity_cache" in ws and ws["record_MiB_per_pool_gpu"] > 0
    pf = x8["cfg4"]["speculative_prefetch_depth4"]
    assert pf["depth_k"] == 4 and pf["pages_per_step"] > 0 and pf["ms_submit_to_landed"] > 0 and pf["pipelined"]["pages"] > 0
    rx = d8["roofline_xgmi"]
    assert rx["bound"] == "xgmi" and rx["links"] == 7 and rx["layout"].startswith("cfg4") and rx["unit"] == "GB/s"
    assert abs(rx["peak_nominal_per_direction"] - 7 * 153.6) < 0.1 and abs(rx["peak_nominal_bidirectional"] - 7 * 76.8) < 0.1
    assert rx["engine"] in ("fused_peer_load_kernel", "copy_engines_then_local_decompress") and rx["achieved"] > 0
    assert "ONE-GPU DRY RUN" in rx["note"]                      # no link was crossed: the line says so itself
    assert d8["roofline"]["xgmi"]["links"] == 7 and d8["roofline"]["xgmi"]["frac"] == rx["frac"]      # north_star's second fraction inside `roofline`
    # round 5: the remote figure at the top level of the N > 1 line, and the engines compared bit for bit inside every mode
    assert d8["value_remote_fetch_blocks_per_s"] > 0 and d8["value_remote_fetch_GBps_inbound"] > 0 and "replica" in d8["value_note"]
    for mode in ("cfg3", "cfg4", "symmetric"):
        assert x8[mode]["engines_bit_identical"] is True, mode
    # the headline's evidence: the per-dispatch trace of the driver's command agrees with the bench's own HIP events
    s = json.load(open(os.path.join(root, "profiles", "r06f_summary.json")))["traced_run"]
    for variant in ("as_called", "ramped", "sustained"):
        assert abs(s[variant]["trace_vs_hip_events"]) < 0.02, (variant, s[variant])
        assert abs(s[variant]["frac_from_trace"] - s[variant]["bench_frac_hbm"]) < 0.01


def test_real_8_gpu_branch_of_the_remote_phase_by_rank():
    """VERDICT r5 #8 (first-contact readiness): the branch of bench.py's remote phase that a REAL 8-GPU node takes (not the
    SPECKV_BENCH_SINGLE_GPU_TEST dry run) as a pure function, asserted for every rank with 8 devices visible: the pool list each
    engine is opened with, the copy engine's per-peer streams, the working set (>= 10 x the 256 MiB Infinity Cache on
    every pool GPU) and a pessimistic wall-time estimate that must stay far inside the driver's 1 800 s."""
    sys.path.insert(0, ROOT)
    import bench
    world, set_bytes = 8, 131072 * 4096
    for rank in range(world):
        plans = {m: bench.xgmi_mode_plan(m, rank, world, set_bytes, False, 8) for m in bench.XGMI_MODES}
        others = [d for d in range(world) if d != rank]
        # configs[2]: rank 0 computes, pool on GPU 1; configs[3]: rank 0 computes, pool striped page % 7 over GPUs 1..7; the rest idle
        if rank == 0:
            assert plans["cfg3"]["pool_devices_env"] == "1" and plans["cfg3"]["peer_streams"] == 1
            assert plans["cfg4"]["pool_devices_env"] == "1,2,3,4,5,6,7" and plans["cfg4"]["peer_streams"] == 7
        else:
            assert not plans["cfg3"]["active"] and not plans["cfg4"]["active"] and plans["cfg4"]["pool_devices_env"] is None
        assert plans["symmetric"]["active"] and plans["symmetric"]["pool_devices_env"] == ",".join(map(str, others)) and plans["symmetric"]["peer_streams"] == 7
        assert all(p["error"] is None for p in plans.values())
        # every rank agrees on the shape of a mode (the barriers and reductions of the phase depend on it)
        assert [plans[m]["links"] for m in bench.XGMI_MODES] == [1, 7, 7]
        assert plans["cfg4"]["n_sets"] == 37 and plans["cfg4"]["working_set_bytes"] == 37 * 512 * 2**20       # 18.5 GiB, 2.64 GiB per pool GPU
        assert plans["cfg3"]["n_sets"] == 6
        for m in bench.XGMI_MODES:
            assert plans[m]["working_set_bytes_per_pool_gpu"] * (4080 / 4096) >= 10 * bench.MALL_BYTES
            assert plans[m]["expected_wall_s_at_40GBps_per_link"] < 300.0                                       # three modes: well inside the driver's 1 800 s
    # a rank that sees fewer devices than the world says so instead of opening a pool on a GPU that is not there
    assert "only 4 devices" in bench.xgmi_mode_plan("cfg4", 0, 8, set_bytes, False, 4)["error"]
    # ... and the one-GPU dry run keeps every "peer" on GPU 0 with a small working set
    dry = bench.xgmi_mode_plan("cfg4", 0, 8, set_bytes, True, 1)
    assert dry["pool_devices_env"] == "0,0,0,0,0,0,0" and dry["n_sets"] == 2 and dry["error"] is None


def test_host_cpu_info_reads_model_and_physical_cores():
    sys.path.insert(0, ROOT)
    import bench
    model, physical, logical = bench.host_cpu_info()
    assert isinstance(model, str) and model and logical >= 1 and (physical is None or 1 <= physical <= logical)


def test_dump_outputs_sample_is_fixed_and_bounded():
    """--dump-outputs writes the same blocks on every run of a shape (two builds compare output for output), first and last
    included, within the 64 MB a dump may take as float32; a plain run keeps the headline alone, --full is off by default."""
    sys.path.insert(0, ROOT)
    import bench
    import numpy as np
    for n in (5, bench.DUMP_ROWS, 131072):
        rows = bench.dump_rows(n)
        assert np.array_equal(rows, bench.dump_rows(n)) and rows[0] == 0 and rows[-1] == n - 1
        assert np.all(np.diff(rows) > 0) and len(rows) == min(n, bench.DUMP_ROWS)
        assert len(rows) * bench.BLOCK_ELEMS * 4 <= 64 * 1000 * 1000
    saved = sys.argv
    try:
        sys.argv = ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"]
        a = bench.parse_args()
        sys.argv += ["--full", "--dump-outputs", "out"]
        b = bench.parse_args()
    finally:
        sys.argv = saved
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, None) and (b.full, b.dump_outputs) == (True, "out")
