"""Repeated fetch_range over one range: does alternating the sweep direction (tuning key fetch_sweep) let the Infinity Cache serve part
of it?  Settings: 0 ascending, non-temporal stores; 1 the shipped rule (a repeat walks the other way, plain stores); 2 always descending
with plain stores; 3 the directions of 1 with non-temporal stores.  One process, one pool per shape (placement differs by +-4 % between processes, so settings are compared inside one):

    python profiles/tools/sweep_direction.py [--blocks 131072,32768,524288] [--legs 6] [--steps 50] [--settings 0,1,2,3]

Per shape: an untimed ramp as bench.py does (the same step for --ramp-ms of wall time), then `legs` rounds; a round runs one leg of
`steps` back-to-back fetch_range calls per setting, in the order given, so the settings interleave.  A leg is timed by two HIP events on the
launch stream; its first step is run untimed in front of the events (it sets up the direction the setting leaves behind the previous leg's).
Printed per setting: the median of the leg means, the lowest and the highest leg, and the ratio of the medians to setting 0.
Settings 2 and 3 are the controls: plain stores without alternation, alternation without plain stores -- what each half is worth alone.
SPECKV_LIB_PATH picks an A/B build (make EXTRA=-DSPECKV_PLAIN_LOAD / -DSPECKV_PLAIN_STORE OUT=...); the line names the library."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
import torch
import cxl_speckv_amd as pkg

PAGE = 4096
HBM_PEAK_GBPS = 8000.0

ap = argparse.ArgumentParser()
ap.add_argument("--blocks", default="131072,32768,524288")
ap.add_argument("--legs", type=int, default=6)
ap.add_argument("--steps", type=int, default=50)
ap.add_argument("--settings", default="0,1,2,3")
ap.add_argument("--ramp-ms", type=float, default=60.0)
ap.add_argument("--scheme", type=int, default=2)
args = ap.parse_args()
settings = [int(v) for v in args.settings.split(",")]
assert settings[0] == 0, "setting 0 is what the others are compared with"

lib_path = pkg.library_path()
lib = pkg.SpeckvLib(lib_path, "hip:0")
lib.set_compression_scheme(args.scheme)
stream = torch.cuda.Stream()
sp = stream.cuda_stream
print(f"library {os.path.relpath(lib_path)}  scheme {args.scheme}  legs {args.legs} x {args.steps} steps per setting, interleaved  "
      f"device {torch.cuda.get_device_name(0)}", flush=True)

for n in [int(v) for v in args.blocks.split(",")]:
    h = lib.alloc(n * PAGE)
    g = torch.Generator(device="cuda"); g.manual_seed(2001)
    before = lib.stats().compressed_bytes
    for p0 in range(0, n, 65536):
        x = torch.randn((min(65536, n - p0), 2048), generator=g, device="cuda", dtype=torch.float32).to(torch.float16)
        lib.write(h, p0 * PAGE, x.data_ptr(), x.numel() * 2, True)
    del x
    alg = lib.stats().compressed_bytes - before + n * (4 + PAGE)
    dst = torch.empty((n, 2048), dtype=torch.float16, device="cuda")

    def step():
        lib.fetch_range(h, 0, n, dst.data_ptr(), False, sp)

    lib.set_tuning("fetch_sweep", settings[0])
    t0 = time.perf_counter()
    while (time.perf_counter() - t0) * 1e3 < args.ramp_ms:
        for _ in range(8):
            step()
        torch.cuda.synchronize()
    legs = {s: [] for s in settings}
    for _ in range(args.legs):
        for s in settings:
            lib.set_tuning("fetch_sweep", s)
            step()                                         # untimed: from here on the leg's steps see what this setting left behind
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            for _ in range(args.steps):
                step()
            b.record(stream)
            torch.cuda.synchronize()
            legs[s].append(a.elapsed_time(b) * 1e3 / args.steps)          # us per step
    print(f"blocks {n}  ({(alg + (1 << 19)) >> 20} MiB algorithmic per step)", flush=True)
    med0 = statistics.median(legs[0])
    for s in settings:
        v = legs[s]
        med = statistics.median(v)
        print(f"  fetch_sweep {s}: median {med:8.2f} us  lowest {min(v):8.2f}  highest {max(v):8.2f}  range {max(v) - min(v):6.2f}  "
              f"frac {alg / med / 1e3 / HBM_PEAK_GBPS:.4f}  ratio to 0 {med / med0:.4f}   legs " + " ".join(f"{t:.1f}" for t in v), flush=True)
    if 1 in legs:
        gain = med0 - statistics.median(legs[1])
        rng0 = max(legs[0]) - min(legs[0])
        print(f"  setting 1 is lower by {gain:.2f} us = {100.0 * gain / med0:.2f} %;  twice setting 0's leg-to-leg range = {2 * rng0:.2f} us", flush=True)
    lib.set_tuning("fetch_sweep", 1)
    del dst
    lib.free(h)
    torch.cuda.empty_cache()
lib.finalize()
