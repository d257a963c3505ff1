"""Torontonians (sup_torontonian) on one MI355X next to the host twin on 16
threads: DESIGN.md §8j's timing table.  One order per process, so a job script
can give every step its own time limit.

  --n N        the first N modes of one random 32-mode O (dyadic entries,
               Gershgorin row sums in [0.5, 0.9])
  --twin       also time the host twin on --threads threads (the same bits)
  --scratch    also time the twin factoring every subset from nothing
               (TOR_TWIN_TAIL=0: the reuse's speedup on the host, N <= 20)

The device call is run once unmeasured (code object load, buffer growth), then
`--reps` times; every time is listed and the median is the figure.  Kernel
times are the calls' own HIP events (sup_stats.kernel_ms).  The fp64 issue
fraction is subsets/s x est_ops_per_step (the census of DESIGN.md §8j) over the
device's peak fp64 vector rate in lane-operations (--peak-gops, default 256 CUs
x 4 SIMDs x 16 lanes x 2.4 GHz = 39,322 G/s, an fma counting as one; the census
counts it as two, so it is halved here).

Appends one JSON line to stdout and to <--out>/probe_torontonian.log."""
import argparse
import json
import math
import os
import platform
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", ".."))
import numpy as np  # noqa: E402

import superman_amd as S  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, required=True)
ap.add_argument("--twin", action="store_true")
ap.add_argument("--scratch", action="store_true")
ap.add_argument("--threads", type=int, default=16)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--peak-gops", type=float, default=256 * 4 * 16 * 2.4)
ap.add_argument("--out", default=os.path.join(os.path.dirname(__file__), "..", "..", "profiles", "torontonian"))
args = ap.parse_args()

if S.device_count() < 1:
    sys.exit("probe_torontonian: no HIP device (a CPU run measures nothing)")
os.makedirs(args.out, exist_ok=True)

M = 32
rng = np.random.default_rng(3200)
N = 2 * M
k = int(0.3 * 1024 / ((N - 1) * math.sqrt(2)))
A = np.tril(rng.integers(-k, k + 1, (N, N)) + 1j * rng.integers(-k, k + 1, (N, N)), -1)
A = A + A.conj().T
O = (A + np.diag(np.floor(0.7 * 1024 - np.abs(A).sum(1)))) / 1024
n = args.n
modes = np.arange(n)


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return r, (time.perf_counter() - t0) * 1e3


def run():
    return S.torontonian_batch(O, modes, return_stats=True)


run()  # warm-up
wall, kern = [], []
for _ in range(args.reps):
    (v, st), w = timed(run)
    wall.append(w), kern.append(st["kernel_ms"])
km = statistics.median(kern)
rate = float(st["visited_steps"]) / (km / 1e3)
plain = sum(math.comb(n, j) / 2.0 ** n * 8 * (2 * j) ** 3 / 6 for j in range(n + 1))
row = {
    "box": platform.node(), "abi": S._lib.load().sup_abi_version(), "n": n, "subsets": st["visited_steps"],
    "grid": st["grid"], "value": v, "wall_ms": [round(x, 3) for x in wall], "kernel_ms": [round(x, 3) for x in kern],
    "kernel_ms_median": round(km, 3), "wall_ms_median": round(statistics.median(wall), 3),
    "subsets_per_s_kernel": rate, "est_ops_per_subset": st["est_ops_per_step"], "plain_ops_per_subset": plain,
    "census_reuse_ratio": plain / st["est_ops_per_step"], "useful_gflops": rate * st["est_ops_per_step"] / 1e9,
    "fp64_issue_fraction": rate * st["est_ops_per_step"] / 2 / (args.peak_gops * 1e9),
}
if args.twin:
    (tv, _), tw = timed(lambda: S.torontonian_batch(O, modes, cpu=True, threads=args.threads, return_stats=True))
    row.update({"twin_threads": args.threads, "twin_wall_ms": round(tw, 3), "twin_over_kernel": tw / km,
                "twin_bits_equal": bool(np.float64(tv).view(np.uint64) == np.float64(v).view(np.uint64))})
if args.scratch:
    os.environ["TOR_TWIN_TAIL"] = "0"
    (sv, _), sw = timed(lambda: S.torontonian_batch(O, modes, cpu=True, threads=args.threads, return_stats=True))
    del os.environ["TOR_TWIN_TAIL"]
    row.update({"twin_scratch_wall_ms": round(sw, 3),
                "scratch_bits_equal": bool(np.float64(sv).view(np.uint64) == np.float64(v).view(np.uint64))})
    if args.twin:
        row["twin_reuse_speedup"] = sw / row["twin_wall_ms"]
line = json.dumps(row)
print(line, flush=True)
with open(os.path.join(args.out, "probe_torontonian.log"), "a") as log:
    log.write(line + "\n")
