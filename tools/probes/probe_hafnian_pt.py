"""Power-trace hafnians (sup_hafnian_complex_pt / sup_loop_hafnian_complex_pt) on
one MI355X next to the Kan walk (sup_hafnian_complex) on the same collision-free
matrix: DESIGN.md §8i's timing table.  One order per process, so a job script
can give every step its own time limit.

  --n N        N distinct indices of one 64 x 64 matrix
  --loop       the loop hafnian
  --kan        also time the Kan walk at this order (2^(N-1) states: N <= 40)

The device call is run once unmeasured (code object load, buffer growth), then
`--reps` times; every time is listed and the median is the figure.  Kernel
times are the calls' own HIP events (sup_stats.kernel_ms).  The fp64 issue
fraction is subsets/s x est_ops_per_step (the census of DESIGN.md §8i: useful
operations on the rows and columns of each subset) over the device's peak fp64
vector rate in instructions (--peak-gops, default 256 CUs x 4 SIMDs x 16 lanes
x 2.4 GHz = 39,322 G lane-operations/s).

Appends one JSON line to stdout and to <--out>/probe_hafnian_pt.log."""
import argparse
import json
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
ap.add_argument("--loop", action="store_true")
ap.add_argument("--kan", action="store_true")
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--peak-gops", type=float, default=256 * 4 * 16 * 2.4)
ap.add_argument("--out", default=os.path.join(os.path.dirname(__file__), "..", "..", "profiles", "hafnian_pt"))
args = ap.parse_args()

if S.device_count() < 1:
    sys.exit("probe_hafnian_pt: no HIP device (a CPU run measures nothing)")
os.makedirs(args.out, exist_ok=True)

M = 64
rng = np.random.default_rng(2400)
A = rng.standard_normal((M, M)) + 1j * rng.standard_normal((M, M))
A = (A + A.T) / 8
mu = np.diag(A).copy()
n = args.n
idx = rng.choice(M, n, replace=False)


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return r, (time.perf_counter() - t0) * 1e3


def run():
    return S.hafnian_powertrace_batch(A, idx, mu=mu, loop=args.loop, return_stats=True)


run()  # warm-up
wall, kern = [], []
for _ in range(args.reps):
    (v, st), w = timed(run)
    wall.append(w), kern.append(st["kernel_ms"])
k = statistics.median(kern)
rate = float(st["visited_steps"]) / (k / 1e3)
row = {
    "box": platform.node(), "abi": S._lib.load().sup_abi_version(), "n": n, "loop": args.loop,
    "subsets": st["visited_steps"], "grid": st["grid"], "value": [v.real, v.imag],
    "wall_ms": [round(x, 3) for x in wall], "kernel_ms": [round(x, 3) for x in kern],
    "kernel_ms_median": round(k, 3), "wall_ms_median": round(statistics.median(wall), 3),
    "subsets_per_s_kernel": rate, "est_ops_per_subset": st["est_ops_per_step"],
    "useful_gflops": rate * st["est_ops_per_step"] / 1e9,
    "fp64_issue_fraction": rate * st["est_ops_per_step"] / (args.peak_gops * 1e9),
}
if args.kan:
    S.hafnian_batch(A, idx, mu=mu, loop=args.loop)
    kk = []
    for _ in range(args.reps):
        kv, kst = S.hafnian_batch(A, idx, mu=mu, loop=args.loop, return_stats=True)
        kk.append(kst["kernel_ms"])
    km = statistics.median(kk)
    row.update({"kan_kernel_ms": [round(x, 3) for x in kk], "kan_kernel_ms_median": round(km, 3),
                "kan_states_per_s": float(kst["visited_steps"]) / (km / 1e3), "kan_over_powertrace": km / k,
                "kan_value": [kv.real, kv.imag], "relative_difference": abs(kv - v) / abs(kv)})
line = json.dumps(row)
print(line, flush=True)
with open(os.path.join(args.out, "probe_hafnian_pt.log"), "a") as log:
    log.write(line + "\n")
