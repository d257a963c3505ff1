"""Exact hafnians (sup_hafnian_complex_exact) on one MI355X next to the fp64 Kan
walk (sup_hafnian_complex / sup_loop_hafnian_complex) on the same input in the
same run: DESIGN.md §8k's timing table.  One case per process, so a job script
can give every step its own time limit.

  --case n24   six groups of four, count 4096: T = 12,500 per matrix
  --case n30   30 distinct indices, count 1:   T = 2^29
  --case n36   36 distinct indices, count 1:   T = 2^35
  --n N        with n30 / n36: another collision-free order
  --loop       the loop hafnian

Entries are in {-1,0,1} + {-1,0,1} i.  Each entry is run once unmeasured (code
object load, buffer growth), then `--reps` times; every time is listed and the
median is the figure.  Kernel times are the calls' own HIP events
(sup_stats.kernel_ms).  Recorded beside them: the primes and walk launches, the
two censuses (est_ops_per_step), their ratio and the time ratio, and the fp64
issue fraction of both, states/s x est_ops_per_step over the device's peak
fp64 vector rate in instructions (--peak-gops, default 256 CUs x 4 SIMDs x 16
lanes x 2.4 GHz = 39,322 G instructions/s), as probe_hafnian.py computes it.

Appends one JSON line to stdout and to <--out>/probe_hafnian_exact.log."""
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
ap.add_argument("--case", required=True, choices=["n24", "n30", "n36"])
ap.add_argument("--n", type=int, default=0)
ap.add_argument("--loop", action="store_true")
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--count", type=int, default=4096)
ap.add_argument("--peak-gops", type=float, default=256 * 4 * 16 * 2.4)
ap.add_argument("--out", default=os.path.join(os.path.dirname(__file__), "..", "..", "profiles", "hafnian_exact"))
args = ap.parse_args()

if S.device_count() < 1:
    sys.exit("probe_hafnian_exact: no HIP device (a CPU run measures nothing)")
os.makedirs(args.out, exist_ok=True)

M = 48
rng = np.random.default_rng(2400)
A = rng.integers(-1, 2, (M, M)) + 1j * rng.integers(-1, 2, (M, M))
A = np.triu(A) + np.triu(A, 1).T
mu = np.diag(A).copy()
if args.case == "n24":
    n = 24
    idx = np.stack([np.repeat(rng.choice(M, 6, replace=False), 4) for _ in range(args.count)])
else:
    n = args.n or int(args.case[1:])
    idx = rng.choice(M, n, replace=False)[None, :]
T = int(S.hafnian_plan(idx[0]))


def measure(fn):
    fn()  # warm-up
    wall, kern = [], []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        v, st = fn()
        wall.append((time.perf_counter() - t0) * 1e3), kern.append(st["kernel_ms"])
    return v, st, wall, kern


def issue(st, k):
    return float(st["visited_steps"]) / (k / 1e3) * st["est_ops_per_step"] / (args.peak_gops * 1e9)


xv, xst, xwall, xkern = measure(lambda: S.hafnian_exact_batch(A, idx, mu=mu, loop=args.loop, return_stats=True))
fv, fst, fwall, fkern = measure(lambda: S.hafnian_batch(A, idx, mu=mu, loop=args.loop, return_stats=True))
xk, fk = statistics.median(xkern), statistics.median(fkern)
fv = np.atleast_1d(fv)
row = {
    "box": platform.node(), "abi": S._lib.load().sup_abi_version(), "case": args.case, "n": n, "loop": args.loop,
    "count": int(idx.shape[0]), "terms": T, "visited_steps": xst["visited_steps"], "grid": xst["grid"],
    "primes": xst["seg_cached_bits"], "launches": xst["seg_pair_bits"],
    "exact_kernel_ms": [round(x, 3) for x in xkern], "exact_kernel_ms_median": round(xk, 3),
    "exact_wall_ms_median": round(statistics.median(xwall), 3), "exact_est_ops_per_step": xst["est_ops_per_step"],
    "exact_fp64_issue_fraction": issue(xst, xk),
    "fp64_kernel_ms": [round(x, 3) for x in fkern], "fp64_kernel_ms_median": round(fk, 3),
    "fp64_wall_ms_median": round(statistics.median(fwall), 3), "fp64_est_ops_per_step": fst["est_ops_per_step"],
    "fp64_fp64_issue_fraction": issue(fst, fk),
    "op_ratio": xst["est_ops_per_step"] / fst["est_ops_per_step"], "time_ratio": xk / fk,
    "result_bits": max(abs(v).bit_length() for pair in xv for v in pair),
    # the fp64 walk judged from the exact integers: the largest |error| over the batch
    "fp64_max_abs_error": max(abs(complex(z.real - t[0], z.imag - t[1]))
                              for z, t in zip(fv, xv)),
}
line = json.dumps(row)
print(line, flush=True)
with open(os.path.join(args.out, "probe_hafnian_exact.log"), "a") as log:
    log.write(line + "\n")
