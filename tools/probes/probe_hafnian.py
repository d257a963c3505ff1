"""Hafnians with repeats (sup_hafnian_complex / sup_loop_hafnian_complex) on one
MI355X against their host twin on 16 threads, next to the collision-aware
permanent entry (sup_perman_complex_fock) at the same order: DESIGN.md §8h's
timing table.  One case per process, so a job script can give every step its
own time limit.

  --case n24   six groups of four, count 4096: T = 12,500 per matrix
  --case n30   30 distinct indices, count 1:   T = 2^29
  --case n40   40 distinct indices, count 1:   T = 2^39
  --n N        with n30 / n40: another collision-free order (a step that would
               pass its time limit is shrunk, not given longer)
  --loop       the loop hafnian
  --cpu-n N    the host twin is timed at this collision-free order when the
               case's own is out of its reach (default min(n, 28)); its rate
               in states per second is what is compared

The device call is run once unmeasured (code object load, buffer growth), then
`--reps` times; every time is listed and the median is the figure.  Kernel
times are the calls' own HIP events (sup_stats.kernel_ms).  The fp64 issue
fraction is states/s x est_ops_per_step (the census of DESIGN.md §8h) over the
device's peak fp64 vector rate in instructions (--peak-gops, default 256 CUs x
4 SIMDs x 16 lanes x 2.4 GHz = 39,322 G instructions/s).

Appends one JSON line to stdout and to <--out>/probe_hafnian.log."""
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
ap.add_argument("--case", required=True, choices=["n24", "n30", "n40"])
ap.add_argument("--n", type=int, default=0)
ap.add_argument("--loop", action="store_true")
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--count", type=int, default=4096)
ap.add_argument("--cpu-n", type=int, default=0)
ap.add_argument("--fock", action="store_true", help="also time perman_complex_fock at the same order and pattern")
ap.add_argument("--peak-gops", type=float, default=256 * 4 * 16 * 2.4)
ap.add_argument("--out", default=os.path.join(os.path.dirname(__file__), "..", "..", "profiles", "hafnian"))
args = ap.parse_args()

if S.device_count() < 1:
    sys.exit("probe_hafnian: no HIP device (a CPU run measures nothing)")
os.makedirs(args.out, exist_ok=True)

M = 48
rng = np.random.default_rng(2400)
A = rng.standard_normal((M, M)) + 1j * rng.standard_normal((M, M))
A = (A + A.T) / 8
mu = np.diag(A).copy()
if args.case == "n24":
    n = 24
    idx = np.stack([np.repeat(rng.choice(M, 6, replace=False), 4) for _ in range(args.count)])
else:
    n = args.n or int(args.case[1:])
    idx = rng.choice(M, n, replace=False)[None, :]
T = int(S.hafnian_plan(idx[0]))


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return r, (time.perf_counter() - t0) * 1e3


def run(**kw):
    return S.hafnian_batch(A, idx, mu=mu, loop=args.loop, return_stats=True, **kw)


run()  # warm-up
wall, kern = [], []
for _ in range(args.reps):
    (v, st), w = timed(run)
    wall.append(w), kern.append(st["kernel_ms"])
k = statistics.median(kern)
rate = float(st["visited_steps"]) / (k / 1e3)
row = {
    "box": platform.node(), "abi": S._lib.load().sup_abi_version(), "case": args.case, "n": n, "loop": args.loop,
    "count": int(idx.shape[0]), "terms": T, "visited_steps": st["visited_steps"], "grid": st["grid"],
    "wall_ms": [round(x, 3) for x in wall], "kernel_ms": [round(x, 3) for x in kern],
    "kernel_ms_median": round(k, 3), "wall_ms_median": round(statistics.median(wall), 3),
    "states_per_s_kernel": rate, "est_ops_per_step": st["est_ops_per_step"],
    "fp64_issue_fraction": rate * st["est_ops_per_step"] / (args.peak_gops * 1e9),
}
# the host twin on 16 threads, at an order it reaches
cn = args.cpu_n or min(n, 28)
cidx = idx if (args.case == "n24" or cn == n) else idx[:, :cn]
if args.case == "n24":
    cidx = idx[:256]
(cv, cst), cw = timed(lambda: S.hafnian_batch(A, cidx, mu=mu, loop=args.loop, cpu=True, threads=16,
                                              return_stats=True))
row.update({"cpu_n": int(cidx.shape[1]), "cpu_count": int(cidx.shape[0]), "cpu_wall_ms": round(cw, 3),
            "cpu_states_per_s": float(cst["visited_steps"]) / (cw / 1e3)})
row["gpu_over_cpu_rate"] = rate / row["cpu_states_per_s"]
if cidx.shape == idx.shape:
    row["same_bits_as_host_twin"] = bool(np.array_equal(np.atleast_1d(v).view(np.uint64),
                                                        np.atleast_1d(cv).view(np.uint64)))
if args.fock:  # the permanent entry at the same order: rows distinct, the columns in the hafnian's pattern
    rows = np.stack([rng.choice(M, n, replace=False) for _ in range(idx.shape[0])])
    S.perman_complex_fock(A, rows, idx)
    (fv, fst), fw = timed(lambda: S.perman_complex_fock(A, rows, idx, return_stats=True))
    frate = float(fst["visited_steps"]) / (fst["kernel_ms"] / 1e3)
    row.update({"fock_terms": int(S.perman_complex_fock_plan(rows[0], idx[0])[0]), "fock_kernel_ms": fst["kernel_ms"],
                "fock_wall_ms": round(fw, 3), "fock_states_per_s_kernel": frate,
                "fock_est_ops_per_step": fst["est_ops_per_step"],
                "fock_fp64_issue_fraction": frate * fst["est_ops_per_step"] / (args.peak_gops * 1e9)})
line = json.dumps(row)
print(line, flush=True)
with open(os.path.join(args.out, "probe_hafnian.log"), "a") as log:
    log.write(line + "\n")
