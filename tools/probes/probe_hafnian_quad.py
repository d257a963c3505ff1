"""Double-double hafnians (sup_hafnian_complex_quad / sup_loop_hafnian_complex_quad)
on one MI355X: DESIGN.md §8q's two tables.  One case per process, so a job
script can give every step its own time limit.

  --case n24   six groups of four, count 4096: T = 12,500 per matrix
  --case n30   30 distinct indices, count 1:   T = 2^29
  --case n36   36 distinct indices, count 1:   T = 2^35
  --n N        with n30 / n36: another collision-free order
  --loop       the loop hafnian
  --study      instead of the timing: the relative error of the fp64 Kan walk
               (hafnian_batch) and of the power-trace entry against the
               double-double value, on a random complex symmetric matrix
               (Gaussian entries, not integers) at the case's order

Timing: the device call is run once unmeasured (code object load, buffer
growth), then `--reps` times; every time is listed and the median is the
figure.  Kernel times are the calls' own HIP events (sup_stats.kernel_ms).
The fp64 Kan walk runs on the same lists in the same process beside it.  The
fp64 issue fraction is states/s x est_ops_per_step (the censuses of DESIGN.md
§8h and §8q) over the device's peak fp64 vector rate in instructions
(--peak-gops, default 256 CUs x 4 SIMDs x 16 lanes x 2.4 GHz = 39,322 G
instructions/s).

Appends one JSON line to stdout and to <--out>/probe_hafnian_quad.log."""
import argparse
import json
import os
import platform
import statistics
import sys
from fractions import Fraction

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", ".."))
import numpy as np  # noqa: E402

import superman_amd as S  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--case", required=True, choices=["n24", "n30", "n36"])
ap.add_argument("--n", type=int, default=0)
ap.add_argument("--loop", action="store_true")
ap.add_argument("--study", action="store_true")
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--count", type=int, default=4096)
ap.add_argument("--peak-gops", type=float, default=256 * 4 * 16 * 2.4)
ap.add_argument("--out", default=os.path.join(os.path.dirname(__file__), "..", "..", "profiles", "hafnian_quad"))
args = ap.parse_args()

if S.device_count() < 1:
    sys.exit("probe_hafnian_quad: no HIP device (a CPU run measures nothing)")
os.makedirs(args.out, exist_ok=True)

M = 48
rng = np.random.default_rng(2900)
A = rng.standard_normal((M, M)) + 1j * rng.standard_normal((M, M))
A = (A + A.T) / 8
mu = np.diag(A).copy()
if args.case == "n24":
    n = 24
    idx = np.stack([np.repeat(rng.choice(M, 6, replace=False), 4) for _ in range(args.count)])
else:
    n = args.n or int(args.case[1:])
    idx = rng.choice(M, n, replace=False)[None, :]
row = {"box": platform.node(), "abi": S._lib.load().sup_abi_version(), "case": args.case, "n": n, "loop": args.loop,
       "count": int(idx.shape[0]), "terms": int(S.hafnian_plan(idx[0]))}


def median_of(fn):
    fn()  # warm-up
    kern, last = [], None
    for _ in range(args.reps):
        last = fn()
        kern.append(last[1]["kernel_ms"])
    return last, kern, statistics.median(kern)


def exact(v4):
    """[count, 4] double-double results as pairs of Fractions."""
    return [(Fraction(r[0]) + Fraction(r[1]), Fraction(r[2]) + Fraction(r[3])) for r in v4]


def rel_err(v, truth):
    """max over the matrices of |v - truth| / |truth|, the difference in exact arithmetic."""
    worst = 0.0
    for z, (tr, ti) in zip(np.atleast_1d(v), truth):
        dr, di = Fraction(float(z.real)) - tr, Fraction(float(z.imag)) - ti
        worst = max(worst, float(dr * dr + di * di) ** 0.5 / float(tr * tr + ti * ti) ** 0.5)
    return worst


if args.study:
    q, qst = S.hafnian_quad_batch(A, idx, mu=mu, loop=args.loop, return_stats=True)
    truth = exact(q)
    kan, kst = S.hafnian_batch(A, idx, mu=mu, loop=args.loop, return_stats=True)
    pt, pst = S.hafnian_powertrace_batch(A, idx, mu=mu, loop=args.loop, return_stats=True)
    row.update({"study": True, "dd_kernel_ms": round(qst["kernel_ms"], 3), "kan_kernel_ms": round(kst["kernel_ms"], 3),
                "powertrace_kernel_ms": round(pst["kernel_ms"], 3), "value_hi": [float(q[0][0]), float(q[0][2])],
                "kan_rel_err": rel_err(kan, truth), "powertrace_rel_err": rel_err(pt, truth)})
else:
    (q, qst), qk, qm = median_of(lambda: S.hafnian_quad_batch(A, idx, mu=mu, loop=args.loop, return_stats=True))
    (f, fst), fk, fm = median_of(lambda: S.hafnian_batch(A, idx, mu=mu, loop=args.loop, return_stats=True))
    qrate, frate = qst["visited_steps"] / (qm / 1e3), fst["visited_steps"] / (fm / 1e3)
    row.update({"visited_steps": qst["visited_steps"], "grid": qst["grid"], "dd_kernel_ms": [round(x, 3) for x in qk],
                "dd_kernel_ms_median": round(qm, 3), "fp64_kernel_ms": [round(x, 3) for x in fk],
                "fp64_kernel_ms_median": round(fm, 3), "dd_states_per_s": qrate, "fp64_states_per_s": frate,
                "dd_est_ops_per_step": qst["est_ops_per_step"], "fp64_est_ops_per_step": fst["est_ops_per_step"],
                "time_ratio": qm / fm, "op_ratio": qst["est_ops_per_step"] / fst["est_ops_per_step"],
                "dd_fp64_issue_fraction": qrate * qst["est_ops_per_step"] / (args.peak_gops * 1e9),
                "fp64_fp64_issue_fraction": frate * fst["est_ops_per_step"] / (args.peak_gops * 1e9),
                "fp64_rel_err_vs_dd": rel_err(f, exact(q))})
line = json.dumps(row)
print(line, flush=True)
with open(os.path.join(args.out, "probe_hafnian_quad.log"), "a") as log:
    log.write(line + "\n")
