"""Exact complex residue walk (sup_perman_complex_exact) on one MI355X, beside
the fp64 complex walk (sup_perman_complex) and the complex double-double walk
(sup_perman_complex_quad) on the same matrix in the same session.

Whole permanents at n = 24, 30 and 36 of a random matrix with entries in
{-1, 0, 1} + {-1, 0, 1} i.  Each entry runs once unmeasured and then `--reps`
times; every kernel and wall time is listed and the medians are the figures.
Reported per order: G, the prime count and the launches it takes, the exact
walk's fp64 instructions per second at est_ops_per_step summed over its
launches, and the time ratios against both floating walks.  The three results
are compared: the fp64 walk's relative error against the exact integers, and
whether the double-double walk's high words are the exact integers rounded."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", ".."))
import numpy as np  # noqa: E402

import superman_amd as S  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--orders", type=int, nargs="*", default=[24, 30, 36])
args = ap.parse_args()

warm = np.random.default_rng(1).integers(-1, 2, (20, 20))
S.perman_complex(warm + 1j * warm.T)  # HIP initialisation, context and code object load
S.perman_complex_quad(warm + 1j * warm.T)
S.perman_complex_exact(warm + 1j * warm.T)


def timed(call):
    """kernel_ms and wall_ms of `reps` runs after one unmeasured run, and the last result."""
    call()
    k, w = [], []
    for _ in range(args.reps):
        v, st = call()
        k.append(st["kernel_ms"])
        w.append(st["wall_ms"])
    return k, w, v, st


def ops(n, G, primes):
    """sum over the launches of est_ops_per_step (include/superman.h)."""
    K = (n + G - 1) // G
    launches = (primes + 3) // 4
    return launches * (2 * n + (4 * (n // 2) if G == 2 else 0)) + primes * (10 * K - 2)


for n in args.orders:
    rng = np.random.default_rng(2000 + n)
    a = rng.integers(-1, 2, (n, n)) + 1j * rng.integers(-1, 2, (n, n))
    primes = len(S.perman_complex_exact_range(a, 0, 0, cpu=True)["primes"])
    ek, ew, ev, est = timed(lambda: S.perman_complex_exact(a, return_stats=True))
    ck, cw, cv, _ = timed(lambda: S.perman_complex(a, return_stats=True))
    row = {"n": n, "lane_bits": est["lane_bits"], "walk_bits": est["walk_bits"], "grid": est["grid"],
           "gray_steps": 1 << (n - 1), "G": est["seg_pair_bits"], "primes": primes, "launches": (primes + 3) // 4,
           "est_ops_per_step_one_launch": est["est_ops_per_step"], "ops_per_step_all_launches": ops(n, est["seg_pair_bits"], primes),
           "exact_kernel_ms": [round(x, 3) for x in ek], "exact_wall_ms": [round(x, 3) for x in ew],
           "complex_kernel_ms": [round(x, 3) for x in ck], "complex_wall_ms": [round(x, 3) for x in cw]}
    em, cm = statistics.median(ek), statistics.median(ck)
    row.update({"exact_ms_median": round(em, 3), "complex_ms_median": round(cm, 3),
                "exact_fp64_insts_per_s": (1 << (n - 1)) * ops(n, est["seg_pair_bits"], primes) / (em / 1e3),
                "complex_ops_per_s": (1 << (n - 1)) * (6 * n - 2) / (cm / 1e3),
                "exact_over_complex": em / cm, "op_ratio_exact_over_complex": ops(n, est["seg_pair_bits"], primes) / (6 * n - 2)})
    row["complex_rel_err"] = abs(cv - complex(ev[0], ev[1])) / max(abs(complex(ev[0], ev[1])), 1.0)
    if n <= S.COMPLEX_QUAD_MAX_DEVICE_N:
        qk, qw, qv, _ = timed(lambda: S.perman_complex_quad(a, return_stats=True))
        qm = statistics.median(qk)
        row.update({"quad_kernel_ms": [round(x, 3) for x in qk], "quad_wall_ms": [round(x, 3) for x in qw],
                    "quad_ms_median": round(qm, 3), "exact_over_quad": em / qm,
                    "op_ratio_exact_over_quad": ops(n, est["seg_pair_bits"], primes) / (86 * n - 28)})
        row["quad_hi_is_the_rounded_exact_value"] = (qv[0][0], qv[1][0]) == (float(ev[0]), float(ev[1]))
    row["value"] = [str(ev[0]), str(ev[1])]
    print(json.dumps(row), flush=True)
