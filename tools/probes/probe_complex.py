"""Complex fp64 walk (sup_perman_complex) throughput on one MI355X, beside the
plain dense fp64 walk on the real part of the same matrix.

For each order (default 30 and 40; `--n 30` runs one) on a dense
standard-normal complex matrix: kernel_ms of perman_complex, kernel_ms of
perman(kernel="dense_plain") on the real part, Gray steps/s and fp64 ops/s at
6n - 2 ops per step, and the time ratio against the op-count ratio
(6n - 2) / (2n + 1).  Each walk runs `--reps` times; every time is listed and
the median is the figure.  n = 40 is 2^39 Gray steps: give that run its own
time limit, sized from the n = 30 figure (x 2^10 x 238 / 178).

`--ranges N...` instead times a range of min(chunks, 16384) wave-chunks at
walk_log2 = 10 (2^30 Gray steps) per order, the way to compare builds at
orders whose whole walk is out of reach (the occupancy request, n up to 64):
first launch dropped, median of the next three."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", ".."))
import numpy as np  # noqa: E402

import superman_amd as S  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, nargs="*", default=[30, 40])
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--ranges", type=int, nargs="*", default=None)
args = ap.parse_args()

warm = np.random.default_rng(1).standard_normal((20, 20))
S.perman_complex(warm + 1j * warm.T)  # HIP initialisation, context and code object load
S.perman(warm, kernel="dense_plain")

for n in args.ranges or []:
    rng = np.random.default_rng(n)
    a = rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))
    cnt = min(1 << max(n - 17, 0), 16384)
    ms = []
    for _ in range(4):
        v, st = S.perman_complex_range(a, 0, cnt, walk_log2=10, return_stats=True)
        ms.append(st["kernel_ms"])
    med = statistics.median(ms[1:])
    print(json.dumps({"n": n, "walk_bits": st["walk_bits"], "chunks": cnt, "grid": st["grid"],
                      "kernel_ms": [round(x, 3) for x in ms], "median_ms": round(med, 3),
                      "steps_per_s": st["gray_steps"] / (med / 1e3),
                      "ops_per_s": st["gray_steps"] * (6 * n - 2) / (med / 1e3)}), flush=True)

for n in ([] if args.ranges is not None else args.n):
    rng = np.random.default_rng(1000 + n)
    a = rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))
    re = np.ascontiguousarray(a.real)
    steps = float(1 << (n - 1))
    cms, pms = [], []
    for _ in range(args.reps):
        v, st = S.perman_complex(a, return_stats=True)
        cms.append(st["kernel_ms"])
        p, sp = S.perman(re, kernel="dense_plain", return_stats=True)
        pms.append(sp["kernel_ms"])
    c, d = statistics.median(cms), statistics.median(pms)
    print(json.dumps({
        "n": n, "lane_bits": st["lane_bits"], "walk_bits": st["walk_bits"], "grid": st["grid"],
        "complex_kernel_ms": [round(x, 3) for x in cms], "dense_plain_kernel_ms": [round(x, 3) for x in pms],
        "complex_ms_median": round(c, 3), "dense_plain_ms_median": round(d, 3),
        "gray_steps_per_s": steps / (c / 1e3), "fp64_ops_per_s": steps * (6 * n - 2) / (c / 1e3),
        "dense_plain_gray_steps_per_s": steps / (d / 1e3), "dense_plain_walk_kind": sp["walk_kind"],
        "time_ratio": c / d, "op_ratio": (6 * n - 2) / (2 * n + 1),
        "permanent": [v.real, v.imag],
    }), flush=True)
