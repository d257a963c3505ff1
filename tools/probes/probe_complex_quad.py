"""Complex double-double walk (sup_perman_complex_quad) throughput on one
MI355X, beside the fp64 complex walk (sup_perman_complex) on the same matrix in
the same session.

Default: kernel time of both walks on a dense standard-normal complex matrix
at n = 30 (whole permanent, 2^29 Gray steps) and on a 2^30-step range at
n = 40 (16384 wave-chunks at walk_log2 = 10).  Each walk runs once unmeasured
and then `--reps` times; every time is listed and the median is the figure.
Reported: Gray steps/s, fp64 ops/s at the nominal 86n - 28 (and at the 88n - 28
fp64 instructions the kernel's loop holds), and the time ratio against the op
ratio (86n - 28) / (6n - 2).

`--ranges N...` instead times a range of min(chunks, 16384) wave-chunks at
walk_log2 = 10 per order for both walks: the way to see what the AGPR moves of
the large orders cost (walk_cplxdd_resources.log) and to compare builds."""
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
ap.add_argument("--ranges", type=int, nargs="*", default=None)
args = ap.parse_args()

warm = np.random.default_rng(1).standard_normal((20, 20))
S.perman_complex(warm + 1j * warm.T)  # HIP initialisation, context and code object load
S.perman_complex_quad(warm + 1j * warm.T)


def timed(call):
    """kernel_ms of `reps` runs after one unmeasured run, and the last result."""
    call()
    ms = []
    for _ in range(args.reps):
        v, st = call()
        ms.append(st["kernel_ms"])
    return ms, v, st


def report(n, what, q, c, st, steps, v):
    qm, cm = statistics.median(q), statistics.median(c)
    print(json.dumps({
        "n": n, "what": what, "lane_bits": st["lane_bits"], "walk_bits": st["walk_bits"], "grid": st["grid"],
        "gray_steps": steps, "quad_kernel_ms": [round(x, 3) for x in q], "complex_kernel_ms": [round(x, 3) for x in c],
        "quad_ms_median": round(qm, 3), "complex_ms_median": round(cm, 3),
        "quad_gray_steps_per_s": steps / (qm / 1e3), "quad_nominal_ops_per_s": steps * (86 * n - 28) / (qm / 1e3),
        "quad_fp64_insts_per_s": steps * (88 * n - 28) / (qm / 1e3),
        "complex_ops_per_s": steps * (6 * n - 2) / (cm / 1e3),
        "time_ratio": qm / cm, "op_ratio": (86 * n - 28) / (6 * n - 2), "inst_ratio": (88 * n - 28) / (6 * n - 2),
        "value": [list(p) for p in v],
    }), flush=True)


def range_pair(n):
    rng = np.random.default_rng(1000 + n)
    a = rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))
    cnt = min(1 << max(n - 17, 0), 16384)
    q, v, st = timed(lambda: S.perman_complex_quad_range(a, 0, cnt, walk_log2=10, return_stats=True))
    c, _, sc = timed(lambda: S.perman_complex_range(a, 0, cnt, walk_log2=10, return_stats=True))
    assert sc["gray_steps"] == st["gray_steps"]
    report(n, f"range of {cnt} chunks", q, c, st, st["gray_steps"], v)


if args.ranges is not None:
    for n in args.ranges:
        range_pair(n)
else:
    n = 30
    rng = np.random.default_rng(1000 + n)
    a = rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))
    q, v, st = timed(lambda: S.perman_complex_quad(a, return_stats=True))
    c, w, _ = timed(lambda: S.perman_complex(a, return_stats=True))
    assert abs(complex(v[0][0], v[1][0]) - w) <= 1e-6 * abs(w)
    report(n, "whole", q, c, st, 1 << (n - 1), v)
    range_pair(40)
