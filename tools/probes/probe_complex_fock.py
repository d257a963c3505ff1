"""Collision-aware complex permanents (sup_perman_complex_fock) against the
submatrix entry (sup_perman_complex_submatrices) on the same index lists, on
one MI355X: DESIGN.md §8c's timing table.  One (n, pattern) per process, so a
job script can give every step its own time limit.

  --n 16|20|24, --pattern collide|distinct, --count 4096, U a 32 x 32 unitary
  collide   the rows distinct, the columns in groups of four (n / 4 groups):
            T = 4 * 5^(n/4 - 1) <= 2^(n-1) / 64
  distinct  no repeated index on either side: T = 2^(n-1) (recorded only;
            there is no routing between the two entries)

Both calls are run once unmeasured (code object load, buffer growth), then
`--reps` times alternating; every time is listed and the median is the figure.
Wall times are a host clock around calls that end in a stream synchronise;
kernel times are the calls' own HIP events (sup_stats.kernel_ms).  The ideal
ratio is 2^(n-1) / T * (6n - 2) / 6n: the terms saved, times the fp64
instructions per step of the two walks.

Appends one JSON line to stdout and to <--out>/probe_complex_fock.log."""
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
ap.add_argument("--n", type=int, required=True, choices=[16, 20, 24])
ap.add_argument("--pattern", required=True, choices=["collide", "distinct"])
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--count", type=int, default=4096)
ap.add_argument("--out", default=os.path.join(os.path.dirname(__file__), "..", "..", "profiles", "complex_fock"))
args = ap.parse_args()

if S.device_count() < 1:
    sys.exit("probe_complex_fock: no HIP device (a CPU run measures nothing)")
os.makedirs(args.out, exist_ok=True)

n, R = args.n, 32
rng = np.random.default_rng(1600 + n)
U = np.linalg.qr(rng.standard_normal((R, R)) + 1j * rng.standard_normal((R, R)))[0]
rows = np.stack([rng.choice(R, n, replace=False) for _ in range(args.count)])
if args.pattern == "collide":
    cols = np.stack([np.repeat(rng.choice(R, n // 4, replace=False), 4) for _ in range(args.count)])
else:
    cols = np.stack([rng.choice(R, n, replace=False) for _ in range(args.count)])
terms, side = S.perman_complex_fock_plan(rows, cols)
T = int(terms[0])
assert (terms == T).all()


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return r, (time.perf_counter() - t0) * 1e3


S.perman_complex_fock(U, rows, cols)  # warm-up: this shape's code objects and buffers
S.perman_complex_submatrices(U, rows, cols)
fw, fk, sw, sk = [], [], [], []
for _ in range(args.reps):  # alternating
    (vf, stf), w = timed(lambda: S.perman_complex_fock(U, rows, cols, return_stats=True))
    fw.append(w), fk.append(stf["kernel_ms"])
    (vs, sts), w = timed(lambda: S.perman_complex_submatrices(U, rows, cols, return_stats=True))
    sw.append(w), sk.append(sts["kernel_ms"])
f, k, s, q = (statistics.median(x) for x in (fw, fk, sw, sk))
ideal = float(1 << (n - 1)) / T * (6 * n - 2) / (6 * n)
row = {
    "box": platform.node(), "abi": S._lib.load().sup_abi_version(), "n": n, "pattern": args.pattern,
    "count": args.count, "U": [R, R], "terms": T, "nominal_terms": 1 << (n - 1), "side": int(side[0]),
    "visited_steps": stf["visited_steps"], "grid": stf["grid"],
    "fock_wall_ms": [round(x, 3) for x in fw], "fock_kernel_ms": [round(x, 3) for x in fk],
    "submatrices_wall_ms": [round(x, 3) for x in sw], "submatrices_kernel_ms": [round(x, 3) for x in sk],
    "fock_wall_ms_median": round(f, 3), "fock_kernel_ms_median": round(k, 3),
    "submatrices_wall_ms_median": round(s, 3), "submatrices_kernel_ms_median": round(q, 3),
    "ideal_ratio": ideal, "wall_ratio": s / f, "kernel_ratio": q / k,
    "fock_steps_per_s_kernel": float(stf["visited_steps"]) / (k / 1e3),
    "fock_wall_not_kernel_ms": round(f - k, 3),
    "max_rel_diff": float(np.max(np.abs(vf - vs) / np.abs(vs))),
}
line = json.dumps(row)
print(line, flush=True)
with open(os.path.join(args.out, "probe_complex_fock.log"), "a") as log:
    log.write(line + "\n")
