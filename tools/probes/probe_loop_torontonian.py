"""Loop torontonians (sup_loop_torontonian) on one MI355X next to the
torontonian kernel on the same O and modes and to the host twin on 16 threads:
DESIGN.md §8l's timing table.  One order per process, so a job script can give
every step its own time limit.

  --n N        the first N modes of one random 32-mode O (dyadic entries,
               Gershgorin row sums in [0.5, 0.9]) and a dyadic gamma whose
               whole exponent 1/2 gamma^H (I - O)^-1 gamma is about 4
  --twin       also time the host twin on --threads threads (the same bits)

Each device call is run once unmeasured (code object load, buffer growth), then
`--reps` times; every time is listed and the median is the figure.  Kernel
times are the calls' own HIP events (sup_stats.kernel_ms).  `ratio` is the
loop torontonian's median over the torontonian's; `census_ratio` is what the
two censuses (est_ops_per_step) predict.

Appends one JSON line to stdout and to <--out>/probe_loop_torontonian.log."""
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
ap.add_argument("--threads", type=int, default=16)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--out", default=os.path.join(os.path.dirname(__file__), "..", "..", "profiles", "loop_torontonian"))
args = ap.parse_args()

if S.device_count() < 1:
    sys.exit("probe_loop_torontonian: no HIP device (a CPU run measures nothing)")
os.makedirs(args.out, exist_ok=True)

M = 32
rng = np.random.default_rng(3200)
N = 2 * M
k = int(0.3 * 1024 / ((N - 1) * math.sqrt(2)))
A = np.tril(rng.integers(-k, k + 1, (N, N)) + 1j * rng.integers(-k, k + 1, (N, N)), -1)
A = A + A.conj().T
O = (A + np.diag(np.floor(0.7 * 1024 - np.abs(A).sum(1)))) / 1024
g = rng.normal(size=N) + 1j * rng.normal(size=N)
x = 0.5 * (g.conj() @ np.linalg.solve(np.eye(N) - O, g)).real
gamma = np.round(g * math.sqrt(4.0 / x) * 1024) / 1024
n = args.n
modes = np.arange(n)


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return r, (time.perf_counter() - t0) * 1e3


def bits(v):
    return int(np.float64(v).view(np.uint64))


def measure(fn):
    fn()  # warm-up
    wall, kern, out = [], [], None
    for _ in range(args.reps):
        out, w = timed(fn)
        wall.append(w), kern.append(out[1]["kernel_ms"])
    return out, wall, kern


(v, st), wall, kern = measure(lambda: S.loop_torontonian_batch(O, gamma, modes, return_stats=True))
(tv, tst), twall, tkern = measure(lambda: S.torontonian_batch(O, modes, return_stats=True))
km, tkm = statistics.median(kern), statistics.median(tkern)
rate = float(st["visited_steps"]) / (km / 1e3)
row = {
    "box": platform.node(), "abi": S._lib.load().sup_abi_version(), "n": n, "subsets": st["visited_steps"],
    "grid": st["grid"], "value": v, "wall_ms": [round(x, 3) for x in wall], "kernel_ms": [round(x, 3) for x in kern],
    "kernel_ms_median": round(km, 3), "wall_ms_median": round(statistics.median(wall), 3),
    "torontonian_kernel_ms": [round(x, 3) for x in tkern], "torontonian_kernel_ms_median": round(tkm, 3),
    "torontonian_grid": tst["grid"], "ratio": km / tkm,
    "est_ops_per_subset": st["est_ops_per_step"], "torontonian_est_ops_per_subset": tst["est_ops_per_step"],
    "census_ratio": st["est_ops_per_step"] / tst["est_ops_per_step"],
    "subsets_per_s_kernel": rate, "useful_gflops": rate * st["est_ops_per_step"] / 1e9,
}
if args.twin:
    (wv, _), tw = timed(lambda: S.loop_torontonian_batch(O, gamma, modes, cpu=True, threads=args.threads, return_stats=True))
    row.update({"twin_threads": args.threads, "twin_wall_ms": round(tw, 3), "twin_over_kernel": tw / km,
                "twin_bits_equal": bits(wv) == bits(v)})
line = json.dumps(row)
print(line, flush=True)
with open(os.path.join(args.out, "probe_loop_torontonian.log"), "a") as log:
    log.write(line + "\n")
