"""Torontonian tables (sup_torontonian_table) on one MI355X: DESIGN.md §8m's
timing table.  One order per process, so a job script can give every step its
own time limit.

  --n N        the first N modes of one random 32-mode O (dyadic entries,
               Gershgorin row sums in [0.5, 0.9])
  --loop       also the loop table (a dyadic gamma, whole exponent about 4)
  --bits L,K   also the transform with SUP_MOBIUS_BITS=L,K (6,1: close to one
               naive pass per bit)
  --e2e        also all 2^N click probabilities of a random N-mode state from
               one table against threshold_detection_probs over all patterns
               (one batch call per click count), wall clock

Each device call is run once unmeasured (code object load, buffer growth), then
`--reps` times; every time is listed and the median is the figure.  Kernel
times are the calls' own HIP events (sup_stats.kernel_ms: prepare + walk +
transform).  The transform's time is the transformed table's median minus the
raw table's; its traffic is passes x 2 x 8 x 2^N bytes.

Appends one JSON line to stdout and to <--out>/probe_torontonian_table.log."""
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
ap.add_argument("--loop", action="store_true")
ap.add_argument("--bits", default="")
ap.add_argument("--e2e", action="store_true")
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--out", default=os.path.join(os.path.dirname(__file__), "..", "..", "profiles", "torontonian_table"))
args = ap.parse_args()

if S.device_count() < 1:
    sys.exit("probe_torontonian_table: no HIP device (a CPU run measures nothing)")
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


def measure(fn):
    fn()  # warm-up
    wall, kern = [], []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        out = fn()
        wall.append((time.perf_counter() - t0) * 1e3), kern.append(out[1]["kernel_ms"])
    return out, [round(w, 3) for w in wall], [round(v, 3) for v in kern]


def passes(L, K):
    return 1 if n <= L else 1 + -(-(n - L) // K)


def transform_row(raw_ms, tab_ms, L, K):
    ms = tab_ms - raw_ms
    gb = passes(L, K) * 16.0 * 2 ** n / 1e9
    return {"bits": [L, K], "passes": passes(L, K), "transform_ms": round(ms, 3), "traffic_gb": round(gb, 4),
            "gb_per_s": round(gb / (ms / 1e3), 1) if ms > 0 else None}


(tv, tst), _, tkern = measure(lambda: S.torontonian_batch(O, modes, return_stats=True))
(raw, rst), rwall, rkern = measure(lambda: S.torontonian_table(O, modes, transform=False, return_stats=True))
(tab, st), wall, kern = measure(lambda: S.torontonian_table(O, modes, return_stats=True))
tm, rm, km = statistics.median(tkern), statistics.median(rkern), statistics.median(kern)
row = {
    "box": platform.node(), "abi": S._lib.load().sup_abi_version(), "n": n, "grid": st["grid"],
    "torontonian_kernel_ms": tkern, "torontonian_kernel_ms_median": tm,
    "raw_table_kernel_ms": rkern, "raw_table_kernel_ms_median": rm, "raw_over_torontonian": rm / tm,
    "table_kernel_ms": kern, "table_kernel_ms_median": km, "table_wall_ms": wall, "raw_table_wall_ms": rwall,
    "transform": transform_row(rm, km, S.MOBIUS_TILE_BITS, S.MOBIUS_PASS_BITS),
    "table_full_minus_torontonian": float(tab[-1] - tv), "est_ops_per_subset": st["est_ops_per_step"],
}
del raw, tab
if args.bits:
    L, K = (int(v) for v in args.bits.split(","))
    os.environ["SUP_MOBIUS_BITS"] = args.bits
    _, _, bkern = measure(lambda: S.torontonian_table(O, modes, return_stats=True))
    del os.environ["SUP_MOBIUS_BITS"]
    row["transform_forced"] = transform_row(rm, statistics.median(bkern), L, K)
    row["table_kernel_ms_forced"] = bkern
if args.loop:
    (lv, _), _, lkern = measure(lambda: S.loop_torontonian_batch(O, gamma, modes, return_stats=True))
    _, _, lrkern = measure(lambda: S.loop_torontonian_table(O, gamma, modes, transform=False, return_stats=True))
    row.update({"loop_torontonian_kernel_ms": lkern, "loop_raw_table_kernel_ms": lrkern,
                "loop_raw_over_loop_torontonian": statistics.median(lrkern) / statistics.median(lkern)})
if args.e2e:
    srng = np.random.default_rng(3300 + n)
    B = srng.normal(size=(2 * n, 2 * n)) * 0.35 / math.sqrt(n / 4.0)
    B = (B + B.T) / 2
    J = np.block([[np.zeros((n, n)), np.eye(n)], [-np.eye(n), np.zeros((n, n))]])
    Sp, term = np.eye(2 * n), np.eye(2 * n)
    for j in range(1, 40):
        term = term @ (J @ B) / j
        Sp = Sp + term
    cov = Sp @ np.diag(np.tile(2.0 * (srng.uniform(0.0, 0.5, n) + 0.5), 2)) @ Sp.T
    cov, mu = (cov + cov.T) / 2, srng.normal(size=2 * n) * math.sqrt(2.0) * 0.7
    pats = (np.arange(1 << n)[:, None] >> np.arange(n)[None, :]) & 1
    S.threshold_detection_distribution(mu, cov)
    t0 = time.perf_counter()
    p = S.threshold_detection_distribution(mu, cov)
    t_tab = (time.perf_counter() - t0) * 1e3
    S.threshold_detection_probs(mu, cov, pats[:2])
    t0 = time.perf_counter()
    q = S.threshold_detection_probs(mu, cov, pats)
    t_pat = (time.perf_counter() - t0) * 1e3
    row["e2e"] = {"distribution_wall_ms": round(t_tab, 3), "per_pattern_wall_ms": round(t_pat, 3),
                  "speedup": t_pat / t_tab, "max_abs_difference": float(np.max(np.abs(p - q))),
                  "sum_minus_one": float(math.fsum(p) - 1.0)}
line = json.dumps(row)
print(line, flush=True)
with open(os.path.join(args.out, "probe_torontonian_table.log"), "a") as log:
    log.write(line + "\n")
