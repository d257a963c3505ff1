"""Loop-hafnian tables (sup_loop_hafnian_table) on one MI355X: DESIGN.md §8o's
timing table.  One shape per process, so a job script can give every step its
own time limit.

  --d D --m M  dims (D,) * M of one random M-mode B and zeta (entries scaled so
               that the amplitudes stay of order one)
  --low E      also the table with SUP_LHAF_TABLE_LOW=E (1: every slab a launch)
  --each       also sup_loop_hafnian_complex_each over ALL prod dims patterns in
               the same run (kernel time and wall clock), and the largest
               difference from the table
  --twin       also the host twin on 16 threads (wall clock) and whether the
               bits agreed

Each device call is run once unmeasured (code object load, buffer growth), then
`--reps` times; every time is listed and the median is the figure.  Kernel
times are the calls' own HIP events (sup_stats.kernel_ms: the low kernel and
every slab launch).  The streamed traffic is taken as 48 bytes per entry: the
load of t[m], the load from slab c - 2 and the store; the loads at -stride_j
re-read slab c - 1.

Appends one JSON line to stdout and to <--out>/probe_lhaf_table.log."""
import argparse
import itertools
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
ap.add_argument("--d", type=int, required=True)
ap.add_argument("--m", type=int, required=True)
ap.add_argument("--low", type=int, default=0)
ap.add_argument("--each", action="store_true")
ap.add_argument("--twin", action="store_true")
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--out", default=os.path.join(os.path.dirname(__file__), "..", "..", "profiles", "lhaf_table"))
args = ap.parse_args()

if S.device_count() < 1:
    sys.exit("probe_lhaf_table: no HIP device (a CPU run measures nothing)")
os.makedirs(args.out, exist_ok=True)

M, dims = args.m, (args.d,) * args.m
rng = np.random.default_rng(2700 + M)
B = rng.standard_normal((M, M)) + 1j * rng.standard_normal((M, M))
B = (B + B.T) * (0.25 / math.sqrt(M))
zeta = (rng.standard_normal(M) + 1j * rng.standard_normal(M)) * 0.25


def measure(fn):
    fn()  # warm-up
    wall, kern = [], []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        out = fn()
        wall.append((time.perf_counter() - t0) * 1e3), kern.append(out[1]["kernel_ms"])
    return out, [round(w, 3) for w in wall], [round(v, 4) for v in kern]


def ubits(a):
    return a.reshape(-1, order="F").view(np.uint64)


def table_row(kern, wall, st):
    km = statistics.median(kern)
    gb = 48.0 * st["visited_steps"] / 1e9
    return {"kernel_ms": kern, "kernel_ms_median": km, "wall_ms": wall, "launches": st["launches"], "grid": st["grid"],
            "traffic_gb": round(gb, 4), "gb_per_s": round(gb / (km / 1e3), 1), "entries_per_s": st["visited_steps"] / (km / 1e3)}


(tab, st), wall, kern = measure(lambda: S.loop_hafnian_table(B, zeta, dims, return_stats=True))
row = {"box": platform.node(), "abi": S._lib.load().sup_abi_version(), "dims": list(dims), "entries": st["visited_steps"],
       "ops_per_entry": st["est_ops_per_step"], "table": table_row(kern, wall, st),
       "max_abs_entry": float(np.max(np.abs(tab)))}
if args.low:
    os.environ["SUP_LHAF_TABLE_LOW"] = str(args.low)
    (low_tab, lst), lwall, lkern = measure(lambda: S.loop_hafnian_table(B, zeta, dims, return_stats=True))
    del os.environ["SUP_LHAF_TABLE_LOW"]
    row["table_forced_low"] = dict(table_row(lkern, lwall, lst), low=args.low,
                                   same_bits=bool(np.array_equal(ubits(low_tab), ubits(tab))))
    del low_tab
if args.twin:
    t0 = time.perf_counter()
    twin = S.loop_hafnian_table(B, zeta, dims, cpu=True, threads=16)
    row["twin"] = {"wall_ms": round((time.perf_counter() - t0) * 1e3, 3),
                   "same_bits": bool(np.array_equal(ubits(twin), ubits(tab)))}
    del twin
if args.each:
    pats = [p[::-1] for p in itertools.product(range(args.d), repeat=M)]  # mode 0 fastest: the table's order
    lists = [np.repeat(np.arange(M), p) for p in pats]
    of = np.zeros(len(lists), np.int32)
    (v, est), ewall, ekern = measure(lambda: S.loop_hafnian_each(B, zeta[None, :], lists, mu_of=of, return_stats=True))
    fac = np.array([math.sqrt(math.prod(math.factorial(k) for k in p)) for p in pats])
    row["each"] = {"items": len(lists), "kernel_ms": ekern, "kernel_ms_median": statistics.median(ekern), "wall_ms": ewall,
                   "wall_ms_median": statistics.median(ewall),
                   "max_abs_difference": float(np.max(np.abs(v / fac - tab.reshape(-1, order="F")))),
                   "wall_over_table_wall": statistics.median(ewall) / statistics.median(wall)}
line = json.dumps(row)
print(line, flush=True)
with open(os.path.join(args.out, "probe_lhaf_table.log"), "a") as log:
    log.write(line + "\n")
