"""Batched complex permanents (sup_perman_complex_batch, _submatrices) on one
MI355X: DESIGN.md §8b's measurements b, c and d.  One session; every shape is
run once unmeasured first (code object load, buffer growth), then `--reps`
times; every time is listed and the median is the figure.  Wall times are a
host clock around calls that end in a stream synchronise; kernel times are the
calls' own HIP events (sup_stats.kernel_ms: prepare + walk + fold per slab).

  b  one perman_complex_batch call against a Python loop of perman_complex
     over the same matrices, n = 12, 16, 20, 24, count = 4096 (the loop is the
     single-matrix path as it was before the batch entries existed); the
     results are compared bit for bit
  c  Gray steps/s and fp64 instructions/s (6n - 2 per step) of the batch at
     n = 20 and 24, count = 4096, from kernel_ms, and what of the call's wall
     time is not kernel time (upload, launches, download)
  d  the submatrix form against the batch form on the same gathered matrices,
     n = 16, count = 65536, U 32 x 32

Writes one JSON line per row to stdout and to <--out>/probe_complex_batch.log."""
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
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--count", type=int, default=4096)
ap.add_argument("--sub-count", type=int, default=65536)
ap.add_argument("--n", type=int, nargs="*", default=[12, 16, 20, 24])
ap.add_argument("--out", default=os.path.join(os.path.dirname(__file__), "..", "..", "profiles", "complex_batch"))
args = ap.parse_args()

if S.device_count() < 1:
    sys.exit("probe_complex_batch: no HIP device (a CPU run measures nothing)")
os.makedirs(args.out, exist_ok=True)
log = open(os.path.join(args.out, "probe_complex_batch.log"), "w")


def emit(row):
    line = json.dumps(row)
    print(line, flush=True)
    log.write(line + "\n")
    log.flush()


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return r, (time.perf_counter() - t0) * 1e3


def bits(v):
    return np.ascontiguousarray(v).view(np.uint64)


emit({"box": platform.node(), "machine": platform.machine(), "devices": S.device_count(), "reps": args.reps,
      "abi": S._lib.load().sup_abi_version()})

for n in args.n:
    rng = np.random.default_rng(500 + n)
    mats = rng.standard_normal((args.count, n, n)) + 1j * rng.standard_normal((args.count, n, n))
    S.perman_complex_batch(mats)  # warm-up: this shape's code object and buffers
    [S.perman_complex(a) for a in mats[:64]]
    bw, bk, lw, lk = [], [], [], []
    for _ in range(args.reps):  # alternating
        (vb, st), w = timed(lambda: S.perman_complex_batch(mats, return_stats=True))
        bw.append(w), bk.append(st["kernel_ms"])
        rs, w = timed(lambda: [S.perman_complex(a, return_stats=True) for a in mats])
        lw.append(w), lk.append(sum(r[1]["kernel_ms"] for r in rs))
    vl = np.array([r[0] for r in rs], dtype=np.complex128)
    steps = float(args.count) * float(1 << (n - 1))
    b, k, l = statistics.median(bw), statistics.median(bk), statistics.median(lw)
    emit({
        "measurement": "b+c", "n": n, "count": args.count, "lane_bits": st["lane_bits"], "walk_bits": st["walk_bits"],
        "chunks_per_matrix": 1 << (n - 1 - st["lane_bits"] - st["walk_bits"]), "grid": st["grid"],
        "batch_wall_ms": [round(x, 3) for x in bw], "batch_kernel_ms": [round(x, 3) for x in bk],
        "loop_wall_ms": [round(x, 3) for x in lw], "loop_kernel_ms_sum": [round(x, 3) for x in lk],
        "batch_wall_ms_median": round(b, 3), "batch_kernel_ms_median": round(k, 3), "loop_wall_ms_median": round(l, 3),
        "loop_over_batch": l / b, "bit_equal": bool(np.array_equal(bits(vb), bits(vl))),
        "gray_steps_per_s_kernel": steps / (k / 1e3), "fp64_insts_per_s_kernel": steps * (6 * n - 2) / (k / 1e3),
        "gray_steps_per_s_wall": steps / (b / 1e3), "wall_not_kernel_ms": round(b - k, 3),
    })

# d: the submatrix form against the batch form on the same gathered matrices
n, R = 16, 32
rng = np.random.default_rng(16)
U = np.linalg.qr(rng.standard_normal((R, R)) + 1j * rng.standard_normal((R, R)))[0]
rows = np.sort(rng.integers(0, R, (args.sub_count, n)), axis=1)  # sorted mode lists: collisions repeat a row
cols = np.sort(rng.integers(0, R, (args.sub_count, n)), axis=1)
gathered = np.ascontiguousarray(U[rows[:, :, None], cols[:, None, :]])
S.perman_complex_submatrices(U, rows, cols)
S.perman_complex_batch(gathered)
sw, sk, gw, gk = [], [], [], []
for _ in range(args.reps):
    (vs, st), w = timed(lambda: S.perman_complex_submatrices(U, rows, cols, return_stats=True))
    sw.append(w), sk.append(st["kernel_ms"])
    (vg, sg), w = timed(lambda: S.perman_complex_batch(gathered, return_stats=True))
    gw.append(w), gk.append(sg["kernel_ms"])
s, g = statistics.median(sw), statistics.median(gw)
emit({
    "measurement": "d", "n": n, "count": args.sub_count, "U": [R, R],
    "submatrices_wall_ms": [round(x, 3) for x in sw], "submatrices_kernel_ms": [round(x, 3) for x in sk],
    "batch_wall_ms": [round(x, 3) for x in gw], "batch_kernel_ms": [round(x, 3) for x in gk],
    "submatrices_wall_ms_median": round(s, 3), "batch_wall_ms_median": round(g, 3), "batch_over_submatrices": g / s,
    "input_bytes_batch": int(gathered.nbytes), "input_bytes_submatrices": int(U.nbytes + 4 * rows.size + 4 * cols.size),
    "bit_equal": bool(np.array_equal(bits(vs), bits(vg))),
})
log.close()
