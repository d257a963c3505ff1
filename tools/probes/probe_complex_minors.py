"""One-walk permanent minors (sup_perman_complex_minors) and the boson sampler
(sup_boson_sample) on one MI355X: DESIGN.md §8d's measurements.  One session;
every shape is run once unmeasured first (code object load, buffer growth),
then `--reps` times, the two routes alternating; every time is listed and the
median is the figure.  Wall times are a host clock around calls that end in a
stream synchronise; kernel times are the calls' own HIP events
(sup_stats.kernel_ms: prepare + walk + fold per slab).

  a  perman_complex_minors_submatrices of `--count` matrices (n rows of a
     32 x 32 unitary's transpose, n - 1 of its columns) against the route it
     replaces: perman_complex_batch on the n * count materialised minors, in
     the same process; n = 16, 20, 24.  Call and kernel times, their ratios,
     the ideal n(6n - 8)/(16n - 24), Gray steps/s and fp64 instructions/s
     (16n - 24 per step) of the minors walk.
  b  boson_sample at M = 64, n = 16, 20, 24, `--samples` samples: samples/s and
     the share of the wall time inside the minors calls and inside the host pmf
     stage.
  --kernels-only N: three minors calls at n = N and nothing else (the run
     rocprofv3 --kernel-trace wraps for the prepare / walk / fold split).

Writes one JSON line per row to stdout and to <--out>/probe_complex_minors.log."""
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
ap.add_argument("--samples", type=int, default=1024)
ap.add_argument("--n", type=int, nargs="*", default=[16, 20, 24])
ap.add_argument("--kernels-only", type=int, nargs="*", default=None)
ap.add_argument("--out", default=os.path.join(os.path.dirname(__file__), "..", "..", "profiles", "complex_minors"))
args = ap.parse_args()

if S.device_count() < 1:
    sys.exit("probe_complex_minors: no HIP device (a CPU run measures nothing)")


def haar(M, seed):
    rng = np.random.default_rng(seed)
    q, r = np.linalg.qr(rng.standard_normal((M, M)) + 1j * rng.standard_normal((M, M)))
    d = np.diag(r)
    return q * (d / np.abs(d))


def lists(n, count, R, seed):
    rng = np.random.default_rng(seed)
    rows = np.stack([rng.permutation(R)[:n] for _ in range(count)])  # distinct input modes
    cols = np.sort(rng.integers(0, R, (count, n - 1)), axis=1)       # output modes drawn so far: collisions repeat
    return rows, cols


if args.kernels_only is not None:
    U = haar(32, 32)
    for n in args.kernels_only:
        rows, cols = lists(n, args.count, 32, 600 + n)
        for _ in range(4):
            S.perman_complex_minors_submatrices(U, rows, cols)
    sys.exit(0)

os.makedirs(args.out, exist_ok=True)
log = open(os.path.join(args.out, "probe_complex_minors.log"), "w")


def emit(row):
    line = json.dumps(row)
    print(line, flush=True)
    log.write(line + "\n")
    log.flush()


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return r, (time.perf_counter() - t0) * 1e3


emit({"box": platform.node(), "machine": platform.machine(), "devices": S.device_count(), "reps": args.reps,
      "abi": S._lib.load().sup_abi_version()})

U = haar(32, 32)
for n in args.n:
    q = n - 1
    rows, cols = lists(n, args.count, 32, 600 + n)
    B = U[rows[:, :, None], cols[:, None, :]]                                    # count x n x q
    keep = np.array([[i for i in range(n) if i != j] for j in range(n)])           # n x q
    mats = np.ascontiguousarray(B[:, keep, :]).reshape(args.count * n, q, q)       # minor (k, j) at k n + j
    S.perman_complex_minors_submatrices(U, rows, cols)  # warm-up
    S.perman_complex_batch(mats[: 64 * n])
    mw, mk, bw, bk = [], [], [], []
    for _ in range(args.reps):  # alternating
        (vm, st), w = timed(lambda: S.perman_complex_minors_submatrices(U, rows, cols, return_stats=True))
        mw.append(w), mk.append(st["kernel_ms"])
        (vb, sb), w = timed(lambda: S.perman_complex_batch(mats, return_stats=True))
        bw.append(w), bk.append(sb["kernel_ms"])
    vb = vb.reshape(args.count, n)
    rel = float(np.max(np.abs(vm - vb) / np.abs(vb)))
    steps = float(args.count) * float(1 << (n - 2))
    m, k, b, kb = (statistics.median(x) for x in (mw, mk, bw, bk))
    emit({
        "measurement": "a", "n": n, "count": args.count, "lane_bits": st["lane_bits"], "walk_bits": st["walk_bits"],
        "chunks_per_matrix": 1 << (q - 1 - st["lane_bits"] - st["walk_bits"]), "grid": st["grid"],
        "minors_wall_ms": [round(x, 3) for x in mw], "minors_kernel_ms": [round(x, 3) for x in mk],
        "batch_wall_ms": [round(x, 3) for x in bw], "batch_kernel_ms": [round(x, 3) for x in bk],
        "minors_wall_ms_median": round(m, 3), "minors_kernel_ms_median": round(k, 3),
        "batch_wall_ms_median": round(b, 3), "batch_kernel_ms_median": round(kb, 3),
        "batch_over_minors_wall": b / m, "batch_over_minors_kernel": kb / k,
        "ideal_ratio": n * (6 * n - 8) / (16 * n - 24), "max_rel_difference": rel,
        "gray_steps_per_s_kernel": steps / (k / 1e3), "fp64_insts_per_s_kernel": steps * (16 * n - 24) / (k / 1e3),
        "batch_fp64_insts_per_s_kernel": float(args.count * n) * float(1 << (q - 1)) * (6 * q - 2) / (kb / 1e3),
        "wall_not_kernel_ms": round(m - k, 3),
    })

M = 64
UM = haar(M, 64)
for n in args.n:
    inputs = np.arange(n)
    S.boson_sample(UM, inputs, args.samples, seed=1)  # warm-up
    ws, ks, ms_, ps = [], [], [], []
    for r in range(args.reps):
        (s, st), w = timed(lambda: S.boson_sample(UM, inputs, args.samples, seed=2 + r, return_stats=True))
        ws.append(w), ks.append(st["kernel_ms"]), ms_.append(st["minors_ms"]), ps.append(st["pmf_ms"])
    w = statistics.median(ws)
    emit({
        "measurement": "b", "M": M, "n": n, "samples": args.samples,
        "wall_ms": [round(x, 3) for x in ws], "kernel_ms": [round(x, 3) for x in ks],
        "minors_calls_ms": [round(x, 3) for x in ms_], "pmf_stage_ms": [round(x, 3) for x in ps],
        "wall_ms_median": round(w, 3), "samples_per_s": args.samples / (w / 1e3),
        "minors_share_of_wall": statistics.median(ms_) / w, "pmf_share_of_wall": statistics.median(ps) / w,
        "kernel_share_of_wall": statistics.median(ks) / w,
        "collision_free_fraction": float(np.mean((np.diff(s, axis=1) > 0).all(axis=1))),
    })
log.close()
