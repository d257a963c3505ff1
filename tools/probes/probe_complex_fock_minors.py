"""Collision-aware one-walk minors (sup_perman_complex_fock_minors) and the
sampler on them (sup_boson_sample_fock) on one MI355X against the entries they
extend, in the same process: DESIGN.md §8e's measurements.  One session; every
shape is run once unmeasured first (code object load, buffer growth), then
`--reps` times, the two routes alternating; every time is listed and the median
is the figure.  Wall times are a host clock around calls that end in a stream
synchronise; kernel times are the calls' own HIP events (sup_stats.kernel_ms:
prepare + walk + fold per slab).  No ratio is fixed in advance: the yardstick
is the parent's entry in the same session, the ideal the term ratio times
(16n - 24)/(16n - 20).

  a  `--count` matrices from a 32 x 32 unitary at n = 17, 21, 25.
     "collide": the n - 1 columns in groups of four, against
     perman_complex_minors_submatrices on the same lists.
     "distinct": no repeated column (T = 2^(n-2)), recorded only — with the
     parent's time on the collide lists beside it, since the parent's walk does
     not depend on the lists.
  b  boson_sample against collision_aware=True, `--samples` samples, at
     (n, M) = (16, 64), (20, 64), (24, 64), (24, 32): wall time, kernel ms, the
     share of the wall time in the minors calls and in the host pmf stage, and
     the term ratio gray_steps / visited_steps from the stats.

  --kernels-only N...: four collide calls at each n = N and nothing else (the
     run rocprofv3 --kernel-trace wraps for the prepare / walk / fold split).

Writes one JSON line per row to stdout and to <--out>/probe_complex_fock_minors.log."""
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
ap.add_argument("--n", type=int, nargs="*", default=[17, 21, 25])
ap.add_argument("--kernels-only", type=int, nargs="*", default=None)
ap.add_argument("--out", default=os.path.join(os.path.dirname(__file__), "..", "..", "profiles", "complex_fock_minors"))
args = ap.parse_args()

if S.device_count() < 1:
    sys.exit("probe_complex_fock_minors: no HIP device (a CPU run measures nothing)")


def haar(M, seed):
    rng = np.random.default_rng(seed)
    q, r = np.linalg.qr(rng.standard_normal((M, M)) + 1j * rng.standard_normal((M, M)))
    d = np.diag(r)
    return q * (d / np.abs(d))


def lists(n, count, R, seed, group):
    """rows: n distinct of R; cols: n - 1 in groups of `group` equal values (the
    remainder a smaller last group), ascending as a sampler's drawn modes are."""
    rng = np.random.default_rng(seed)
    q = n - 1
    K = (q + group - 1) // group
    rows = np.stack([rng.permutation(R)[:n] for _ in range(count)])
    cols = np.stack([np.repeat(np.sort(rng.permutation(R)[:K]), group)[:q] for _ in range(count)])
    return rows, cols


if args.kernels_only is not None:
    U = haar(32, 32)
    for n in args.kernels_only:
        rows, cols = lists(n, args.count, 32, 700 + n, 4)
        for _ in range(4):
            S.perman_complex_fock_minors_submatrices(U, rows, cols)
    sys.exit(0)

os.makedirs(args.out, exist_ok=True)
log = open(os.path.join(args.out, "probe_complex_fock_minors.log"), "w")


def emit(row):
    line = json.dumps(row)
    print(line, flush=True)
    log.write(line + "\n")
    log.flush()


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return r, (time.perf_counter() - t0) * 1e3


def med(x):
    return statistics.median(x)


emit({"box": platform.node(), "machine": platform.machine(), "devices": S.device_count(), "reps": args.reps,
      "abi": S._lib.load().sup_abi_version()})

U = haar(32, 32)
for n in args.n:
    rows, cols = lists(n, args.count, 32, 700 + n, 4)
    _, dcols = lists(n, args.count, 32, 800 + n, 1)
    S.perman_complex_fock_minors_submatrices(U, rows, cols)  # warm-up
    S.perman_complex_fock_minors_submatrices(U, rows[:64], dcols[:64])
    S.perman_complex_minors_submatrices(U, rows, cols)
    fw, fk, pw, pk, dw, dk = [], [], [], [], [], []
    for _ in range(args.reps):  # alternating
        (vf, sf), w = timed(lambda: S.perman_complex_fock_minors_submatrices(U, rows, cols, return_stats=True))
        fw.append(w), fk.append(sf["kernel_ms"])
        (vp, sp), w = timed(lambda: S.perman_complex_minors_submatrices(U, rows, cols, return_stats=True))
        pw.append(w), pk.append(sp["kernel_ms"])
        (_, sd), w = timed(lambda: S.perman_complex_fock_minors_submatrices(U, rows, dcols, return_stats=True))
        dw.append(w), dk.append(sd["kernel_ms"])
    ratio = sp["gray_steps"] / sf["visited_steps"]
    ideal = ratio * (16 * n - 24) / (16 * n - 20)
    emit({
        "measurement": "a", "pattern": "collide", "n": n, "count": args.count, "grid": sf["grid"],
        "terms_per_matrix": sf["visited_steps"] // args.count, "parent_steps_per_matrix": 1 << (n - 2),
        "fock_wall_ms": [round(x, 3) for x in fw], "fock_kernel_ms": [round(x, 3) for x in fk],
        "parent_wall_ms": [round(x, 3) for x in pw], "parent_kernel_ms": [round(x, 3) for x in pk],
        "fock_wall_ms_median": round(med(fw), 3), "fock_kernel_ms_median": round(med(fk), 3),
        "parent_wall_ms_median": round(med(pw), 3), "parent_kernel_ms_median": round(med(pk), 3),
        "parent_over_fock_wall": med(pw) / med(fw), "parent_over_fock_kernel": med(pk) / med(fk),
        "term_ratio": ratio, "ideal_ratio": ideal, "kernel_ratio_over_ideal": med(pk) / med(fk) / ideal,
        "wall_not_kernel_ms": round(med(fw) - med(fk), 3),
        "states_per_s_kernel": sf["visited_steps"] / (med(fk) / 1e3),
        "fp64_insts_per_s_kernel": sf["visited_steps"] * (16 * n - 20) / (med(fk) / 1e3),
        "max_rel_difference": float(np.max(np.abs(vf - vp) / np.abs(vp))),
    })
    emit({
        "measurement": "a", "pattern": "distinct", "n": n, "count": args.count, "grid": sd["grid"],
        "terms_per_matrix": sd["visited_steps"] // args.count,
        "fock_wall_ms": [round(x, 3) for x in dw], "fock_kernel_ms": [round(x, 3) for x in dk],
        "fock_wall_ms_median": round(med(dw), 3), "fock_kernel_ms_median": round(med(dk), 3),
        "parent_kernel_ms_median_on_the_collide_lists": round(med(pk), 3),
        "parent_over_fock_kernel": med(pk) / med(dk),
        "states_per_s_kernel": sd["visited_steps"] / (med(dk) / 1e3),
        "fp64_insts_per_s_kernel": sd["visited_steps"] * (16 * n - 20) / (med(dk) / 1e3),
    })

for n, M in ((16, 64), (20, 64), (24, 64), (24, 32)):
    UM = haar(M, M)
    inputs = np.arange(n)
    S.boson_sample(UM, inputs, args.samples, seed=1)  # warm-up
    S.boson_sample(UM, inputs, args.samples, seed=1, collision_aware=True)
    rec = {False: ([], [], [], []), True: ([], [], [], [])}
    stats = {}
    same = True
    for r in range(args.reps):  # alternating, the same seed for both
        out = {}
        for aware in (False, True):
            (s, st), w = timed(lambda: S.boson_sample(UM, inputs, args.samples, seed=2 + r, return_stats=True,
                                                      collision_aware=aware))
            ws, ks, ms_, ps = rec[aware]
            ws.append(w), ks.append(st["kernel_ms"]), ms_.append(st["minors_ms"]), ps.append(st["pmf_ms"])
            stats[aware], out[aware] = st, s
        same = same and bool(np.array_equal(out[False], out[True]))
    ratio = stats[True]["gray_steps"] / stats[True]["visited_steps"]
    ideal = ratio * (16 * n - 24) / (16 * n - 20)
    (pw, pk, pm, pp), (fw, fk, fm_, fp) = rec[False], rec[True]
    emit({
        "measurement": "b", "n": n, "M": M, "samples": args.samples,
        "parent_wall_ms": [round(x, 3) for x in pw], "parent_kernel_ms": [round(x, 3) for x in pk],
        "fock_wall_ms": [round(x, 3) for x in fw], "fock_kernel_ms": [round(x, 3) for x in fk],
        "parent_wall_ms_median": round(med(pw), 3), "parent_kernel_ms_median": round(med(pk), 3),
        "fock_wall_ms_median": round(med(fw), 3), "fock_kernel_ms_median": round(med(fk), 3),
        "parent_over_fock_wall": med(pw) / med(fw), "parent_over_fock_kernel": med(pk) / med(fk),
        "term_ratio": ratio, "ideal_ratio": ideal, "kernel_ratio_over_ideal": med(pk) / med(fk) / ideal,
        "fock_minors_calls_ms_median": round(med(fm_), 3), "fock_pmf_stage_ms_median": round(med(fp), 3),
        "fock_minors_calls_not_kernel_ms": round(med(fm_) - med(fk), 3),
        "parent_minors_calls_ms_median": round(med(pm), 3), "parent_pmf_stage_ms_median": round(med(pp), 3),
        "fock_samples_per_s": args.samples / (med(fw) / 1e3), "parent_samples_per_s": args.samples / (med(pw) / 1e3),
        "same_samples_every_rep": same,
        "collision_free_fraction": float(np.mean((np.diff(out[True], axis=1) > 0).all(axis=1))),
    })
log.close()
