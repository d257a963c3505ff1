"""The ragged loop torontonian batch and the threshold-detector chain-rule
sampler on one MI355X: DESIGN.md §8p's timing table.  One case per process, so
a job script can give every step its own time limit.

  --case each      one chain-rule step's worth of loop torontonians: --samples
                   (4,096) samples x 2 items, sample s with 4 + s % 9 clicks so
                   far (orders 4..13 in one call) over 16 modes, every sample
                   with its own gamma row.  One loop_torontonian_each call is
                   timed against the only way without it: one
                   loop_torontonian_batch call per item (--parent-samples of the
                   samples, every one by default), kernel and wall time, and the
                   bits are compared.
  --case sampler   samples/s of threshold_sample at --modes modes (16, 24, 40):
                   equal squeezing with a mean photon number of --photons (8) in
                   all and a random unitary; kernel, each-call and host-stage
                   time of the run, the mean click count and the failed count.
                   --table also times threshold_detection_sample, the table's
                   sampler, on the same state (at most 28 modes).
  --cpu            the host twin on 16 threads instead of the device (a check of
                   the script, not a measurement for the table)

The device is used once unmeasured first (code object load, buffer growth).
Kernel times are the calls' own HIP events (sup_stats.kernel_ms).
Appends one JSON line to stdout and to <--out>/probe_threshold_chain.log."""
import argparse
import json
import os
import platform
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", ".."))
import numpy as np  # noqa: E402

import superman_amd as S  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--case", required=True, choices=["each", "sampler"])
ap.add_argument("--samples", type=int, default=4096)
ap.add_argument("--parent-samples", type=int, default=0)
ap.add_argument("--modes", type=int, default=16)
ap.add_argument("--photons", type=float, default=8.0)
ap.add_argument("--table", action="store_true")
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--cpu", action="store_true")
ap.add_argument("--out", default=os.path.join(os.path.dirname(__file__), "..", "..", "profiles", "threshold_chain"))
args = ap.parse_args()

if not args.cpu and S.device_count() < 1:
    sys.exit("probe_threshold_chain: no HIP device (a CPU run measures nothing; --cpu checks the script)")
os.makedirs(args.out, exist_ok=True)
kw = dict(cpu=True, threads=16) if args.cpu else {}
row = {"box": platform.node(), "abi": S._lib.load().sup_abi_version(), "case": args.case, "cpu": args.cpu}


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return r, (time.perf_counter() - t0) * 1e3


def squeezed_state(M, photons, seed):
    """cov (hbar = 2) of M equal squeezers behind a random unitary."""
    r = float(np.arcsinh(np.sqrt(photons / M)))
    rng = np.random.default_rng(seed)
    q, rr = np.linalg.qr(rng.standard_normal((M, M)) + 1j * rng.standard_normal((M, M)))
    U = q * (np.diag(rr) / np.abs(np.diag(rr)))[None, :]
    Sq = np.diag(np.concatenate([np.full(M, np.exp(-r)), np.full(M, np.exp(r))]))
    P = np.block([[U.real, -U.imag], [U.imag, U.real]]) @ Sq
    cov = P @ P.T
    return r, (cov + cov.T) / 2


if args.case == "each":
    M = 16
    _, cov = squeezed_state(M, 8.0, 2800)
    B, _, _ = S.gbs_pure_state(None, cov)
    O = np.zeros((2 * M, 2 * M), complex)
    O[:M, M:], O[M:, :M] = B, B.conj()
    rng = np.random.default_rng(2800)
    z = (rng.standard_normal((args.samples, M)) + 1j * rng.standard_normal((args.samples, M))) / 4
    gammas = np.concatenate([z, z.conj()], axis=1)
    lists, gamma_of = [], []
    for s in range(args.samples):
        c = 4 + s % 9
        k = c + int(rng.integers(0, M - c))  # the mode being drawn; the clicks live on the modes below it
        C = np.sort(rng.permutation(k)[:c])
        lists.append(C), lists.append(np.concatenate([C, [k]]))
        gamma_of += [s, s]
    S.loop_torontonian_each(O, gammas, lists[:2], gamma_of=gamma_of[:2], **kw)  # warm-up
    wall, kern = [], []
    for _ in range(args.reps):
        (v, st), w = timed(lambda: S.loop_torontonian_each(O, gammas, lists, gamma_of=gamma_of, return_stats=True, **kw))
        wall.append(w), kern.append(st["kernel_ms"])
    ps = args.parent_samples or args.samples
    S.loop_torontonian_batch(O, gammas[0], lists[0], **kw)  # warm-up
    pk, same = 0.0, True
    t0 = time.perf_counter()
    for i in range(ps * 2):
        pv, pst = S.loop_torontonian_batch(O, gammas[gamma_of[i]], lists[i], return_stats=True, **kw)
        pk += pst["kernel_ms"]
        same = same and np.array_equal(np.array([pv]).view(np.uint64), v[i:i + 1].view(np.uint64))
    pw = (time.perf_counter() - t0) * 1e3
    scale = args.samples / ps
    row.update({"samples": args.samples, "items": len(lists), "visited_steps": st["visited_steps"],
                "est_ops_per_step": st["est_ops_per_step"], "grid": st["grid"],
                "each_wall_ms": [round(x, 3) for x in wall], "each_kernel_ms": [round(x, 3) for x in kern],
                "each_wall_ms_median": round(float(np.median(wall)), 3),
                "each_kernel_ms_median": round(float(np.median(kern)), 3),
                "parent_calls": ps * 2, "parent_wall_ms": round(pw, 3), "parent_kernel_ms": round(pk, 3),
                "parent_wall_ms_scaled_to_all": round(pw * scale, 3),
                "parent_kernel_ms_scaled_to_all": round(pk * scale, 3),
                "wall_ratio_parent_over_each": pw * scale / float(np.median(wall)),
                "kernel_ratio_parent_over_each": (pk * scale / float(np.median(kern))) if np.median(kern) > 0 else None,
                "same_bits_as_single_calls": bool(same)})
else:
    M = args.modes
    r, cov = squeezed_state(M, args.photons, 2800 + M)
    S.threshold_sample(None, cov, 16, 1, **kw)  # warm-up
    wall, kern, each, host = [], [], [], []
    for _ in range(args.reps):
        (smp, st), w = timed(lambda: S.threshold_sample(None, cov, args.samples, 2800, return_stats=True, **kw))
        wall.append(w), kern.append(st["kernel_ms"]), each.append(st["each_ms"]), host.append(st["host_ms"])
    ok = smp[smp.min(1) >= 0]
    tot = ok.sum(1)
    w = float(np.median(wall))
    row.update({"modes": M, "squeezing_r": r, "samples": args.samples, "wall_ms": [round(x, 3) for x in wall],
                "wall_ms_median": round(w, 3), "samples_per_s": args.samples / (w / 1e3),
                "kernel_ms_median": round(float(np.median(kern)), 3), "each_ms_median": round(float(np.median(each)), 3),
                "host_ms_median": round(float(np.median(host)), 3), "failed": st["failed"],
                "visited_steps": st["visited_steps"], "est_ops_per_step": st["est_ops_per_step"],
                "mean_clicks": float(tot.mean()), "max_clicks": int(tot.max())})
    if args.table:
        tkw = dict(cpu=True, threads=16) if args.cpu else {}
        S.threshold_detection_sample(None, cov, 16, 1, **tkw)  # warm-up
        tw = []
        for _ in range(args.reps):
            ts, t = timed(lambda: S.threshold_detection_sample(None, cov, args.samples, 2800, **tkw))
            tw.append(t)
        row.update({"table_wall_ms": [round(x, 3) for x in tw], "table_wall_ms_median": round(float(np.median(tw)), 3),
                    "table_samples_per_s": args.samples / (float(np.median(tw)) / 1e3),
                    "table_mean_clicks": float(ts.sum(1).mean())})
line = json.dumps(row)
print(line, flush=True)
with open(os.path.join(args.out, "probe_threshold_chain.log"), "a") as log:
    log.write(line + "\n")
