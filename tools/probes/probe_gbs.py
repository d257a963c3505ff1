"""The ragged loop-hafnian batch and the PNR sampler on one MI355X: DESIGN.md
§8n's timing table.  One case per process, so a job script can give every step
its own time limit.

  --case each      one chain-rule step's worth of loop hafnians: --samples
                   (4,096) samples x 9 candidates, sample s with a prefix of
                   4 + s % 9 photons (orders 4..20 in one call) over 16 modes,
                   every sample with its own displacement row.  One
                   loop_hafnian_each call is timed against the only way without
                   it: one hafnian_batch(loop=True) call per sample and per
                   order (--parent-samples of the samples, every one by default),
                   kernel and wall time, and the bits are compared.
  --case sampler   samples/s of gbs_sample at --modes modes (16, 24): equal
                   squeezing with a mean photon number of --photons (8) in all,
                   a random unitary, cutoff --cutoff (6); kernel, each-call and
                   host-stage time of the run.
  --cpu            the host twin on 16 threads instead of the device (a check of
                   the script, not a measurement for the table)

The device is used once unmeasured first (code object load, buffer growth).
Kernel times are the calls' own HIP events (sup_stats.kernel_ms).
Appends one JSON line to stdout and to <--out>/probe_gbs.log."""
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
ap.add_argument("--cutoff", type=int, default=6)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--cpu", action="store_true")
ap.add_argument("--out", default=os.path.join(os.path.dirname(__file__), "..", "..", "profiles", "gbs"))
args = ap.parse_args()

if not args.cpu and S.device_count() < 1:
    sys.exit("probe_gbs: no HIP device (a CPU run measures nothing; --cpu checks the script)")
os.makedirs(args.out, exist_ok=True)
kw = dict(cpu=True, threads=16) if args.cpu else {}
row = {"box": platform.node(), "abi": S._lib.load().sup_abi_version(), "case": args.case, "cpu": args.cpu}


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return r, (time.perf_counter() - t0) * 1e3


if args.case == "each":
    M, C = 16, 9
    rng = np.random.default_rng(2600)
    B = rng.standard_normal((M, M)) + 1j * rng.standard_normal((M, M))
    B = (B + B.T) / 8
    mus = (rng.standard_normal((args.samples, M)) + 1j * rng.standard_normal((args.samples, M))) / 2
    lists, mu_of = [], []
    for s in range(args.samples):
        k = 8 + s % 8  # the mode being drawn; the prefix lives on the modes below it
        prefix = np.sort(rng.integers(0, k, 4 + s % 9))
        for c in range(C):
            lists.append(np.concatenate([prefix, np.full(c, k)]))
            mu_of.append(s)
    S.loop_hafnian_each(B, mus, lists[:C], mu_of=mu_of[:C], **kw)  # warm-up
    wall, kern = [], []
    for _ in range(args.reps):
        (v, st), w = timed(lambda: S.loop_hafnian_each(B, mus, lists, mu_of=mu_of, return_stats=True, **kw))
        wall.append(w), kern.append(st["kernel_ms"])
    ps = args.parent_samples or args.samples
    S.hafnian_batch(B, lists[0], mu=mus[0], loop=True, **kw)  # warm-up
    pk, same = 0.0, True
    t0 = time.perf_counter()
    for i in range(ps * C):
        if len(lists[i]) == 0:
            continue
        pv, pst = S.hafnian_batch(B, lists[i], mu=mus[mu_of[i]], loop=True, return_stats=True, **kw)
        pk += pst["kernel_ms"]
        same = same and np.array_equal(np.array([pv]).view(np.uint64), v[i:i + 1].view(np.uint64))
    pw = (time.perf_counter() - t0) * 1e3
    scale = args.samples / ps
    row.update({"samples": args.samples, "candidates": C, "items": len(lists), "visited_steps": st["visited_steps"],
                "est_ops_per_step": st["est_ops_per_step"], "grid": st["grid"],
                "each_wall_ms": [round(x, 3) for x in wall], "each_kernel_ms": [round(x, 3) for x in kern],
                "each_wall_ms_median": round(float(np.median(wall)), 3),
                "each_kernel_ms_median": round(float(np.median(kern)), 3),
                "parent_calls": ps * C, "parent_wall_ms": round(pw, 3), "parent_kernel_ms": round(pk, 3),
                "parent_wall_ms_scaled_to_all": round(pw * scale, 3),
                "parent_kernel_ms_scaled_to_all": round(pk * scale, 3),
                "wall_ratio_parent_over_each": pw * scale / float(np.median(wall)),
                "kernel_ratio_parent_over_each": (pk * scale / float(np.median(kern))) if np.median(kern) > 0 else None,
                "same_bits_as_single_calls": bool(same)})
else:
    M = args.modes
    r = float(np.arcsinh(np.sqrt(args.photons / M)))
    rng = np.random.default_rng(2600 + M)
    q, rr = np.linalg.qr(rng.standard_normal((M, M)) + 1j * rng.standard_normal((M, M)))
    U = q * (np.diag(rr) / np.abs(np.diag(rr)))[None, :]
    Sq = np.diag(np.concatenate([np.full(M, np.exp(-r)), np.full(M, np.exp(r))]))
    P = np.block([[U.real, -U.imag], [U.imag, U.real]]) @ Sq
    cov = P @ P.T  # hbar = 2: the vacuum is the identity
    cov = (cov + cov.T) / 2
    S.gbs_sample(None, cov, 16, 1, cutoff=args.cutoff, **kw)  # warm-up
    (smp, st), w = timed(lambda: S.gbs_sample(None, cov, args.samples, 2600, cutoff=args.cutoff, return_stats=True,
                                              **kw))
    tot = smp.sum(1)
    row.update({"modes": M, "squeezing_r": r, "cutoff": args.cutoff, "samples": args.samples,
                "wall_ms": round(w, 3), "samples_per_s": args.samples / (w / 1e3), "kernel_ms": st["kernel_ms"],
                "each_ms": st["each_ms"], "host_ms": st["host_ms"], "failed": st["failed"],
                "visited_steps": st["visited_steps"], "est_ops_per_step": st["est_ops_per_step"],
                "mean_photons": float(tot.mean()), "max_photons": int(tot.max()),
                "at_cutoff_fraction": float((smp == args.cutoff).mean())})
line = json.dumps(row)
print(line, flush=True)
with open(os.path.join(args.out, "probe_gbs.log"), "a") as log:
    log.write(line + "\n")
