"""Compiler resource report and walk-loop census of the complex walk kernels,
by cross-compiling for gfx950 (no GPU needed).

For every N of the chosen kernel it prints one line in the columns of
profiles/complex/walk_cplx_resources.log: hipcc's
-Rpass-analysis=kernel-resource-usage figures, then a scan of the -S output:
the walk loop (the innermost loop with the most fp64 VALU instructions: one odd
+ one even Gray step, 2(6N - 2) of them; the collision-aware walk's loop is one
step, 6N of them: 2N column adds, 4(N - 1) for the product, 4 for acc += w term;
the one-walk minors' loop is 2(16N - 24): per step 2N column adds, 12N - 24 for
the prefix/suffix chain, 2N accumulates; the collision-aware minors' loop is
one step, 16N - 20: those and 4 multiplies by the state's weight; the complex
double-double walk's loop is 2(88N - 28): per step 20N for the column adds
(dd_add_d is 10 instructions: a 6-instruction two_sum, an add, a fast_two_sum;
dd.hpp's nominal count, which est_ops_per_step = 86N - 28 follows, says 9),
68(N - 1) for the product, 40 for the accumulate)
with its scratch instructions, AGPR
moves, v_mov and readlane / writelane, and the scratch instructions of the
whole kernel.

  python tools/probes/cplx_resources.py batch > profiles/complex_batch/walk_cplx_batch_resources.log
  python tools/probes/cplx_resources.py fock > profiles/complex_fock/walk_cplx_fock_resources.log
  python tools/probes/cplx_resources.py minors > profiles/complex_minors/walk_cplx_minors_resources.log
  python tools/probes/cplx_resources.py fock_minors > profiles/complex_fock_minors/walk_cplx_fock_minors_resources.log
  python tools/probes/cplx_resources.py quad > profiles/complex_quad/walk_cplxdd_resources.log
  python tools/probes/cplx_resources.py exact > profiles/complex_exact/walk_cplxexact_resources.log   # both G
  python tools/probes/cplx_resources.py exact --ranges 62_64 > profiles/complex_exact/walk_cplxexact_resources_above_the_cap.log
  python tools/probes/cplx_resources.py single --ranges 1_16 17_32   # walk_cplx<N>, to diff against its log
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "superman_amd", "csrc")
KERNELS = {"batch": ("walk_cplxb.hip", "walk_cplx_batch", ["1_16", "17_32"]),
           "single": ("walk_cplx.hip", "walk_cplx", ["1_16", "17_32", "33_48", "49_64"]),
           "minors": ("walk_cplxm.hip", "walk_cplx_minors", ["1_16", "17_32"]),
           "fock_minors": ("walk_cplxfm.hip", "walk_cplx_fock_minors", ["1_16", "17_32"]),
           "quad": ("walk_cplxdd.hip", "walk_cplxdd", ["1_16", "17_32", "33_40"]),
           "exact": ("walk_cplxexact.hip", "walk_cplxexact", ["1_16", "17_32", "33_48", "49_61"]),
           "fock": ("walk_cplxf.hip", "walk_cplx_fock", ["1_16", "17_32", "33_48", "49_64"])}
# fp64 VALU instructions of the walk loop at order n, and how the logs name that count
LOOP = {"fock": (lambda n: 6 * n, "6N", "one step"),
        "fock_minors": (lambda n: 16 * n - 20, "16N-20", "one walked step"),
        "minors": (lambda n: 2 * (16 * n - 24), "2(16N-24)", "one odd + one even Gray step"),
        "quad": (lambda n: 2 * (88 * n - 28), "2(88N-28)", "one odd + one even Gray step")}
EXACT_PRIMES = 4  # kMaxCxPrimes (cxexact.hpp): the loop holds every prime's chain


def exact_f64(n, g):
    """2 cxe_ops_per_step(n, g, EXACT_PRIMES): cxexact.hpp's formula for one odd + one even Gray step."""
    k = (n + g - 1) // g
    return 2 * (2 * n + (4 * (n // 2) if g == 2 else 0) + EXACT_PRIMES * (10 * k - 2))


loop_f64, loop_name, loop_what = LOOP.get(sys.argv[1] if len(sys.argv) > 1 else "", (
    lambda n: 2 * (6 * n - 2), "2(6N-2)", "one odd + one even Gray step"))
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-Wall", "-Wno-unused-function"]

ap = argparse.ArgumentParser()
ap.add_argument("kernel", choices=sorted(KERNELS))
ap.add_argument("--ranges", nargs="*", default=None)
ap.add_argument("--define", nargs="*", default=[], help="extra -D macros (NAME=VALUE), e.g. a waves-per-SIMD request")
ap.add_argument("--group", type=int, choices=[1, 2], default=None, help="exact: one G only (default: both)")
ap.add_argument("--hipcc", default=os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"))
args = ap.parse_args()
src, kname, ranges = KERNELS[args.kernel]
ranges = args.ranges or ranges


def census(body):
    """Loops of one function's assembly as (first line, last line) of backward branches."""
    labels = {m.group(1): i for i, l in enumerate(body) if (m := re.match(r"^(\.LBB\d+_\d+):", l))}
    loops = []
    for i, l in enumerate(body):
        m = re.match(r"^\s*s_c?branch\w*\s+(\.LBB\d+_\d+)", l)
        if m and labels.get(m.group(1), i) < i:
            loops.append((labels[m.group(1)], i))
    inner = [a for a in loops if not any(b != a and a[0] <= b[0] and b[1] <= a[1] for b in loops)]
    count = lambda lines, rx: sum(1 for l in lines if re.match(rx, l))  # noqa: E731
    f64 = r"^\s*v_\w+_f64"
    scratch = r"^\s*(scratch_|buffer_load|buffer_store)"
    best = max(inner, key=lambda a: count(body[a[0]:a[1] + 1], f64), default=None)
    lines = body[best[0]:best[1] + 1] if best else []
    return (count(lines, f64), count(lines, scratch), count(lines, r"^\s*v_accvgpr"), count(lines, r"^\s*v_mov_b"),
            count(lines, r"^\s*v_(readlane|writelane)"), count(body, scratch))


def census_annotated(body):
    """The same counts with the loops taken from LLVM's own block comments
    ("in Loop: Header=... Depth=d"): a kernel whose loop body branches round
    parts of itself (the exact walk's prime pairs) has blocks laid out of line,
    which the backward-branch scan above takes for loops of their own."""
    count = lambda lines, rx: sum(1 for l in lines if re.match(rx, l))  # noqa: E731
    f64 = r"^\s*v_\w+_f64"
    scratch = r"^\s*(scratch_|buffer_load|buffer_store)"
    loops, depth, cur = {}, {}, None
    for l in body:
        if m := re.match(r"^\.L(BB\d+_\d+):(.*)", l):
            h = re.search(r"in Loop: Header=(BB\d+_\d+) Depth=(\d+)", m.group(2))
            if h:
                cur = h.group(1)
                depth[cur] = int(h.group(2))
            elif "Loop Header" in m.group(2) or "Parent Loop" in m.group(2):
                cur = m.group(1)
            else:
                cur = None
            continue
        if cur is not None:
            if d := re.search(r"Loop Header: Depth=(\d+)", l):
                depth[cur] = int(d.group(1))
            loops.setdefault(cur, []).append(l)
    # the walk loop: the deepest loop, and of those the one with the most fp64 instructions
    best = max(loops, key=lambda k: (depth.get(k, 0), count(loops[k], f64)), default=None)
    lines = loops[best] if best else []
    return (count(lines, f64), count(lines, scratch), count(lines, r"^\s*v_accvgpr"), count(lines, r"^\s*v_mov_b"),
            count(lines, r"^\s*v_(readlane|writelane)"), count(body, scratch))


rows = {}
for r in ranges:
    lo, hi = r.split("_")
    with tempfile.TemporaryDirectory() as tmp:
        asm = os.path.join(tmp, "k.s")
        p = subprocess.run([args.hipcc, *FLAGS, *[f"-D{d}" for d in args.define], f"-DSUP_N_LO={lo}", f"-DSUP_N_HI={hi}", "--cuda-device-only", "-S",
                            "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(CSRC, src), "-o", asm],
                           capture_output=True, text=True, cwd=CSRC)
        if p.returncode:
            sys.exit(p.stderr[-4000:])
        text = open(asm).read().splitlines()
    res, cur = {}, None
    for l in p.stderr.splitlines():
        if m := re.search(r"remark: Function Name: (\S+)", l):
            k = re.search(rf"{kname}ILi(\d+)E(?:Li(\d+)E)?", m.group(1))
            cur = (int(k.group(1)), int(k.group(2)) if k.group(2) else 0) if k else None
            if cur is not None:
                res[cur] = {}
        elif cur is not None and (m := re.search(r"remark:\s+([A-Za-z \[\]/]+?): (\S+)", l)):
            res[cur][m.group(1).strip()] = m.group(2)
    for (n, g), d in res.items():
        if args.group and g != args.group:
            continue
        targs = f"ILi{n}E" + (f"Li{g}E" if g else "")
        start = next(i for i, l in enumerate(text) if re.match(rf"^_ZN3sup\d+{kname}{targs}\w*:", l))
        end = next(i for i in range(start, len(text)) if text[i].startswith(".Lfunc_end"))
        c = (census_annotated if args.kernel == "exact" else census)(text[start:end])
        rows[(n, g)] = (f"{n} {d['Occupancy [waves/SIMD]']} {d['VGPRs']} {d['AGPRs']} {d['TotalSGPRs']} {d['VGPRs Spill']} "
                        f"{d['SGPRs Spill']} {d['ScratchSize [bytes/lane]']} | {c[0]} {c[1]} {c[2]} {c[3]} {c[4]} | {c[5]}")

if args.kernel == "exact":
    print(f"# {kname}<N, G>, gfx950, hipcc -O3 -ffp-contract=off: -Rpass-analysis=kernel-resource-usage per (N, G), and the")
    print(f"# walk loop (the innermost loop with the most fp64 VALU instructions: one odd + one even Gray step, every one of")
    print(f"# the launch's {EXACT_PRIMES} primes) scanned in the -S output.  formula = 2 cxe_ops_per_step(N, G, {EXACT_PRIMES}) (cxexact.hpp).")
    print("# G N waves/SIMD VGPRs AGPRs SGPRs spilled_VGPRs spilled_SGPRs scratch_bytes | loop: f64_insts scratch_insts "
          "accvgpr_moves v_mov readlane/writelane | kernel_scratch_insts | formula")
    bad = []
    for (n, g) in sorted(rows, key=lambda k: (k[1], k[0])):
        r = rows[(n, g)]
        print(f"{g} {r} | {exact_f64(n, g)}")
        f = r.split()
        if f[5] != "0" or f[7] != "0" or f[-1] != "0" or not re.search(rf"\| {exact_f64(n, g)} 0 ", r):
            bad.append((n, g))
    clean = 0
    while all((clean + 1, g) in rows and (clean + 1, g) not in bad for g in {k[1] for k in rows}):
        clean += 1
    print(f"# condition (0 spilled VGPRs, 0 scratch bytes, no scratch instruction in the kernel, loop = formula): "
          f"{'holds at every (N, G)' if not bad else 'FAILS at (N, G) = ' + ', '.join(map(str, bad))}")
    print(f"# largest N with every N' <= N clean for every G listed: {clean}")
    sys.exit(0)
rows = {n: r for (n, g), r in rows.items()}

print(f"# {kname}<N>, gfx950, hipcc -O3 -ffp-contract=off: -Rpass-analysis=kernel-resource-usage per N, and the walk loop")
print(f"# (the innermost loop holding {loop_name} fp64 VALU instructions: {loop_what}) scanned in the -S output.")
print("# N waves/SIMD VGPRs AGPRs SGPRs spilled_VGPRs spilled_SGPRs scratch_bytes | loop: f64_insts scratch_insts "
      "accvgpr_moves v_mov readlane/writelane | kernel_scratch_insts")
for n in sorted(rows):
    print(rows[n])
bad = [n for n in sorted(rows) if not re.search(rf"\| {loop_f64(n)} 0 ", rows[n]) or rows[n].split()[5] != "0"
       or rows[n].split()[7] != "0"]
if args.kernel == "fock":
    # the collision-aware walk's condition is on the walk loop; spills outside it (the chunk start) are listed
    bad = [n for n in sorted(rows) if not re.search(rf"\| {loop_f64(n)} 0 ", rows[n])]
    out = [n for n in sorted(rows) if rows[n].split()[5] != "0"]
    print(f"# condition (walk loop = {loop_name} fp64 instructions, no scratch instruction in it): "
          f"{'holds at every N' if not bad else 'FAILS at N = ' + ', '.join(map(str, bad))}")
    print(f"# VGPRs spilled outside the walk loop (chunk start; to scratch where scratch_bytes > 0, else to AGPRs): "
          f"{'none' if not out else 'N = ' + ', '.join(map(str, out))}")
elif args.kernel == "fock_minors":
    # no scratch anywhere in the kernel; VGPRs the allocator moved to AGPRs are listed, not hidden
    bad = [n for n in sorted(rows) if not re.search(rf"\| {loop_f64(n)} 0 ", rows[n]) or rows[n].split()[7] != "0"
           or rows[n].split()[-1] != "0"]
    out = [n for n in sorted(rows) if rows[n].split()[5] != "0"]
    moves = [n for n in sorted(rows) if rows[n].split("|")[1].split()[2] != "0"]
    print(f"# condition (0 scratch bytes, no scratch instruction in the kernel, walk loop = {loop_name} fp64 "
          f"instructions): {'holds at every N' if not bad else 'FAILS at N = ' + ', '.join(map(str, bad))}")
    print(f"# VGPRs spilled to AGPRs (scratch_bytes = 0): {'none' if not out else 'N = ' + ', '.join(map(str, out))}")
    print(f"# AGPR moves in the walk loop: {'none' if not moves else 'N = ' + ', '.join(map(str, moves))}")
else:
    print(f"# condition (0 spilled VGPRs, 0 scratch bytes, loop = {loop_name} fp64 instructions, no scratch in it): "
          f"{'holds at every N' if not bad else 'FAILS at N = ' + ', '.join(map(str, bad))}")
