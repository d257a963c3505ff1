"""Compiler resource report of the exact hafnian walk (walk_hafexact.hip) for each
scanned value of kHafxPrimes (primes per launch), by cross-compiling for gfx950
(no GPU needed): hipcc's -Rpass-analysis=kernel-resource-usage figures per
kernel, then the -S output scanned for scratch instructions, readlane /
writelane (SGPRs spilled to VGPR lanes) and fp64 VALU instructions, in the
columns of profiles/hafnian/walk_haf_resources.log.

  python tools/probes/hafexact_resources.py > profiles/hafnian_exact/walk_hafexact_resources.log
  python tools/probes/hafexact_resources.py --primes 8     # the built value only
"""
import argparse
import os
import re
import subprocess
import tempfile

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "superman_amd", "csrc")
ap = argparse.ArgumentParser()
ap.add_argument("--primes", type=int, nargs="*", default=[4, 8, 12, 16])
ap.add_argument("--hipcc", default="/opt/rocm/bin/hipcc")
args = ap.parse_args()
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off"]
NAMES = {"walk_hafexactILb0": "walk_hafexact<false>", "walk_hafexactILb1": "walk_hafexact<true>",
         "hafx_prepare": "hafx_prepare", "hafx_fold": "hafx_fold"}
FIELDS = ["Occupancy [waves/SIMD]", "VGPRs", "AGPRs", "TotalSGPRs", "VGPRs Spill", "SGPRs Spill",
          "ScratchSize [bytes/lane]"]

print("# walk_hafexact.hip, gfx950, hipcc -O3 -ffp-contract=off, per value of kHafxPrimes (-DSUP_HAFX_PRIMES):")
print("# -Rpass-analysis=kernel-resource-usage per kernel, and the -S output scanned for scratch and lane-spill")
print("# instructions.  One walk kernel per form (LOOP), every n.")
print("# primes kernel waves/SIMD VGPRs AGPRs SGPRs spilled_VGPRs spilled_SGPRs scratch_bytes | kernel: f64_insts "
      "scratch_insts readlane/writelane")
for pr in args.primes:
    with tempfile.TemporaryDirectory() as tmp:
        src = os.path.join(CSRC, "walk_hafexact.hip")
        rep = subprocess.run([args.hipcc, *FLAGS, f"-DSUP_HAFX_PRIMES={pr}", "-Rpass-analysis=kernel-resource-usage",
                              "-c", src, "-o", os.path.join(tmp, "w.o")], capture_output=True, text=True, check=True).stderr
        asm = os.path.join(tmp, "w.s")
        subprocess.run([args.hipcc, *FLAGS, f"-DSUP_HAFX_PRIMES={pr}", "--cuda-device-only", "-S", src, "-o", asm],
                       capture_output=True, text=True, check=True)
        text = open(asm).read()
    res = {}
    cur = None
    for line in rep.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = next((v for k, v in NAMES.items() if k in m.group(1)), None)
            res[cur] = {}
        for f in FIELDS:
            m = re.search(re.escape(f) + r": (\d+)", line)
            if m and cur and f not in res[cur]:
                res[cur][f] = m.group(1)
    for key, name in NAMES.items():
        m = re.search(rf"^(_ZN3sup\d*{key}\w*):[^\n]*\n(.*?)s_endpgm", text, re.S | re.M)
        body = m.group(2) if m else ""
        f64 = len(re.findall(r"\bv_(?:fma|mul|add|rndne|fmac)_f64", body))
        scratch = len(re.findall(r"\bscratch_", body))
        lanes = len(re.findall(r"\bv_(?:readlane|writelane)_b32", body))
        print(pr, name, *[res.get(name, {}).get(f, "?") for f in FIELDS], "|", f64, scratch, lanes)
