"""A plain `bench.py --gpus 1 --steps N --warmup W` run: the headline line
only (nothing of what --full adds), ms_per_step over exactly N timed steps,
and --dump-outputs DIR writing what the last timed step returned."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def test_plain_bench_line_and_dumped_outputs(tmp_path):
    e = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        e.pop(k, None)
    out = tmp_path / "out"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--dump-outputs", str(out)], capture_output=True, text=True, timeout=300, env=e)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    rec = lines[0]
    assert rec["unit"] == "gray-steps/s" and rec["higher_is_better"] is True and rec["dtype"] == "f64"
    assert rec["steps"] == 2 and rec["warmup"] == 1 and rec["n_gpus"] == 1
    # value = steps x 2^39 Gray steps / elapsed and ms_per_step = elapsed / steps: the same clock
    assert rec["ms_per_step"] > 0
    assert rec["value"] == pytest.approx(float(1 << 39) / (rec["ms_per_step"] * 1e-3), rel=1e-9)
    assert len(rec["kernel_ms_per_rank"]) == 1 and 0 < rec["kernel_ms_per_rank"][0] <= rec["ms_per_step"]
    for k in ("densities", "configs", "roofline", "cpu_baseline", "cold_start", "rel_err_vs_cpu"):
        assert k not in rec, k
    assert sorted(os.listdir(out)) == ["permanent.npy"]
    got = np.load(out / "permanent.npy")
    assert got.dtype == np.float64 and got.shape == (1,)
    assert float(got[0]) == rec["permanent"]
    # the bound tests/test_gpu_pinned.py holds this walk to
    exact = json.load(open(os.path.join(ROOT, "tests", "golden", "exact_corpus.json")))["double__40_0.50_0"]
    assert abs(rec["permanent"] - exact) <= 1e-10 * abs(exact)
