"""The complex fp64 walk on the GPU, order by order (walk_cplx.hip through
sup_perman_complex_range): every walk_cplx<N>, N = 1 ... 64, runs on windows of
eight wave-chunks (fp64_range_truth.py: the first, a scattered one and the
last) of a matrix of entries (p + q i) / 8 and returns the host twin's bits
and, per part, a value within F 2^-53 S of the exact sum over Gaussian
integers, S the exact sum of |Re term| + |Im term| and
F = complex_range_truth.factor (soundness without a GPU: test_fp64_range.py).
The last tests assert that every order ran on a device and print the worst
|err| / (2^-53 S)."""
import pytest

import complex_range_truth as CT
import fp64_range_truth as R
from test_fp64_range import complex_ratio, complex_within

pytestmark = pytest.mark.gpu

# N of every device launch of this module (in-process only)
LEDGER = set()
WORST = {}


@pytest.fixture(scope="module", autouse=True)
def need_gpu(sup):
    if sup.device_count() < 1:
        pytest.fail("no HIP device visible: -m gpu tests must run on the MI355X box")


@pytest.mark.parametrize("n", range(1, 65))
def test_every_order(sup, n):
    a = R.complex_matrix(n) if n > 1 else R.complex_matrix(1) + (0.375 - 1.25j)  # n = 1: one term, a / 2, not zero
    L, m, _ = R.layout(n)
    for c0, c1 in R.windows(n):
        v, st = sup.perman_complex_range(a, c0, c1, walk_log2=R.WALK_LOG2, return_stats=True)
        assert (st["lane_bits"], st["walk_bits"], st["gray_steps"]) == (L, m, (c1 - c0) << (L + m))
        assert st["devices_used"] == 1 and st["kernel_ms"] > 0
        LEDGER.add(n)
        assert v == sup.perman_complex_range(a, c0, c1, cpu=True, threads=16, walk_log2=R.WALK_LOG2), (n, (c0, c1))
        tr, ti, scale = CT.range_sum_abs_float(a, L, m, c0, c1)
        R.note("complex", complex_ratio(v, tr, ti, scale), (n, (c0, c1)), WORST)
        assert complex_within(v, tr, ti, scale, n), (n, (c0, c1), v, float(tr), float(ti))


def test_every_order_was_launched(sup):
    """Runs last: walk_cplx<N> ran on a device for every N."""
    assert set(range(1, 65)) - LEDGER == set()


def test_print_worst_ratios(capsys):
    assert all(0.0 <= ratio <= CT.factor(64, 6, 51) for ratio, _ in WORST.values())
    with capsys.disabled():
        print()
        for kind, (ratio, where) in sorted(WORST.items()):
            print(f"fp64 range, GPU, {kind}: worst |err| / (2^-53 S) = {ratio:.3f} at (n, window) = {where}")
