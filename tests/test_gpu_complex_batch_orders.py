"""The batched complex walk on the GPU, order by order (walk_cplxb.hip through
sup_perman_complex_submatrices): every walk_cplx_batch<N>, N = 1 ... 32, runs
three gathers (two from N = 25) of a 66 x 66 matrix of entries (p + q i) / 8
(fock_truth.py): distinct rows, columns of multiplicities thirds(N), the first
N - 1 shuffled and the single last.  The kernel walks all 2^(N-1) subsets of
each gathered matrix, while the exact sum and its scale S cost the T <= 1452
terms of the collapsed sum (fock_truth.collapsed_sum; S is the Ryser scale of
the gathered matrix: test_fock_orders.py).  Result k has the bits of
perman_complex on gathered matrix k on the device (the documented contract),
of perman_complex_batch of the gathered stack and, up to N = 24, of the host
twin (above that the twin takes tens of seconds), and lies per part within
F 2^-53 S of the exact sum, F = complex_range_truth.factor(N, m, h) of the
engine's layout: test_gpu_complex_orders.py's tolerance.  The last tests assert
that every order ran on a device and print the worst |err| / (2^-53 S) and the
kernel time of the largest launch."""
from fractions import Fraction

import numpy as np
import pytest

import complex_range_truth as CT
import fock_truth as F
import fp64_range_truth as R
from test_complex_batch import bits
from test_fock_orders import fock_ratio

pytestmark = pytest.mark.gpu

# N of every device launch of this module (in-process only)
LEDGER = set()
WORST = {}
KERNEL_MS = {}


@pytest.fixture(scope="module", autouse=True)
def need_gpu(sup):
    if sup.device_count() < 1:
        pytest.fail("no HIP device visible: -m gpu tests must run on the MI355X box")


@pytest.mark.parametrize("n", range(1, 33))
def test_every_order(sup, n):
    U = F.matrix()
    rows, cols = F.batch_lists(n)
    count = len(rows)
    assert count == (3 if n <= 24 else 2)
    v, st = sup.perman_complex_submatrices(U, rows, cols, return_stats=True)
    LEDGER.add(n)
    KERNEL_MS[n] = st["kernel_ms"]
    L, m, h = sup.layout(n)
    assert st["devices_used"] == 1 and st["kernel_ms"] > 0 and (st["lane_bits"], st["walk_bits"]) == (L, m)
    assert st["leaves"] == count and st["gray_steps"] == count << (n - 1) and st["est_ops_per_step"] == 6 * n
    gathered = np.stack([U[np.ix_(rows[k], cols[k])] for k in range(count)])
    one = np.array([sup.perman_complex(a) for a in gathered], dtype=np.complex128)
    assert np.array_equal(bits(v), bits(one)), n
    assert np.array_equal(bits(v), bits(sup.perman_complex_batch(gathered))), n
    if n <= 24:
        assert np.array_equal(bits(v), bits(sup.perman_complex_submatrices(U, rows, cols, cpu=True, threads=16))), n
    for k in range(count):
        truth = F.truth(U, rows[k], cols[k])
        tol = CT.factor(n, m, h) * R.EPS * truth[2]
        R.note("batch", fock_ratio(v[k], truth), (n, k), WORST)
        assert abs(Fraction(v[k].real) - truth[0]) <= tol and abs(Fraction(v[k].imag) - truth[1]) <= tol, \
            (n, k, v[k], float(truth[0]), float(truth[1]))


def test_every_order_was_launched(sup):
    """Runs last: walk_cplx_batch<N> ran on a device for every N."""
    assert set(range(1, 33)) - LEDGER == set()


def test_print_worst_ratios(capsys):
    assert all(0.0 <= ratio <= CT.factor(32, 10, 15) for ratio, _ in WORST.values())
    with capsys.disabled():
        print()
        for kind, (ratio, where) in sorted(WORST.items()):
            print(f"batch orders, GPU, {kind}: worst |err| / (2^-53 S) = {ratio:.3f} at (n, gather) = {where}")
        for n in sorted(KERNEL_MS)[-3:]:
            print(f"batch orders, GPU: walk_cplx_batch<{n}>, {2 if n > 24 else 3} x 2^{n - 1} Gray steps: "
                  f"kernel_ms = {KERNEL_MS[n]:.1f}")
