"""The collision-aware complex walk on the GPU, order by order (walk_cplxf.hip
through sup_perman_complex_fock): every walk_cplx_fock<N>, N = 1 ... 64, runs
one call on submatrices of a 66 x 66 matrix of entries (p + q i) / 8
(fock_truth.py) with
(a) N distinct rows and columns of multiplicities thirds(N): T = 512, Tw = 8
    at N = 22 up to T = 10,648, Tw = 22, H = 484 at N = 64, the last chunk
    ragged from N = 11;
(b) the two sides swapped, so the rows are collapsed wherever they have fewer
    terms (every N but 1, 2 and 4);
(c) for 8 <= N <= 21, where (a) has Tw = 1 and never adds a step's column,
    distinct rows and columns in groups of two and singles (with groups of three
    at N = 19, 20, 21: fock_truth.PAIRS) with 128 <= T <= 2^14 and Tw >= 2.
    No list of order N <= 7 has T >= 128 (at most 2^6 terms), so no lane of
    those orders can walk: H >= 64 is kept first.
The shapes are asserted from a restatement of the layout rule
(test_fock_orders.fock_shapes).  The call returns the host twin's bits, item
(a) alone has the bits it has in the batch, and every item lies per part
within 2^-52 (Tw + N) S of the exact sum over Gaussian integers (soundness
without a GPU: test_fock_orders.py).  The last tests assert that every order
ran on a device and print the worst |err| / (2^-53 S)."""
import numpy as np
import pytest

import fock_truth as F
import fp64_range_truth as R
from test_complex_batch import bits
from test_fock_orders import fock_ratio, fock_shapes, fock_within

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
    U = F.matrix()
    shapes = fock_shapes(n)
    rows, cols = np.stack([s[1] for s in shapes]), np.stack([s[2] for s in shapes])
    v, st = sup.perman_complex_fock(U, rows, cols, return_stats=True)
    LEDGER.add(n)
    assert st["devices_used"] == 1 and st["kernel_ms"] > 0 and st["leaves"] == len(shapes)
    assert st["visited_steps"] == sum(s[3][0] for s in shapes) and st["est_ops_per_step"] == 6 * n
    assert np.array_equal(bits(v), bits(sup.perman_complex_fock(U, rows, cols, cpu=True, threads=16))), n
    assert bits(sup.perman_complex_fock(U, rows[0], cols[0])).tolist() == bits(v[0]).tolist(), n
    for k, (name, r, c, (T, side, Tw, H)) in enumerate(shapes):
        truth = F.truth(U, r, c, side)
        R.note("fock", fock_ratio(v[k], truth), (n, name), WORST)
        assert fock_within(v[k], truth, Tw, n), (n, name, v[k], float(truth[0]), float(truth[1]))


def test_every_order_was_launched(sup):
    """Runs last: walk_cplx_fock<N> ran on a device for every N."""
    assert set(range(1, 65)) - LEDGER == set()


def test_print_worst_ratios(capsys):
    assert all(0.0 <= ratio <= 2 * (1024 + 64) for ratio, _ in WORST.values())
    with capsys.disabled():
        print()
        for kind, (ratio, where) in sorted(WORST.items()):
            print(f"fock orders, GPU, {kind}: worst |err| / (2^-53 S) = {ratio:.3f} at (n, item) = {where}")
