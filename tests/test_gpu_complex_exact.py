"""The exact complex residue walk on the GPU, instance by instance
(walk_cplxexact.hip through sup_perman_complex_exact and its range entry):
every walk_cplxexact<N, G>, N = 1 ... COMPLEX_EXACT_MAX_DEVICE_N, G = 1 and 2,
runs on at most eight wave-chunks and returns the host twin's residues as
integers, and at a spread of orders range_sum's exact integers mod p.  Then
whole matrices against closed forms, several launches of primes, the fold of
the accumulator, device counts, the cap, and the fp64 and double-double device
walks judged against the device's exact result."""
from fractions import Fraction

import numpy as np
import pytest

import complex_exact_cases as X
import range_truth as T
from test_complex import err_over_scale, gauss_int_case, walk_bound
from test_complex_quad import _parts, _whole_tol

pytestmark = pytest.mark.gpu

CAP = 61
TRUTH_N = (set(range(1, 14)) | {17, 24, 31, 32, 33, 40, 48, 56, 64, CAP}) & set(range(1, CAP + 1))


@pytest.fixture(scope="module", autouse=True)
def need_gpu(sup):
    if sup.device_count() < 1:
        pytest.fail("no HIP device visible: -m gpu tests must run on the MI355X box")
    assert sup.COMPLEX_EXACT_MAX_DEVICE_N == CAP


@pytest.mark.parametrize("n", range(1, CAP + 1))
def test_every_order_every_instance(sup, n):
    a = X.as_array(X.instance(n))
    L, m, c0, c1 = X.instance_range(sup, n)
    assert c1 - c0 <= 8
    for G in (1, 2):
        r, st = sup.perman_complex_exact_range(a, c0, c1, group=G, walk_log2=X.WALK_LOG2, return_stats=True)
        assert st["devices_used"] == 1 and st["kernel_ms"] > 0 and st["grid"] >= 1
        assert st["lane_bits"] == L and st["walk_bits"] == m and st["seg_pair_bits"] == G
        assert st["est_ops_per_step"] == X.expected_ops(n, G, len(r["primes"]))
        host = sup.perman_complex_exact_range(a, c0, c1, group=G, cpu=True, threads=8, walk_log2=X.WALK_LOG2)
        assert r == host, (n, G, r, host)
        if n in TRUTH_N:
            assert X.residues_match(r, X.instance_truth(sup, n)), (n, G)


@pytest.mark.parametrize("n", [1, 2])
def test_single_lane_orders_whole(sup, n):
    """N = 1 has one valid lane, N = 2 two: the other lanes add zeros."""
    A = X.random_gauss(n, 40 + n, -9, 9)
    assert sup.perman_complex_exact(X.as_array(A)) == X.ryser(A)
    assert sup.perman_complex_exact([[3 - 2j]]) == (3, -2)


@pytest.mark.parametrize("n", [7, 8, 14, 18, 24, 30])
@pytest.mark.parametrize("form", [X.rank_one, X.j_plus_diag], ids=lambda f: f.__name__)
def test_whole_matrices_closed_forms(sup, form, n):
    A, want = form(n)
    v, st = sup.perman_complex_exact(X.as_array(A), return_stats=True)
    assert v == want
    assert st["devices_used"] == 1 and st["kernel_ms"] > 0 and st["gray_steps"] == 1 << (n - 1)
    assert st["wall_ms"] >= st["kernel_ms"] and st["leaves"] == 1 and st["seg_pair_bits"] in (1, 2)


def test_whole_random_matrix_equals_the_host_twin(sup):
    a = X.as_array(X.random_gauss(18, 41))
    assert sup.perman_complex_exact(a) == sup.perman_complex_exact(a, cpu=True, threads=16)


def test_more_primes_than_one_launch(sup):
    n = 12
    A = X.random_gauss(n, 11, -(1 << 20), 1 << 20)
    a = X.as_array(A)
    r = sup.perman_complex_exact_range(a, 0, 1)
    assert len(r["primes"]) >= 9  # more than two launches of 4, the last one odd or not
    assert r == sup.perman_complex_exact_range(a, 0, 1, cpu=True)
    assert sup.perman_complex_exact(a) == X.ryser(A)
    # every count of primes in the last launch: 1 (padded to a pair), 2, 3 (padded), 4, and 5 = 4 + 1
    for k, count in ((2, 1), (5, 2), (10, 3), (14, 4), (17, 5), (22, 7)):
        b = X.as_array([[((1 << k) - 1, 1 - (1 << k))] * 6 for _ in range(6)])
        rr = sup.perman_complex_exact_range(b, 0, 1, group=1)
        assert len(rr["primes"]) == count
        assert rr == sup.perman_complex_exact_range(b, 0, 1, group=1, cpu=True), k


def test_long_walk_folds_the_accumulator(sup):
    """walk_log2 = 9 at n = 20: 512 steps per lane, acc folded inside the walk."""
    a = X.as_array(X.random_gauss(20, 42))
    chunks = T.chunk_count(sup, 20, 9)
    c0 = T.scattered_start(chunks)
    for G in (1, 2):
        r, st = sup.perman_complex_exact_range(a, c0, c0 + 8, group=G, walk_log2=9, return_stats=True)
        assert st["walk_bits"] == 9
        assert r == sup.perman_complex_exact_range(a, c0, c0 + 8, group=G, cpu=True, threads=16, walk_log2=9)


def test_all_devices_same_integers(sup):
    n = 18
    a = X.as_array(X.random_gauss(n, 43))
    ndev = sup.device_count()
    v, st = sup.perman_complex_exact(a, gpu_num=ndev, return_stats=True)
    assert st["devices_used"] == min(ndev, T.chunk_count(sup, n)) and st["kernel_ms"] > 0
    assert v == sup.perman_complex_exact(a) == sup.perman_complex_exact(a, cpu=True, threads=16)
    assert sup.perman_complex_exact(a, device_id=ndev - 1) == v


def test_above_the_cap_is_unsupported(sup):
    big = X.as_array(X.instance(CAP + 1))
    for call in (lambda: sup.perman_complex_exact(big), lambda: sup.perman_complex_exact_range(big, 0, 1)):
        with pytest.raises(sup.SupError) as e:
            call()
        assert e.value.code == -7 and str(CAP) in str(e.value)


def _scale(a):
    """S = sum over subsets of |prod_j x_j(S)| (test_complex.np_ryser's scale),
    in blocks of 2^16 subsets."""
    n = a.shape[0]
    x0 = a[:, n - 1] - a.sum(axis=1) / 2
    cols = a[:, : n - 1].T  # (n - 1) x n
    total = 0.0
    for base in range(0, 1 << (n - 1), 1 << 16):
        s = np.arange(base, min(base + (1 << 16), 1 << (n - 1)), dtype=np.int64)
        bits = ((s[:, None] >> np.arange(n - 1)) & 1).astype(np.float64)
        total += float(np.abs(np.prod(x0[None, :] + bits @ cols, axis=1)).sum())
    return total


def test_floating_device_walks_against_the_exact_permanent(sup):
    """n = 22, entries in {-1, 0, 1} + {-1, 0, 1} i: the double-double device
    walk within test_complex_quad.py's bound per part, the fp64 device walk
    within test_complex.py's walk_bound with its floor e_np = 2^-52 (the
    stricter end of that bound: no complex128 yardstick is run at this order),
    both measured from the device's exact integers."""
    n = 22
    a = gauss_int_case(n, 53)
    er, ei = sup.perman_complex_exact(a)
    truth = (Fraction(er), Fraction(ei))
    q = _parts(sup.perman_complex_quad(a))
    tol = _whole_tol(sup, a)
    dq = [abs(q[p] - truth[p]) for p in (0, 1)]
    scale = _scale(a)
    m = sup.layout(n)[1]
    e_walk = err_over_scale(sup.perman_complex(a), truth, scale)
    print(f"n={n} exact {er} {ei} dd err {float(dq[0]):.3e} {float(dq[1]):.3e} tol {float(tol):.3e} "
          f"fp64 e_walk {e_walk:.3e} bound {walk_bound(0.0, m, n):.3e}")
    assert dq[0] <= tol and dq[1] <= tol
    assert e_walk <= walk_bound(0.0, m, n)
