"""The truth, the scale and the inputs of the per-order device tests of the
collision-aware and the batched complex walks, shown sound without a GPU
(fock_truth.py), and the collision-aware host twin (cplx_fock.cpp through
perman_complex_fock(cpu=True)) at every order N = 1 ... 64 on the inputs of
test_gpu_complex_fock_orders.py: per part within 2^-52 (Tw + n) S of the exact
sum, test_complex_fock.fock_bound without the yardstick's own error.  The last
test prints the worst |err| / (2^-53 S)."""
import math
from fractions import Fraction

import numpy as np
import pytest

import complex_range_truth as CT
import fock_truth as F
import fp64_range_truth as R
from test_complex import exact_perm
from test_complex_fock import fock_bound, plan

# kind -> (worst ratio, (n, item)); filled by the tests below
WORST = {}


def fock_shapes(n):
    """[(name, rows, cols, (T, side, Tw, H))] of fock_truth.fock_items(n), the
    shapes checked against what the items are there for."""
    out = []
    for name, rows, cols in F.fock_items(n):
        assert len(set(rows.tolist() if name != "b" else cols.tolist())) == n
        T, side, Tw, H = p = plan(rows, cols)
        if name == "a":
            assert (T, side) == (math.prod(t + 1 for t in F.thirds(n)[:-1]), 0)  # one of the singles is held
            assert Tw == 1 or n >= 22
        elif name == "b":
            a = out[0][3]
            # the rule: the rows only where they have fewer terms than the 2^(n-1) of the distinct columns
            assert (T, side) == ((a[0], 1) if a[0] < 1 << (n - 1) else (1 << (n - 1), 0))
            assert side == 1 or n in (1, 2, 4)
            assert (Tw, H) == a[2:] or side == 0
        else:
            assert side == 0 and 128 <= T <= 1 << 14 and Tw >= 2 and set(F.PAIRS[n]) <= {1, 2, 3}
        assert T == Tw * H
        out.append((name, rows, cols, p))
    assert [s[0] for s in out] == (["a", "b", "c"] if 8 <= n <= 21 else ["a", "b"])
    return out


def fock_within(got, truth, Tw, n):
    """Per part within fock_bound(0, Tw, n) S = 2^-52 (Tw + n) S."""
    tol = Fraction(fock_bound(0.0, Tw, n)) * truth[2]
    return abs(Fraction(got.real) - truth[0]) <= tol and abs(Fraction(got.imag) - truth[1]) <= tol


def fock_ratio(got, truth):
    return max(R.ratio(got.real, truth[0], truth[2]), R.ratio(got.imag, truth[1], truth[2]))


def test_thirds():
    assert [F.thirds(n) for n in (1, 2, 3, 4, 5, 6)] == [(1,), (1, 1), (2, 1), (1, 1, 1, 1), (2, 1, 1, 1), (2, 2, 1, 1)]
    assert F.thirds(22) == (7, 7, 7, 1) and F.thirds(63) == (21, 21, 20, 1) and F.thirds(64) == (21, 21, 21, 1)
    for n in range(4, 65):
        t = F.thirds(n)
        assert sum(t) == n and t[3] == 1 and t[0] >= t[1] >= t[2] >= t[0] - 1


def test_shapes_of_every_order():
    """What the inputs are chosen for: (a) does not walk below n = 22 (Tw = 1),
    its last chunk is ragged from n = 11; T = 512, Tw = 8 at n = 22 and
    T = 10,648, Tw = 22, H = 484 at n = 64; (b) collapses the rows; (c) walks."""
    shapes = {n: fock_shapes(n) for n in range(1, 65)}
    assert shapes[22][0][3] == (512, 0, 8, 64) and shapes[64][0][3] == (10648, 0, 22, 484)
    assert shapes[64][1][3] == (10648, 1, 22, 484)
    assert shapes[10][0][3][3] == 64 and shapes[11][0][3][3] == 80
    assert all(shapes[n][0][3][3] > 64 for n in range(11, 22))
    assert all(shapes[n][0][3][2] >= 2 for n in range(22, 65))
    assert {n for n in range(1, 65) if len(shapes[n]) == 3} == set(F.PAIR_ORDERS) == set(F.PAIRS)
    assert all(sum(F.PAIRS[n]) == n for n in F.PAIRS)
    # no list of order <= 7 has 128 terms: without repeats T = 2^(n-1) <= 64
    assert all(plan(range(n), range(n))[0] < 128 for n in range(1, 8))


# (n, rows multiplicities, cols multiplicities): both sides, ties, one group, the held group not the last
EXACT = [(1, (1,), (1,)), (2, (1, 1), (2,)), (3, (1, 1, 1), (2, 1)), (5, (1,) * 5, (2, 1, 1, 1)),
         (5, (2, 2, 1), (3, 2)), (6, (1,) * 6, (1, 3, 2)), (7, (1,) * 7, (3, 2, 2)), (7, (2, 2, 2, 1), (1,) * 7),
         (8, (1,) * 8, (3, 2, 2, 1)), (8, (4, 4), (2, 2, 2, 2)), (8, (1,) * 8, (1,) * 8)]


@pytest.mark.parametrize("n,rm,cm", EXACT)
def test_collapsed_sum_is_the_exact_permanent(n, rm, cm):
    """Against Ryser over Python integers on the expanded matrix, either side
    collapsed (the other may repeat too: the sum does not need it distinct)."""
    rng = np.random.default_rng(90 + n)
    U = F.matrix()
    rows, cols = F.repeated(rng, rm), F.repeated(rng, cm)
    rng.shuffle(rows)
    rng.shuffle(cols)
    want = exact_perm(U[np.ix_(rows, cols)])
    assert F.collapsed_sum(U, rows, cols)[:2] == want
    assert F.collapsed_sum(U.T, cols, rows)[:2] == want
    assert F.truth(U, rows, cols, 0)[:2] == want and F.truth(U, rows, cols, 1)[:2] == want


@pytest.mark.parametrize("n", range(1, 11))
def test_scale_is_the_ryser_scale_of_the_expanded_matrix(n):
    """The lists of the batched test, the single column last: S is the sum of
    |Re term| + |Im term| over all 2^(n-1) column subsets of the gathered
    matrix, and the permanent (4 (n & 1) - 2) times the signed sum."""
    U = F.matrix()
    rows, cols = F.batch_lists(n)
    L, m, chunks = R.layout(n)
    for k in range(len(rows)):
        assert cols[k, -1] not in cols[k, :-1]
        assert sorted(F.thirds(n)) == sorted(np.unique(cols[k], return_counts=True)[1])
        tr, ti, scale = CT.range_sum_abs_float(U[np.ix_(rows[k], cols[k])], L, m, 0, chunks)
        re, im, S = F.collapsed_sum(U, rows[k], cols[k])
        assert S == scale > 0
        assert (re, im) == ((4 * (n & 1) - 2) * tr, (4 * (n & 1) - 2) * ti)


@pytest.mark.parametrize("n", range(1, 65))
def test_host_twin_within_tolerance_of_truth(sup, n):
    U = F.matrix()
    shapes = fock_shapes(n)
    rows, cols = np.stack([s[1] for s in shapes]), np.stack([s[2] for s in shapes])
    got, st = sup.perman_complex_fock(U, rows, cols, cpu=True, return_stats=True)
    assert st["visited_steps"] == sum(s[3][0] for s in shapes) and st["est_ops_per_step"] == 6 * n
    assert sup.perman_complex_fock_plan(rows, cols)[1].tolist() == [s[3][1] for s in shapes]
    for k, (name, r, c, (T, side, Tw, H)) in enumerate(shapes):
        truth = F.truth(U, r, c, side)
        R.note("fock twin", fock_ratio(got[k], truth), (n, name), WORST)
        assert fock_within(got[k], truth, Tw, n), (n, name, got[k], float(truth[0]), float(truth[1]))


def test_print_worst_ratios(capsys):
    """Runs last: the worst |err| / (2^-53 S) over the orders above (the
    tolerance is 2 (Tw + n) of these units, at least 4)."""
    assert all(0.0 <= ratio <= 2 * (1024 + 64) for ratio, _ in WORST.values())
    with capsys.disabled():
        print()
        for kind, (ratio, where) in sorted(WORST.items()):
            print(f"fock orders, CPU, {kind}: worst |err| / (2^-53 S) = {ratio:.3f} at (n, item) = {where}")
