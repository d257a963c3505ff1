"""Exact truth and inputs for the per-order tests of the collision-aware and
the batched complex walks (walk_cplx_fock<N>, N = 1 ... 64, and
walk_cplx_batch<N>, N = 1 ... 32): shared by test_fock_orders.py,
test_gpu_complex_fock_orders.py and test_gpu_complex_batch_orders.py.  Nothing
here calls the engine or the oracle.

The sum is DESIGN.md 8c's, over the multiplicity vectors of the repeated
columns of A[j][c] = U[rows[j]][cols[c]]: distinct columns b_k with
multiplicities t_k in order of first appearance, one copy of the rarest group
(the first on a tie) held, t'_k = t_k - 1 there and t_k elsewhere,

    per(A) = 2 sum_{0 <= v_k <= t'_k} (-1)^(sum v) prod_k C(t'_k, v_k) prod_j x_j(v),
    x_j(v) = 1/2 sum_k t_k b_k[j] - sum_k v_k b_k[j],

T = prod (t'_k + 1) terms where the expanded matrix has 2^(n-1).  S is the sum
under the 2 with every term replaced by prod_k C(t'_k, v_k) (|Re prod_j x_j| +
|Im prod_j x_j|): the scale of test_complex_fock.py's bound (the factor 2 of the
result is that bound's 2^-52) and, with no column repeated, the scale of
complex_range_truth.range_sum_abs over the whole plan.
"""
from fractions import Fraction
from math import comb

import numpy as np

SIDE = 66
PAIR_ORDERS = range(8, 22)


def thirds(n):
    """The multiplicities of the per-order inputs: n - 1 in three near-equal
    groups, the largest first, and a single; (n - 1, 1) up to n = 3."""
    if n == 1:
        return (1,)
    if n <= 3:
        return (n - 1, 1)
    q, r = divmod(n - 1, 3)
    return tuple(q + (i < r) for i in range(3)) + (1,)


def collapsed_sum(U, rows, cols):
    """(re, im, S) of the permanent of U[np.ix_(rows, cols)] as Fractions, by
    the sum above in Python integers: every part of every entry of the
    complex128 matrix U is k 2^-s exactly, so the sum runs on the Gaussian
    integers 2 U 2^s (1/2 sum_k t_k b_k is then an integer vector) and is
    scaled back by 2^-(n (s + 1)).  S is accumulated as an integer: a float
    overflows from about n = 60.  The columns are the collapsed side; for the
    rows call it on (U.T, cols, rows).  The multiplicity vectors are counted
    lowest digit first, a step of digit k subtracting b_k and a wrap adding
    t'_k b_k back."""
    rows, cols = [int(r) for r in rows], [int(c) for c in cols]
    n = len(rows)
    assert len(cols) == n >= 1
    seen = {}
    for c in cols:
        seen[c] = seen.get(c, 0) + 1
    vals, t = list(seen), list(seen.values())
    K = len(vals)
    held = min(range(K), key=lambda k: (t[k], k))
    tp = [t[k] - (k == held) for k in range(K)]
    fr = [[(Fraction(float(complex(U[r][c]).real)), Fraction(float(complex(U[r][c]).imag))) for r in rows]
          for c in vals]
    s = max(p.denominator for col in fr for z in col for p in z).bit_length() - 1
    b = [[(int(2 * z[0] * (1 << s)), int(2 * z[1] * (1 << s))) for z in col] for col in fr]
    assert all(Fraction(b[k][j][p], 2 << s) == fr[k][j][p] for k in range(K) for j in range(n) for p in (0, 1))
    xr = [sum(t[k] * b[k][j][0] for k in range(K)) // 2 for j in range(n)]
    xi = [sum(t[k] * b[k][j][1] for k in range(K)) // 2 for j in range(n)]
    binom = [[comb(tp[k], v) for v in range(tp[k] + 1)] for k in range(K)]
    v = [0] * K
    tr = ti = scale = 0
    while True:
        pr, pi = 1, 0
        for r, i in zip(xr, xi):
            pr, pi = pr * r - pi * i, pr * i + pi * r
        w = 1
        for k in range(K):
            w *= binom[k][v[k]]
        if sum(v) & 1:
            tr, ti = tr - w * pr, ti - w * pi
        else:
            tr, ti = tr + w * pr, ti + w * pi
        scale += w * (abs(pr) + abs(pi))
        k = 0
        while k < K and v[k] == tp[k]:
            if tp[k]:
                for j in range(n):
                    xr[j] += tp[k] * b[k][j][0]
                    xi[j] += tp[k] * b[k][j][1]
                v[k] = 0
            k += 1
        if k == K:
            break
        v[k] += 1
        for j in range(n):
            xr[j] -= b[k][j][0]
            xi[j] -= b[k][j][1]
    den = 1 << (n * (s + 1))
    return Fraction(2 * tr, den), Fraction(2 * ti, den), Fraction(scale, den)


# ---- the inputs of the per-order tests ------------------------------------------

def matrix():
    """U: 66 x 66, dense, entries (p + q i) / 8 with p, q in -16 ... 16."""
    rng = np.random.default_rng(6600)
    return (rng.integers(-16, 17, (SIDE, SIDE)) + 1j * rng.integers(-16, 17, (SIDE, SIDE))) / 8.0


# Item (c): n -> multiplicities in the order of first appearance, the groups of
# two first: the most twos with 128 <= T <= 2^14 and at least two steps per
# lane (Tw >= 2), the rest singles.  That is no two at n = 8 (only eight
# singles reach T = 128), one at n = 9 (two leave H = 48 < 64 beside the first
# walk digit) and n // 2 from n = 10 to 18.  At n = 19, 20, 21 no list of twos
# and singles stays within 2^14 terms (the fewest are 3^9 = 19683, 2 3^9 and
# 3^10), so there groups of three take the place of twos, as few as bring T
# under 2^14: two, three and six of them.
PAIRS = {8: (1,) * 8, 9: (2,) + (1,) * 7}
PAIRS.update({n: (2,) * (n // 2) + (1,) * (n % 2) for n in range(10, 19)})
PAIRS.update({19: (2,) * 6 + (3,) * 2 + (1,), 20: (2,) * 5 + (3,) * 3 + (1,), 21: (2,) + (3,) * 6 + (1,)})


def distinct(rng, count):
    return rng.choice(SIDE, size=count, replace=False)


def repeated(rng, mult):
    """An index list whose distinct values have multiplicities `mult`, the
    groups contiguous and in the order given."""
    return np.repeat(distinct(rng, len(mult)), mult)


def fock_items(n):
    """[(name, rows, cols)] of order n for perman_complex_fock: (a) rows
    distinct, cols with multiplicities thirds(n); (b) the two sides swapped;
    (c), 8 <= n <= 21, rows distinct and cols in groups of two and singles."""
    rng = np.random.default_rng(6600 + n)
    items = [("a", distinct(rng, n), repeated(rng, thirds(n))),
             ("b", repeated(rng, thirds(n)), distinct(rng, n))]
    if n in PAIRS:
        items.append(("c", distinct(rng, n), repeated(rng, PAIRS[n])))
    return items


def batch_lists(n):
    """(rows, cols), each [count, n], for perman_complex_submatrices: count = 3
    up to n = 24 and 2 above; rows distinct, cols with multiplicities
    thirds(n), the first n - 1 entries shuffled and the single last."""
    rng = np.random.default_rng(3200 + n)
    count = 3 if n <= 24 else 2
    rows = np.stack([distinct(rng, n) for _ in range(count)])
    cols = np.stack([repeated(rng, thirds(n)) for _ in range(count)])
    for k in range(count):
        rng.shuffle(cols[k, :n - 1])
    return rows, cols


_TRUTH = {}


def truth(U, rows, cols, side=0):
    """collapsed_sum of the matrix U[np.ix_(rows, cols)] with the columns
    (side 0) or the rows (side 1) collapsed, computed once per run."""
    key = (tuple(int(r) for r in rows), tuple(int(c) for c in cols), side)
    if key not in _TRUTH:
        _TRUTH[key] = collapsed_sum(U.T, cols, rows) if side else collapsed_sum(U, rows, cols)
    return _TRUTH[key]
