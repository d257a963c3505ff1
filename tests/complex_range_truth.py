"""Exact truth for the range entry of the complex double-double walk
(sup_perman_complex_quad_range) over Gaussian integers and
fractions.Fraction: shared by test_complex_quad.py and test_gpu_complex_quad.py,
and (range_sum_abs: the sum and the scale of its tolerance) by the per-order
tests of the complex fp64 walk, test_fp64_range.py and
test_gpu_complex_orders.py.  Nothing here calls the engine or the oracle.

It is range_truth.range_sum's enumeration with complex values and the identity
column map: a range of wave-chunks [c0, c1) of a plan with L lane bits and m
walk bits covers the subsets S of columns 0..n-2 whose bits >= L + m are
gray(a) = a ^ (a >> 1) for an a in [c0, c1) and whose low L + m bits are
arbitrary, and its sum is

    sum_S (-1)^|S| prod_j (x0_j + sum_{c in S} a_jc),
    x0_j = a_j,n-1 - 1/2 sum_c a_jc.

A complex value is a pair (re, im) of Python ints.
"""
from fractions import Fraction
from math import prod


def _cprod(x):
    pr, pi = 1, 0
    for r, i in x:
        pr, pi = pr * r - pi * i, pr * i + pi * r
    return pr, pi


def range_sum(A, L, m, c0, c1):
    """The sum above for a matrix of Gaussian integers, rows of (re, im) pairs of
    Python ints whose row sums are even in both parts (a doubled matrix), as a
    pair of ints.  The low bits are walked with a Gray code, one column add
    per step."""
    n = len(A)
    lo = L + m
    assert lo <= n - 1
    sums = [(sum(z[0] for z in row), sum(z[1] for z in row)) for row in A]
    assert all(s[0] % 2 == 0 and s[1] % 2 == 0 for s in sums)
    x0 = [(A[j][n - 1][0] - sums[j][0] // 2, A[j][n - 1][1] - sums[j][1] // 2) for j in range(n)]
    cols = [[A[j][e] for j in range(n)] for e in range(n - 1)]
    tr = ti = 0
    for a in range(c0, c1):
        x = list(x0)
        sign = 1
        g, e = a ^ (a >> 1), lo
        while g:
            if g & 1:
                x = [(u[0] + v[0], u[1] + v[1]) for u, v in zip(x, cols[e])]
                sign = -sign
            g >>= 1
            e += 1
        pr, pi = _cprod(x)
        tr, ti = tr + sign * pr, ti + sign * pi
        for t in range(1, 1 << lo):
            k = (t & -t).bit_length() - 1
            if ((t >> k) ^ (t >> (k + 1))) & 1:  # bit k of gray(t): set by this step
                x = [(u[0] + v[0], u[1] + v[1]) for u, v in zip(x, cols[k])]
            else:
                x = [(u[0] - v[0], u[1] - v[1]) for u, v in zip(x, cols[k])]
            sign = -sign
            pr, pi = _cprod(x)
            tr, ti = tr + sign * pr, ti + sign * pi
    return tr, ti


def range_sum_float(a, L, m, c0, c1):
    """The sum for a complex128 matrix, as (Fraction re, Fraction im): every
    part of every entry is k 2^-s exactly, so the walk runs on the Gaussian
    integers 2 a 2^s and the result is scaled back by 2^-(n (s + 1))."""
    n = len(a)
    fr = [[(Fraction(float(complex(z).real)), Fraction(float(complex(z).imag))) for z in row] for row in a]
    s = max(p.denominator for row in fr for z in row for p in z).bit_length() - 1
    ints = [[(int(2 * z[0] * (1 << s)), int(2 * z[1] * (1 << s))) for z in row] for row in fr]
    assert all(Fraction(ints[j][c][p], 2 << s) == fr[j][c][p] for j in range(n) for c in range(n) for p in (0, 1))
    tr, ti = range_sum(ints, L, m, c0, c1)
    return Fraction(tr, 1 << (n * (s + 1))), Fraction(ti, 1 << (n * (s + 1)))


def range_sum_abs(A, L, m, c0, c1):
    """range_sum with a second accumulator: (re, im, scale) with scale the exact
    sum of |Re term| + |Im term| over the same subsets (the fp64 walk's
    tolerance is a multiple of it: test_fp64_range.py).  A step touches the
    nonzeros of its column only."""
    n = len(A)
    lo = L + m
    assert lo <= n - 1
    sums = [(sum(z[0] for z in row), sum(z[1] for z in row)) for row in A]
    assert all(s[0] % 2 == 0 and s[1] % 2 == 0 for s in sums)
    xr = [A[j][n - 1][0] - sums[j][0] // 2 for j in range(n)]
    xi = [A[j][n - 1][1] - sums[j][1] // 2 for j in range(n)]
    cols = [[(j, A[j][e][0], A[j][e][1]) for j in range(n) if A[j][e] != (0, 0)] for e in range(n - 1)]

    def cprod(r, i):
        pr, pi = 1, 0
        for u, v in zip(r, i):
            pr, pi = pr * u - pi * v, pr * v + pi * u
        return pr, pi

    tr = ti = scale = 0
    for a in range(c0, c1):
        r, i = list(xr), list(xi)
        sign = 1
        g, e = a ^ (a >> 1), lo
        while g:
            if g & 1:
                for j, u, v in cols[e]:
                    r[j] += u
                    i[j] += v
                sign = -sign
            g >>= 1
            e += 1
        pr, pi = cprod(r, i)
        tr, ti, scale = tr + sign * pr, ti + sign * pi, scale + abs(pr) + abs(pi)
        for t in range(1, 1 << lo):
            k = (t & -t).bit_length() - 1
            if ((t >> k) ^ (t >> (k + 1))) & 1:  # bit k of gray(t): set by this step
                for j, u, v in cols[k]:
                    r[j] += u
                    i[j] += v
            else:
                for j, u, v in cols[k]:
                    r[j] -= u
                    i[j] -= v
            sign = -sign
            pr, pi = cprod(r, i)
            tr, ti, scale = tr + sign * pr, ti + sign * pi, scale + abs(pr) + abs(pi)
    return tr, ti, scale


def range_sum_abs_float(a, L, m, c0, c1):
    """(re, im, scale) for a complex128 matrix, as Fractions: range_sum_float's
    scaling of range_sum_abs."""
    n = len(a)
    fr = [[(Fraction(float(complex(z).real)), Fraction(float(complex(z).imag))) for z in row] for row in a]
    s = max(p.denominator for row in fr for z in row for p in z).bit_length() - 1
    ints = [[(int(2 * z[0] * (1 << s)), int(2 * z[1] * (1 << s))) for z in row] for row in fr]
    assert all(Fraction(ints[j][c][p], 2 << s) == fr[j][c][p] for j in range(n) for c in range(n) for p in (0, 1))
    den = 1 << (n * (s + 1))
    tr, ti, scale = range_sum_abs(ints, L, m, c0, c1)
    return Fraction(tr, den), Fraction(ti, den), Fraction(scale, den)


def subsets(L, m, c0, c1):
    return (c1 - c0) << (L + m)


def bound(a, n_subsets):
    """B of the tolerance: subsets in range x prod_j sum_c (|Re a_jc| + |Im a_jc|), exact."""
    return n_subsets * prod(sum(abs(Fraction(float(complex(z).real))) + abs(Fraction(float(complex(z).imag)))
                                for z in row) for row in a)


def factor(n, m, h):
    """Relative-error factor of a complex double-double range per part, in
    units of 2^-103 B: range_truth.dd_factor's derivation with one change.  A
    complex product costs each part two dd_mul and one dd_add; measured against
    the submultiplicative norm |re| + |im| each of those is within 2^-103, so
    at most 3 units per factor of the product, and 4n is taken (the real walk
    takes 2n).  n^2 for the column adds, 2^m for a lane's sequential
    accumulation, 6 + h for the lane butterfly and the chunk tree."""
    return n * n + 4 * n + (1 << m) + 6 + h
