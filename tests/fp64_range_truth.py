"""Exact truth, inputs, windows and the derived tolerance for the per-order
tests of the fp64 walks (walk_dense, walk_sparse, walk_skip, walk_lds and the
segmented walk through sup_partial): shared by test_fp64_range.py and
test_gpu_fp64_range.py.  Nothing here calls the engine or the oracle.

The sum is range_truth.py's: a range of wave-chunks [c0, c1) of a plan with L
lane bits, m walk bits and the column map `colmap` covers the subsets S of
engine bits whose bits >= L + m are gray(a) for an a in [c0, c1) and whose low
L + m bits are arbitrary,

    sum_S (-1)^|S| prod_j (x0_j + sum_{e in S} A[j][colmap[e]]),
    x0_j = A[j][n-1] - 1/2 sum_c A[j][c].

With the identity map these are the reference Gray indices
[c0 << (L + m), c1 << (L + m)) of sup_partial, index 0 (the p0 term) included.

Tolerance.  |got - truth| <= F 2^-53 S with S the exact sum of |term| over the
same subsets and F = range_truth.dd_factor(n, m, h) = n^2 + 2n + 2^m + 6 + h
roundings on the way of any one term into the result: n^2 for the column adds
that built its X, 2n for its product, 2^m for the lane's sequential
accumulation, 6 + h for the lane butterfly and the chunk tree.  At 2^15 subsets
one wrong or missing term is about 2^-15 S; the tolerance is below 5e-13 S.
"""
from fractions import Fraction
from math import prod

import range_truth as T

EPS = Fraction(1, 1 << 53)
WALK_LOG2 = 6
WINDOW = 8
# sup_stats.walk_kind of sup_partial's kernels
KERNELS = (("dense_plain", 0), ("sparse", 1), ("skip", 2), ("dense_lds", 4))
MIRROR = {"dense_plain": "dense", "sparse": "sparse", "skip": "skip"}
SEG_ORDERS = (10, 11, 16, 17, 24, 25, 31, 32, 33, 40, 41, 48, 49, 57, 63, 64)


def range_sum_abs(A, colmap, L, m, c0, c1):
    """range_truth.range_sum with a second accumulator: (sum, sum of |term|)
    over the same subsets, for a matrix of Python ints or Fractions.  A step
    touches the nonzeros of its column only."""
    n = len(A)
    lo = L + m
    assert len(colmap) >= n - 1 and lo <= n - 1
    x0 = [A[j][n - 1] - Fraction(sum(A[j]), 2) for j in range(n)]
    if all(v.denominator == 1 for v in x0):
        x0 = [int(v) for v in x0]
    cols = [[(j, A[j][colmap[e]]) for j in range(n) if A[j][colmap[e]] != 0] for e in range(n - 1)]
    total = scale = 0
    for a in range(c0, c1):
        x = list(x0)
        sign = 1
        g, e = a ^ (a >> 1), lo
        while g:
            if g & 1:
                for j, v in cols[e]:
                    x[j] += v
                sign = -sign
            g >>= 1
            e += 1
        p = prod(x)
        total += sign * p
        scale += abs(p)
        for t in range(1, 1 << lo):
            k = (t & -t).bit_length() - 1
            if ((t >> k) ^ (t >> (k + 1))) & 1:  # bit k of gray(t): set by this step
                for j, v in cols[k]:
                    x[j] += v
            else:
                for j, v in cols[k]:
                    x[j] -= v
            sign = -sign
            p = prod(x)
            total += sign * p
            scale += abs(p)
    return total, scale


def range_sum_abs_float(a, colmap, L, m, c0, c1):
    """(sum, sum of |term|) for a matrix of floats, as Fractions: every entry is
    k 2^-s exactly, so the walk runs on the integers 2 a 2^s and both results
    are scaled back by 2^-(n (s + 1)) (range_truth.range_sum_float's scaling)."""
    n = len(a)
    fr = [[Fraction(float(v)) for v in row] for row in a]
    s = max(max(v.denominator for v in row) for row in fr).bit_length() - 1
    ints = [[int(2 * v * (1 << s)) for v in row] for row in fr]
    assert all(Fraction(ints[j][c], 2 << s) == fr[j][c] for j in range(n) for c in range(n))
    total, scale = range_sum_abs(ints, colmap, L, m, c0, c1)
    return Fraction(total, 1 << (n * (s + 1))), Fraction(scale, 1 << (n * (s + 1)))


def int_matrix(n):
    """The integer flavour: entries in {-1, 1, 2} at density 0.35."""
    import numpy as np
    return T.sparse_int_matrix(n, 300 + n).astype(np.float64)


def dyadic_matrix(n):
    """The dyadic flavour: Bernoulli(0.5) pattern, entries k / 8 with k in
    1 ... 40, one permutation set to 1.0."""
    import numpy as np
    rng = np.random.default_rng(900 + n)
    a = np.where(rng.random((n, n)) < 0.5, rng.integers(1, 41, (n, n)) / 8.0, 0.0)
    a[np.arange(n), rng.permutation(n)] = 1.0
    return a


FLAVOURS = (("int", int_matrix), ("dyadic", dyadic_matrix))


def complex_matrix(n):
    """Entries (p + q i) / 8 with p, q in -16 ... 16 at density 0.5."""
    import numpy as np
    rng = np.random.default_rng(700 + n)
    z = (rng.integers(-16, 17, (n, n)) + 1j * rng.integers(-16, 17, (n, n))) / 8.0
    return np.where(rng.random((n, n)) < 0.5, z, 0.0)


def layout(n):
    """(L, m, chunks) of the order-n plan with WALK_LOG2 walk bits."""
    L = min(6, n - 1)
    m = min(WALK_LOG2, n - 1 - L)
    return L, m, 1 << (n - 1 - L - m)


def windows(n):
    """Chunk ranges [c0, c1) of at most WINDOW chunks: the whole space when it
    is that small; otherwise the first (the p0 term at index 0), one at
    range_truth.scattered_start, and the last (the top bits of the chunk
    index set).  Coinciding windows are listed once."""
    chunks = layout(n)[2]
    if chunks <= WINDOW:
        return [(0, chunks)]
    out = []
    for c0 in (0, T.scattered_start(chunks, WINDOW), chunks - WINDOW):
        if (c0, c0 + WINDOW) not in out:
            out.append((c0, c0 + WINDOW))
    return out


def gray_range(n, c0, c1):
    """The reference Gray indices [s, e) of chunks [c0, c1)."""
    L, m, _ = layout(n)
    return c0 << (L + m), c1 << (L + m)


def factor(n):
    L, m, chunks = layout(n)
    return T.dd_factor(n, m, chunks.bit_length() - 1)


def ratio(got, truth, scale):
    """|got - truth| in units of 2^-53 S, as a float (for the printed figures)."""
    return float(abs(Fraction(got) - truth) / (EPS * scale))


def within(got, truth, scale, n):
    return abs(Fraction(got) - truth) <= factor(n) * EPS * scale


_TRUTH = {}


def truth(n, flavour, c0, c1):
    """(matrix, exact sum, exact sum of |term|) of a flavour's window with the
    identity column map, computed once and shared by the tests of a run."""
    key = (n, flavour, c0, c1)
    if key not in _TRUTH:
        a = dict(FLAVOURS)[flavour](n)
        L, m, _ = layout(n)
        _TRUTH[key] = (a,) + range_sum_abs_float(a, list(range(n - 1)), L, m, c0, c1)
    return _TRUTH[key]


def note(kind, value, where, worst):
    """Keep the worst ratio per kind in `worst`: kind -> (ratio, where)."""
    if value >= worst.get(kind, (-1.0, None))[0]:
        worst[kind] = (value, where)
