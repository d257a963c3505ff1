"""Exact truth for the range entries of the residue walk and the double-double
walk (sup_perman_exact_range, sup_perman_quad_range), in plain Python integers
and fractions.Fraction: shared by test_exact_range.py, test_quad_range.py and
their GPU counterparts.  Nothing here calls the engine or the oracle.

A range of wave-chunks [c0, c1) of a plan with L lane bits, m walk bits and the
column map `colmap` (engine bit e = matrix column colmap[e]) covers exactly the
subsets S of engine bits whose bits >= L + m are gray(a) = a ^ (a >> 1) for an
a in [c0, c1) and whose low L + m bits are arbitrary.  Its sum is

    sum_S (-1)^|S| prod_j (x0_j + sum_{e in S} A[j][colmap[e]]),
    x0_j = A[j][n-1] - 1/2 sum_c A[j][c].
"""
from fractions import Fraction
from math import prod


def range_sum(A, colmap, L, m, c0, c1):
    """The sum above for a matrix of Python ints or Fractions (lists of rows).
    The low bits are walked with a Gray code, one column add per step.  Ints
    stay ints when every row sum is even (the doubled matrix 2A)."""
    n = len(A)
    lo = L + m
    assert len(colmap) >= n - 1 and lo <= n - 1
    x0 = [A[j][n - 1] - Fraction(sum(A[j]), 2) for j in range(n)]
    if all(v.denominator == 1 for v in x0):
        x0 = [int(v) for v in x0]
    cols = [[A[j][colmap[e]] for j in range(n)] for e in range(n - 1)]
    total = 0
    for a in range(c0, c1):
        x = list(x0)
        sign = 1
        g, e = a ^ (a >> 1), lo
        while g:
            if g & 1:
                x = [u + v for u, v in zip(x, cols[e])]
                sign = -sign
            g >>= 1
            e += 1
        total += sign * prod(x)
        for t in range(1, 1 << lo):
            k = (t & -t).bit_length() - 1
            if ((t >> k) ^ (t >> (k + 1))) & 1:  # bit k of gray(t): set by this step
                x = [u + v for u, v in zip(x, cols[k])]
            else:
                x = [u - v for u, v in zip(x, cols[k])]
            sign = -sign
            total += sign * prod(x)
    return total


def subsets(L, m, c0, c1):
    return (c1 - c0) << (L + m)


def doubled(a):
    """2A as rows of Python ints (a: an integer-valued array)."""
    return [[2 * int(v) for v in row] for row in a]


def range_sum_float(a, colmap, L, m, c0, c1):
    """The sum for a matrix of floats, as a Fraction: every entry is k 2^-s
    exactly, so the walk runs on the integers 2 a 2^s and the result is scaled
    back by 2^-(n (s + 1)) (the same rational number, in integer arithmetic)."""
    n = len(a)
    fr = [[Fraction(float(v)) for v in row] for row in a]
    s = max(max(v.denominator for v in row) for row in fr).bit_length() - 1
    ints = [[int(2 * v * (1 << s)) for v in row] for row in fr]
    assert all(Fraction(ints[j][c], 2 << s) == fr[j][c] for j in range(n) for c in range(n))
    return Fraction(range_sum(ints, colmap, L, m, c0, c1), 1 << (n * (s + 1)))


def permanent(a):
    """The permanent of a small matrix of ints or Fractions by expansion along
    the first row with memoised column sets (no Ryser, no Gray code)."""
    n = len(a)
    memo = {}

    def sub(row, used):
        if row == n:
            return 1
        key = (row, used)
        if key not in memo:
            memo[key] = sum(a[row][c] * sub(row + 1, used | (1 << c)) for c in range(n)
                            if not (used >> c) & 1 and a[row][c] != 0)
        return memo[key]

    return sub(0, 0)


def crt_signed(residues, primes):
    """The integer in (-M/2, M/2] with the given residues, M = prod primes."""
    x, M = 0, 1
    for r, p in zip(residues, primes):
        x += M * (((r - x) * pow(M, -1, p)) % p)
        M *= p
    return x - M if 2 * x > M else x


def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def dd_add(a, b):
    """(hi, lo) + (hi, lo) in double-double: two_sum of both parts, two
    renormalisations (the sum the entries' own chunk tree uses; IEEE adds
    only, so Python floats give the same bits)."""
    s, se = _two_sum(a[0], b[0])
    t, te = _two_sum(a[1], b[1])
    se += t
    s, se = s + se, se - ((s + se) - s)
    se += te
    return s + se, se - ((s + se) - s)


def fold_pairwise(parts, add):
    """One fixed pairwise tree (an odd last element moves up as it is)."""
    parts = list(parts)
    while len(parts) > 1:
        parts = [add(parts[i], parts[i + 1]) if i + 1 < len(parts) else parts[i] for i in range(0, len(parts), 2)]
    return parts[0]


def chunk_count(sup, n, walk_log2=0):
    """Wave-chunks of the order-n plan with walk_log2 walk bits (0: default layout)."""
    L, m, _ = sup.layout(n)
    if walk_log2:
        m = min(walk_log2, n - 1 - L)
    return 1 << (n - 1 - L - m)


def scattered_start(chunks, count=8):
    """A chunk index with scattered bits, up to the top of the chunk space, that
    leaves `count` chunks above it; 0 when there are no more than `count`."""
    if chunks <= count:
        return 0
    c0 = 0x5A5A5A5A5A5A5A5B & (chunks - 1)
    return min(c0, chunks - count)


def sparse_int_matrix(n, seed):
    """Density ~0.35, entries in {-1, 1, 2}, one permutation filled in (no zero
    row); row sums of |a| <= 127, so the residue walk may group 4 rows at any
    order up to 64."""
    import numpy as np
    rng = np.random.default_rng(seed)
    mask = rng.random((n, n)) < 0.35
    mask[np.arange(n), rng.permutation(n)] = True
    a = np.where(mask, rng.choice(np.array([-1, 1, 2]), (n, n)), 0).astype(np.int32)
    assert np.abs(a).sum(1).max() <= 127 and np.abs(a).sum(1).min() >= 1
    return a


def chunk_end_matrix():
    """n = 36, integers: columns 0..17 are sparse and live in rows 0..31 only, so
    the greedy order takes its walk and lane columns from them and rows 32..35
    are chunk-end rows (touched by high columns only).  Each of those rows
    holds two 1s in high columns: X = -2 + 2 [p in S] + 2 [q in S] is exactly
    zero for half of the chunks."""
    import numpy as np
    n = 36
    rng = np.random.default_rng(36)
    a = np.zeros((n, n), np.int32)
    for c in range(18):
        a[rng.choice(32, 2, replace=False), c] = rng.choice(np.array([-1, 1, 2]), 2)
    a[:32, 18:] = np.where(rng.random((32, 18)) < 0.5, rng.choice(np.array([-1, 1, 2]), (32, 18)), 0)
    a[np.arange(32), rng.permutation(32)] |= 1
    a[:32, 35] += (a[:32].sum(1) + 1) % 2  # odd row sums: X_j of 2A is odd, rows 0..31 are never zero
    for i, r in enumerate(range(32, 36)):
        a[r, 18 + 2 * i] = a[r, 19 + 2 * i + 4] = 1
    return a


def chunk_end_rows(a, info):
    """Matrix rows no walk and no lane column of the plan touches."""
    cols = info["colmap"][: info["L"] + info["m"]]
    return [j for j in range(len(a)) if not any(a[j][c] for c in cols)]


def ended_chunks(a, info, c0, c1, rows):
    """Per chunk of [c0, c1): True when one of the chunk-end rows `rows` of 2A
    is exactly zero at the chunk's start (it is constant over the chunk, so
    every term is 0)."""
    n, lo = len(a), info["L"] + info["m"]
    out = []
    for ch in range(c0, c1):
        g = ch ^ (ch >> 1)
        x = {j: 2 * int(a[j][n - 1]) - sum(int(v) for v in a[j]) for j in rows}
        for b in range(n - 1 - lo):
            if (g >> b) & 1:
                for j in rows:
                    x[j] += 2 * int(a[j][info["colmap"][lo + b]])
        out.append(any(v == 0 for v in x.values()))
    return out


def mixed_window(a, info, rows, start, count=8, tries=4096):
    """The first c0 = start + 5 k whose chunks [c0, c0 + count) neither all end
    nor are all walked, and which chunks of it end."""
    for k in range(tries):
        c0 = start + 5 * k
        ended = ended_chunks(a, info, c0, c0 + count, rows)
        if any(ended) and not all(ended):
            return c0, ended
    raise AssertionError("no range with ended and walked chunks")


def dd_bound(a, n_subsets):
    """B of the double-double tolerance: subsets in range x prod_j sum_c |a_jc|, exact."""
    return n_subsets * prod(sum(abs(Fraction(float(v))) for v in row) for row in a)


def dd_factor(n, m, h):
    """Relative-error factor of a double-double range in units of 2^-103, each
    dd.hpp operation within 2^-103: n^2 for the column adds, 2n for the
    products, 2^m for a lane's sequential accumulation, 6 + h for the lane
    butterfly and the chunk tree."""
    return n * n + 2 * n + (1 << m) + 6 + h
