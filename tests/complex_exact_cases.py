"""Matrices of Gaussian integers and their exact truth in Python ints, shared
by test_complex_exact.py and test_gpu_complex_exact.py.  Nothing here calls
the engine; a Gaussian integer is a pair (re, im) of Python ints, a matrix a
list of rows of such pairs.

Whole permanents come from closed forms that are exact at any n:
  rank one, a_jc = u_j v_c       perm = n! prod u_j prod v_c
  J + (x - 1) I                  perm = sum_k C(n, k) (x - 1)^k (n - k)!
  c J_n                          perm = c^n n!
and, for n <= 12, from a Ryser sum in Python ints.  Ranges come from
complex_range_truth.range_sum on the doubled matrix.
"""
import functools
import random
from math import comb, factorial

import numpy as np

import complex_range_truth as CT
import range_truth as T


def cmul(a, b):
    return a[0] * b[0] - a[1] * b[1], a[0] * b[1] + a[1] * b[0]


def cpow(a, k):
    r = (1, 0)
    for _ in range(k):
        r = cmul(r, a)
    return r


def as_array(A):
    """complex128 array of a matrix whose parts are below 2^53."""
    return np.array([[complex(z[0], z[1]) for z in row] for row in A], dtype=np.complex128)


def doubled(A):
    return [[(2 * z[0], 2 * z[1]) for z in row] for row in A]


def random_gauss(n, seed, lo=-3, hi=3):
    rng = random.Random(seed)
    return [[(rng.randint(lo, hi), rng.randint(lo, hi)) for _ in range(n)] for _ in range(n)]


def ryser(A):
    """The permanent by Ryser's formula over Python ints (n <= 12): sum over
    column subsets in Gray order, (-1)^(n - |S|) prod_j sum_{c in S} a_jc."""
    n = len(A)
    sr, si = [0] * n, [0] * n
    tr = ti = 0
    for g in range(1, 1 << n):
        c = (g & -g).bit_length() - 1
        s = 1 if ((g ^ (g >> 1)) >> c) & 1 else -1
        for j in range(n):
            sr[j] += s * A[j][c][0]
            si[j] += s * A[j][c][1]
        p = (1, 0)
        for j in range(n):
            p = cmul(p, (sr[j], si[j]))
        if (n - bin(g ^ (g >> 1)).count("1")) & 1:
            p = (-p[0], -p[1])
        tr, ti = tr + p[0], ti + p[1]
    return tr, ti


# ---- the three closed forms: (matrix, permanent) ---------------------------------

def rank_one(n, seed=5):
    rng = random.Random(seed * 1000 + n)
    pick = lambda: rng.choice([(1, 0), (0, 1), (-1, 0), (0, -1), (1, 1), (1, -1), (2, 1), (-1, 2)])  # noqa: E731
    u, v = [pick() for _ in range(n)], [pick() for _ in range(n)]
    p = (factorial(n), 0)
    for z in u + v:
        p = cmul(p, z)
    return [[cmul(u[j], v[c]) for c in range(n)] for j in range(n)], p


def j_plus_diag(n, x=(2, -3)):
    """J + (x - 1) I: ones off the diagonal, x on it."""
    d = (x[0] - 1, x[1])
    tr = ti = 0
    for k in range(n + 1):
        t = cpow(d, k)
        f = comb(n, k) * factorial(n - k)
        tr, ti = tr + f * t[0], ti + f * t[1]
    return [[x if j == c else (1, 0) for c in range(n)] for j in range(n)], (tr, ti)


def const_matrix(n, c=(1, -2)):
    p = cpow(c, n)
    f = factorial(n)
    return [[c] * n for _ in range(n)], (f * p[0], f * p[1])


CLOSED_FORMS = (rank_one, j_plus_diag, const_matrix)


# ---- instance by instance: every N, at most 8 chunks, walk_log2 = 3 -----------------

WALK_LOG2 = 3


def layout(sup, n, walk_log2=WALK_LOG2):
    L, m, _ = sup.layout(n)
    if walk_log2:
        m = min(walk_log2, n - 1 - L)
    return L, m, n - 1 - L - m


@functools.lru_cache(maxsize=None)
def instance(n):
    """The order-n instance: entries in [-3, 3] + [-3, 3] i (row bounds <= 384, so
    both G are eligible at every n).  No engine call: the range comes from the
    layout rule (6 lane bits, walk_log2 walk bits)."""
    return random_gauss(n, 7000 + n)


def instance_range(sup, n):
    L, m, h = layout(sup, n)
    chunks = 1 << h
    c0 = T.scattered_start(chunks)
    return L, m, c0, min(chunks, c0 + 8)


_TRUTH = {}


def instance_truth(sup, n):
    """range_sum of the instance's range on 2A, computed once per n."""
    if n not in _TRUTH:
        L, m, c0, c1 = instance_range(sup, n)
        _TRUTH[n] = CT.range_sum(doubled(instance(n)), L, m, c0, c1)
    return _TRUTH[n]


def residues_match(r, truth):
    """The range entry's residues against an exact (re, im)."""
    return (len(r["primes"]) > 0 and [truth[0] % p for p in r["primes"]] == r["re"]
            and [truth[1] % p for p in r["primes"]] == r["im"])


def expected_ops(n, G, primes):
    """est_ops_per_step of include/superman.h: the column add, the exact pair
    products at G = 2, and per prime of a launch (at most 4) the chain and the
    accumulate."""
    K = (n + G - 1) // G
    return 2 * n + (4 * (n // 2) if G == 2 else 0) + min(primes, 4) * (10 * K - 2)
