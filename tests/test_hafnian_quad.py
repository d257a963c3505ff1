"""Double-double hafnians and loop hafnians on host threads (hafnian_quad.cpp,
the host twin of walk_hafdd.hip, through hafnian_quad_batch(cpu=True)).  Truth
is always exact: Python integers or Fractions (test_hafnian.py's helpers, Kan's
sum restated for the loop form below, the rank-one closed form, or the exact
CRT entry for Gaussian integers); never a floating-point library value.

The error bound is derived, not fitted.  Convention (DESIGN.md 8f, 8q;
complex_range_truth.factor): every dd_add, dd_add_d, dd_mul, dd_mul_d and dd_div
is within 2^-103 of the 1-norm |re| + |im| of what it forms, a two-product and a
scaling by 2 are exact, and a cxdd_mul puts at most 3 such units on each part
(two dd_mul and one dd_add).  Units are counted along the path of one summand
from the table to the fold, with K distinct values, Tw states per lane, at most
K high digits and m = n / 2:

  the table    (B h(0))_k: K dd_add.  Q(0): per k a dd_mul_d and a dd_add on top
               of (B h(0))_k: 2K + 1.  r(0), G_e(0): K.
  chunk start  per high digit (at most K): t = (B h(0))_j (K) plus at most K
               dd_add; then a dd_mul_d and two dd_add on Q: K (2K + 3) on Q, and
               K more on every G_e and on r.
  steps        at most Tw; each puts a dd_add and a dd_add_d on Q and brings in
               G_d, which carries K (table) + K (chunk start) + Tw (one dd_add_d
               per step) units: Tw (Tw + 2K + 2) on Q; r carries at most 2K + Tw.
  uQ = 2K + 1 + K (2K + 3) + Tw (Tw + 2K + 2) bounds the units on Q and on r.
  the term     plain: Q^m multiplies the relative error of Q by m, and its at
               most m cxdd_mul add 3 each: m (uQ + 3).  loop: a monomial
               c_j Q^j r^(n-2j) has j + (n - 2j) <= n factors: n uQ; Horner's
               form spends per j a cxdd_mul (3), a dd_mul, a dd_add and the
               power of R (3), at most 8 m = 4 n, plus R and the odd factor (6);
               c_j = 1 / (j! (n-2j)!) comes from at most n dd_mul_d, a dd_mul
               and a dd_div: n + 3.  In all n (uQ + 5) + 9.
  the tail     w x term (1), the lane's sequential accumulation (Tw), the high
               weight's K dd_mul and its application (K + 1), the butterfly (6),
               the chunk tree (at most 24 levels) and the division by m! (1):
               Tw + K + 33.

  factor = m (uQ + 3) + Tw + K + 33          plain
         = n (uQ + 5) + 9 + Tw + K + 33      loop

and every part obeys |hi + lo - truth| <= factor 2^-103 S with
S = 2 sum_v |w(v) term(v)|_1 (/ m!), |z|_1 = |re z| + |im z|, term the summand
(the loop form: the polynomial's value).  S is formed in numpy from the exact
weights; it only scales the bound.  Every asserted case checks factor 2^-103 <
2^-80, so a lost low word (an error near 2^-53) is never inside the bound.
Measured / bound, as printed by these tests: see DESIGN.md 8q.
"""
import itertools
import math
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from test_hafnian import (exact_entries, hetero_lists, kan_haf, kan_states, rank_one_haf_case, rec_haf, sym_dyadic,
                          sym_gauss_int, walk_shape)

U = Fraction(1, 2 ** 103)


def qbits(v):
    return np.ascontiguousarray(np.asarray(v, dtype=np.float64)).view(np.uint64)


def factor(n, Tw, K, loop):
    m = n // 2
    uq = 2 * K + 1 + K * (2 * K + 3) + Tw * (Tw + 2 * K + 2)
    return n * (uq + 5) + 9 + Tw + K + 33 if loop else m * (uq + 3) + Tw + K + 33


def scale(A, mu, idx, loop):
    """S = 2 sum |w term|_1 (/ m!) from numpy."""
    idx = [int(i) for i in idx]
    n, m = len(idx), len(idx) // 2
    vals = list(dict.fromkeys(idx))
    mult = [idx.count(v) for v in vals]
    V, w = kan_states(mult)
    wf = np.abs(np.array([float(x) for x in w]))
    h = np.array(mult)[None, :] / 2 - V
    qh = np.einsum("tk,kl,tl->t", h, np.asarray(A)[np.ix_(vals, vals)] / 2, h)
    if loop:
        r = h @ np.asarray(mu)[vals]
        t = sum(qh ** j / math.factorial(j) * r ** (n - 2 * j) / math.factorial(n - 2 * j) for j in range(m + 1))
        return 2 * float(np.sum(wf * (np.abs(t.real) + np.abs(t.imag))))
    p = qh ** m
    return 2 * float(np.sum(wf * (np.abs(p.real) + np.abs(p.imag)))) / math.factorial(m)


def fmul(a, b):
    return (a[0] * b[0] - a[1] * b[1], a[0] * b[1] + a[1] * b[0])


def kan_loop(E, Emu, idx, den):
    """Kan's sum for the loop hafnian of the gather of the exact pairs E / den
    with displacement Emu / den:
    2 sum_v w sum_j (q/2)^j / j! r^(n-2j) / (n-2j)!,  q = h^T A h, r = mu . h,
    over Python integers: with Q = (2h)^T E (2h) = 8 den (q/2) and r' = (2h) . Emu
    = 2 den r, monomial j is a_j Q^j r'^(n-2j) / D with a_j = n! / (j! (n-2j)!)
    2^(m-j) den^j (an integer) and D = n! 2^(n+m) den^n."""
    idx = [int(i) for i in idx]
    n, m = len(idx), len(idx) // 2
    vals = list(dict.fromkeys(idx))
    mult = [idx.count(v) for v in vals]
    V, w = kan_states(mult)
    a = [math.factorial(n) // (math.factorial(j) * math.factorial(n - 2 * j)) * 2 ** (m - j) * den ** j
         for j in range(m + 1)]
    tr = ti = 0
    for wt, v in zip(w, V):
        h2 = [s - 2 * int(x) for s, x in zip(mult, v)]  # 2 h
        q = (sum(x * E[vals[k]][vals[l]][0] * y for k, x in enumerate(h2) for l, y in enumerate(h2)),
             sum(x * E[vals[k]][vals[l]][1] * y for k, x in enumerate(h2) for l, y in enumerate(h2)))
        r = (sum(x * Emu[vals[k]][0] for k, x in enumerate(h2)), sum(x * Emu[vals[k]][1] for k, x in enumerate(h2)))
        R = fmul(r, r)
        P = (a[m], 0)  # Horner in q with the powers of R = r'^2
        Rp = R
        for j in range(m - 1, -1, -1):
            P = fmul(P, q)
            P = (P[0] + a[j] * Rp[0], P[1] + a[j] * Rp[1])
            if j:
                Rp = fmul(Rp, R)
        if n & 1:
            P = fmul(P, r)
        tr, ti = tr + wt * P[0], ti + wt * P[1]
    D = math.factorial(n) * 2 ** (n + m) * den ** n
    return Fraction(2 * tr, D), Fraction(2 * ti, D)


def check(sup, A, mu, idx, loop, truth, tag, **kw):
    """Asserts the derived bound per part; returns (value, measured / bound)."""
    T, Tw, H, K = walk_shape(idx)
    n = len(idx)
    f = factor(n, Tw, K, loop)
    assert f * U < Fraction(1, 2 ** 80), (tag, f)  # the bound cannot go vacuous
    S = scale(A, mu, idx, loop)
    v = sup.hafnian_quad_batch(A, idx, mu=mu, loop=loop, cpu=True, **kw)
    bound = f * U * Fraction(S)
    e = [abs(Fraction(hi) + Fraction(lo) - t) for (hi, lo), t in zip(v, truth)]
    ratio = float(max(e) / bound) if bound else 0.0
    print(f"{tag} n={n} loop={loop} T={T} Tw={Tw} H={H} K={K} factor={f} measured/bound={ratio:.3e}")
    assert all(x <= bound for x in e), (tag, [float(x) for x in e], float(bound))
    for hi, lo in v:
        assert hi + lo == hi  # a normalised pair
    return v, ratio


def dyadic_truth(A, mu, idx, loop, den=2 ** 10):
    E, Emu = exact_entries(A, den), exact_entries(np.asarray(mu)[None, :], den)[0]
    if not loop:
        return kan_haf(E, idx, den)
    Ef = [[(Fraction(p[0], den), Fraction(p[1], den)) for p in row] for row in E]
    muf = [(Fraction(p[0], den), Fraction(p[1], den)) for p in Emu]
    return rec_haf(Ef, idx, muf)


# ---- 1, 2. accuracy against exact truth -------------------------------------------

@pytest.mark.parametrize("n", range(2, 13))
def test_dyadic_distinct_lists_within_the_derived_bound(sup, n):
    A = sym_dyadic(n, 140 + n)
    mu = np.diag(sym_dyadic(n, 190 + n))
    for loop in (False, True):
        if loop or n % 2 == 0:
            check(sup, A, mu, np.arange(n), loop, dyadic_truth(A, mu, np.arange(n), loop), "distinct")


@pytest.mark.parametrize("mult", [(3, 3, 3, 3), (2,) * 6])
def test_dyadic_repeats_at_n12(sup, mult):
    M = len(mult)
    A = sym_dyadic(M, 52)
    mu = np.diag(sym_dyadic(M, 53))
    idx = np.repeat(np.arange(M), mult)
    for loop in (False, True):
        check(sup, A, mu, idx, loop, dyadic_truth(A, mu, idx, loop), f"mult={mult}")


def test_every_multiplicity_vector_of_total_6_over_four_modes(sup):
    A = sym_dyadic(4, 76)
    mu = np.diag(sym_dyadic(4, 86))
    vecs = [s for s in itertools.product(range(7), repeat=4) if sum(s) == 6]
    assert len(vecs) == 84
    worst = 0.0
    for s in vecs:
        idx = np.repeat(np.arange(4), s)
        for loop in (False, True):
            v, ratio = check(sup, A, mu, idx, loop, dyadic_truth(A, mu, idx, loop), f"s={s}")
            worst = max(worst, ratio)
            r = sup.hafnian_quad_repeated(A, s, mu=mu, loop=loop, cpu=True)  # the repeated form names the same gather
            assert qbits(np.ravel(r)).tolist() == qbits(np.ravel(v)).tolist()
    print(f"worst measured/bound over 84 vectors = {worst:.3e}")


def test_closed_forms(sup):
    A = np.array([[0.5 - 1.25j, 2 + 0.75j], [2 + 0.75j, -3 + 0.5j]])
    mu = np.array([1.5 - 0.5j, -2 + 3j])
    for k in range(2):
        v = sup.hafnian_quad_batch(A, [k], mu=mu, loop=True, cpu=True)  # n = 1 loop: mu, low words 0
        assert v == ((mu[k].real, 0.0), (mu[k].imag, 0.0))
        v = sup.hafnian_quad_batch(A, [k, k], cpu=True)
        assert v == ((A[k, k].real, 0.0), (A[k, k].imag, 0.0))
    assert sup.hafnian_quad(A, cpu=True) == ((2.0, 0.0), (0.75, 0.0))
    z = A[0, 1] + mu[0] * mu[1]  # n = 2 loop: A01 + mu0 mu1, exact in a double here
    assert sup.loop_hafnian_quad(A, mu=mu, cpu=True) == ((z.real, 0.0), (z.imag, 0.0))
    assert sup.loop_hafnian_quad(A[:1, :1], cpu=True) == ((0.5, 0.0), (-1.25, 0.0))  # mu defaults to the diagonal
    assert sup.HAFNIAN_QUAD_MAX_DEVICE_N == 64


# ---- 3. Gaussian integers ---------------------------------------------------------

def gauss_case(sup, A, mu, tag):
    n = A.shape[0]
    T, Tw, H, K = walk_shape(range(n))
    for loop in (False, True):
        f = factor(n, Tw, K, loop)
        assert f * U < Fraction(1, 2 ** 80)
        S = scale(A, mu, range(n), loop)
        assert f * U * Fraction(S) < Fraction(1, 2)  # the bound itself says the rounded value is the integer
        (rh, rl), (ih, il) = sup.hafnian_quad_batch(A, np.arange(n), mu=mu, loop=loop, cpu=True)
        want = sup.loop_hafnian_exact(A, mu=mu, cpu=True) if loop else sup.hafnian_exact(A, cpu=True)
        got = (round(Fraction(rh) + Fraction(rl)), round(Fraction(ih) + Fraction(il)))
        print(f"{tag} n={n} loop={loop} bound x S = {float(f * U * Fraction(S)):.3e} value={want}")
        assert got == tuple(want)
    return want


@pytest.mark.parametrize("n", [4, 6, 8, 10, 12, 14, 16])
def test_gaussian_integers_round_to_the_exact_integer(sup, n):
    A = sym_gauss_int(n, 300 + n)
    gauss_case(sup, A, np.diag(A), "unit")


def test_gaussian_integers_beyond_2_53(sup):
    rng = np.random.default_rng(1000)
    a = rng.integers(-1000, 1001, (12, 12)) + 1j * rng.integers(-1000, 1001, (12, 12))
    A = np.triu(a) + np.triu(a, 1).T
    # the loop form takes a displacement with parts in {-1, 0, 1}: with the diagonal (parts up to 1000) the
    # loop hafnian itself is near 1e34, past the 106 bits of a double-double, and no bound can reach 1/2
    want = gauss_case(sup, A, np.diag(sym_gauss_int(12, 312)), "parts up to 1000")
    assert max(abs(int(want[0])), abs(int(want[1]))) > 2 ** 53


# ---- 4. rank one ------------------------------------------------------------------

@pytest.mark.parametrize("n,mult,loop", [(24, (4,) * 6, False), (64, (16, 16, 16, 16), False),
                                         (63, (16, 16, 16, 15), True)])
def test_rank_one_closed_form_and_closer_than_fp64(sup, n, mult, loop):
    A, mu, u, idx, truth = rank_one_haf_case(n, mult, loop, 600 + n)
    v, _ = check(sup, A, mu, idx, loop, truth, "rank one", threads=16)
    f = sup.hafnian_batch(A, idx, mu=mu, loop=loop, cpu=True)
    e_dd = [abs(Fraction(hi) + Fraction(lo) - t) for (hi, lo), t in zip(v, truth)]
    e_f = [abs(Fraction(f.real) - truth[0]), abs(Fraction(f.imag) - truth[1])]
    tn = float(abs(truth[0]) + abs(truth[1]))
    print(f"n={n} S/|truth|_1={scale(A, mu, idx, loop) / tn:.3e} fp64 error/|truth|_1={float(max(e_f)) / tn:.3e} "
          f"dd error/|truth|_1={float(max(e_dd)) / tn:.3e}")
    assert max(e_dd) < max(e_f) and sum(e_dd) < sum(e_f)  # strictly closer to the truth


# ---- 5. weights beyond 2^53 -------------------------------------------------------

WEIGHTS = [([0] * 57 + list(range(1, 8)), (3712, 58, 64), False, (57, 28)),  # C(57, 28) in the step program
           ([0] * 62 + [1, 1], (126, 1, 126), False, (62, 31)),            # C(62, 31) in the high-digit table
           # n = 63: no list walks a digit of radix 58 (H >= 64 would take seven more indices), so the
           # nearest lists put the large binomials in the high-digit table; the step program's side is
           # covered by the loop form of the n = 64 list
           ([0] * 57 + list(range(1, 8)), (3712, 58, 64), True, (57, 28)),
           ([0] * 57 + list(range(1, 7)), (1856, 1, 1856), True, (57, 28)),
           ([0] * 61 + [1, 1], (124, 1, 124), True, (61, 30))]


@pytest.mark.parametrize("idx,shape,loop,big", WEIGHTS)
def test_weights_beyond_2_53(sup, idx, shape, loop, big):
    """The smallest shapes at which a one-double weight goes wrong."""
    assert walk_shape(idx)[:3] == shape
    assert math.comb(*big) > 2 ** 53 and idx.count(0) == big[0]
    M = max(idx) + 1
    A = sym_dyadic(M, 58)
    mu = np.diag(sym_dyadic(M, 59))
    den = 2 ** 10
    E, Emu = exact_entries(A, den), exact_entries(mu[None, :], den)[0]
    truth = kan_loop(E, Emu, idx, den) if loop else kan_haf(E, idx, den)
    check(sup, A, mu, idx, loop, truth, "weights")


def test_kan_loop_is_the_recursive_definition():
    A = sym_dyadic(4, 3)
    mu = np.diag(sym_dyadic(4, 4))
    for idx in ([0, 1, 2, 3, 1], [2, 2, 2, 0, 0, 3], [1]):
        den = 2 ** 10
        E, Emu = exact_entries(A, den), exact_entries(mu[None, :], den)[0]
        assert kan_loop(E, Emu, idx, den) == dyadic_truth(A, mu, idx, True)


# ---- 6. the fp64 walk agrees with the hi words within its own bound ---------------

@pytest.mark.parametrize("n,mult", [(8, (1,) * 8), (10, (1,) * 10), (12, (1,) * 12), (12, (3, 3, 3, 3)), (12, (2,) * 6),
                                    (10, (4, 3, 2, 1)), (11, (1,) * 11), (9, (3, 3, 2, 1))])
def test_fp64_walk_agrees_with_the_hi_words(sup, n, mult):
    """test_hafnian.test_random_dyadic_error_over_scale's cases and bound:
    2^-52 (m or n) (Tw + K) S, S from moduli with the loop monomials summed."""
    M = len(mult)
    A = sym_dyadic(M, 40 + n + M)
    mu = np.diag(sym_dyadic(M, 90 + n))
    idx = np.repeat(np.arange(M), mult)
    m = n // 2
    V, w = kan_states(list(mult))
    wf = np.abs(np.array([float(x) for x in w]))
    h = np.array(mult)[None, :] / 2 - V
    qh = np.abs(np.einsum("tk,kl,tl->t", h, A / 2, h))
    r = np.abs(h @ mu)
    T, Tw, H, K = walk_shape(idx)
    for loop in (False, True):
        if not loop and n % 2:
            continue
        if loop:
            S = 2 * float(np.sum(wf * sum(qh ** j / math.factorial(j) * r ** (n - 2 * j) / math.factorial(n - 2 * j)
                                          for j in range(m + 1))))
        else:
            S = 2 * float(np.sum(wf * qh ** m)) / math.factorial(m)
        (rh, _), (ih, _) = sup.hafnian_quad_batch(A, idx, mu=mu, loop=loop, cpu=True)
        f = sup.hafnian_batch(A, idx, mu=mu, loop=loop, cpu=True)
        bound = 2.0 ** -52 * (n if loop else m) * (Tw + K) * S
        d = abs(complex(rh, ih) - f)
        print(f"n={n} mult={mult} loop={loop} |hi - fp64|/S={d / S:.3e} bound/S={bound / S:.3e}")
        assert d <= bound


# ---- 7. plumbing ------------------------------------------------------------------

def generic_case(seed, M=12):
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((M, M)) + 1j * rng.standard_normal((M, M))
    return A + A.T, rng.standard_normal(M) + 1j * rng.standard_normal(M)


def test_same_bits_on_any_thread_count_and_batch_is_the_single_call(sup):
    A, mu = generic_case(9)
    idx = hetero_lists(10, 65, 410)
    assert len(set(sup.hafnian_plan(idx).tolist())) >= 6
    for loop in (False, True):
        one = np.array([np.ravel(sup.hafnian_quad_batch(A, idx[k], mu=mu, loop=loop, cpu=True, threads=1))
                        for k in range(65)])
        for threads in (1, 3, 16):
            v = sup.hafnian_quad_batch(A, idx, mu=mu, loop=loop, cpu=True, threads=threads)
            assert v.shape == (65, 4) and np.array_equal(qbits(v), qbits(one))
    assert sup.hafnian_quad_batch(A, np.zeros((0, 10), dtype=int), cpu=True).shape == (0, 4)


def test_permuting_idx_within_the_groups_keeps_the_bits(sup):
    A, mu = generic_case(5, 7)
    rng = np.random.default_rng(5)
    base = np.repeat([5, 2, 6, 0], [4, 3, 3, 2])
    perms = [base]
    while len(perms) < 6:
        p = rng.permutation(base)
        if list(dict.fromkeys(p.tolist())) == [5, 2, 6, 0]:  # the order of first appearance orders the digits
            perms.append(p)
    for loop in (False, True):
        v = sup.hafnian_quad_batch(A, np.stack(perms), mu=mu, loop=loop, cpu=True)
        assert len({tuple(qbits(x).tolist()) for x in v}) == 1


@pytest.mark.parametrize("slab", ["1", "3"])
def test_slab_boundaries_keep_the_bits(sup, monkeypatch, slab):
    A, mu = generic_case(8)
    idx = hetero_lists(12, 7, 812)
    for loop in (False, True):
        whole = sup.hafnian_quad_batch(A, idx, mu=mu, loop=loop, cpu=True)
        monkeypatch.setenv("SUP_HAFNIAN_SLAB", slab)  # read at every call
        assert np.array_equal(qbits(sup.hafnian_quad_batch(A, idx, mu=mu, loop=loop, cpu=True)), qbits(whole))
        monkeypatch.delenv("SUP_HAFNIAN_SLAB")


@pytest.mark.parametrize("n", [1, 3, 7, 63])
def test_odd_order_is_exactly_zero_without_a_walk(sup, n):
    A = sym_dyadic(5, 11)
    idx = np.random.default_rng(n).integers(0, 5, (3, n))
    v, st = sup.hafnian_quad_batch(A, idx, cpu=True, return_stats=True)
    assert qbits(v).tolist() == [[0] * 4] * 3  # +0.0, not -0.0
    assert st["visited_steps"] == 0 and st["leaves"] == 3


def test_errors_name_the_place_and_write_nothing(sup):
    A = sym_dyadic(6, 8)
    mu = np.diag(A).copy()
    bad = A.copy()
    bad[4, 2] = np.nextafter(bad[4, 2].real, 9.0) + 1j * bad[4, 2].imag
    for loop, name in ((False, "sup_hafnian_complex_quad"), (True, "sup_loop_hafnian_complex_quad")):
        with pytest.raises(sup.SupError, match=rf"{name}: A\[2\]\[4\] and A\[4\]\[2\] differ.*symmetric") as e:
            sup.hafnian_quad_batch(bad, [0, 1], loop=loop, cpu=True)
        assert e.value.code == -1
        with pytest.raises(sup.SupError, match=rf"{name}: idx\[k = 1\]\[position 2\] = 6 outside \[0, 6\)") as e:
            sup.hafnian_quad_batch(A, [[0, 1, 2, 3], [0, 1, 6, 3]], loop=loop, cpu=True)
        assert e.value.code == -1
        with pytest.raises(sup.SupError, match=r"position 0\] = -1 outside") as e:
            sup.hafnian_quad_batch(A, [-1, 1], loop=loop, cpu=True)
        assert e.value.code == -1
    z = np.zeros((2, 2), dtype=np.complex128)
    z[0, 1] = complex(-0.0, 0.0)  # -0.0 against +0.0 is an asymmetric pair: bit for bit
    with pytest.raises(sup.SupError, match="symmetric"):
        sup.hafnian_quad(z, cpu=True)
    with pytest.raises(ValueError, match=r"n = 65 outside \[1, 64\]"):
        sup.hafnian_quad_batch(A, np.zeros(65, dtype=int), cpu=True)
    with pytest.raises(ValueError, match="mu must have shape"):
        sup.loop_hafnian_quad(A, mu=mu[:3], cpu=True)
    with pytest.raises(ValueError, match="rpt"):
        sup.hafnian_quad_repeated(A, [1, 1], cpu=True)
    # the C ABI itself: every SUP_EINVAL leaves out as it was
    lib = sup._lib.load()
    a, b = np.ascontiguousarray(A), np.ascontiguousarray(bad)
    ix = np.zeros(65, np.int32)
    far = np.array([0, 9], np.int32)
    out = np.full(8, 7.25)
    plain, loopf = lib.sup_hafnian_complex_quad, lib.sup_loop_hafnian_complex_quad
    P = lambda x: x.ctypes.data
    calls = [(plain, (P(a), 6, P(ix), 0, 1, None, 1, P(out), None), "n = 0 outside [1, 64]"),
             (plain, (P(a), 6, P(ix), 65, 1, None, 1, P(out), None), "n = 65 outside [1, 64]"),
             (loopf, (P(a), 6, P(mu), P(ix), 65, 1, None, 1, P(out), None), "n = 65 outside [1, 64]"),
             (plain, (None, 6, P(ix), 2, 1, None, 1, P(out), None), "sup_hafnian_complex_quad: null pointer"),
             (plain, (P(a), 6, None, 2, 1, None, 1, P(out), None), "sup_hafnian_complex_quad: null pointer"),
             (loopf, (P(a), 6, None, P(ix), 2, 1, None, 1, P(out), None), "sup_loop_hafnian_complex_quad: null pointer"),
             (plain, (P(a), 0, P(ix), 2, 1, None, 1, P(out), None), "at least one row (M = 0)"),
             (plain, (P(b), 6, P(ix), 2, 1, None, 1, P(out), None), "A[2][4] and A[4][2] differ"),
             (loopf, (P(a), 6, P(mu), P(far), 2, 1, None, 1, P(out), None), "idx[k = 0][position 1] = 9 outside [0, 6)")]
    for fn, args, msg in calls:
        assert fn(*args) == -1 and msg in lib.sup_last_error().decode(), (msg, lib.sup_last_error())
        assert (out == 7.25).all()
    assert plain(P(a), 6, P(ix), 2, 1, None, 1, None, None) == -1
    assert "sup_hafnian_complex_quad: null pointer" in lib.sup_last_error().decode()


def test_too_many_chunks_is_refused_before_any_work(sup):
    """42 distinct indices: T = 2^41, Tw = 2^10, H = 2^31, 2^25 wave-chunks."""
    A = np.ones((42, 42), dtype=np.complex128)
    for loop in (False, True):
        with pytest.raises(sup.SupError, match="matrix k = 1 has 2199023255552 terms") as e:
            sup.hafnian_quad_batch(A, [[0] * 42, list(range(42))], loop=loop, cpu=True)
        assert e.value.code == -7


def test_no_device_is_an_error_not_a_cpu_fallback(sup):
    A = sym_dyadic(6, 9)
    idx = np.random.default_rng(1).integers(0, 6, (4, 6))
    if sup.device_count() == 0:
        for loop in (False, True):
            with pytest.raises(sup.SupError) as e:
                sup.hafnian_quad_batch(A, idx, loop=loop)
            assert e.value.code == -2
    else:  # a box with a device: the device walk, the host twin's bits
        assert np.array_equal(qbits(sup.hafnian_quad_batch(A, idx)), qbits(sup.hafnian_quad_batch(A, idx, cpu=True)))


def test_the_cap_macro_and_the_abi(sup):
    import os
    txt = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "superman.h")).read()
    assert f"#define SUP_HAFNIAN_QUAD_MAX_DEVICE_N {sup.HAFNIAN_QUAD_MAX_DEVICE_N}\n" in txt
    assert sup._lib.load().sup_abi_version() >= 29


def ops(W, n, loop):
    """hafdd.hpp hafdd_ops, restated."""
    m = n // 2
    g = 72 if W <= 4 else 180
    if not loop:
        return 116 + g + 68 * (m.bit_length() - 1 + bin(m).count("1") - 1)
    return 202 + g + (190 * m - 68 if m else 0) + (68 if n & 1 else 0)


def test_est_ops_per_step_is_the_census(sup):
    A = sym_dyadic(16, 4)
    # list, walk digits W: ten distinct (T = 512, H = 64, W = 3), (3,3,3,3) (W = 1), 16 distinct (W = 9), one index (W = 0)
    for idx, W in ((np.arange(10), 3), (np.repeat(np.arange(4), 3), 1), (np.arange(16), 9), ([5], 0)):
        idx = np.asarray(idx)
        n = len(idx)
        T, Tw, H, K = walk_shape(idx)
        assert (W == 0 and Tw == 1) or (W == 1 and Tw == 3) or Tw == 2 ** W
        for loop in (False, True):
            if not loop and n % 2:
                continue
            _, st = sup.hafnian_quad_batch(A, idx, loop=loop, cpu=True, return_stats=True)
            assert st["est_ops_per_step"] == ops(W, n, loop), (idx, loop, Tw)
            assert st["visited_steps"] == T and st["gray_steps"] == 1 << (n - 1) and st["leaves"] == 1
    assert ops(9, 30, False) == 704 and ops(9, 30, True) == 3164


def run_cli(sup, *args):
    return subprocess.run([sup._lib.PERMAN_BIN, *args], capture_output=True, text=True, timeout=120)


def test_cli_hafnian_quad_on_host_threads(sup, tmp_path):
    A = sym_dyadic(5, 21)
    path = tmp_path / "h5.mtx"
    with open(path, "w") as f:
        f.write("%%MatrixMarket matrix coordinate complex symmetric\n5 5 15\n")
        for i in range(5):
            for j in range(i + 1):
                f.write(f"{i + 1} {j + 1} {float(A[i, j].real)!r} {float(A[i, j].imag)!r}\n")
    for extra, want in ((("--rpt", "1,1,1,1"), sup.hafnian_quad(A[:4, :4], cpu=True)),
                        (("--rpt", "2,0,3,0,1"), sup.hafnian_quad_repeated(A, [2, 0, 3, 0, 1], cpu=True)),
                        (("--loop",), sup.loop_hafnian_quad(A, cpu=True)),
                        (("--loop", "--rpt", "0,2,1"), sup.hafnian_quad_repeated(A, [0, 2, 1, 0, 0], loop=True, cpu=True))):
        r = run_cli(sup, "-f", str(path), "--hafnian", "--quad", "-c", *extra)
        assert r.returncode == 0, r.stderr
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("Hafnian (double-double): ")]
        name = "cpu_loop_hafnian64_complex_quad" if "--loop" in extra else "cpu_hafnian64_complex_quad"
        assert len(line) == 1 and name in r.stdout
        got = [float(x) for x in line[0].split()[2:]]
        assert qbits(got).tolist() == qbits(np.ravel(want)).tolist(), (extra, line, want)
    r = run_cli(sup, "-f", str(path), "--hafnian", "--quad", "-c")  # the whole 5 x 5 matrix: odd n
    assert r.returncode == 0 and "Hafnian (double-double): 0.00000000000000000e+00 0.0" in r.stdout
    for bad, msg in ((("--hafnian", "--quad", "--powertrace"), "--hafnian --quad does not combine with --powertrace"),
                     (("--hafnian", "--quad", "--exact"), "--hafnian --quad does not combine with --exact"),
                     (("--hafnian", "--quad", "--complex"), "--hafnian does not combine with --complex"),
                     (("--hafnian", "--quad", "--complex-quad"), "--hafnian does not combine with --complex-quad"),
                     (("--hafnian", "--quad", "-s"), "--hafnian does not combine with -s"),
                     (("--hafnian", "-q"), "--hafnian does not combine with -q"),
                     (("--quad", "--loop"), "--loop and --rpt go with --hafnian"),
                     (("--torontonian", "--quad"), "does not combine with -q")):
        r = run_cli(sup, "-f", str(path), "-c", *bad)
        assert r.returncode == 1 and msg in r.stderr, (bad, r.stderr)
