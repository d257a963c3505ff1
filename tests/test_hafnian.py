"""Hafnians and loop hafnians with repeats on host threads (hafnian.cpp, the
host twin of walk_haf.hip, through hafnian_batch(cpu=True)) and the plan entry
hafnian_plan.

Matrix k is A[np.ix_(idx[k], idx[k])].  Truth is exact arithmetic written
here: the recursive definition in Python integers or Fractions, Kan's sum over
Python integers, or the rank-one closed form in Fractions; never the library.
"""
import itertools
import math
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from test_complex import gauss_int_case
from test_complex_batch import bits
from test_complex_fock import cmul, dyadic_phases, groups, layout


# ---- exact arithmetic -----------------------------------------------------------

def cadd(a, b):
    return (a[0] + b[0], a[1] + b[1])


def cpow(a, k):
    r = (1, 0)
    for _ in range(k):
        r = cmul(r, a)
    return r


def exact_entries(A, den=1):
    """A as pairs of Python integers: den x A must be integral."""
    out = [[(int(round(z.real * den)), int(round(z.imag * den))) for z in row] for row in np.atleast_2d(A)]
    assert all(complex(p[0], p[1]) / den == z for row, zr in zip(out, np.atleast_2d(A)) for p, z in zip(row, zr))
    return out


def rec_haf(E, idx, mu=None):
    """The recursive definition on the gather by idx, over exact pairs E (and
    the vector mu of pairs for the loop form): the first index pairs with one
    of the others (or, loop form, with itself through mu)."""
    memo = {}

    def go(ix):
        if not ix:
            return (1, 0)
        if ix in memo:
            return memo[ix]
        s = (0, 0)
        if mu is not None:
            s = cmul(mu[ix[0]], go(ix[1:]))
        elif len(ix) % 2:
            return (0, 0)
        for j in range(1, len(ix)):
            s = cadd(s, cmul(E[ix[0]][ix[j]], go(ix[1:j] + ix[j + 1:])))
        memo[ix] = s
        return s

    return go(tuple(int(i) for i in idx))


def kan_states(mult):
    """(V, w): the multiplicity vectors v of Kan's halved sum (one copy of the
    first rarest group held) as an int64 array [T, K], and their weights
    (-1)^(sum v) prod C(s'_k, v_k) as Python integers."""
    held = min(range(len(mult)), key=lambda k: (mult[k], k))
    sp = [s - (k == held) for k, s in enumerate(mult)]
    V = np.array(list(itertools.product(*[range(t + 1) for t in sp])), dtype=np.int64).reshape(-1, len(mult))
    w = [(-1) ** int(v.sum()) * math.prod(math.comb(t, int(x)) for t, x in zip(sp, v)) for v in V]
    return V, w


def kan_q4(Ebar, mult, V):
    """4 q(v) = (2h)^T Abar (2h) per state as pairs of Python integers, 2h = s - 2v
    (int64 numpy: the entries and counts here keep it far below 2^63)."""
    H2 = np.array(mult, dtype=np.int64)[None, :] - 2 * V
    re = np.array([[p[0] for p in row] for row in Ebar], dtype=np.int64)
    im = np.array([[p[1] for p in row] for row in Ebar], dtype=np.int64)
    qr = np.einsum("tk,kl,tl->t", H2, re, H2)
    qi = np.einsum("tk,kl,tl->t", H2, im, H2)
    return [(int(a), int(b)) for a, b in zip(qr, qi)]


def kan_haf(E, idx, den=1):
    """Kan's sum for the hafnian of the gather of the exact pairs E / den:
    2 sum_v w (4 q)^m / (8^m m! den^m), the division asserted exact when den = 1."""
    idx = [int(i) for i in idx]
    vals = list(dict.fromkeys(idx))
    mult = [idx.count(v) for v in vals]
    m = len(idx) // 2
    Ebar = [[E[a][b] for b in vals] for a in vals]
    V, w = kan_states(mult)
    tr = ti = 0
    for wt, q in zip(w, kan_q4(Ebar, mult, V)):
        p = cpow(q, m)
        tr, ti = tr + wt * p[0], ti + wt * p[1]
    d = 8 ** m * math.factorial(m) * den ** m
    if den == 1:
        assert (2 * tr) % d == 0 and (2 * ti) % d == 0  # the division is exact
    return Fraction(2 * tr, d), Fraction(2 * ti, d)


def err(v, truth):
    dr, di = Fraction(v.real) - truth[0], Fraction(v.imag) - truth[1]
    return float(dr * dr + di * di) ** 0.5


def sym_gauss_int(M, seed):
    a = gauss_int_case(M, seed)
    return np.triu(a) + np.triu(a, 1).T


def sym_dyadic(M, seed, bits_=10):
    rng = np.random.default_rng(seed)
    a = (rng.integers(-2 ** bits_, 2 ** bits_ + 1, (M, M)) + 1j * rng.integers(-2 ** bits_, 2 ** bits_ + 1, (M, M)))
    a = a / 2 ** bits_
    return np.triu(a) + np.triu(a, 1).T


def walk_shape(idx):
    """(T, Tw, H, K) of a list: the layout rule restated in test_complex_fock."""
    g = groups(idx)
    return layout(g) + (len(g),)


# ---- 1. closed forms, asserted with == ------------------------------------------

def test_closed_forms(sup):
    A = np.array([[0.5 - 1.25j, 2 + 0.75j, -1.5 + 1j, 0.25j],
                  [2 + 0.75j, -3 + 0.5j, 1 - 2j, 1.5 + 1.5j],
                  [-1.5 + 1j, 1 - 2j, 0.75 + 0j, -2.25 + 1j],
                  [0.25j, 1.5 + 1.5j, -2.25 + 1j, 1 + 1j]])
    mu = np.array([1.5 - 0.5j, -2 + 3j, 0.25 + 0.25j, 4 - 1j])
    for k in range(4):
        assert sup.hafnian_batch(A, [k], mu=mu, loop=True, cpu=True) == mu[k]  # n = 1 loop: mu
        assert sup.hafnian_batch(A, [k, k], cpu=True) == A[k, k]              # two copies of one mode pair
    assert sup.loop_hafnian(A[:1, :1], cpu=True) == A[0, 0]                   # mu defaults to the diagonal
    assert sup.hafnian(A[:2, :2], cpu=True) == A[0, 1]
    assert sup.hafnian_batch(A, [3, 1], cpu=True) == A[1, 3]
    # n = 4: the three perfect matchings; dyadic entries, every product and sum exact
    assert sup.hafnian(A, cpu=True) == A[0, 1] * A[2, 3] + A[0, 2] * A[1, 3] + A[0, 3] * A[1, 2]
    # n = 2 loop: A01 + mu0 mu1
    assert sup.hafnian_batch(A, [0, 1], mu=mu, loop=True, cpu=True) == A[0, 1] + mu[0] * mu[1]


@pytest.mark.parametrize("n", [1, 3, 7, 63])
def test_odd_order_is_exactly_zero_without_a_walk(sup, n):
    A = sym_dyadic(5, 11)
    idx = np.random.default_rng(n).integers(0, 5, (3, n))
    v, st = sup.hafnian_batch(A, idx, cpu=True, return_stats=True)
    assert bits(v).tolist() == [0] * 6  # +0.0, not -0.0
    assert st["visited_steps"] == 0 and st["leaves"] == 3


# ---- 2. exact truth -------------------------------------------------------------

@pytest.mark.parametrize("n", [4, 6, 8, 10, 12, 14, 16])
def test_gaussian_integers_round_to_the_exact_integer(sup, n):
    """Entries in {-1,0,1} + {-1,0,1} i: truth is Kan's sum over Python integers
    with 2h integral, the division by 8^m m! asserted exact."""
    A = sym_gauss_int(n, 300 + n)
    truth = kan_haf(exact_entries(A), range(n))
    assert truth[0].denominator == 1 and truth[1].denominator == 1
    if n <= 8:
        assert truth == tuple(Fraction(x) for x in rec_haf(exact_entries(A), range(n)))  # Kan's sum is the hafnian
    v, st = sup.hafnian(A, cpu=True, return_stats=True)
    assert st["visited_steps"] == 2 ** (n - 1)
    print(f"n={n} haf={truth[0]}+{truth[1]}i |v - truth|={err(v, truth):.3e}")
    assert err(v, truth) < 0.5


# n, multiplicities: Tw = 2, 8, 32 without repeats; Tw = 3 and 6 with
DYADIC = [(8, (1,) * 8), (10, (1,) * 10), (12, (1,) * 12), (12, (3, 3, 3, 3)), (12, (2,) * 6), (10, (4, 3, 2, 1)),
          (11, (1,) * 11), (9, (3, 3, 2, 1))]


@pytest.mark.parametrize("n,mult,loop", [(n, mult, loop) for n, mult in DYADIC for loop in (False, True)
                                         if loop or n % 2 == 0])
def test_random_dyadic_error_over_scale(sup, n, mult, loop):
    """error / S <= max(e_np, 2^-52) m (Tw + K): the incremental q carries at
    most Tw + K roundings and the m-th power multiplies a relative error by m.
    e_np: a numpy restatement that recomputes q from scratch at every state.
    The loop form takes n for m (its polynomial has degree n in r and n / 2 in
    q; r carries Tw + K roundings as q does).  Measured error / S (this test's
    print): 1e-17 .. 2e-16, the bound is 1e-14 .. 1e-13 here."""
    M, den = len(mult), 2 ** 10
    A = sym_dyadic(M, 40 + n + len(mult))
    mu = np.diag(sym_dyadic(M, 90 + n))
    idx = np.repeat(np.arange(M), mult)
    E, Emu = exact_entries(A, den), exact_entries(mu[None, :], den)[0]
    m = n // 2
    if loop:  # the recursive definition in Fractions
        Ef = [[(Fraction(p[0], den), Fraction(p[1], den)) for p in row] for row in E]
        muf = [(Fraction(p[0], den), Fraction(p[1], den)) for p in Emu]
        truth = rec_haf(Ef, idx, muf)
    else:
        truth = kan_haf(E, idx, den)
    # numpy restatement: q from scratch per state, the power by repeated products
    V, w = kan_states(list(mult))
    h = np.array(mult)[None, :] / 2 - V
    qh = np.einsum("tk,kl,tl->t", h, A / 2, h)
    wf = np.array([float(x) for x in w])
    if loop:
        r = h @ mu
        terms = [qh ** j / math.factorial(j) * r ** (n - 2 * j) / math.factorial(n - 2 * j) for j in range(m + 1)]
        v_np, S = 2 * np.sum(wf * np.sum(terms, axis=0)), 2 * float(np.sum(np.abs(wf) * np.sum(np.abs(terms), axis=0)))
    else:
        p = np.ones_like(qh)
        for _ in range(m):
            p = p * qh
        v_np, S = 2 * np.sum(wf * p) / math.factorial(m), 2 * float(np.sum(np.abs(wf) * np.abs(p))) / math.factorial(m)
    e_np = err(complex(v_np), truth) / S
    v = sup.hafnian_batch(A, idx, mu=mu, loop=loop, cpu=True)
    T, Tw, H, K = walk_shape(idx)
    e = err(v, truth) / S
    bound = max(e_np, 2.0 ** -52) * (n if loop else m) * (Tw + K)
    print(f"n={n} mult={mult} loop={loop} T={T} Tw={Tw} e={e:.3e} e_np={e_np:.3e} bound={bound:.3e} S/|v|={S / abs(v):.1f}")
    assert e <= bound


# ---- 3. repeats -----------------------------------------------------------------

def mult_vectors(total, modes=4):
    return [s for s in itertools.product(range(total + 1), repeat=modes) if sum(s) == total]


@pytest.mark.parametrize("total", [6, 8])
def test_every_multiplicity_vector_against_the_recursive_definition(sup, total):
    """Gaussian-integer A and mu on 4 modes: the (loop) hafnian of the gather is
    a Gaussian integer, so the result must round to the recursive definition's."""
    A = sym_gauss_int(4, 70 + total)
    mu = gauss_int_case(4, 80 + total)[0]
    E, Emu = exact_entries(A), exact_entries(mu[None, :])[0]
    vecs = mult_vectors(total)
    assert len(vecs) == math.comb(total + 3, 3)
    idx = np.stack([np.repeat(np.arange(4), s) for s in vecs])
    got = sup.hafnian_batch(A, idx, cpu=True)
    gotl = sup.hafnian_batch(A, idx, mu=mu, loop=True, cpu=True)
    terms = sup.hafnian_plan(idx)
    for k, s in enumerate(vecs):
        t, tl = rec_haf(E, idx[k]), rec_haf(E, idx[k], Emu)
        assert err(got[k], t) < 0.5 and err(gotl[k], tl) < 0.5, (s, got[k], t, gotl[k], tl)
        assert got[k] == complex(*t), s  # every operation of the plain form is exact here
        assert terms[k] == layout([x for x in s if x])[0]
        # the repeated form names the same gather: the same bits
        assert bits(sup.hafnian_repeated(A, s, cpu=True)).tolist() == bits(got[k]).tolist()
        assert bits(sup.hafnian_repeated(A, s, mu=mu, loop=True, cpu=True)).tolist() == bits(gotl[k]).tolist()


def test_permuting_idx_within_the_groups_keeps_the_bits(sup):
    rng = np.random.default_rng(5)
    A = rng.standard_normal((7, 7)) + 1j * rng.standard_normal((7, 7))
    A = A + A.T
    mu = rng.standard_normal(7) + 1j * rng.standard_normal(7)
    base = np.repeat([5, 2, 6, 0], [4, 3, 3, 2])
    perms = [base]
    while len(perms) < 6:
        p = rng.permutation(base)
        if list(dict.fromkeys(p.tolist())) == [5, 2, 6, 0]:  # the order of first appearance orders the digits
            perms.append(p)
    assert any(not np.array_equal(p, base) for p in perms)
    for loop in (False, True):
        v = sup.hafnian_batch(A, np.stack(perms), mu=mu, loop=loop, cpu=True)
        assert len({tuple(bits(x).tolist()) for x in v}) == 1


# ---- 4. large orders by the rank-one closed form ---------------------------------

def cfrac(z):
    return (Fraction(float(z.real)), Fraction(float(z.imag)))


RANK_ONE = [(64, (16, 16, 16, 16), False), (24, (4,) * 6, False), (24, (4,) * 6, True), (17, (5, 4, 4, 4), True),
            (63, (16, 16, 16, 15), True)]


def rank_one_haf_case(n, mult, loop, seed):
    """A = u u^T: haf = (n-1)!! prod u_idx; with mu = c u, lhaf = prod u_idx
    sum_j n! / (2^j j! (n-2j)!) c^(n-2j).  u: dyadic phases; c = (2 + i) / 4."""
    rng = np.random.default_rng(seed)
    K = len(mult)
    u = dyadic_phases(rng, K)
    c = (2 + 1j) / 4
    A, mu = np.outer(u, u), c * u
    idx = np.repeat(np.arange(K), mult)
    rng.shuffle(idx[1:])  # group 0 appears first; the others in any order
    prod = (Fraction(1), Fraction(0))
    for i in idx:
        prod = cmul(prod, cfrac(u[i]))
    if loop:
        s = (Fraction(0), Fraction(0))
        for j in range(n // 2 + 1):
            coef = Fraction(math.factorial(n), 2 ** j * math.factorial(j) * math.factorial(n - 2 * j))
            p = cpow(cfrac(c), n - 2 * j)
            s = cadd(s, (coef * p[0], coef * p[1]))
        truth = cmul(prod, s)
    else:
        dfact = math.prod(range(n - 1, 0, -2))
        truth = (dfact * prod[0], dfact * prod[1])
    return A, mu, u, idx, truth


def rank_one_scale(n, idx, u, mu, loop):
    """S = 2 sum |w| |term| (/ m!) of the rank-one case, from numpy."""
    m = n // 2
    gm = groups(idx)
    V, w = kan_states(gm)
    wf = np.abs(np.array([float(x) for x in w]))
    vals = list(dict.fromkeys(idx.tolist()))
    h = np.array(gm)[None, :] / 2 - V
    qh = np.abs(h @ u[vals]) ** 2 / 2  # |q / 2|, q = (h . u)^2
    if loop:
        r = np.abs(h @ mu[vals])
        return 2 * float(np.sum(wf * sum(qh ** j / math.factorial(j) * r ** (n - 2 * j) / math.factorial(n - 2 * j)
                                         for j in range(m + 1))))
    return 2 * float(np.sum(wf * qh ** m)) / math.factorial(m)


def rank_one_bound(n, Tw, K, loop):
    """error / S <= 2^-52 (m or n) (Tw + K), plus 2^-52 (n + 2) for the loop
    form's rounded coefficients 1 / (j! (n-2j)!) (one rounding each, n for the
    factorials)."""
    return 2.0 ** -52 * ((n if loop else n // 2) * (Tw + K) + ((n + 2) if loop else 0))


@pytest.mark.parametrize("n,mult,loop", RANK_ONE)
def test_rank_one_closed_form(sup, n, mult, loop):
    A, mu, u, idx, truth = rank_one_haf_case(n, mult, loop, 600 + n)
    v, st = sup.hafnian_batch(A, idx, mu=mu, loop=loop, cpu=True, return_stats=True)
    T, Tw, H, K = walk_shape(idx)
    assert st["visited_steps"] == T == sup.hafnian_plan(idx)
    S = rank_one_scale(n, idx, u, mu, loop)
    e = err(v, truth) / S
    bound = rank_one_bound(n, Tw, K, loop)
    print(f"n={n} mult={mult} loop={loop} T={T} Tw={Tw} H={H} e={e:.3e} bound={bound:.3e} "
          f"S/|truth|={S / err(0j, truth):.1f}")
    assert e <= bound


# ---- 5. the project's own truth ---------------------------------------------------

@pytest.mark.parametrize("n", [8, 11])
def test_bipartite_block_matrix_is_the_exact_permanent(sup, n):
    B = gauss_int_case(n, 900 + n)
    Z = np.zeros((n, n))
    A = np.block([[Z, B], [B.T, Z]])
    v = sup.hafnian(A, cpu=True)
    assert (round(v.real), round(v.imag)) == sup.perman_complex_exact(B, cpu=True)
    assert abs(v.real - round(v.real)) < 0.5 and abs(v.imag - round(v.imag)) < 0.5


# ---- 6. plan ----------------------------------------------------------------------

def test_plan_is_the_layout_rule(sup):
    rng = np.random.default_rng(12)
    idx = rng.integers(0, 5, (40, 10))
    idx[::3] = rng.integers(0, 30, (14, 10))
    terms = sup.hafnian_plan(idx)
    want = [layout(groups(idx[k]))[0] for k in range(40)]
    assert terms.tolist() == want
    assert sup.hafnian_plan(idx[7]) == want[7]
    assert sup.hafnian_plan(np.arange(24) // 4) == 12500  # six groups of four
    assert sup.hafnian_plan(np.arange(9)) == 2 ** 8
    A = sym_dyadic(30, 3)
    for loop in (False, True):
        _, st = sup.hafnian_batch(A, idx, loop=loop, cpu=True, return_stats=True)
        assert st["visited_steps"] == sum(want) and st["leaves"] == 40 and st["gray_steps"] == 40 << 9
        assert st["est_ops_per_step"] > 0
    lib = sup._lib.load()
    i32 = idx.astype(np.int32)
    assert lib.sup_hafnian_complex_plan(i32.ctypes.data, 10, 40, None) == 0
    assert lib.sup_hafnian_complex_plan(None, 10, 40, None) == -1
    assert lib.sup_hafnian_complex_plan(i32.ctypes.data, 65, 1, None) == -1
    assert lib.sup_hafnian_complex_plan(i32.ctypes.data, 0, 1, None) == -1


# ---- 7. errors --------------------------------------------------------------------

def test_errors_name_the_place(sup):
    A = sym_dyadic(6, 8)
    mu = np.diag(A).copy()
    bad = A.copy()
    bad[4, 2] = np.nextafter(bad[4, 2].real, 9.0) + 1j * bad[4, 2].imag
    for loop, name in ((False, "sup_hafnian_complex"), (True, "sup_loop_hafnian_complex")):
        with pytest.raises(sup.SupError, match=rf"{name}: A\[2\]\[4\] and A\[4\]\[2\] differ.*symmetric") as e:
            sup.hafnian_batch(bad, [0, 1], loop=loop, cpu=True)  # the pair is checked even when no list touches it
        assert e.value.code == -1
        with pytest.raises(sup.SupError, match=rf"{name}: idx\[k = 1\]\[position 2\] = 6 outside \[0, 6\)") as e:
            sup.hafnian_batch(A, [[0, 1, 2, 3], [0, 1, 6, 3]], loop=loop, cpu=True)
        assert e.value.code == -1
        with pytest.raises(sup.SupError, match=r"position 0\] = -1 outside") as e:
            sup.hafnian_batch(A, [-1, 1], loop=loop, cpu=True)
        assert e.value.code == -1
    # -0.0 against +0.0 is an asymmetric pair: bit for bit
    z = np.zeros((2, 2), dtype=np.complex128)
    z[0, 1] = complex(-0.0, 0.0)
    with pytest.raises(sup.SupError, match="symmetric"):
        sup.hafnian(z, cpu=True)
    with pytest.raises(ValueError, match=r"n = 65 outside \[1, 64\]"):
        sup.hafnian_batch(A, np.zeros(65, dtype=int), cpu=True)
    with pytest.raises(ValueError, match="mu must have shape"):
        sup.loop_hafnian(A, mu=mu[:3], cpu=True)
    with pytest.raises(ValueError, match="rpt"):
        sup.hafnian_repeated(A, [1, 1], cpu=True)
    # the C ABI itself: n outside [1, 64] and null pointers
    lib = sup._lib.load()
    a = np.ascontiguousarray(A)
    ix = np.zeros(65, np.int32)
    out = np.zeros(2)
    for n in (0, 65):
        assert lib.sup_hafnian_complex(a.ctypes.data, 6, ix.ctypes.data, n, 1, None, 1, out.ctypes.data, None) == -1
        assert f"n = {n} outside [1, 64]" in lib.sup_last_error().decode()
        assert lib.sup_loop_hafnian_complex(a.ctypes.data, 6, mu.ctypes.data, ix.ctypes.data, n, 1, None, 1,
                                            out.ctypes.data, None) == -1
    for args in ((None, 6, ix.ctypes.data, 2, 1, None, 1, out.ctypes.data, None),
                 (a.ctypes.data, 6, None, 2, 1, None, 1, out.ctypes.data, None),
                 (a.ctypes.data, 6, ix.ctypes.data, 2, 1, None, 1, None, None)):
        assert lib.sup_hafnian_complex(*args) == -1
        assert "sup_hafnian_complex: null pointer" in lib.sup_last_error().decode()
    assert lib.sup_loop_hafnian_complex(a.ctypes.data, 6, None, ix.ctypes.data, 2, 1, None, 1, out.ctypes.data,
                                        None) == -1
    assert "sup_loop_hafnian_complex: null pointer" in lib.sup_last_error().decode()
    assert lib.sup_hafnian_complex(a.ctypes.data, 0, ix.ctypes.data, 2, 1, None, 1, out.ctypes.data, None) == -1


def test_too_many_chunks_is_refused_before_any_work(sup):
    """42 distinct indices: T = 2^41, Tw = 2^10, H = 2^31, 2^25 wave-chunks."""
    A = np.ones((42, 42), dtype=np.complex128)
    for loop in (False, True):
        with pytest.raises(sup.SupError, match="matrix k = 1 has 2199023255552 terms") as e:
            sup.hafnian_batch(A, [[0] * 42, list(range(42))], loop=loop, cpu=True)
        assert e.value.code == -7
    assert sup.hafnian_plan(np.arange(42)) == 2 ** 41  # the plan entry still answers


def test_no_device_is_an_error_not_a_cpu_fallback(sup):
    A = sym_dyadic(6, 9)
    idx = np.random.default_rng(1).integers(0, 6, (4, 6))
    if sup.device_count() == 0:
        for loop in (False, True):
            with pytest.raises(sup.SupError) as e:
                sup.hafnian_batch(A, idx, loop=loop)
            assert e.value.code == -2
    else:  # a box with a device: the device walk, the host twin's bits
        assert np.array_equal(bits(sup.hafnian_batch(A, idx)), bits(sup.hafnian_batch(A, idx, cpu=True)))


# ---- 8. batches ---------------------------------------------------------------------

def hetero_lists(n, count, seed, M=12):
    """count index lists of order n with different collision patterns."""
    rng = np.random.default_rng(seed)
    idx = np.zeros((count, n), dtype=np.int64)
    for k in range(count):
        idx[k] = rng.integers(0, (2, 3, 5, M, 1)[k % 5], n)
    return idx


@pytest.mark.parametrize("n", [6, 9, 14])
def test_batch_result_is_the_single_call(sup, n):
    rng = np.random.default_rng(n)
    A = rng.standard_normal((12, 12)) + 1j * rng.standard_normal((12, 12))
    A = A + A.T
    mu = rng.standard_normal(12) + 1j * rng.standard_normal(12)
    idx = hetero_lists(n, 65, 400 + n)
    assert len(set(sup.hafnian_plan(idx).tolist())) >= 6  # heterogeneous: many different sums in one call
    for loop in (False, True):
        if n % 2 and not loop:
            continue
        one = np.array([sup.hafnian_batch(A, idx[k], mu=mu, loop=loop, cpu=True, threads=1) for k in range(65)])
        for threads in (1, 16):
            v = sup.hafnian_batch(A, idx, mu=mu, loop=loop, cpu=True, threads=threads)
            assert np.array_equal(bits(v), bits(one))
    assert isinstance(sup.hafnian_batch(A, idx[0], cpu=True), complex)
    assert sup.hafnian_batch(A, np.zeros((0, n), dtype=int), cpu=True).shape == (0,)


# ---- 9. the CLI -----------------------------------------------------------------------

def run_cli(sup, *args):
    return subprocess.run([sup._lib.PERMAN_BIN, *args], capture_output=True, text=True, timeout=120)


def test_cli_hafnian_on_host_threads(sup, tmp_path):
    """--hafnian [--loop] [--rpt ...] -c on a symmetric MatrixMarket file: the
    library's own bits, in --complex's line shape."""
    A = sym_dyadic(5, 21)
    path = tmp_path / "h5.mtx"
    with open(path, "w") as f:
        f.write("%%MatrixMarket matrix coordinate complex symmetric\n5 5 15\n")
        for i in range(5):
            for j in range(i + 1):
                f.write(f"{i + 1} {j + 1} {float(A[i, j].real)!r} {float(A[i, j].imag)!r}\n")
    for extra, want in (((), sup.hafnian(A[:4, :4], cpu=True)),
                        (("--rpt", "1,1,1,1,0"), sup.hafnian(A[:4, :4], cpu=True)),
                        (("--rpt", "2,0,3,0,1"), sup.hafnian_repeated(A, [2, 0, 3, 0, 1], cpu=True)),
                        (("--loop",), sup.loop_hafnian(A, cpu=True)),
                        (("--loop", "--rpt", "0,2,1"), sup.hafnian_repeated(A, [0, 2, 1, 0, 0], loop=True, cpu=True))):
        if not extra:
            extra = ("--rpt", "1,1,1,1")
        r = run_cli(sup, "-f", str(path), "--hafnian", "-c", *extra)
        assert r.returncode == 0, r.stderr
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("Hafnian: ")]
        assert len(line) == 1 and ("cpu_loop_hafnian64_complex" if "--loop" in extra else "cpu_hafnian64_complex") in r.stdout
        re_, im_ = (float(x) for x in line[0].split()[1:])
        assert complex(re_, im_) == want, (extra, line, want)
    r = run_cli(sup, "-f", str(path), "--hafnian", "-c")  # the whole 5 x 5 matrix: odd n
    assert r.returncode == 0 and "Hafnian: 0.00000000000000000e+00 0.00000000000000000e+00" in r.stdout
    for bad, msg in ((("--hafnian", "--complex"), "--hafnian does not combine with --complex"),
                     (("--hafnian", "-s"), "--hafnian does not combine with -s"),
                     (("--loop",), "--loop and --rpt go with --hafnian"),
                     (("--hafnian", "--rpt", "1,x"), "--rpt takes"),
                     (("--hafnian", "--rpt", "1,1,1,1,1,1"), "--rpt takes")):
        r = run_cli(sup, "-f", str(path), "-c", *bad)
        assert r.returncode == 1 and msg in r.stderr, (bad, r.stderr)
