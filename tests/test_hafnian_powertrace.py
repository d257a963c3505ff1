"""Power-trace hafnians and loop hafnians on host threads (hafnian_pt.cpp, the
host twin of walk_hafpt.hip, through hafnian_powertrace_batch(cpu=True)), the
range entry and the plan entry.

Truth is the recursive definition in Python integers or Fractions, restated
here; the yardstick for the rounding error is a numpy complex128 restatement
of the same sum that uses `@` for every product.  With S = sum_z |f(z)|,
    error / S <= 8 max(e_np, n 2^-52)
where e_np is the restatement's own error / S on the same case: the factor 8
covers the differing summation orders and fused against unfused products, the
floor is one rounding per power step.  Every figure is printed.
"""
import itertools
import math
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from test_complex_batch import bits
from test_hafnian import kan_states, sym_dyadic, sym_gauss_int, walk_shape

EPS = 2.0 ** -52


# ---- exact truth: the recursive definition --------------------------------------------

def cmul(a, b):
    return (a[0] * b[0] - a[1] * b[1], a[0] * b[1] + a[1] * b[0])


def rec_haf(E, idx, mu=None):
    """The first index pairs with one of the others, or (loop form) with itself
    through mu; E and mu hold exact (re, im) pairs."""
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
            t = cmul(E[ix[0]][ix[j]], go(ix[1:j] + ix[j + 1:]))
            s = (s[0] + t[0], s[1] + t[1])
        memo[ix] = s
        return s

    return go(tuple(int(i) for i in idx))


def exact(A, den=1):
    a = np.atleast_2d(A)
    out = [[(Fraction(int(round(z.real * den)), den), Fraction(int(round(z.imag * den)), den)) for z in row] for row in a]
    assert all(complex(float(p[0]), float(p[1])) == z for row, zr in zip(out, a) for p, z in zip(row, zr))
    return out


def err(v, truth):
    dr, di = Fraction(v.real) - truth[0], Fraction(v.imag) - truth[1]
    return float(dr * dr + di * di) ** 0.5


# ---- the numpy restatement -------------------------------------------------------------

def padded(A, idx, mu):
    """(N, d, m): the gather, padded by one virtual index (zero row and column,
    d = 1) when the order is odd."""
    idx = np.asarray(idx)
    N = np.asarray(A, dtype=np.complex128)[np.ix_(idx, idx)]
    d = None if mu is None else np.asarray(mu, dtype=np.complex128)[idx]
    n = len(idx)
    if n % 2:
        N = np.pad(N, ((0, 1), (0, 1)))
        d = np.append(d, 1.0)
    return N, d, (n + 1) // 2


def np_f(N, d, m, z):
    rows = [r for b in range(m) if (z >> b) & 1 for r in (2 * b, 2 * b + 1)]
    swap = [r ^ 1 for r in rows]
    Cm = N[np.ix_(rows, swap)]
    P = np.eye(len(rows), dtype=np.complex128)
    c = [0j] * (m + 1)
    y = None if d is None else d[rows]
    for j in range(1, m + 1):
        P = P @ Cm
        c[j] = np.trace(P) / (2 * j)
        if d is not None:
            c[j] += (d[swap] @ y) / 2
            y = Cm @ y
    g = [1 + 0j]
    for s in range(1, m + 1):
        g.append(sum(j * c[j] * g[s - j] for j in range(1, s + 1)) / s)
    return g[m]


def np_sum(A, idx, mu, z0=1, z1=None):
    """(sum over z in [z0, z1) of the signed f(z), S = sum |f(z)|)."""
    N, d, m = padded(A, idx, mu)
    z1 = 2 ** m if z1 is None else z1
    f = np.array([(-1) ** (m - bin(z).count("1")) * np_f(N, d, m, z) for z in range(max(1, z0), z1)])
    return complex(f.sum()), float(np.abs(f).sum())


def measured(sup, A, idx, mu, truth, tag):
    """Asserts the entry's error against truth within 8 max(e_np, n 2^-52) S and
    returns (e, e_np)."""
    n = len(idx)
    loop = mu is not None
    v_np, S = np_sum(A, idx, mu)
    v = sup.hafnian_powertrace_batch(A, idx, mu=mu, loop=loop, cpu=True)
    e, e_np = err(v, truth) / S, err(v_np, truth) / S
    bound = 8 * max(e_np, n * EPS)
    print(f"{tag} n={n} loop={loop} e={e:.3e} e_np={e_np:.3e} bound={bound:.3e} S/|v|={S / max(abs(v), 1e-300):.1f}")
    assert e <= bound
    return e, e_np


# ---- 1. exact truth ---------------------------------------------------------------------

@pytest.mark.parametrize("n", range(2, 13))
def test_gaussian_integers_against_the_recursive_definition(sup, n):
    A = sym_gauss_int(n, 500 + n)
    mu = np.diag(sym_gauss_int(n, 600 + n)).copy()
    E, Emu = exact(A), exact(mu[None, :])[0]
    idx = np.arange(n)
    if n % 2 == 0:
        measured(sup, A, idx, None, rec_haf(E, idx), "gauss")
    else:
        v, st = sup.hafnian_powertrace(A, cpu=True, return_stats=True)
        assert bits(v).tolist() == [0, 0] and st["visited_steps"] == 0  # plain form, odd n: exactly +0
    if n % 2 == 0 or n in (3, 5, 9, 11):
        measured(sup, A, idx, mu, rec_haf(E, idx, Emu), "gauss")


@pytest.mark.parametrize("n", range(2, 11))
def test_dyadic_against_the_recursive_definition(sup, n):
    den = 2 ** 10
    A = sym_dyadic(n, 700 + n)
    mu = np.diag(sym_dyadic(n, 800 + n)).copy()
    E, Emu = exact(A, den), exact(mu[None, :], den)[0]
    idx = np.arange(n)
    if n % 2 == 0:
        measured(sup, A, idx, None, rec_haf(E, idx), "dyadic")
    measured(sup, A, idx, mu, rec_haf(E, idx, Emu), "dyadic")


# ---- 2. against the Kan entries ---------------------------------------------------------

def kan_scale(A, idx, mu, loop):
    """(S, bound) of hafnian_batch on this list: the scale and the relative
    bound of test_hafnian.test_random_dyadic_error_over_scale."""
    idx = [int(i) for i in idx]
    n, m = len(idx), len(idx) // 2
    vals = list(dict.fromkeys(idx))
    mult = [idx.count(v) for v in vals]
    V, w = kan_states(mult)
    h = np.array(mult)[None, :] / 2 - V
    qh = np.einsum("tk,kl,tl->t", h, np.asarray(A)[np.ix_(vals, vals)] / 2, h)
    wf = np.abs(np.array([float(x) for x in w]))
    if loop:
        r = h @ np.asarray(mu)[vals]
        terms = [np.abs(qh) ** j / math.factorial(j) * np.abs(r) ** (n - 2 * j) / math.factorial(n - 2 * j)
                 for j in range(m + 1)]
        S = 2 * float(np.sum(wf * np.sum(terms, axis=0)))
    else:
        S = 2 * float(np.sum(wf * np.abs(qh) ** m)) / math.factorial(m)
    T, Tw, H, K = walk_shape(np.array(idx))
    return S, EPS * (n if loop else m) * (Tw + K)


def agree_with_kan(sup, A, idx, mu, loop, tag):
    """The two algorithms on identical arguments: within the sum of their own
    bounds, each on its own scale (the power-trace bound at its floor)."""
    n = len(idx)
    a = sup.hafnian_batch(A, idx, mu=mu, loop=loop, cpu=True)
    b = sup.hafnian_powertrace_batch(A, idx, mu=mu, loop=loop, cpu=True)
    if n % 2 and not loop:
        assert a == 0 and b == 0
        return
    mu_ = np.diag(A) if (loop and mu is None) else mu
    S_pt = np_sum(A, idx, mu_ if loop else None)[1]
    S_kan, b_kan = kan_scale(A, idx, mu_, loop)
    tol = 8 * n * EPS * S_pt + b_kan * S_kan
    print(f"{tag} n={n} loop={loop} |pt - kan|={abs(a - b):.3e} tol={tol:.3e} |v|={abs(a):.3e}")
    assert abs(a - b) <= tol


@pytest.mark.parametrize("n", range(2, 17))
def test_distinct_lists_agree_with_the_kan_walk(sup, n):
    rng = np.random.default_rng(900 + n)
    A = rng.standard_normal((20, 20)) + 1j * rng.standard_normal((20, 20))
    A = A + A.T
    mu = rng.standard_normal(20) + 1j * rng.standard_normal(20)
    idx = rng.choice(20, n, replace=False)
    agree_with_kan(sup, A, idx, None, False, "distinct")
    agree_with_kan(sup, A, idx, mu, True, "distinct")
    agree_with_kan(sup, A, idx, None, True, "distinct default mu")


def mult_vectors(total, modes):
    return [s for s in itertools.product(range(total + 1), repeat=modes) if sum(s) == total]


def test_lists_with_repeats_agree_with_the_kan_walk(sup):
    rng = np.random.default_rng(77)
    A = rng.standard_normal((4, 4)) + 1j * rng.standard_normal((4, 4))
    A = A + A.T
    mu = rng.standard_normal(4) + 1j * rng.standard_normal(4)
    vecs = mult_vectors(6, 3)
    assert len(vecs) == 28
    for s in vecs + [(4, 4, 4, 4)]:
        idx = np.repeat(np.arange(len(s)), s)
        agree_with_kan(sup, A, idx, None, False, f"repeats {s}")
        agree_with_kan(sup, A, idx, mu, True, f"repeats {s}")


@pytest.mark.parametrize("n", [6, 9, 12])
def test_batch_is_the_single_call_on_any_thread_count(sup, n):
    rng = np.random.default_rng(n)
    A = rng.standard_normal((12, 12)) + 1j * rng.standard_normal((12, 12))
    A = A + A.T
    mu = rng.standard_normal(12) + 1j * rng.standard_normal(12)
    idx = rng.integers(0, 12, (65, n))
    for loop in (False, True):
        one = np.array([sup.hafnian_powertrace_batch(A, idx[k], mu=mu, loop=loop, cpu=True, threads=1)
                        for k in range(65)])
        for threads in (1, 16):
            v, st = sup.hafnian_powertrace_batch(A, idx, mu=mu, loop=loop, cpu=True, threads=threads,
                                                 return_stats=True)
            assert np.array_equal(bits(v), bits(one))
            sub = 0 if (n % 2 and not loop) else 2 ** ((n + 1) // 2) - 1
            assert st["leaves"] == 65 and st["visited_steps"] == 65 * sub and st["gray_steps"] == 65 * 2 ** (n - 1)
    assert isinstance(sup.hafnian_powertrace_batch(A, idx[0], cpu=True), complex)
    assert sup.hafnian_powertrace_batch(A, np.zeros((0, n), dtype=int), cpu=True).shape == (0,)
    # one wide matrix on 1 and 16 threads: the subsets are shared, the bits stay
    w = rng.choice(12, 12, replace=False)
    assert bits(sup.hafnian_powertrace_batch(A, w, cpu=True, threads=1)).tolist() == \
        bits(sup.hafnian_powertrace_batch(A, w, cpu=True, threads=16)).tolist()


# ---- 3. closed forms ---------------------------------------------------------------------

@pytest.mark.parametrize("n", [8, 12, 16])
def test_all_ones_closed_forms(sup, n):
    """haf J_n = (n-1)!!; lhaf J_n with d = 1 = the number of involutions.  To
    the measured bound, not ==: the 1 / s table is not exact."""
    J = np.ones((n, n), dtype=np.complex128)
    one = np.ones(n, dtype=np.complex128)
    idx = np.arange(n)
    dfact = math.prod(range(n - 1, 0, -2))
    inv = [1, 1]
    for k in range(2, n + 1):
        inv.append(inv[-1] + (k - 1) * inv[-2])
    measured(sup, J, idx, None, (Fraction(dfact), Fraction(0)), "ones")
    measured(sup, J, idx, one, (Fraction(inv[n]), Fraction(0)), "ones")


# ---- 4. the range entry -------------------------------------------------------------------

def cxadd(a, b):
    return complex(a.real + b.real, a.imag + b.imag)


def tree(parts):
    """The pairwise tree over the index (an odd last element moves up as it is)."""
    parts = list(parts)
    while len(parts) > 1:
        parts = [cxadd(parts[i], parts[i + 1]) if i + 1 < len(parts) else parts[i] for i in range(0, len(parts), 2)]
    return parts[0]


@pytest.mark.parametrize("loop", [False, True])
def test_ranges_fold_to_the_whole_result(sup, loop):
    """n = 12 (m = 6, one subset per wave-chunk): the whole range has the batch
    entry's bits; aligned power-of-two cuts added pairwise reproduce them; at
    any cut the single subsets' partials folded by the tree do, and the two
    pieces' plain sum agrees to rounding."""
    A = sym_dyadic(12, 31)
    mu = np.diag(sym_dyadic(12, 32)).copy() if loop else None
    idx = np.arange(12)
    kw = dict(mu=mu, loop=loop, cpu=True)
    whole = sup.hafnian_powertrace_batch(A, idx, **kw)
    full, st = sup.hafnian_powertrace_range(A, idx, 0, 64, return_stats=True, **kw)
    assert bits(full).tolist() == bits(whole).tolist() and st["visited_steps"] == 63
    for cuts in ([0, 32, 64], [0, 16, 32, 48, 64], list(range(0, 65, 8))):
        parts = [sup.hafnian_powertrace_range(A, idx, a, b, **kw) for a, b in zip(cuts, cuts[1:])]
        assert bits(tree(parts)).tolist() == bits(whole).tolist(), cuts
    single = [sup.hafnian_powertrace_range(A, idx, z, z + 1, **kw) for z in range(64)]
    assert single[0] == 0  # z = 0 is no subset
    assert bits(tree(single)).tolist() == bits(whole).tolist()
    S = np_sum(A, idx, mu)[1]
    for cut in (1, 7, 21, 37, 63):
        a, b = sup.hafnian_powertrace_range(A, idx, 0, cut, **kw), sup.hafnian_powertrace_range(A, idx, cut, 64, **kw)
        assert bits(a).tolist() == bits(tree(single[:cut])).tolist()
        assert bits(b).tolist() == bits(tree(single[cut:])).tolist()
        assert abs(cxadd(a, b) - whole) <= 8 * 12 * EPS * S
    assert sup.hafnian_powertrace_range(A, idx, 5, 5, **kw) == 0


N64 = [((1 << 32) - 64, 1 << 32), (1, 65)]


@pytest.mark.parametrize("loop", [False, True])
def test_order_64_ranges_match_the_restatement(sup, loop):
    """n = 64: 2^14 subsets per wave-chunk, so each range lies inside one chunk
    and its result is the ascending sum of its signed f(z)."""
    rng = np.random.default_rng(64)
    A = (rng.standard_normal((64, 64)) + 1j * rng.standard_normal((64, 64))) / 8
    A = A + A.T
    mu = (rng.standard_normal(64) + 1j * rng.standard_normal(64)) if loop else None
    idx = np.arange(64)
    for z0, z1 in N64:
        v, st = sup.hafnian_powertrace_range(A, idx, z0, z1, mu=mu, loop=loop, cpu=True, return_stats=True)
        v_np, S = np_sum(A, idx, mu, z0, z1)
        print(f"n=64 loop={loop} z in [{z0}, {z1}): |v - v_np| / S = {abs(v - v_np) / S:.3e}")
        assert abs(v - v_np) <= 8 * 64 * EPS * S
        assert st["visited_steps"] == z1 - z0
        assert bits(v).tolist() == bits(sup.hafnian_powertrace_range(A, idx, z0, z1, mu=mu, loop=loop, cpu=True,
                                                                     threads=1)).tolist()


# ---- 5. errors, plan, CLI ------------------------------------------------------------------

def test_errors_name_the_place(sup):
    A = sym_dyadic(6, 8)
    mu = np.diag(A).copy()
    bad = A.copy()
    bad[4, 2] = np.nextafter(bad[4, 2].real, 9.0) + 1j * bad[4, 2].imag
    for loop, name in ((False, "sup_hafnian_complex_pt"), (True, "sup_loop_hafnian_complex_pt")):
        with pytest.raises(sup.SupError, match=rf"{name}: A\[2\]\[4\] and A\[4\]\[2\] differ.*symmetric") as e:
            sup.hafnian_powertrace_batch(bad, [0, 1], loop=loop, cpu=True)
        assert e.value.code == -1
        with pytest.raises(sup.SupError, match=rf"{name}: idx\[k = 1\]\[position 2\] = 6 outside \[0, 6\)") as e:
            sup.hafnian_powertrace_batch(A, [[0, 1, 2, 3], [0, 1, 6, 3]], loop=loop, cpu=True)
        assert e.value.code == -1
        with pytest.raises(sup.SupError, match=r"position 0\] = -1 outside") as e:
            sup.hafnian_powertrace_batch(A, [-1, 1], loop=loop, cpu=True)
        assert e.value.code == -1
    with pytest.raises(ValueError, match=r"n = 65 outside \[1, 64\]"):
        sup.hafnian_powertrace_batch(A, np.zeros(65, dtype=int), cpu=True)
    with pytest.raises(ValueError, match="mu must have shape"):
        sup.loop_hafnian_powertrace(A, mu=mu[:3], cpu=True)
    # the range entry: m = 3 for n = 6
    for z0, z1 in ((5, 4), (0, 9)):
        with pytest.raises(sup.SupError, match=r"sup_hafnian_complex_pt_range: subsets \[%d, %d\) outside" % (z0, z1)) as e:
            sup.hafnian_powertrace_range(A, np.arange(6), z0, z1, cpu=True)
        assert e.value.code == -1
    with pytest.raises(sup.SupError, match=r"sup_hafnian_complex_pt_range: idx\[k = 0\]\[position 1\] = 9 outside"):
        sup.hafnian_powertrace_range(A, [0, 9], 0, 2, cpu=True)
    # the C ABI itself: n outside [1, 64] and null pointers
    lib = sup._lib.load()
    a = np.ascontiguousarray(A)
    ix = np.zeros(65, np.int32)
    out = np.zeros(2)
    for n in (0, 65):
        assert lib.sup_hafnian_complex_pt(a.ctypes.data, 6, ix.ctypes.data, n, 1, None, 1, out.ctypes.data, None) == -1
        assert f"n = {n} outside [1, 64]" in lib.sup_last_error().decode()
        assert lib.sup_loop_hafnian_complex_pt(a.ctypes.data, 6, mu.ctypes.data, ix.ctypes.data, n, 1, None, 1,
                                               out.ctypes.data, None) == -1
        assert lib.sup_hafnian_complex_pt_range(a.ctypes.data, 6, None, ix.ctypes.data, n, 0, 1, None, 1,
                                                out.ctypes.data, None) == -1
        assert lib.sup_hafnian_complex_pt_plan(n, 0, None, None) == -1
    for args in ((None, 6, ix.ctypes.data, 2, 1, None, 1, out.ctypes.data, None),
                 (a.ctypes.data, 6, None, 2, 1, None, 1, out.ctypes.data, None),
                 (a.ctypes.data, 6, ix.ctypes.data, 2, 1, None, 1, None, None)):
        assert lib.sup_hafnian_complex_pt(*args) == -1
        assert "sup_hafnian_complex_pt: null pointer" in lib.sup_last_error().decode()
    assert lib.sup_loop_hafnian_complex_pt(a.ctypes.data, 6, None, ix.ctypes.data, 2, 1, None, 1, out.ctypes.data,
                                           None) == -1
    assert "sup_loop_hafnian_complex_pt: null pointer" in lib.sup_last_error().decode()
    assert lib.sup_hafnian_complex_pt_range(a.ctypes.data, 6, None, ix.ctypes.data, 2, 0, 1, None, 1, None, None) == -1
    assert "sup_hafnian_complex_pt_range: null pointer" in lib.sup_last_error().decode()
    assert lib.sup_hafnian_complex_pt(a.ctypes.data, 0, ix.ctypes.data, 2, 1, None, 1, out.ctypes.data, None) == -1


def test_device_cap_and_no_device(sup):
    """Above the cap the device path is refused on any machine; with no device
    the device path is an error, never a CPU fallback."""
    cap = sup.HAFNIAN_PT_MAX_DEVICE_N
    assert 50 <= cap <= 64
    A = np.ones((64, 64), dtype=np.complex128)
    if cap < 64:
        for loop in (False, True):
            with pytest.raises(sup.SupError, match=f"above the device cap SUP_HAFNIAN_PT_MAX_DEVICE_N = {cap}") as e:
                sup.hafnian_powertrace_range(A, np.arange(cap + 1), 1, 2, loop=loop)
            assert e.value.code == -7
    B = sym_dyadic(6, 9)
    idx = np.random.default_rng(1).integers(0, 6, (4, 6))
    if sup.device_count() == 0:
        for loop in (False, True):
            with pytest.raises(sup.SupError) as e:
                sup.hafnian_powertrace_batch(B, idx, loop=loop)
            assert e.value.code == -2
    else:
        assert np.array_equal(bits(sup.hafnian_powertrace_batch(B, idx)),
                              bits(sup.hafnian_powertrace_batch(B, idx, cpu=True)))


def census(m, loop):
    """hafpt.hpp hafpt_ops restated."""
    def one(k):
        R, A = 2.0 * k, (m + 1) // 2
        ops = 8 * R ** 3 * (A - 1) + (m - 1) * (8 * R * R + 2 * R) + 2 * R
        if loop:
            ops += (m - 1) * 8 * R * R + m * 8 * R
        return ops + 4 * m * (m + 1) + 6 * m
    w = [math.comb(m, k) for k in range(1, m + 1)]
    return sum(c * one(k) for c, k in zip(w, range(1, m + 1))) / sum(w)


def test_plan(sup):
    for n in (1, 2, 7, 16, 50, 64):
        for loop in (False, True):
            subsets, ops = sup.hafnian_powertrace_plan(n, loop)
            m = (n + 1) // 2
            if n % 2 and not loop:
                assert (subsets, ops) == (0, 0.0)
            else:
                assert subsets == 2 ** m - 1
                assert ops == pytest.approx(census(m, loop), rel=1e-12)
    st = sup.hafnian_powertrace(np.ones((10, 10)), cpu=True, return_stats=True)[1]
    assert st["est_ops_per_step"] == sup.hafnian_powertrace_plan(10)[1]
    with pytest.raises(sup.SupError, match=r"n = 65 outside \[1, 64\]"):
        sup.hafnian_powertrace_plan(65)


def run_cli(sup, *args):
    return subprocess.run([sup._lib.PERMAN_BIN, *args], capture_output=True, text=True, timeout=120)


def test_cli_powertrace_on_host_threads(sup, tmp_path):
    A = sym_dyadic(5, 21)
    path = tmp_path / "h5.mtx"
    with open(path, "w") as f:
        f.write("%%MatrixMarket matrix coordinate complex symmetric\n5 5 15\n")
        for i in range(5):
            for j in range(i + 1):
                f.write(f"{i + 1} {j + 1} {float(A[i, j].real)!r} {float(A[i, j].imag)!r}\n")
    rep = lambda r: np.repeat(np.arange(5), r)  # noqa: E731
    for extra, want in ((("--rpt", "1,1,1,1"), sup.hafnian_powertrace(A[:4, :4], cpu=True)),
                        (("--rpt", "2,0,3,0,1"), sup.hafnian_powertrace_batch(A, rep([2, 0, 3, 0, 1]), cpu=True)),
                        (("--loop",), sup.loop_hafnian_powertrace(A, cpu=True)),
                        (("--loop", "--rpt", "0,2,1"),
                         sup.hafnian_powertrace_batch(A, rep([0, 2, 1, 0, 0]), loop=True, cpu=True))):
        r = run_cli(sup, "-f", str(path), "--hafnian", "--powertrace", "-c", *extra)
        assert r.returncode == 0, r.stderr
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("Hafnian: ")]
        name = ("cpu_loop_hafnian64_complex" if "--loop" in extra else "cpu_hafnian64_complex") + "_powertrace"
        assert len(line) == 1 and name in r.stdout
        re_, im_ = (float(x) for x in line[0].split()[1:])
        assert complex(re_, im_) == want, (extra, line, want)
    r = run_cli(sup, "-f", str(path), "--hafnian", "--powertrace", "-c")  # the whole 5 x 5 matrix: odd n
    assert r.returncode == 0 and "Hafnian: 0.00000000000000000e+00 0.00000000000000000e+00" in r.stdout
    r = run_cli(sup, "-f", str(path), "--powertrace", "-c")
    assert r.returncode == 1 and "--powertrace goes with --hafnian" in r.stderr
