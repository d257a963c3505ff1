"""Collision-aware complex permanents on host threads (cplx_fock.cpp, the host
twin of walk_cplxf.hip, through perman_complex_fock(cpu=True)) and the plan
entry perman_complex_fock_plan.

Matrix k is U[np.ix_(rows[k], cols[k])].  Truth is exact arithmetic on the
expanded matrix (test_complex.exact_perm) or, at orders no brute force
reaches, the rank-one closed form in Python fractions.
"""
import ctypes as C
import math
from fractions import Fraction

import numpy as np
import pytest

from test_complex import as_complex, err_over_scale, exact_perm, gauss_int_case, np_ryser
from test_complex_batch import bits


# ---- the layout rule, restated ---------------------------------

def groups(idx):
    """Multiplicities of the distinct values of idx, order of first appearance."""
    seen = {}
    for v in idx:
        seen[int(v)] = seen.get(int(v), 0) + 1
    return list(seen.values())


def layout(mult):
    """(T, Tw, H) of a multiplicity vector: one copy of the rarest group held
    (the first on a tie); digits = the groups with t' >= 1, radix t' + 1; walk
    digits = the longest prefix with Tw <= 2^10 that leaves H >= 64."""
    held = min(range(len(mult)), key=lambda k: (mult[k], k))
    radix = [t - (k == held) + 1 for k, t in enumerate(mult) if t - (k == held) >= 1]
    T = math.prod(radix)
    Tw, H = 1, T
    for r in radix:
        if Tw * r > 1024 or H // r < 64:
            break
        Tw, H = Tw * r, H // r
    return T, Tw, H


def plan(rows, cols):
    """(T, side, Tw, H): the side with fewer terms is collapsed, columns on a tie."""
    c, r = layout(groups(cols)), layout(groups(rows))
    return (r[0], 1, r[1], r[2]) if r[0] < c[0] else (c[0], 0, c[1], c[2])


def lists_with(rng, mult, universe):
    """A shuffled index list whose distinct values have multiplicities `mult`."""
    vals = rng.choice(universe, size=len(mult), replace=False)
    out = np.repeat(vals, mult)
    rng.shuffle(out)
    return out


# ---- plan -----------------------------------------------------------------------

PLAN_CASES = [
    # rows, cols, T, side
    ([0], [0], 1, 0),                                            # n = 1
    ([0, 1, 2, 3, 4], [4, 3, 2, 1, 0], 16, 0),                   # no repeats: 2^(n-1), a tie
    ([0, 1, 2, 3, 4, 5], [2, 2, 2, 2, 2, 2], 6, 0),              # all columns equal: T = n
    ([1, 1, 1, 2, 2, 2], [0, 1, 2, 3, 4, 5], 3 * 4, 1),          # rows more collapsed than columns
    ([1, 1, 2, 2, 3], [4, 4, 0, 0, 1], 3 * 3, 0),                # both repeat alike: a tie, columns
    ([0, 1, 2, 3, 4, 5, 6], [0, 0, 1, 1, 1, 2, 2], 2 * 4 * 3, 0),  # the smallest group (the first of two) is held
    ([3, 1, 3, 1, 3, 0, 0], [0, 1, 2, 3, 4, 5, 5], 4 * 2 * 3, 1),  # first appearance orders the groups
    ([0] * 24, sum(([k] * 4 for k in range(6)), []), 24, 1),     # 24 equal rows beat six groups of four
    (list(range(24)), sum(([k] * 4 for k in range(6)), []), 4 * 5 ** 5, 0),  # the issue's 12,500
]


@pytest.mark.parametrize("rows,cols,T,side", PLAN_CASES)
def test_plan_terms_and_side(sup, rows, cols, T, side):
    assert plan(rows, cols)[:2] == (T, side)  # the restatement agrees with the hand count
    assert sup.perman_complex_fock_plan(rows, cols) == (T, side)


def test_plan_batch_and_null_outputs(sup):
    rng = np.random.default_rng(3)
    rows = rng.integers(0, 5, (40, 9))
    cols = rng.integers(0, 4, (40, 9))
    terms, side = sup.perman_complex_fock_plan(rows, cols)
    want = [plan(rows[k], cols[k]) for k in range(40)]
    assert terms.tolist() == [w[0] for w in want] and side.tolist() == [w[1] for w in want]
    assert 0 in side and 1 in side
    lib = sup._lib.load()
    r32, c32 = rows.astype(np.int32), cols.astype(np.int32)
    t = np.zeros(40, np.uint64)
    s = np.zeros(40, np.int32)
    assert lib.sup_perman_complex_fock_plan(r32.ctypes.data, c32.ctypes.data, 9, 40, t.ctypes.data, None) == 0
    assert lib.sup_perman_complex_fock_plan(r32.ctypes.data, c32.ctypes.data, 9, 40, None, s.ctypes.data) == 0
    assert t.tolist() == terms.tolist() and s.tolist() == side.tolist()
    assert lib.sup_perman_complex_fock_plan(None, c32.ctypes.data, 9, 40, None, None) == -1
    assert lib.sup_perman_complex_fock_plan(r32.ctypes.data, c32.ctypes.data, 65, 1, None, None) == -1
    assert lib.sup_perman_complex_fock_plan(r32.ctypes.data, c32.ctypes.data, 0, 1, None, None) == -1


# ---- exactness ------------------------------------------------------------------

@pytest.mark.parametrize("n,seed", [(1, 1), (2, 2), (3, 3), (5, 4), (7, 5), (8, 6)])
def test_gaussian_integer_submatrices_exact(sup, n, seed):
    """Entries in {-1,0,1} + i{-1,0,1}, n <= 8: 2 x_j(v) = sum_k (t_k - 2 v_k) b_k[j]
    is a Gaussian integer of modulus <= sqrt(2) n, a product of k factors times
    2^k one of modulus <= (sqrt(2) 8)^8 = 2.7e8; the weights are integers
    <= C(8, 4) per digit with product <= 2^8; every partial sum over the at
    most 2^7 weighted terms stays below 2^53 times the common power-of-two
    denominator: every operation is exact, so the result equals Ryser over
    Python integers on the expanded matrix."""
    rng = np.random.default_rng(seed)
    U = gauss_int_case(6, 100 + seed)
    count = 12
    rows = rng.integers(0, 6, (count, n))
    cols = rng.integers(0, 6, (count, n))
    rows[::2] = rng.integers(0, 2, (count // 2, n))   # rows repeat more: side 1 when n > 1
    cols[1::3] = rng.integers(0, 2, (count // 3, n))  # columns repeat more
    got = sup.perman_complex_fock(U, rows, cols, cpu=True)
    sides = set()
    for k in range(count):
        assert got[k] == as_complex(exact_perm(U[np.ix_(rows[k], cols[k])])), k
        sides.add(plan(rows[k], cols[k])[1])
    if n >= 5:
        assert sides == {0, 1}
    # shape [n] lists return one complex
    one = sup.perman_complex_fock(U, rows[3], cols[3], cpu=True)
    assert isinstance(one, complex) and one == got[3]


def test_integer_case_with_thirty_terms(sup):
    """An integer n = 8 matrix whose collapsed side has 30 terms instead of 128."""
    U = np.arange(1, 26, dtype=float).reshape(5, 5) % 7 - 3
    rows, cols = [0, 1, 2, 3, 4, 0, 1, 2], [0, 0, 0, 0, 1, 1, 2, 3]
    assert sup.perman_complex_fock_plan(rows, cols) == (5 * 3 * 2 * 1, 0)
    v, st = sup.perman_complex_fock(U, rows, cols, cpu=True, return_stats=True)
    assert v == as_complex(exact_perm(U[np.ix_(rows, cols)]))
    assert st["visited_steps"] == 30 and st["gray_steps"] == 128 and st["leaves"] == 1
    assert st["est_ops_per_step"] == 48 and st["devices_used"] == 0


# ---- accuracy ---------------------------------------------------------------------

# (n, rows multiplicities, cols multiplicities, seed)
ACCURACY = [
    (4, (1, 1, 1, 1), (2, 2), 61),
    (7, (1,) * 7, (3, 2, 2), 62),            # 24 terms instead of 64: t' = (3, 1, 2)
    (9, (4, 4, 1), (1,) * 9, 63),            # rows collapsed
    (10, (1,) * 10, (1,) * 10, 64),          # no repeats: 2^9 terms
    (12, (3, 3, 3, 3), (6, 6), 65),
    (13, (1,) * 13, (4, 4, 4, 1), 66),       # T = 125, two wave-chunks
    (13, (2, 2, 2, 2, 2, 2, 1), (1,) * 13, 67),  # rows collapsed, T = 729: walk digits
]
_ACC = {}


def accuracy_case(n, rm, cm, seed):
    """(U, rows, cols, exact truth, S, e_np) of the expanded matrix, once per case."""
    key = (n, rm, cm, seed)
    if key not in _ACC:
        rng = np.random.default_rng(seed)
        U = rng.standard_normal((16, 16)) + 1j * rng.standard_normal((16, 16))
        rows, cols = lists_with(rng, rm, 16), lists_with(rng, cm, 16)
        a = U[np.ix_(rows, cols)]
        truth = exact_perm(a)
        v, scale = np_ryser(a)
        _ACC[key] = (U, rows, cols, truth, scale, err_over_scale(v, truth, scale))
    return _ACC[key]


def fock_bound(e_np, Tw, n):
    return max(e_np, 2.0 ** -52) * (Tw + n)


@pytest.mark.parametrize("n,rm,cm,seed", ACCURACY)
def test_random_complex_against_exact_truth(sup, n, rm, cm, seed):
    """|fock - truth| / S <= max(e_np, 2^-52) (Tw + n): test_complex's bound
    with 2^m replaced by the plan's steps per lane Tw.  Measured table:
    DESIGN.md 8c."""
    U, rows, cols, truth, scale, e_np = accuracy_case(n, rm, cm, seed)
    T, side, Tw, H = plan(rows, cols)
    v, st = sup.perman_complex_fock(U, rows, cols, cpu=True, return_stats=True)
    assert st["visited_steps"] == T == Tw * H
    e = err_over_scale(v, truth, scale)
    print(f"n={n} rows={rm} cols={cm} T={T} side={side} Tw={Tw} H={H} e_np={e_np:.3e} e_fock={e:.3e} "
          f"bound={fock_bound(e_np, Tw, n):.3e}")
    assert e <= fock_bound(e_np, Tw, n)


@pytest.mark.parametrize("n,rm,cm,seed", ACCURACY)
def test_agrees_with_the_submatrix_entry(sup, n, rm, cm, seed):
    """Within the sum of both bounds (the submatrix entry's: 2^m + n steps)."""
    U, rows, cols, truth, scale, e_np = accuracy_case(n, rm, cm, seed)
    Tw = plan(rows, cols)[2]
    f = sup.perman_complex_fock(U, rows, cols, cpu=True)
    s = sup.perman_complex_submatrices(U, rows[None, :], cols[None, :], cpu=True)[0]
    m = sup.layout(n)[1]
    assert abs(f - s) / scale <= fock_bound(e_np, Tw, n) + max(e_np, 2.0 ** -52) * (2 ** m + n)


# ---- rank one: the closed form at orders no brute force reaches -------------------

def dyadic_phases(rng, k):
    """k Gaussian dyadic numbers (a + b i) / 4, a and b odd in [-7, 7]: products
    of two have 8-bit numerators, so u_r v_c is exact in fp64."""
    odd = np.array([-7, -5, -3, -1, 1, 3, 5, 7])
    return (rng.choice(odd, k) + 1j * rng.choice(odd, k)) / 4


def cmul(a, b):
    return (a[0] * b[0] - a[1] * b[1], a[0] * b[1] + a[1] * b[0])


def rank_one_case(n, mult, seed):
    """U = u v^T exactly, rows and cols with the same multiplicities `mult` (a
    tie: the columns are collapsed).  Truth n! prod u_rows prod v_cols in
    fractions; S = sum over column subsets of |prod_j x_j| of the expanded
    matrix, summed over the multiplicity vectors: x_j(v) = u_rows[j] s(v) / 2,
    s(v) = sum_k (t_k - 2 v_k) v_k-th distinct column value, C(t'_k, v_k)
    subsets each."""
    rng = np.random.default_rng(seed)
    K = len(mult)
    u, v = dyadic_phases(rng, K), dyadic_phases(rng, K)
    U = np.outer(u, v)
    rows, cols = lists_with(rng, mult, K), lists_with(rng, mult, K)
    truth = (Fraction(math.factorial(n)), Fraction(0))
    for z in list(u[rows]) + list(v[cols]):
        truth = cmul(truth, (Fraction(float(z.real)), Fraction(float(z.imag))))
    # the groups of cols in order of first appearance, as the layout sees them
    seen = {}
    for cidx in cols:
        seen[int(cidx)] = seen.get(int(cidx), 0) + 1
    vals, t = list(seen.keys()), list(seen.values())
    held = min(range(K), key=lambda k: (t[k], k))
    tp = [t[k] - (k == held) for k in range(K)]
    log_pu = sum(math.log(abs(z)) for z in u[rows])
    scale = 0.0
    vk = [0] * K
    while True:
        s = sum((t[k] - 2 * vk[k]) * v[vals[k]] for k in range(K)) / 2
        w = math.prod(math.comb(tp[k], vk[k]) for k in range(K))
        if s != 0:
            scale += w * math.exp(log_pu + n * math.log(abs(s)))
        k = 0
        while k < K and vk[k] == tp[k]:
            vk[k] = 0
            k += 1
        if k == K:
            break
        vk[k] += 1
    return U, rows, cols, truth, scale


RANK_ONE = [(17, (4, 4, 4, 4, 1)), (17, (8, 8, 1)), (33, (8, 8, 8, 8, 1)), (49, (12, 12, 12, 12, 1)),
            (64, (16, 16, 16, 15, 1))]


@pytest.mark.parametrize("n,mult", RANK_ONE)
def test_rank_one_closed_form(sup, n, mult):
    """e <= 2^-52 (Tw + n) against the closed form (no e_np at these orders)."""
    U, rows, cols, truth, scale = rank_one_case(n, mult, 700 + n)
    T, side, Tw, H = plan(rows, cols)
    assert side == 0 and T == math.prod(t + 1 for t in mult[:-1])
    v, st = sup.perman_complex_fock(U, rows, cols, cpu=True, return_stats=True)
    assert st["visited_steps"] == T and st["est_ops_per_step"] == 6 * n
    e = err_over_scale(v, truth, scale)
    print(f"n={n} mult={mult} T={T} Tw={Tw} H={H} e_fock={e:.3e} bound={fock_bound(0.0, Tw, n):.3e}")
    assert e <= fock_bound(0.0, Tw, n)


# ---- bits -------------------------------------------------------------------------

def hetero_batch(n, count, seed):
    """count index-list pairs of order n with different collision patterns."""
    rng = np.random.default_rng(seed)
    U = rng.standard_normal((12, 14)) + 1j * rng.standard_normal((12, 14))
    rows = np.zeros((count, n), dtype=np.int64)
    cols = np.zeros((count, n), dtype=np.int64)
    for k in range(count):
        rows[k] = rng.integers(0, (2, 3, 5, 12)[k % 4], n)
        cols[k] = rng.integers(0, (14, 2, 4, 6, 3)[k % 5], n)
    return U, rows, cols


@pytest.mark.parametrize("n", [6, 9, 13])
def test_batch_result_is_the_single_call(sup, n):
    U, rows, cols = hetero_batch(n, 65, 800 + n)
    got, st = sup.perman_complex_fock(U, rows, cols, cpu=True, return_stats=True)
    assert got.shape == (65,) and got.dtype == np.complex128
    one = np.array([sup.perman_complex_fock(U, rows[k], cols[k], cpu=True) for k in range(65)])
    assert np.array_equal(bits(got), bits(one))
    plans = [plan(rows[k], cols[k]) for k in range(65)]
    assert len({p[0] for p in plans}) > 5 and {p[1] for p in plans} == {0, 1}
    assert st["visited_steps"] == sum(p[0] for p in plans) and st["leaves"] == 65
    assert st["gray_steps"] == 65 << (n - 1)


def test_threads_and_slab_change_no_bit(sup, monkeypatch):
    U, rows, cols = hetero_batch(11, 23, 811)
    v1 = sup.perman_complex_fock(U, rows, cols, cpu=True, threads=1)
    for t in (3, 16):
        assert np.array_equal(bits(v1), bits(sup.perman_complex_fock(U, rows, cols, cpu=True, threads=t)))
    for slab in ("1", "3", "1000"):
        monkeypatch.setenv("SUP_CPLX_FOCK_SLAB", slab)  # read at every call
        assert np.array_equal(bits(v1), bits(sup.perman_complex_fock(U, rows, cols, cpu=True, threads=3)))


# ---- errors -----------------------------------------------------------------------

def test_empty_batch(sup):
    U = np.ones((3, 3), dtype=np.complex128)
    w, st = sup.perman_complex_fock(U, np.zeros((0, 2), dtype=np.int32), np.zeros((0, 2), dtype=np.int32), cpu=True,
                                    return_stats=True)
    assert w.shape == (0,) and st["leaves"] == 0 and st["visited_steps"] == 0


def test_argument_errors(sup):
    U = np.ones((3, 4), dtype=np.complex128)
    with pytest.raises(ValueError, match="shape"):
        sup.perman_complex_fock(U, np.zeros((2, 3), dtype=int), np.zeros((2, 4), dtype=int), cpu=True)
    with pytest.raises(ValueError, match="integer"):
        sup.perman_complex_fock(U, np.zeros((2, 3)), np.zeros((2, 3)), cpu=True)
    with pytest.raises(ValueError, match="outside"):
        sup.perman_complex_fock(U, np.zeros((1, 65), dtype=int), np.zeros((1, 65), dtype=int), cpu=True)
    with pytest.raises(ValueError, match="2-d"):
        sup.perman_complex_fock(np.ones(3), [0], [0], cpu=True)


def test_index_errors_name_the_offender(sup):
    U = np.ones((3, 4), dtype=np.complex128)
    rows = np.zeros((5, 2), dtype=np.int32)
    cols = np.zeros((5, 2), dtype=np.int32)
    bad = rows.copy()
    bad[3, 1] = 3  # R = 3
    with pytest.raises(sup.SupError, match=r"rows\[k = 3\]\[position 1\] = 3 outside \[0, 3\)") as e:
        sup.perman_complex_fock(U, bad, cols, cpu=True)
    assert e.value.code == -1
    bad = cols.copy()
    bad[4, 0] = -1
    with pytest.raises(sup.SupError, match=r"cols\[k = 4\]\[position 0\] = -1 outside \[0, 4\)"):
        sup.perman_complex_fock(U, rows, bad, cpu=True)


def test_c_abi_null_and_range_errors(sup):
    lib = sup._lib.load()
    out = (C.c_double * 4)()
    m = np.ones(2 * 2 * 4)
    idx = np.zeros(4, dtype=np.int32)
    call = lib.sup_perman_complex_fock
    for R, Cc in ((0, 2), (2, 0)):
        assert call(m.ctypes.data, R, Cc, idx.ctypes.data, idx.ctypes.data, 2, 2, None, 1, out, None) == -1
    assert call(None, 2, 2, idx.ctypes.data, idx.ctypes.data, 2, 2, None, 1, out, None) == -1
    assert call(m.ctypes.data, 2, 2, None, idx.ctypes.data, 2, 2, None, 1, out, None) == -1
    assert call(m.ctypes.data, 2, 2, idx.ctypes.data, None, 2, 2, None, 1, out, None) == -1
    assert call(m.ctypes.data, 2, 2, idx.ctypes.data, idx.ctypes.data, 2, 2, None, 1, None, None) == -1
    for n in (0, 65, -1):
        assert call(m.ctypes.data, 2, 2, idx.ctypes.data, idx.ctypes.data, n, 1, None, 1, out, None) == -1
    o = sup._opts(walk_log2=40)  # checked as the submatrix entry checks it
    assert call(m.ctypes.data, 2, 2, idx.ctypes.data, idx.ctypes.data, 2, 2, C.byref(o), 1, out, None) == -1
    out[0] = 7.0  # count == 0 writes nothing
    assert call(m.ctypes.data, 2, 2, idx.ctypes.data, idx.ctypes.data, 2, 0, None, 1, out, None) == 0
    assert out[0] == 7.0


def test_too_many_terms_is_refused_before_any_work(sup):
    U = np.ones((64, 64), dtype=np.complex128)
    with pytest.raises(sup.SupError, match="terms") as e:
        sup.perman_complex_fock(U, np.arange(64), np.arange(64), cpu=True)
    assert e.value.code == -7


def test_no_device_is_an_error_not_a_cpu_fallback(sup):
    U, rows, cols = hetero_batch(6, 4, 806)
    if sup.device_count() == 0:
        with pytest.raises(sup.SupError) as e:
            sup.perman_complex_fock(U, rows, cols)
        assert e.value.code == -2
    else:  # a box with a device: the device walk, the host twin's bits
        assert np.array_equal(bits(sup.perman_complex_fock(U, rows, cols)),
                              bits(sup.perman_complex_fock(U, rows, cols, cpu=True)))


def test_nan_stays_in_the_results_that_gather_it(sup):
    U, rows, cols = hetero_batch(8, 30, 808)
    clean = sup.perman_complex_fock(U, rows, cols, cpu=True)
    dirty = U.copy()
    dirty[1, 1] = complex(np.nan, 1.0)
    got = sup.perman_complex_fock(dirty, rows, cols, cpu=True)
    hit = np.array([1 in rows[k] and 1 in cols[k] for k in range(30)])
    assert hit.any() and not hit.all()
    assert np.array_equal(bits(got[~hit]), bits(clean[~hit]))
    assert not np.isfinite(got[hit]).any()
