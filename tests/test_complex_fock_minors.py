"""Collision-aware one-walk permanent minors on host threads
(cplx_fock_minors.cpp, the host twin of walk_cplxfm.hip, through
perman_complex_fock_minors_submatrices(cpu=True)) and the plan entry
perman_complex_fock_minors_plan.  DESIGN.md 8e.

Matrix k is B = U[np.ix_(rows[k], cols[k])], n rows and q = n - 1 columns;
value [k, j] is the permanent of B without row j.  Only the column side is
collapsed: with the column multiplicities t_k (order of first appearance),
one copy of the rarest group held, T = prod (t'_k + 1) states are walked.
The layout (T, Tw, H) is test_complex_fock.layout's restatement of 8c's rule.

Truth: test_complex.exact_perm on every materialised minor.  Error scale of
minor j: S_j = sum over the 2^(q-1) subsets of |prod_{i != j} x_i| on the
expanded minor, which is np_ryser's scale on the materialised minor.  Bound:
max(e_np, 2^-52) (Tw + n), 8c's form (test_complex_fock.fock_bound), e_np the
from-scratch complex128 Ryser's error on that minor.
"""
import ctypes as C

import numpy as np
import pytest

from test_complex import as_complex, err_over_scale, exact_perm, gauss_int_case, np_ryser, walk_bound
from test_complex_batch import bits
from test_complex_fock import fock_bound, groups, layout
from test_complex_fock import plan as square_plan
from test_complex_minors import minors_of


def fm(sup, U, rows, cols, **kw):
    return sup.perman_complex_fock_minors_submatrices(U, np.atleast_2d(rows), np.atleast_2d(cols), cpu=True, **kw)


# ---- plan -----------------------------------------------------------------------

PLAN_CASES = [
    # cols (n - 1 of them), T
    ([5], 1),                                        # n = 2: the one column is held
    ([1, 1], 2),                                     # one group of two, one copy held
    ([0, 1, 2, 3, 4, 5], 32),                        # no repeats: 2^(n-2)
    ([2, 2, 2], 3),                                  # the issue's n = 4, (3)
    ([7, 7, 7, 3, 3, 9], 4 * 3),                     # (3, 2, 1): the single column is held
    ([0, 0, 1, 1, 1, 2, 2], 2 * 4 * 3),              # a tie for the smallest (2, 2): the first is held
    ([4, 0, 4, 0, 1, 1, 4], 4 * 2 * 3),              # first appearance orders the groups: (3, 2, 2), second held
    ([0, 0, 1, 2, 3, 4, 5, 6, 7], 3 * 2 ** 6),       # (2, 1 x 7): the first single is held, T = 192
    ([0] * 4 + [1] * 4 + [2] * 4, 4 * 5 * 5),        # (4, 4, 4): the first group is held, T = 100
    (sum(([k] * 4 for k in range(7)), []) + [7, 7, 7], 5 ** 7 * 3),  # n = 32 in groups of four: the last (3) is held
]


@pytest.mark.parametrize("cols,T", PLAN_CASES)
def test_plan_terms(sup, cols, T):
    """(T, Tw, H) per case from the restated rule; the hand count agrees with it."""
    assert layout(groups(cols))[0] == T
    assert sup.perman_complex_fock_minors_plan(cols) == T


def test_plan_batch_n1_and_errors(sup):
    rng = np.random.default_rng(3)
    cols = rng.integers(0, 4, (40, 9))
    terms = sup.perman_complex_fock_minors_plan(cols)
    assert terms.dtype == np.uint64 and terms.tolist() == [layout(groups(c))[0] for c in cols]
    assert len(set(terms.tolist())) > 5
    assert sup.perman_complex_fock_minors_plan(np.zeros((3, 0), dtype=np.int32)).tolist() == [1, 1, 1]  # n = 1
    lib = sup._lib.load()
    c32 = cols.astype(np.int32)
    t = np.zeros(40, np.uint64)
    assert lib.sup_perman_complex_fock_minors_plan(c32.ctypes.data, 10, 40, t.ctypes.data) == 0
    assert t.tolist() == terms.tolist()
    assert lib.sup_perman_complex_fock_minors_plan(None, 10, 40, t.ctypes.data) == -1
    assert lib.sup_perman_complex_fock_minors_plan(c32.ctypes.data, 10, 40, None) == -1
    assert lib.sup_perman_complex_fock_minors_plan(c32.ctypes.data, 0, 1, t.ctypes.data) == -1
    assert lib.sup_perman_complex_fock_minors_plan(c32.ctypes.data, 33, 1, t.ctypes.data) == -7
    assert lib.sup_perman_complex_fock_minors_plan(None, 1, 2, t.ctypes.data) == 0 and t[:2].tolist() == [1, 1]


# ---- closed forms and exact cases -------------------------------------------------

def test_closed_forms_n1_n2_n3(sup):
    """n = 1: no walk.  n = 2: T = 1, minor j = 2 x_{1-j}(0) = the other row's
    entry.  n = 3 with both columns equal: T = 2 (Tw = 1, H = 2), minor j =
    2 b[a] b[c] for the two other rows; with distinct columns T = 2 as well."""
    assert np.array_equal(sup.perman_complex_fock_minors(np.zeros((1, 0)), cpu=True), [1 + 0j])
    U = np.array([[3 - 2j, 1 + 2j, 3 - 1j], [0.5 + 4j, -2 + 0.5j, 0.25 + 4j], [1j, 2 - 1j, -1 + 1j]])
    got, st = fm(sup, U, [0, 1], [0], return_stats=True)
    assert np.array_equal(got[0], [0.5 + 4j, 3 - 2j])
    assert st["visited_steps"] == 1 and st["gray_steps"] == 1 and st["est_ops_per_step"] == 12 and st["leaves"] == 2
    # small dyadic entries: every product and sum below is exact in fp64
    B = U[:, 1:]
    want = [B[a, 0] * B[b, 1] + B[a, 1] * B[b, 0] for a, b in ((1, 2), (0, 2), (0, 1))]
    assert np.array_equal(sup.perman_complex_fock_minors(B, cpu=True), want)
    b = U[:, 1]
    got, st = fm(sup, U, [0, 1, 2], [1, 1], return_stats=True)
    assert np.array_equal(got[0], [2 * b[1] * b[2], 2 * b[0] * b[2], 2 * b[0] * b[1]])
    assert st["visited_steps"] == 2 and st["gray_steps"] == 2 and st["est_ops_per_step"] == 28


@pytest.mark.parametrize("n,seed", [(2, 1), (3, 2), (4, 3), (6, 4), (8, 5)])
def test_gaussian_integer_minors_exact(sup, n, seed):
    """Entries in {-1,0,1} + i{-1,0,1}, n <= 8 rows (T <= 64, Tw = 1): 2 x_i(v)
    is a Gaussian integer, a term a product of q <= 7 of them over 2^q times an
    integer weight <= 2^7, and prefix and suffix products are sub-products of a
    term: every operation is exact (test_complex_fock's argument), so every
    minor equals the exact Gaussian-integer permanent."""
    rng = np.random.default_rng(seed)
    U = gauss_int_case(6, 100 + seed)
    count = 12
    rows = rng.integers(0, 6, (count, n))
    cols = rng.integers(0, 6, (count, n - 1))
    cols[1::3] = rng.integers(0, 2, (count // 3, n - 1))  # columns repeat more
    got = fm(sup, U, rows, cols)
    assert got.shape == (count, n)
    for k in range(count):
        want = [as_complex(exact_perm(a)) for a in minors_of(U[np.ix_(rows[k], cols[k])])] if n > 2 else \
            [U[rows[k, 1], cols[k, 0]], U[rows[k, 0], cols[k, 0]]]
        assert np.array_equal(got[k], want), k


# ---- accuracy -----------------------------------------------------------------------

# (n, column multiplicities in order of first appearance, seed); (T, Tw, H) by the rule:
# (3) 3, 1, 3; (3, 2, 1) 12, 1, 12; (2, 1 x 7) 192, 3, 64; all distinct 128, 2, 64; (4, 4, 4) 100, 1, 100.
# (3, 2, 1) holds the single column, so t' = (3, 2, 0) and T = 4 x 3 = 12.
ACCURACY = [
    (4, (3,), 71),
    (7, (3, 2, 1), 72),
    (10, (2, 1, 1, 1, 1, 1, 1, 1), 73),
    (9, (1,) * 8, 74),
    (13, (4, 4, 4), 75),
]
LAYOUTS = {(3,): (3, 1, 3), (3, 2, 1): (12, 1, 12), (2, 1, 1, 1, 1, 1, 1, 1): (192, 3, 64), (1,) * 8: (128, 2, 64),
           (4, 4, 4): (100, 1, 100)}
_ACC = {}


def accuracy_case(n, cm, seed):
    """(U, rows, cols, per minor (truth, S_j, e_np)), once per case.  The column
    list is not shuffled: its multiplicities appear in the order given."""
    key = (n, cm, seed)
    if key not in _ACC:
        rng = np.random.default_rng(seed)
        U = rng.standard_normal((16, 16)) + 1j * rng.standard_normal((16, 16))
        rows = rng.permutation(16)[:n]
        cols = np.repeat(rng.choice(16, size=len(cm), replace=False), cm)
        per = []
        for a in minors_of(U[np.ix_(rows, cols)]):
            truth = exact_perm(a)
            v, scale = np_ryser(a)
            per.append((truth, scale, err_over_scale(v, truth, scale)))
        _ACC[key] = (U, rows, cols, per)
    return _ACC[key]


@pytest.mark.parametrize("n,cm,seed", ACCURACY)
def test_random_minors_against_exact_truth(sup, n, cm, seed):
    """|minor_j - truth_j| / S_j <= max(e_np, 2^-52) (Tw + n) for every j.
    (T, Tw, H) per pattern: LAYOUTS above.  Measured table: DESIGN.md 8e.  An
    instance above the bound is a finding, not a constant to widen."""
    U, rows, cols, per = accuracy_case(n, cm, seed)
    T, Tw, H = layout(groups(cols))
    assert (T, Tw, H) == LAYOUTS[cm] and T == Tw * H
    v, st = fm(sup, U, rows, cols, return_stats=True)
    assert st["visited_steps"] == T and st["gray_steps"] == 1 << (n - 2) and st["est_ops_per_step"] == 16 * n - 20
    worst = 0.0
    for j, (truth, scale, e_np) in enumerate(per):
        e = err_over_scale(complex(v[0, j]), truth, scale)
        worst = max(worst, e / fock_bound(e_np, Tw, n))
        print(f"n={n} cols={cm} T={T} Tw={Tw} H={H} j={j} e_np={e_np:.3e} e={e:.3e} bound={fock_bound(e_np, Tw, n):.3e}")
        assert e <= fock_bound(e_np, Tw, n), j
    print(f"n={n} cols={cm} worst e / bound = {worst:.3e}")


@pytest.mark.parametrize("n,cm,seed", ACCURACY)
def test_agrees_with_the_one_walk_minors(sup, n, cm, seed):
    """Not the same bits: within the sum of both bounds over the shared S_j
    (the parent's: 2^m + q steps, test_complex_minors).  (T, Tw, H): LAYOUTS."""
    U, rows, cols, per = accuracy_case(n, cm, seed)
    Tw = layout(groups(cols))[1]
    f = fm(sup, U, rows, cols)[0]
    p = sup.perman_complex_minors_submatrices(U, rows[None, :], cols[None, :], cpu=True)[0]
    m = sup.layout(n - 1)[1]
    for j, (_, scale, e_np) in enumerate(per):
        assert abs(f[j] - p[j]) / scale <= fock_bound(e_np, Tw, n) + walk_bound(e_np, m, n - 1), j


@pytest.mark.parametrize("n,cm,seed", ACCURACY)
def test_laplace_identity_along_an_appended_column(sup, n, cm, seed):
    """sum_j b_j minor_j = perman_complex_fock of [B | b], b a column of U over
    the same rows (a repeat of the first group, and a new column).  Left: the
    minors' bound over S_j weighted by |b_j|, plus the n roundings of the dot
    product (|minor_j| <= 2 S_j).  Right: the square entry's own bound over its
    scale.  (T, Tw, H) of the minors: LAYOUTS."""
    U, rows, cols, per = accuracy_case(n, cm, seed)
    Tw = layout(groups(cols))[1]
    v = fm(sup, U, rows, cols)[0]
    new = next(c for c in range(16) if c not in cols)
    for c in (int(cols[0]), new):
        b = U[rows, c]
        full_cols = np.append(cols, c)
        A = U[np.ix_(rows, full_cols)]
        truth = exact_perm(A)
        v_np, scale_full = np_ryser(A)
        e_full = err_over_scale(v_np, truth, scale_full)
        lhs = complex(sum(b[j] * v[j] for j in range(n)))
        tol = sum(abs(b[j]) * (fock_bound(per[j][2], Tw, n) + n * 2.0 ** -51) * per[j][1] for j in range(n))
        err = err_over_scale(lhs, truth, 1.0)
        full = sup.perman_complex_fock(U, rows, full_cols, cpu=True)
        print(f"n={n} cols={cm} c={c} |lhs - truth| = {err:.3e} tol = {tol:.3e}")
        assert err <= tol
        assert abs(lhs - full) <= tol + fock_bound(e_full, square_plan(rows, full_cols)[2], n) * scale_full


# ---- bits ---------------------------------------------------------------------------

def hetero_batch(n, count, seed):
    """count list pairs of n rows and n - 1 columns with different collision patterns."""
    rng = np.random.default_rng(seed)
    U = rng.standard_normal((12, 14)) + 1j * rng.standard_normal((12, 14))
    rows = np.zeros((count, n), dtype=np.int64)
    cols = np.zeros((count, n - 1), dtype=np.int64)
    for k in range(count):
        rows[k] = rng.integers(0, (12, 3, 5)[k % 3], n)
        cols[k] = rng.integers(0, (14, 2, 4, 6, 3)[k % 5], n - 1)
    return U, rows, cols


@pytest.mark.parametrize("n", [6, 9, 13])
def test_heterogeneous_batch_is_the_single_call(sup, n):
    """Count 65, different patterns at one n.  n = 13: T from 12 to 2^11 (Tw up
    to 32, H >= 64 where T >= 128); n = 6, 9: Tw <= 2."""
    U, rows, cols = hetero_batch(n, 65, 900 + n)
    got, st = fm(sup, U, rows, cols, return_stats=True)
    assert got.shape == (65, n) and got.dtype == np.complex128
    one = np.array([fm(sup, U, rows[k], cols[k])[0] for k in range(65)])
    assert np.array_equal(bits(got), bits(one))
    T = [layout(groups(c))[0] for c in cols]
    assert len(set(T)) >= 4
    assert st["visited_steps"] == sum(T) and st["leaves"] == 65 * n and st["gray_steps"] == 65 << (n - 2)
    assert st["visited_steps"] == int(sup.perman_complex_fock_minors_plan(cols).sum())
    # another batch composition
    assert np.array_equal(bits(fm(sup, U, rows[[5, 2, 2, 64]], cols[[5, 2, 2, 64]])), bits(got[[5, 2, 2, 64]]))


def test_threads_and_slab_change_no_bit(sup, monkeypatch):
    """n = 11, 23 patterns (T up to 2^9, Tw up to 8, H >= 64 there)."""
    U, rows, cols = hetero_batch(11, 23, 911)
    v1 = fm(sup, U, rows, cols, threads=1)
    for t in (3, 8, 16):
        assert np.array_equal(bits(v1), bits(fm(sup, U, rows, cols, threads=t)))
    for slab in ("1", "3", "1000"):
        monkeypatch.setenv("SUP_CPLX_FOCK_MINORS_SLAB", slab)  # read at every call
        assert np.array_equal(bits(v1), bits(fm(sup, U, rows, cols, threads=3)))


def test_repeated_rows_are_only_gathered(sup):
    """Rows 0 and n - 1 equal (n = 8, T <= 64, Tw = 1): the two minors that drop
    one or the other are the same number, and every minor is the raw call's on
    the gathered matrix's row list."""
    rng = np.random.default_rng(5)
    U = rng.standard_normal((9, 11)) + 1j * rng.standard_normal((9, 11))
    n, count = 8, 17
    rows = rng.integers(0, 9, (count, n))
    cols = rng.integers(0, 4, (count, n - 1))
    rows[:, -1] = rows[:, 0]
    got = fm(sup, U, rows, cols)
    par = sup.perman_complex_minors_submatrices(U, rows, cols, cpu=True)
    assert np.allclose(got, par, rtol=1e-10, atol=1e-10)
    assert np.allclose(got[:, 0], got[:, -1], rtol=1e-10, atol=1e-12)
    # the same B through relabelled rows of a permuted U has the same bits
    perm = rng.permutation(9)
    inv = np.argsort(perm)
    assert np.array_equal(bits(fm(sup, U[perm], inv[rows], cols)), bits(got))


# ---- errors ---------------------------------------------------------------------------

def test_empty_batch(sup):
    U = np.ones((3, 3), dtype=np.complex128)
    v, st = sup.perman_complex_fock_minors_submatrices(U, np.zeros((0, 3), dtype=np.int32),
                                                       np.zeros((0, 2), dtype=np.int32), cpu=True, return_stats=True)
    assert v.shape == (0, 3) and v.dtype == np.complex128
    assert st["leaves"] == 0 and st["gray_steps"] == 0 and st["visited_steps"] == 0


def test_python_argument_errors(sup):
    U = np.ones((3, 4), dtype=np.complex128)
    with pytest.raises(ValueError, match="shape"):
        sup.perman_complex_fock_minors_submatrices(U, np.zeros((2, 3), dtype=int), np.zeros((2, 3), dtype=int), cpu=True)
    with pytest.raises(ValueError, match="integer"):
        sup.perman_complex_fock_minors_submatrices(U, np.zeros((2, 3)), np.zeros((2, 2)), cpu=True)
    with pytest.raises(ValueError, match="n x \\(n-1\\)"):
        sup.perman_complex_fock_minors(np.zeros((3, 3)), cpu=True)
    with pytest.raises(ValueError, match="2-d"):
        sup.perman_complex_fock_minors_submatrices(np.ones(3), [[0, 0]], [[0]], cpu=True)


def test_33_rows_are_unsupported(sup):
    U = np.ones((2, 2), dtype=np.complex128)
    with pytest.raises(sup.SupError, match="n = 33") as e:
        sup.perman_complex_fock_minors_submatrices(U, np.zeros((1, 33), dtype=int), np.zeros((1, 32), dtype=int),
                                                   cpu=True)
    assert e.value.code == -7
    with pytest.raises(sup.SupError, match="n = 33") as e:
        sup.perman_complex_fock_minors_plan(np.zeros(32, dtype=int))
    assert e.value.code == -7


def test_index_errors_name_the_offender(sup):
    U = np.ones((3, 4), dtype=np.complex128)
    rows = np.zeros((5, 3), dtype=np.int32)
    cols = np.zeros((5, 2), dtype=np.int32)
    bad = rows.copy()
    bad[3, 2] = 3  # R = 3
    with pytest.raises(sup.SupError, match=r"rows\[k = 3\]\[position 2\] = 3 outside \[0, 3\)") as e:
        sup.perman_complex_fock_minors_submatrices(U, bad, cols, cpu=True)
    assert e.value.code == -1
    bad = cols.copy()
    bad[4, 0] = -1
    with pytest.raises(sup.SupError, match=r"cols\[k = 4\]\[position 0\] = -1 outside \[0, 4\)"):
        sup.perman_complex_fock_minors_submatrices(U, rows, bad, cpu=True)
    bad = cols.copy()
    bad[2, 1] = 4  # C = 4
    with pytest.raises(sup.SupError, match=r"cols\[k = 2\]\[position 1\] = 4 outside \[0, 4\)"):
        sup.perman_complex_fock_minors_submatrices(U, rows, bad, cpu=True)


def test_c_abi_null_and_range_errors(sup):
    lib = sup._lib.load()
    call = lib.sup_perman_complex_fock_minors
    out = (C.c_double * 16)()
    m = np.ones(2 * 2 * 4)
    idx = np.zeros(8, dtype=np.int32)
    u, ix = m.ctypes.data, idx.ctypes.data
    assert call(None, 2, 2, ix, ix, 2, 2, None, 1, out, None) == -1
    assert call(u, 2, 2, None, ix, 2, 2, None, 1, out, None) == -1
    assert call(u, 2, 2, ix, None, 2, 2, None, 1, out, None) == -1  # cols NULL, n = 2
    assert call(u, 2, 2, ix, ix, 2, 2, None, 1, None, None) == -1
    assert call(u, 2, 2, ix, ix, 0, 2, None, 1, out, None) == -1
    assert call(u, 2, 2, ix, ix, -1, 2, None, 1, out, None) == -1
    assert call(u, 2, 2, ix, ix, 33, 0, None, 1, out, None) == -7
    assert call(u, 2, 2, ix, ix, 65, 0, None, 1, out, None) == -7
    for R, Cc in ((0, 2), (2, 0)):
        assert call(u, R, Cc, ix, ix, 2, 2, None, 1, out, None) == -1
    o = sup._opts(walk_log2=40)  # checked as the parent entry checks it
    assert call(u, 2, 2, ix, ix, 2, 2, C.byref(o), 1, out, None) == -1
    # cols may be NULL when n = 1: ones
    assert call(u, 2, 2, ix, None, 1, 3, None, 1, out, None) == 0
    assert list(out[:6]) == [1.0, 0.0, 1.0, 0.0, 1.0, 0.0]
    # count == 0 writes nothing
    out[0] = 7.0
    assert call(u, 2, 2, ix, ix, 2, 0, None, 1, out, None) == 0 and out[0] == 7.0


def test_nan_stays_in_the_results_that_gather_it(sup):
    """n = 8 (T <= 64, Tw = 1).  A matrix that gathers the poisoned entry in one
    row only keeps the minor without that row clean."""
    U, rows, cols = hetero_batch(8, 30, 908)
    rows[:, 0] = 1          # every matrix has row 1 of U first ...
    rows[:, 1:] = np.where(rows[:, 1:] == 1, 2, rows[:, 1:])  # ... and nowhere else
    clean = fm(sup, U, rows, cols)
    dirty = U.copy()
    dirty[1, 1] = complex(np.nan, 1.0)
    got = fm(sup, dirty, rows, cols)
    hit = np.array([1 in cols[k] for k in range(30)])
    assert hit.any() and not hit.all()
    assert np.array_equal(bits(got[~hit]), bits(clean[~hit]))
    assert not np.isfinite(got[hit][:, 1:]).any()
    assert np.array_equal(bits(got[hit][:, 0]), bits(clean[hit][:, 0]))  # the minor without the poisoned row


def test_no_device_is_an_error_not_a_cpu_fallback(sup):
    U, rows, cols = hetero_batch(6, 4, 906)
    if sup.device_count() == 0:
        with pytest.raises(sup.SupError) as e:
            sup.perman_complex_fock_minors_submatrices(U, rows, cols)
        assert e.value.code == -2
    else:  # a box with a device: the device walk, the host twin's bits
        assert np.array_equal(bits(sup.perman_complex_fock_minors_submatrices(U, rows, cols)), bits(fm(sup, U, rows, cols)))
