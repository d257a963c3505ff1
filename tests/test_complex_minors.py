"""One-walk permanent minors (sup_perman_complex_minors, _minors_range): the
host twin, which runs walk_cplxm.hip's operations in its order.  B is n x (n-1)
complex; value j is the permanent of B without row j, all n from one Gray walk
of order q = n - 1.

Truth: test_complex.py's exact_perm on every materialised minor.  Error scale
of minor j: S_j = sum over the walk's 2^(q-1) subsets of |prod_{i != j} x_i|,
which is np_ryser's scale on the materialised minor (x_i depends on row i only).
Bound: test_complex.py's walk_bound(e_np, m, q) — a term of minor j is a product
of q factors like the plain walk's of order q, each x the result of up to
2^m + q additions; the prefix/suffix chain changes the association of the
product, not the number of multiplies per term.
"""
import ctypes as C

import numpy as np
import pytest

from test_complex import as_complex, err_over_scale, exact_perm, gauss_int_case, np_ryser, walk_bound
from test_complex_batch import bits

_CASES = {}


def minors_of(B):
    return [np.delete(B, j, axis=0) for j in range(B.shape[0])]


def random_minors_case(n, seed):
    """(B, per minor: exact truth, S_j, e_np), computed once per (n, seed)."""
    if (n, seed) not in _CASES:
        rng = np.random.default_rng(seed)
        B = rng.standard_normal((n, n - 1)) + 1j * rng.standard_normal((n, n - 1))
        per = []
        for a in minors_of(B):
            truth = exact_perm(a)
            v, scale = np_ryser(a)
            per.append((truth, scale, err_over_scale(v, truth, scale)))
        _CASES[(n, seed)] = (B, per)
    return _CASES[(n, seed)]


def cplx(re, im):
    """re + i im componentwise with no arithmetic (signed zeros survive)."""
    out = np.empty(np.shape(re), dtype=np.complex128)
    out.real, out.imag = re, im
    return out


def batch_B(n, count, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((count, n, n - 1)) + 1j * rng.standard_normal((count, n, n - 1))


def via_lists(sup, Bs, **kw):
    """A stack of raw n x (n-1) matrices through the submatrix entry: U = the
    matrices side by side, matrix k picks its own block of columns."""
    count, n, q = Bs.shape
    U = np.concatenate(list(Bs), axis=1) if q else np.zeros((n, 1), dtype=np.complex128)
    rows = np.tile(np.arange(n), (count, 1))
    cols = np.arange(count)[:, None] * q + np.arange(q)[None, :]
    return sup.perman_complex_minors_submatrices(U, rows, cols, **kw)


# ---- closed forms and exact cases --------------------------------------------

def test_closed_forms_n1_n2_n3(sup):
    assert np.array_equal(sup.perman_complex_minors(np.zeros((1, 0)), cpu=True), [1 + 0j])
    b = np.array([[3 - 2j], [0.5 + 4j]])
    assert np.array_equal(sup.perman_complex_minors(b, cpu=True), [0.5 + 4j, 3 - 2j])  # the other row's entry
    B = np.array([[1 + 2j, 3 - 1j], [-2 + 0.5j, 0.25 + 4j], [2 - 1j, -1 + 1j]])
    # small dyadic entries: every product and sum below is exact in fp64
    want = [B[a, 0] * B[b, 1] + B[a, 1] * B[b, 0] for a, b in ((1, 2), (0, 2), (0, 1))]
    got = sup.perman_complex_minors(B, cpu=True)
    assert got.dtype == np.complex128 and got.shape == (3,)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("n,seed", [(2, 1), (3, 2), (4, 3), (6, 4), (8, 5)])
def test_gaussian_integer_minors_exact(sup, n, seed):
    """Entries in {-1,0,1} + i{-1,0,1}, n <= 8 rows: every intermediate is
    exactly representable (test_complex.py's argument with q = n - 1 <= 7
    factors per term; prefix and suffix products are sub-products of a term),
    so every minor equals the exact Gaussian-integer permanent."""
    B = gauss_int_case(n, seed)[:, : n - 1]
    want = [as_complex(exact_perm(a)) for a in minors_of(B)]
    assert np.array_equal(sup.perman_complex_minors(B, cpu=True), want)
    assert np.array_equal(sup.perman_complex_minors(B, cpu=True, threads=1, walk_log2=1), want)


# ---- accuracy ------------------------------------------------------------------

@pytest.mark.parametrize("n,seed,walk_log2", [(5, 51, 0), (10, 52, 0), (13, 53, 0), (15, 54, 0), (15, 54, 4)])
def test_random_minors_against_exact_truth(sup, n, seed, walk_log2):
    """Measured (max over j of e_walk / bound): see the table
    there.  An instance above the bound is a finding, not a constant to widen."""
    B, per = random_minors_case(n, seed)
    q = n - 1
    v, st = sup.perman_complex_minors(B, cpu=True, walk_log2=walk_log2, return_stats=True)
    L, m0, _ = sup.layout(q)
    m = min(walk_log2, q - 1 - L) if walk_log2 else m0
    assert st["walk_bits"] == m and st["lane_bits"] == L
    assert st["leaves"] == n and st["gray_steps"] == 1 << (q - 1) and st["est_ops_per_step"] == 16 * n - 24
    worst = 0.0
    for j, (truth, scale, e_np) in enumerate(per):
        e_walk = err_over_scale(complex(v[j]), truth, scale)
        worst = max(worst, e_walk / walk_bound(e_np, m, q))
        print(f"n={n} m={m} j={j} e_np={e_np:.3e} e_walk={e_walk:.3e} bound={walk_bound(e_np, m, q):.3e}")
        assert e_walk <= walk_bound(e_np, m, q), j
    print(f"n={n} m={m} worst e_walk / bound = {worst:.3e}")


@pytest.mark.parametrize("n,seed", [(5, 51), (10, 52), (13, 53)])
def test_agrees_with_perman_complex_on_each_minor(sup, n, seed):
    """Not the same bits (the product order differs): within the sum of both
    walks' bounds over the shared scale S_j."""
    B, per = random_minors_case(n, seed)
    q = n - 1
    m = sup.layout(q)[1]
    v = sup.perman_complex_minors(B, cpu=True)
    for j, a in enumerate(minors_of(B)):
        _, scale, e_np = per[j]
        assert abs(v[j] - sup.perman_complex(a, cpu=True)) <= 2 * walk_bound(e_np, m, q) * scale, j


@pytest.mark.parametrize("n,seed", [(5, 51), (10, 52), (13, 53)])
def test_laplace_identity_along_an_appended_column(sup, n, seed):
    """sum_j b[j][c'] minor_j = per([B | column c' of B]): the expansion the
    sampler's weights rely on.  Both sides carry their walk's bound (the
    minors' over S_j weighted by |b[j][c']|, the full walk's over its own S)
    plus the n roundings of the dot product (|minor_j| <= 2 S_j)."""
    B, per = random_minors_case(n, seed)
    q = n - 1
    m = sup.layout(q)[1]
    v = sup.perman_complex_minors(B, cpu=True)
    for c in (0, q - 1):
        A = np.concatenate([B, B[:, c:c + 1]], axis=1)
        truth = exact_perm(A)
        _, scale_full = np_ryser(A)
        lhs = complex(sum(B[j, c] * v[j] for j in range(n)))
        tol = sum(abs(B[j, c]) * (walk_bound(per[j][2], m, q) + n * 2.0 ** -51) * per[j][1] for j in range(n))
        err = err_over_scale(lhs, truth, 1.0)
        full = sup.perman_complex(A, cpu=True)
        print(f"n={n} c={c} |lhs - truth| = {err:.3e} tol = {tol:.3e}")
        assert err <= tol
        assert abs(lhs - full) <= tol + walk_bound(2.0 ** -52, sup.layout(n)[1], n) * scale_full


# ---- determinism ---------------------------------------------------------------

@pytest.mark.parametrize("n,count", [(8, 40), (14, 3), (15, 2)])
def test_thread_count_changes_no_bit(sup, n, count):
    Bs = batch_B(n, count, 7 * n)
    one = via_lists(sup, Bs, cpu=True, threads=1)
    assert one.shape == (count, n)
    assert np.array_equal(bits(one), bits(via_lists(sup, Bs, cpu=True, threads=3)))
    assert np.array_equal(bits(one), bits(via_lists(sup, Bs, cpu=True, threads=16)))


@pytest.mark.parametrize("slab", ["1", "3"])
def test_slab_size_and_batch_composition_change_no_bit(sup, monkeypatch, slab):
    Bs = batch_B(9, 7, 99)
    whole = via_lists(sup, Bs, cpu=True)
    monkeypatch.setenv("SUP_CPLX_MINORS_SLAB", slab)
    assert np.array_equal(bits(via_lists(sup, Bs, cpu=True)), bits(whole))
    monkeypatch.delenv("SUP_CPLX_MINORS_SLAB")
    for k in range(7):  # each matrix alone, and in another batch
        assert np.array_equal(bits(sup.perman_complex_minors(Bs[k], cpu=True)), bits(whole[k]))
    assert np.array_equal(bits(via_lists(sup, Bs[[5, 2, 2]], cpu=True)), bits(whole[[5, 2, 2]]))


def test_submatrix_form_with_repeated_indices_equals_raw(sup):
    rng = np.random.default_rng(5)
    U = rng.standard_normal((9, 11)) + 1j * rng.standard_normal((9, 11))
    n, count = 6, 17
    rows = rng.integers(0, 9, (count, n))
    cols = rng.integers(0, 11, (count, n - 1))
    rows[:, -1] = rows[:, 0]  # every list repeats an entry
    cols[:, 1] = cols[:, 0]
    got = sup.perman_complex_minors_submatrices(U, rows, cols, cpu=True)
    assert got.shape == (count, n)
    for k in range(count):
        raw = sup.perman_complex_minors(U[np.ix_(rows[k], cols[k])], cpu=True)
        assert np.array_equal(bits(got[k]), bits(raw)), k
    # rows 0 and n - 1 are equal: the minors that drop one or the other are the same number
    # (not the same bits: their products associate differently)
    assert np.allclose(got[:, 0], got[:, -1], rtol=1e-12, atol=0)


@pytest.mark.parametrize("k", [1, 3])
def test_aligned_ranges_fold_to_the_whole(sup, k):
    """n = 15 rows (order 14) has 2 wave-chunks in the default layout (k = 1);
    walk_log2 = 4 gives the 8 that k = 3 needs."""
    n = 15
    q = n - 1
    B = random_minors_case(n, 54)[0]
    L, m, h = sup.layout(q)
    w = 0 if h >= k else 4
    chunks = 1 << (h if w == 0 else q - 1 - L - w)
    step = chunks >> k
    assert step >= 1
    parts = [sup.perman_complex_minors_range(B, i * step, (i + 1) * step, cpu=True, threads=4, walk_log2=w)
             for i in range(1 << k)]
    while len(parts) > 1:
        parts = [cplx(parts[i].real + parts[i + 1].real, parts[i].imag + parts[i + 1].imag)
                 for i in range(0, len(parts), 2)]
    f = 4 * (q & 1) - 2
    assert np.array_equal(bits(cplx(f * parts[0].real, f * parts[0].imag)),
                          bits(sup.perman_complex_minors(B, cpu=True, walk_log2=w)))


def test_range_stats_and_errors(sup):
    B = random_minors_case(15, 54)[0]
    v, st = sup.perman_complex_minors_range(B, 1, 2, cpu=True, return_stats=True)
    L, m, h = sup.layout(14)
    assert v.shape == (15,) and st["gray_steps"] == 1 << (L + m) and st["est_ops_per_step"] == 16 * 15 - 24
    with pytest.raises(sup.SupError, match="c0 <= c1") as e:
        sup.perman_complex_minors_range(B, 0, (1 << h) + 1, cpu=True)
    assert e.value.code == -1
    with pytest.raises(sup.SupError, match="c0 <= c1"):
        sup.perman_complex_minors_range(B, 2, 1, cpu=True)
    with pytest.raises(sup.SupError, match=r"outside \[2, 32\]") as e:
        sup.perman_complex_minors_range(np.zeros((33, 32)), 0, 1, cpu=True)
    assert e.value.code == -7
    with pytest.raises(sup.SupError, match=r"outside \[2, 32\]") as e:
        sup.perman_complex_minors_range(np.zeros((1, 0)), 0, 1, cpu=True)
    assert e.value.code == -7
    with pytest.raises(sup.SupError, match="walk_log2 = 32"):
        sup.perman_complex_minors_range(B, 0, 1, cpu=True, walk_log2=32)
    lib = sup._lib.load()
    out = (C.c_double * 30)()
    assert lib.sup_perman_complex_minors_range(None, 15, 0, 1, None, 1, out, None) == -1
    assert lib.sup_perman_complex_minors_range(np.ascontiguousarray(B).ctypes.data, 15, 0, 1, None, 1, None, None) == -1


# ---- argument checks -------------------------------------------------------------

def test_empty_batch(sup):
    U = np.ones((3, 3), dtype=np.complex128)
    v, st = sup.perman_complex_minors_submatrices(U, np.zeros((0, 3), dtype=np.int32), np.zeros((0, 2), dtype=np.int32),
                                                  cpu=True, return_stats=True)
    assert v.shape == (0, 3) and v.dtype == np.complex128
    assert st["leaves"] == 0 and st["gray_steps"] == 0


def test_python_argument_errors(sup):
    U = np.ones((3, 4), dtype=np.complex128)
    with pytest.raises(ValueError, match="shape"):
        sup.perman_complex_minors_submatrices(U, np.zeros((2, 3), dtype=int), np.zeros((2, 3), dtype=int), cpu=True)
    with pytest.raises(ValueError, match="integer"):
        sup.perman_complex_minors_submatrices(U, np.zeros((2, 3)), np.zeros((2, 2)), cpu=True)
    with pytest.raises(ValueError, match="n x \\(n-1\\)"):
        sup.perman_complex_minors(np.zeros((3, 3)), cpu=True)
    with pytest.raises(sup.SupError, match="walk_log2 = 40") as e:
        sup.perman_complex_minors(np.ones((4, 3)), cpu=True, walk_log2=40)
    assert e.value.code == -1


def test_index_errors_name_the_offender(sup):
    U = np.ones((3, 4), dtype=np.complex128)
    rows = np.zeros((5, 3), dtype=np.int32)
    cols = np.zeros((5, 2), dtype=np.int32)
    bad = rows.copy()
    bad[3, 2] = 3  # R = 3
    with pytest.raises(sup.SupError, match=r"rows\[k = 3\]\[position 2\] = 3 outside \[0, 3\)") as e:
        sup.perman_complex_minors_submatrices(U, bad, cols, cpu=True)
    assert e.value.code == -1
    bad = cols.copy()
    bad[4, 0] = -1
    with pytest.raises(sup.SupError, match=r"cols\[k = 4\]\[position 0\] = -1 outside \[0, 4\)"):
        sup.perman_complex_minors_submatrices(U, rows, bad, cpu=True)
    bad = cols.copy()
    bad[2, 1] = 4  # C = 4
    with pytest.raises(sup.SupError, match=r"cols\[k = 2\]\[position 1\] = 4 outside \[0, 4\)"):
        sup.perman_complex_minors_submatrices(U, rows, bad, cpu=True)


def test_c_abi_null_and_range_errors(sup):
    lib = sup._lib.load()
    out = (C.c_double * 16)()
    m = np.ones(2 * 2 * 4)
    idx = np.zeros(8, dtype=np.int32)
    u, ix = m.ctypes.data, idx.ctypes.data
    assert lib.sup_perman_complex_minors(None, 2, 2, ix, ix, 2, 2, None, 1, out, None) == -1
    assert lib.sup_perman_complex_minors(u, 2, 2, None, ix, 2, 2, None, 1, out, None) == -1
    assert lib.sup_perman_complex_minors(u, 2, 2, ix, None, 2, 2, None, 1, out, None) == -1  # cols NULL, n = 2
    assert lib.sup_perman_complex_minors(u, 2, 2, ix, ix, 2, 2, None, 1, None, None) == -1
    assert lib.sup_perman_complex_minors(u, 2, 2, ix, ix, 0, 2, None, 1, out, None) == -1
    assert lib.sup_perman_complex_minors(u, 2, 2, ix, ix, 65, 0, None, 1, out, None) == -1
    for R, Cc in ((0, 2), (2, 0)):
        assert lib.sup_perman_complex_minors(u, R, Cc, ix, ix, 2, 2, None, 1, out, None) == -1
    # cols may be NULL when n = 1: ones
    assert lib.sup_perman_complex_minors(u, 2, 2, ix, None, 1, 3, None, 1, out, None) == 0
    assert list(out[:6]) == [1.0, 0.0, 1.0, 0.0, 1.0, 0.0]
    # count == 0 writes nothing
    out[0] = 7.0
    assert lib.sup_perman_complex_minors(u, 2, 2, ix, ix, 2, 0, None, 1, out, None) == 0 and out[0] == 7.0


def test_nan_stays_in_its_own_matrix(sup):
    Bs = batch_B(7, 9, 31)
    clean = via_lists(sup, Bs, cpu=True)
    dirty = Bs.copy()
    dirty[4, 2, 3] = complex(np.nan, 1.0)
    dirty[6, 0, 0] = complex(0.0, np.inf)
    got = via_lists(sup, dirty, cpu=True)
    keep = [k for k in range(9) if k not in (4, 6)]
    assert np.array_equal(bits(got[keep]), bits(clean[keep]))
    # the minor that drops the poisoned row never multiplies by it, but shares the walk: every other one is non-finite
    assert not np.isfinite(np.delete(got[4], 2)).any() and not np.isfinite(np.delete(got[6], 0)).any()


def test_no_device_is_an_error_not_a_cpu_fallback(sup):
    B = batch_B(5, 1, 3)[0]
    if sup.device_count() == 0:
        for call in (lambda: sup.perman_complex_minors(B), lambda: sup.perman_complex_minors_range(B, 0, 1)):
            with pytest.raises(sup.SupError) as e:
                call()
            assert e.value.code == -2
    else:  # a box with a device: the device walk, the host twin's bits
        assert np.array_equal(bits(sup.perman_complex_minors(B)), bits(sup.perman_complex_minors(B, cpu=True)))
