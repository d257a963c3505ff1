"""sup_perman_quad_range on host threads (cpu_dd_range behind quad.cpp's
planner and both plan forms) against exact rational arithmetic
(range_truth.py): no GPU, no oracle.

The accuracy bound is derived, not fitted: with every dd.hpp operation within
a relative 2^-103, a range's error is at most

    (n^2 + 2n + 2^m + 6 + h) 2^-103 B,   B = (subsets in range) prod_j sum_c |a_jc|

(n^2 column adds, 2n products, 2^m sequential accumulations per lane, 6 + h
levels of the lane butterfly and the chunk tree).  A lost low word shows as an
error near 2^-53 |value|, far outside it."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

import range_truth as T

FORMS = (1, 2)
EPS = Fraction(1, 1 << 103)


def _value(v):
    return Fraction(v[0]) + Fraction(v[1])


def _tol(a, info, c0, c1):
    n = len(a)
    h = n - 1 - info["L"] - info["m"]
    return T.dd_factor(n, info["m"], h) * EPS * T.dd_bound(a, T.subsets(info["L"], info["m"], c0, c1))


@pytest.mark.parametrize("n", range(1, 11))
def test_whole_range_is_the_whole_call(sup, n):
    rng = np.random.default_rng(60 + n)
    a = rng.uniform(-1, 1, (n, n))
    chunks = T.chunk_count(sup, n)
    (hi, lo), info = sup.perman_quad_range(a, 0, chunks, cpu=True, threads=3)
    f = 4.0 * (n & 1) - 2.0
    whole, st = sup.perman_quad(a, cpu=True, threads=2, return_stats=True)
    assert (f * hi, f * lo) == whole
    assert (st["walk_kind"], st["lane_bits"], st["walk_bits"]) == (info["walk_kind"], info["L"], info["m"])
    assert st["est_ops_per_step"] == info["est_ops_per_step"] > 0
    if info["walk_kind"] == 0:
        assert st["est_ops_per_step"] == 16 * n + 13
    # the sign convention, against fractions at full rational precision
    fr = [[Fraction(float(v)) for v in row] for row in a]
    truth = T.range_sum(fr, info["colmap"], info["L"], info["m"], 0, chunks)
    assert truth == T.range_sum_float(a, info["colmap"], info["L"], info["m"], 0, chunks)
    assert (4 * (n & 1) - 2) * truth == T.permanent(fr)
    assert abs(_value((hi, lo)) - truth) <= _tol(a, info, 0, chunks)


@pytest.mark.parametrize("n", [16, 19])
@pytest.mark.parametrize("walk_log2", [0, 1, 4])
def test_range_algebra(sup, n, walk_log2):
    a = T.sparse_int_matrix(n, 100 + n).astype(np.float64)
    a[n // 2] *= 0.1
    chunks = T.chunk_count(sup, n, walk_log2)
    for form in FORMS:
        whole, info = sup.perman_quad_range(a, 0, chunks, cpu=True, walk_log2=walk_log2, form=form)
        assert info["m"] == (walk_log2 or sup.layout(n)[1]) and info["walk_kind"] == form - 1
        assert whole[1] != 0.0
        for pieces in (2, 4, 8):
            step = chunks // pieces
            parts = [sup.perman_quad_range(a, i * step, (i + 1) * step, cpu=True, threads=1 + i,
                                           walk_log2=walk_log2, form=form)[0] for i in range(pieces)]
            assert T.fold_pairwise(parts, T.dd_add) == whole, (form, pieces)
        # the unaligned range [3, 11) (to the plan's end where it has fewer chunks) is another
        # summation order: against truth only (at most 2^15 subsets)
        lo, hi = 3, min(11, chunks)
        v, _ = sup.perman_quad_range(a, lo, hi, cpu=True, walk_log2=walk_log2, form=form)
        ints = T.doubled(T.sparse_int_matrix(n, 100 + n))
        assert T.subsets(info["L"], info["m"], lo, hi) <= 1 << 15
        truth = Fraction(0.1) * Fraction(T.range_sum(ints, info["colmap"], info["L"], info["m"], lo, hi), 1 << n)
        assert abs(_value(v) - truth) <= _tol(a, info, lo, hi), (form, lo, hi)


@pytest.mark.parametrize("n", [33, 41, 57, 63, 64])
def test_truth_by_range_at_large_n(sup, n):
    """Eight chunks high in the chunk space, both kernels' host twins.  One row
    is scaled by 0.1 (not a double-double either), so the low words carry
    digits; the permanent is linear in a row, so the truth is that of the
    integer matrix times the double 0.1."""
    ai = T.sparse_int_matrix(n, 200 + n)
    a = ai.astype(np.float64)
    a[n // 2] *= 0.1
    chunks = T.chunk_count(sup, n, 4)
    c0 = T.scattered_start(chunks)
    truth = {}
    for form in FORMS:
        v, info = sup.perman_quad_range(a, c0, c0 + 8, cpu=True, walk_log2=4, form=form)
        assert (info["L"], info["m"], info["walk_kind"]) == (6, 4, form - 1) and info["gray_steps"] == 8 << 10
        key = tuple(info["colmap"])
        if key not in truth:
            truth[key] = Fraction(0.1) * Fraction(T.range_sum(T.doubled(ai), info["colmap"], 6, 4, c0, c0 + 8), 1 << n)
        assert abs(_value(v) - truth[key]) <= _tol(a, info, c0, c0 + 8), form


def _real_matrix(kind, n, seed):
    rng = np.random.default_rng(seed)
    if kind == "positive":
        return rng.uniform(0.5, 1.5, (n, n))
    if kind == "mixed":
        return rng.uniform(-1.0, 1.0, (n, n))
    return rng.uniform(0.5, 1.0, (n, n)) * np.exp2(rng.integers(-20, 21, (n, n))) * rng.choice([-1.0, 1.0], (n, n))


@pytest.mark.parametrize("kind", ["positive", "mixed", "wide"])
@pytest.mark.parametrize("n", [6, 9, 12])
def test_dd_against_rational_truth(sup, kind, n):
    a = _real_matrix(kind, n, 10 * n + len(kind))
    chunks = T.chunk_count(sup, n)
    for form in FORMS:
        if form == 2 and sup.layout(n)[1] == 0:
            continue  # n = 6: no walk bits, the blocked kernel is refused (test_errors)
        v, info = sup.perman_quad_range(a, 0, chunks, cpu=True, form=form)
        truth = T.range_sum_float(a, info["colmap"], info["L"], info["m"], 0, chunks)
        tol = _tol(a, info, 0, chunks)
        err = abs(_value(v) - truth)
        print(f"dd range n={n} {kind} form={form}: error/tolerance = {float(err / tol):.3e}")
        assert err <= tol, (form, float(err / tol))
        if kind == "positive":  # the tolerance itself is far below one fp64 ulp of the value
            assert tol < abs(truth) * Fraction(1, 1 << 64)


def test_errors(sup):
    lib = sup._lib.load()
    a = np.random.default_rng(3).uniform(-1, 1, (9, 9))
    chunks = T.chunk_count(sup, 9)

    def refused(match, *args, **kw):
        with pytest.raises(sup.SupError, match=match) as e:
            sup.perman_quad_range(*args, cpu=True, **kw)
        assert e.value.code == -1

    refused("c0 <= c1", a, 2, 1)
    refused("c0 <= c1", a, 0, chunks + 1)
    refused("walk_log2", a, 0, 1, walk_log2=32)
    refused("walk_log2", a, 0, 1, walk_log2=-1)
    refused("form", a, 0, 1, form=3)
    for n in range(1, 8):
        refused("form 2", np.ones((n, n)), 0, 1, form=2)
    assert sup.perman_quad_range(a, 1, 1, cpu=True)[0] == (0.0, 0.0)
    hi, lo = C.c_double(0.0), C.c_double(0.0)

    def raw(mat=a.ctypes.data, n=9, c0=0, c1=1, out_hi=C.byref(hi), out_lo=C.byref(lo)):
        return lib.sup_perman_quad_range(mat, 2, n, c0, c1, None, 1, 0, out_hi, out_lo, None, None)

    assert raw() == 0
    assert raw(mat=None) == -1 and raw(out_hi=None) == -1 and raw(out_lo=None) == -1
    assert raw(n=0) == -1 and raw(n=65) == -1 and raw(n=-1) == -1
