"""sup_perman_complex_quad and sup_perman_complex_quad_range on host threads
(cplx_quad.cpp, the host twin of walk_cplxdd.hip) against exact arithmetic: no
GPU, no oracle.

The accuracy bound is derived, not fitted (complex_range_truth.factor): with
every dd.hpp operation within a relative 2^-103, the error of each part of a
range is at most

    (n^2 + 4n + 2^m + 6 + h) 2^-103 B,
    B = (subsets in range) prod_j sum_c (|Re a_jc| + |Im a_jc|).

The whole call scales the whole range by 4(n&1) - 2, so its bound is twice
that.  A lost low word shows as an error near 2^-53 |value|, far outside it.
"""
import ctypes as C
import math
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import complex_range_truth as CT
import range_truth as T
from test_complex import (as_complex, err_over_scale, exact_perm, gauss_int_case, perman_exe, random_case, walk_bound,
                          write_mtx)

EPS = Fraction(1, 1 << 103)


def _parts(v):
    """((re_hi, re_lo), (im_hi, im_lo)) -> (Fraction re, Fraction im)."""
    return Fraction(v[0][0]) + Fraction(v[0][1]), Fraction(v[1][0]) + Fraction(v[1][1])


def _normalised(v):
    return all(p[0] + p[1] == p[0] or math.isnan(p[0]) for p in v)


def _layout(sup, n, walk_log2=0):
    L, m, _ = sup.layout(n)
    if walk_log2:
        m = min(walk_log2, n - 1 - L)
    return L, m, n - 1 - L - m


def _whole_tol(sup, a, walk_log2=0):
    n = len(a)
    L, m, h = _layout(sup, n, walk_log2)
    return 2 * CT.factor(n, m, h) * EPS * CT.bound(a, 1 << (n - 1))


# ---- closed forms ------------------------------------------------------------

def test_n1_n2_closed_forms(sup):
    assert sup.perman_complex_quad([[3 - 2j]], cpu=True) == ((3.0, 0.0), (-2.0, 0.0))
    a = np.array([[1 + 2j, 3 - 1j], [-2 + 0.5j, 0.25 + 4j]])
    # (1+2i)(0.25+4i) + (3-i)(-2+0.5i) = (-7.75 + 4.5i) + (-5.5 + 3.5i): small dyadic values, exact
    assert sup.perman_complex_quad(a, cpu=True) == ((-13.25, 0.0), (8.0, 0.0))
    # entries that are not dyadic-small: the n = 2 permanent a d + b c to ~2^-100
    b = np.array([[0.1 + 0.3j, 0.7 - 0.2j], [-0.9 + 0.6j, 1.1 + 1.3j]])
    f = lambda z: (Fraction(float(z.real)), Fraction(float(z.imag)))  # noqa: E731
    (ar, ai), (br, bi), (cr, ci), (dr, di) = f(b[0, 0]), f(b[0, 1]), f(b[1, 0]), f(b[1, 1])
    want = (ar * dr - ai * di + br * cr - bi * ci, ar * di + ai * dr + br * ci + bi * cr)
    got = _parts(sup.perman_complex_quad(b, cpu=True))
    tol = _whole_tol(sup, b)
    assert abs(got[0] - want[0]) <= tol and abs(got[1] - want[1]) <= tol


@pytest.mark.parametrize("n,seed", [(10, 31), (16, 32)])
def test_real_input(sup, n, seed):
    """A real matrix: the imaginary pair is exactly (+-0, 0), and the real pair
    is perman_quad's value within the sum of both walks' bounds (perman_quad
    orders its columns by its own planner, so the bits may differ)."""
    a = np.random.default_rng(seed).standard_normal((n, n))
    (re, im) = sup.perman_complex_quad(a, cpu=True)
    assert im[0] == 0.0 and im[1] == 0.0
    qh, ql = sup.perman_quad(a, cpu=True)
    L, m, h = _layout(sup, n)
    tol = 2 * (CT.factor(n, m, h) + T.dd_factor(n, m, h)) * EPS * CT.bound(a, 1 << (n - 1))
    d = abs(Fraction(re[0]) + Fraction(re[1]) - Fraction(qh) - Fraction(ql))
    print(f"n={n} complex quad {re!r} perman_quad {(qh, ql)!r} equal bits {re == (qh, ql)} |diff|/tol {float(d / tol):.3e}")
    assert d <= tol


# ---- Gaussian integers: exact ------------------------------------------------

@pytest.mark.parametrize("n,seed", [(3, 1), (6, 2), (8, 3), (11, 4)])
def test_gaussian_integer_matrices_exact(sup, n, seed):
    """Entries in {-1,0,1} + i{-1,0,1}: 2^n times every term is a Gaussian
    integer of modulus <= (sqrt(2) n)^n < 2^45 at n = 11, far inside 106 bits,
    so hi + lo is the exact Gaussian-integer permanent."""
    a = gauss_int_case(n, seed)
    want = exact_perm(a)
    for kw in ({}, {"threads": 1, "walk_log2": 1}):
        v = sup.perman_complex_quad(a, cpu=True, **kw)
        assert _parts(v) == want and _normalised(v)
    assert complex(v[0][0], v[1][0]) == as_complex(want)


# ---- dense standard-normal complex matrices ---------------------------------

@pytest.mark.parametrize("n,seed,walk_log2", [(4, 21, 0), (9, 22, 0), (12, 23, 0), (14, 41, 0), (14, 41, 4)])
def test_whole_matrix_within_the_bound(sup, n, seed, walk_log2):
    a, truth = random_case(n, seed)[:2]
    v, st = sup.perman_complex_quad(a, cpu=True, walk_log2=walk_log2, return_stats=True)
    L, m, h = _layout(sup, n, walk_log2)
    assert st["lane_bits"] == L and st["walk_bits"] == m and st["gray_steps"] == 1 << (n - 1)
    assert st["est_ops_per_step"] == 86 * n - 28 and st["devices_used"] == 0
    got, tol = _parts(v), _whole_tol(sup, a, walk_log2)
    B2 = 2 * CT.bound(a, 1 << (n - 1))
    e = [abs(got[p] - truth[p]) for p in (0, 1)]
    print(f"n={n} m={m} err/B re {float(e[0] / B2):.3e} im {float(e[1] / B2):.3e} "
          f"bound/B {float(tol / B2):.3e} (2^-103 = {float(EPS):.3e})")
    assert _normalised(v) and e[0] <= tol and e[1] <= tol


RANGE_N = (2, 3, 5, 7, 8, 9, 13, 16, 17, 24, 31, 32, 33, 40, 41, 48, 56, 63, 64)


def range_case(sup, n, walk_log2=3):
    """(matrix, c0, c1, L, m, h): at most 8 chunks of the order-n plan with
    walk_log2 walk bits, from a scattered start above n = 20."""
    a = random_matrix(n)
    L, m, h = _layout(sup, n, walk_log2)
    chunks = T.chunk_count(sup, n, walk_log2)
    assert chunks == 1 << h
    c0 = T.scattered_start(chunks) if n > 20 else 0
    return a, c0, min(chunks, c0 + 8), L, m, h


def random_matrix(n):
    rng = np.random.default_rng(700 + n)
    return rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))


def check_range(a, v, c0, c1, L, m, h, who=""):
    n = len(a)
    truth = CT.range_sum_float(a, L, m, c0, c1)
    B = CT.bound(a, CT.subsets(L, m, c0, c1))
    tol = CT.factor(n, m, h) * EPS * B
    got = _parts(v)
    e = [abs(got[p] - truth[p]) for p in (0, 1)]
    print(f"{who}n={n} m={m} chunks [{c0}, {c1}) err/B re {float(e[0] / B):.3e} im {float(e[1] / B):.3e} "
          f"bound/B {float(tol / B):.3e}")
    assert e[0] <= tol and e[1] <= tol, (n, e, tol)


@pytest.mark.parametrize("n", RANGE_N)
def test_ranges_within_the_bound(sup, n):
    a, c0, c1, L, m, h = range_case(sup, n)
    v, st = sup.perman_complex_quad_range(a, c0, c1, cpu=True, threads=4, walk_log2=3, return_stats=True)
    assert st["lane_bits"] == L and st["walk_bits"] == m and st["gray_steps"] == (c1 - c0) << (L + m)
    assert st["est_ops_per_step"] == 86 * n - 28
    check_range(a, v, c0, c1, L, m, h)


# ---- low words -----------------------------------------------------------------

def test_low_words_of_a_non_dyadic_matrix(sup):
    """All entries 0.1 + 0.1i, order 12: perm = 12! d^12 (1 + i)^12 = -64 12!
    d^12 with d the double 0.1 (the test_quad_tiny_and_degenerate idea): the
    double-double start vector keeps the digits the fp64 one rounds away."""
    a = np.full((12, 12), 0.1 + 0.1j)
    re, im = _parts(sup.perman_complex_quad(a, cpu=True))
    want = -64 * Fraction(479001600) * Fraction(0.1) ** 12
    assert abs(re - want) <= abs(want) * Fraction(1, 2 ** 95)
    assert abs(im) <= abs(want) * Fraction(1, 2 ** 95)


@pytest.mark.parametrize("n,seed", [(9, 22), (14, 41)])
def test_hi_parts_agree_with_the_fp64_walk(sup, n, seed):
    """perman_complex's own bound (test_complex.py: |walk - T| / S <= max(e_np,
    2^-52) (2^m + n)) plus the half ulp by which the hi parts miss T."""
    a, truth, scale, e_np = random_case(n, seed)
    v = sup.perman_complex_quad(a, cpu=True)
    hi = complex(v[0][0], v[1][0])
    f64 = sup.perman_complex(a, cpu=True)
    d = err_over_scale(hi, (Fraction(f64.real), Fraction(f64.imag)), scale)
    print(f"n={n} |hi - fp64 walk| / S = {d:.3e}")
    assert d <= walk_bound(e_np, sup.layout(n)[1], n) + 2.0 ** -53


def test_closer_to_the_truth_than_the_fp64_walk(sup):
    n = 14
    a, truth = random_case(n, 41)[:2]
    q = _parts(sup.perman_complex_quad(a, cpu=True))
    f64 = sup.perman_complex(a, cpu=True)
    dq = (q[0] - truth[0]) ** 2 + (q[1] - truth[1]) ** 2
    df = (Fraction(f64.real) - truth[0]) ** 2 + (Fraction(f64.imag) - truth[1]) ** 2
    print(f"n={n} |quad - T| = {float(dq) ** 0.5:.3e} |fp64 walk - T| = {float(df) ** 0.5:.3e}")
    assert dq < df


# ---- determinism -----------------------------------------------------------------

def test_thread_count_changes_no_bit(sup):
    a = random_case(14, 41)[0]
    v1 = sup.perman_complex_quad(a, cpu=True, threads=1)
    assert v1 == sup.perman_complex_quad(a, cpu=True, threads=3) == sup.perman_complex_quad(a, cpu=True, threads=16)


def _cxdd_add(a, b):
    return T.dd_add(a[0], b[0]), T.dd_add(a[1], b[1])


@pytest.mark.parametrize("k", [1, 3])
def test_aligned_ranges_fold_to_the_whole(sup, k):
    """n = 14 has 2 wave-chunks in the default layout (k = 1 splits those);
    walk_log2 = 4 gives the 8 that k = 3 needs, so both walk lengths are run."""
    n = 14
    a = random_case(n, 41)[0]
    L, m, h = sup.layout(n)
    w = 0 if h >= k else 4
    chunks = T.chunk_count(sup, n, w)
    step = chunks >> k
    assert step >= 1
    parts = [sup.perman_complex_quad_range(a, i * step, (i + 1) * step, cpu=True, threads=4, walk_log2=w)
             for i in range(1 << k)]
    total = T.fold_pairwise(parts, _cxdd_add)
    f = 4 * (n & 1) - 2
    scaled = tuple((f * p[0], f * p[1]) for p in total)
    assert scaled == sup.perman_complex_quad(a, cpu=True, walk_log2=w)
    whole = sup.perman_complex_quad_range(a, 0, chunks, cpu=True, walk_log2=w)
    assert tuple(tuple(p) for p in total) == whole


# ---- argument checks -----------------------------------------------------------------

def test_argument_checks(sup):
    lib = sup._lib.load()
    out = (C.c_double * 4)()
    buf = (C.c_double * (2 * 65 * 65))()
    for n in (0, 65, -1):  # the C ABI's own check (the Python wrapper refuses these first)
        for on_cpu in (0, 1):
            assert lib.sup_perman_complex_quad(buf, n, None, on_cpu, out, None) == -1
            assert lib.sup_perman_complex_quad_range(buf, n, 0, 1, None, on_cpu, out, None) == -1
    assert lib.sup_perman_complex_quad(None, 2, None, 1, out, None) == -1
    assert lib.sup_perman_complex_quad(buf, 2, None, 1, None, None) == -1
    assert lib.sup_perman_complex_quad_range(None, 2, 0, 1, None, 1, out, None) == -1
    assert lib.sup_perman_complex_quad_range(buf, 2, 0, 1, None, 1, None, None) == -1
    for bad in (np.zeros((0, 0)), np.zeros((65, 65)), np.zeros((3, 4)), np.zeros(5)):
        with pytest.raises(ValueError):
            sup.perman_complex_quad(bad, cpu=True)
        with pytest.raises(ValueError):
            sup.perman_complex_quad_range(bad, 0, 1, cpu=True)
    a = random_case(9, 22)[0]
    chunks = T.chunk_count(sup, 9)
    zeros = ((0.0, 0.0), (0.0, 0.0))
    assert sup.perman_complex_quad_range(a, chunks, chunks, cpu=True) == zeros  # empty range
    assert sup.perman_complex_quad_range(a, 0, 0, cpu=True) == zeros
    for c0, c1 in ((0, chunks + 1), (2, 1)):
        with pytest.raises(sup.SupError) as e:
            sup.perman_complex_quad_range(a, c0, c1, cpu=True)
        assert e.value.code == -1
    for w in (32, -1):
        with pytest.raises(sup.SupError) as e:
            sup.perman_complex_quad(a, cpu=True, walk_log2=w)
        assert e.value.code == -1
        with pytest.raises(sup.SupError) as e:
            sup.perman_complex_quad_range(a, 0, 1, cpu=True, walk_log2=w)
        assert e.value.code == -1


def test_nan_propagates(sup):
    a = random_case(9, 22)[0].copy()
    a[3, 4] = complex(float("nan"), 1.0)
    (re, im) = sup.perman_complex_quad(a, cpu=True)
    assert math.isnan(re[0]) and math.isnan(im[0])
    (re, im) = sup.perman_complex_quad_range(a, 0, 1, cpu=True)
    assert math.isnan(re[0]) and math.isnan(im[0])


def test_device_cap_and_no_device(sup):
    """on_cpu = 0: the cap is checked before the device (include/superman.h), so
    n above it is SUP_EUNSUPPORTED on any machine; below it a machine without
    a device answers SUP_ENODEV, never a CPU fallback."""
    cap = sup.COMPLEX_QUAD_MAX_DEVICE_N
    assert cap == 40
    big = random_matrix(cap + 1)
    for call in (lambda: sup.perman_complex_quad(big), lambda: sup.perman_complex_quad_range(big, 0, 1)):
        with pytest.raises(sup.SupError) as e:
            call()
        assert e.value.code == -7 and str(cap) in str(e.value)
    # the host twin serves it
    assert _normalised(sup.perman_complex_quad_range(big, 0, 1, cpu=True, walk_log2=1))
    a = random_case(4, 21)[0]
    if sup.device_count() == 0:
        for call in (lambda: sup.perman_complex_quad(a), lambda: sup.perman_complex_quad_range(a, 0, 1)):
            with pytest.raises(sup.SupError) as e:
                call()
            assert e.value.code == -2
    else:  # a box with a device: the device walk, the host twin's bits
        assert sup.perman_complex_quad(a) == sup.perman_complex_quad(a, cpu=True)


# ---- CLI -------------------------------------------------------------------------------

def _mtx(tmp_path, a):
    n = len(a)
    ent = [(i + 1, j + 1, float(a[i, j].real), float(a[i, j].imag)) for i in range(n) for j in range(n)]
    return write_mtx(tmp_path / "m.mtx", "general", n, ent)


def test_cli_complex_quad_cpu(sup, tmp_path):
    a = random_case(9, 22)[0]
    path = _mtx(tmp_path, a)
    want = sup.perman_complex_quad(a, cpu=True)
    for extra in ([], ["--complex"]):  # --complex beside it changes nothing
        r = subprocess.run([perman_exe(sup), "-f", path, "--complex-quad", "-c", "-t", "3"] + extra,
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        line = [l for l in r.stdout.splitlines() if l.startswith("Permanent (double-double):")][0].split()
        assert tuple(float(x) for x in line[2:6]) == want[0] + want[1]
        assert "Result: cpu_perman64_complex_quad" in r.stdout


@pytest.mark.parametrize("opt", [["-s"], ["-o"], ["-u", "2"], ["-E"], ["-q"], ["-a"], ["-b"], ["-i"], ["-r", "1"]])
def test_cli_complex_quad_refused_pairs(sup, tmp_path, opt):
    path = write_mtx(tmp_path / "m.mtx", "general", 2, [(1, 1, 1.0, 0.0), (2, 2, 1.0, 1.0)])
    r = subprocess.run([perman_exe(sup), "-f", path, "--complex-quad", "-c"] + opt, capture_output=True, text=True)
    assert r.returncode == 1
    assert "--complex-quad" in r.stderr and opt[0] in r.stderr
