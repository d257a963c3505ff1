"""Exact Gaussian-integer permanents (sup_perman_complex_exact,
sup_perman_complex_exact_range) on the host twin: no GPU needed.

All truth is Python integers (complex_exact_cases.py, complex_range_truth.py):
closed forms that are exact at any n, a Ryser sum in Python ints for n <= 12,
and range_sum on the doubled matrix for ranges.  The last section judges the
fp64 and double-double complex walks against the exact entry, within the
bounds test_complex.py and test_complex_quad.py derive for those walks.
"""
import ctypes as C
import subprocess
from fractions import Fraction
from math import factorial

import numpy as np
import pytest

import complex_exact_cases as X
import complex_range_truth as CT
import range_truth as T
from test_complex import err_over_scale, gauss_int_case, np_ryser, perman_exe, walk_bound, write_mtx
from test_complex_quad import _parts, _whole_tol


def exact(sup, A, **kw):
    return sup.perman_complex_exact(X.as_array(A), cpu=True, **kw)


# ---- closed forms at n = 1, 2, 3 and a zero row --------------------------------------

def test_small_closed_forms(sup):
    assert exact(sup, [[(3, -2)]]) == (3, -2)
    assert exact(sup, [[(0, -5)]]) == (0, -5)  # purely imaginary
    assert exact(sup, [[(-7, 0)]]) == (-7, 0)  # negative
    # (1+2i)(-3+i) + (2-i)(4i) = (-5-5i) + (4+8i)
    assert exact(sup, [[(1, 2), (2, -1)], [(0, 4), (-3, 1)]]) == (-1, 3)
    # a diagonal: i * i * (-1) = 1; an anti-diagonal of i: i^3 = -i
    assert exact(sup, [[(0, 1), (0, 0), (0, 0)], [(0, 0), (0, 1), (0, 0)], [(0, 0), (0, 0), (-1, 0)]]) == (1, 0)
    assert exact(sup, [[(0, 0), (0, 0), (0, 1)], [(0, 0), (0, 1), (0, 0)], [(0, 1), (0, 0), (0, 0)]]) == (0, -1)
    A = [[(1, 1), (2, 0), (0, -3)], [(-1, 2), (0, 1), (4, 0)], [(2, -2), (1, 1), (-1, -1)]]
    assert exact(sup, A) == X.ryser(A)


def test_zero_row_is_zero_without_a_walk(sup):
    A = X.random_gauss(9, 3)
    A[4] = [(0, 0)] * 9
    v, st = exact(sup, A, return_stats=True)
    assert v == (0, 0) and st["gray_steps"] == 0 and st["kernel_ms"] == 0.0
    # the range entry walks it like any other matrix: every term is zero
    r = sup.perman_complex_exact_range(X.as_array(A), 0, 1, cpu=True)
    assert r["re"] == [0] * len(r["primes"]) and r["im"] == r["re"] and r["primes"]


# ---- against a Ryser sum in Python ints ---------------------------------------------------

@pytest.mark.parametrize("n,seed", [(4, 1), (7, 2), (8, 3), (9, 4), (12, 5)])
def test_random_against_brute_force(sup, n, seed):
    A = X.random_gauss(n, seed, -9, 9)
    v, st = exact(sup, A, return_stats=True)
    assert v == X.ryser(A)
    L, m, _ = sup.layout(n)
    G = st["seg_pair_bits"]
    assert G in (1, 2) and st["lane_bits"] == L and st["walk_bits"] == m and st["gray_steps"] == 1 << (n - 1)
    assert st["devices_used"] == 0 and st["leaves"] == 1
    primes = len(sup.perman_complex_exact_range(X.as_array(A), 0, 0, cpu=True)["primes"])
    assert st["est_ops_per_step"] == X.expected_ops(n, G, primes)


# ---- the three closed forms -------------------------------------------------------------------

@pytest.mark.parametrize("n", [16, 24])
@pytest.mark.parametrize("form", X.CLOSED_FORMS, ids=lambda f: f.__name__)
def test_closed_forms_whole(sup, form, n):
    A, want = form(n)
    assert exact(sup, A) == want


@pytest.mark.parametrize("n", [33, 48, 64])
@pytest.mark.parametrize("form", X.CLOSED_FORMS, ids=lambda f: f.__name__)
def test_closed_form_matrices_by_range(sup, form, n):
    """The same matrices at the large orders: at most 8 chunks of the walk
    against range_sum, both G."""
    A = form(n)[0]
    L, m, h = X.layout(sup, n)
    c0 = T.scattered_start(1 << h)
    truth = CT.range_sum(X.doubled(A), L, m, c0, c0 + 8)
    for G in (1, 2):
        r = sup.perman_complex_exact_range(X.as_array(A), c0, c0 + 8, group=G, cpu=True, walk_log2=X.WALK_LOG2)
        assert X.residues_match(r, truth), (n, G)


# ---- instance by instance -------------------------------------------------------------------------

@pytest.mark.parametrize("n", range(1, 65))
def test_every_order_both_groups(sup, n):
    """Every N, G = 1 and 2, at most 8 chunks from a scattered start with 3
    walk bits: the residues equal range_sum(2A) mod p for every prime."""
    a = X.as_array(X.instance(n))
    L, m, c0, c1 = X.instance_range(sup, n)
    truth = X.instance_truth(sup, n)
    for G in (1, 2):
        r, st = sup.perman_complex_exact_range(a, c0, c1, group=G, cpu=True, walk_log2=X.WALK_LOG2, return_stats=True)
        assert X.residues_match(r, truth), (n, G)
        assert st["seg_pair_bits"] == G and st["lane_bits"] == L and st["walk_bits"] == m
        assert st["gray_steps"] == (c1 - c0) << (L + m)
        assert st["est_ops_per_step"] == X.expected_ops(n, G, len(r["primes"]))


# ---- real input -----------------------------------------------------------------------------------

@pytest.mark.parametrize("n,seed", [(5, 1), (12, 2), (18, 3)])
def test_real_input_equals_perman_exact(sup, n, seed):
    a = np.random.default_rng(seed).integers(-4, 5, (n, n))
    want = int(sup.perman_exact(a.astype(np.int32), cpu=True))
    assert sup.perman_complex_exact(a, cpu=True) == (want, 0)
    assert sup.perman_complex_exact(a.astype(np.float64), cpu=True) == (want, 0)


# ---- the edge of the exactness inequality ---------------------------------------------------

@pytest.mark.parametrize("k,G,pbits", [(27, 1, 20), (26, 1, 21), (11, 2, 20)])
def test_extreme_entries_at_the_eligibility_edge(sup, k, G, pbits):
    """Every entry (2^k - 1)(1 + i) at n = 6: the row bound 12 (2^k - 1) puts
    xbits at the edge of G (G = 1: xbits 31 / 30, primes of 20 / 21 bits, the
    largest residue-times-row products the inequality admits; G = 2: xbits 15,
    primes of 20 bits).  One bit off in the bound and a product rounds."""
    n, v = 6, (1 << k) - 1
    A = [[(v, v)] * n for _ in range(n)]
    c = X.cpow((v, v), n)
    want = (factorial(n) * c[0], factorial(n) * c[1])
    assert X.ryser(A) == want
    r = sup.perman_complex_exact_range(X.as_array(A), 0, 1, group=G, cpu=True)
    assert all(p.bit_length() == pbits for p in r["primes"])
    assert X.residues_match(r, CT.range_sum(X.doubled(A), *sup.layout(n)[:2], 0, 1))
    assert exact(sup, A) == want
    if G == 2:  # one more bit and G = 2 is not eligible
        w = (1 << (k + 1)) - 1
        big = [[(w, w)] * n for _ in range(n)]
        with pytest.raises(sup.SupError) as e:
            sup.perman_complex_exact_range(X.as_array(big), 0, 1, group=2, cpu=True)
        assert e.value.code == -1 and "xbits = 16" in str(e.value)
        c = X.cpow((w, w), n)  # the cost model falls back to G = 1
        assert exact(sup, big) == (factorial(n) * c[0], factorial(n) * c[1])


# ---- several launches' worth of primes; the every-256-steps fold ---------------------------------

def test_more_primes_than_one_launch(sup):
    n = 12
    A = X.random_gauss(n, 11, -(1 << 20), 1 << 20)
    r = sup.perman_complex_exact_range(X.as_array(A), 0, 0, cpu=True)
    assert len(r["primes"]) >= 9  # more than two launches of 4
    assert exact(sup, A) == X.ryser(A)


def test_long_walks_fold_the_accumulator(sup):
    """walk_log2 = 9 at n = 16: 512 steps per lane, so acc is folded inside the walk."""
    n = 16
    A = X.random_gauss(n, 12)
    L, m, h = X.layout(sup, n, 9)
    assert m == 9
    truth = CT.range_sum(X.doubled(A), L, m, 0, 1)
    for G in (1, 2):
        r = sup.perman_complex_exact_range(X.as_array(A), 0, 1, group=G, cpu=True, walk_log2=9)
        assert X.residues_match(r, truth)


# ---- threads and splits -----------------------------------------------------------------------------------

def test_threads_and_aligned_ranges(sup):
    n = 17
    a = X.as_array(X.random_gauss(n, 13))
    chunks = T.chunk_count(sup, n, 3)
    whole = sup.perman_complex_exact_range(a, 0, chunks, cpu=True, walk_log2=3, threads=16)
    for threads in (1, 3):
        assert sup.perman_complex_exact_range(a, 0, chunks, cpu=True, walk_log2=3, threads=threads) == whole
    assert sup.perman_complex_exact(a, cpu=True, threads=1) == sup.perman_complex_exact(a, cpu=True, threads=3)
    k = chunks // 4
    parts = [sup.perman_complex_exact_range(a, i * k, (i + 1) * k, cpu=True, walk_log2=3) for i in range(4)]
    for part in ("re", "im"):
        tot = [sum(p[part][q] for p in parts) % whole["primes"][q] for q in range(len(whole["primes"]))]
        assert tot == whole[part]
    # the whole range is T: CRT of it, scaled, is the permanent
    tr = T.crt_signed(whole["re"], whole["primes"])
    ti = T.crt_signed(whole["im"], whole["primes"])
    s = 1 if n & 1 else -1
    assert (s * tr // (1 << (n - 1)), s * ti // (1 << (n - 1))) == sup.perman_complex_exact(a, cpu=True)
    assert tr % (1 << (n - 1)) == 0 and ti % (1 << (n - 1)) == 0


# ---- every SUP_EINVAL, with its message ---------------------------------------------------------------

def _einval(sup, call, *words):
    with pytest.raises(sup.SupError) as e:
        call()
    assert e.value.code == -1, str(e.value)
    for w in words:
        assert w in str(e.value), str(e.value)


def test_input_limits(sup):
    base = X.as_array(X.random_gauss(5, 21))
    both = (lambda a: sup.perman_complex_exact(a, cpu=True),
            lambda a: sup.perman_complex_exact_range(a, 0, 1, cpu=True))
    a = base.copy()
    a[1, 2] = complex(3.0, 0.5)
    for f in both:
        _einval(sup, lambda: f(a), "row 1, column 2, Im part", "not an integer")
    a = base.copy()
    a[3, 0] = complex(float("nan"), 1.0)
    for f in both:
        _einval(sup, lambda: f(a), "row 3, column 0, Re part", "not an integer")
    a = base.copy()
    a[0, 4] = complex(1.0, float("inf"))
    for f in both:
        _einval(sup, lambda: f(a), "row 0, column 4, Im part", "not an integer")
    a = base.copy()
    a[2, 2] = complex(-(2.0 ** 31), 0.0)
    for f in both:
        _einval(sup, lambda: f(a), "row 2, column 2, Re part", "out of range")
    a[2, 2] = complex(2.0 ** 31 - 1, 0.0)  # the largest part, alone in range; its row bound is not
    a[2, 3] = complex(0.0, -1.0)
    for f in both:
        _einval(sup, lambda: f(a), "row 2", ">= 2^31")
    a = np.zeros((2, 2), dtype=np.complex128)
    a[0] = complex(2.0 ** 29, 2.0 ** 29)  # row bound exactly 2^31
    a[1] = 1.0
    for f in both:
        _einval(sup, lambda: f(a), "row 0", ">= 2^31")
    a[0, 0] = complex(2.0 ** 29 - 1, 2.0 ** 29)  # 2^31 - 1: accepted
    assert sup.perman_complex_exact(a, cpu=True) == (2 ** 30 - 1, 2 ** 30)


def test_python_integers_are_not_rounded(sup):
    big = np.array([[2 ** 53 + 1, 1], [1, 1]], dtype=np.int64)
    for call in (lambda: sup.perman_complex_exact(big, cpu=True),
                 lambda: sup.perman_complex_exact_range(big, 0, 1, cpu=True),
                 lambda: sup.perman_complex_exact([[2 ** 70, 1], [1, 1]], cpu=True)):
        _einval(sup, call, "not exactly representable")
    # below 2^53 the value reaches the library as it is, and is out of range there
    _einval(sup, lambda: sup.perman_complex_exact(np.array([[2 ** 40, 1], [1, 1]], dtype=np.int64), cpu=True),
            "out of range")
    assert sup.perman_complex_exact(np.array([[2, 1], [1, 3]], dtype=np.int64), cpu=True) == (7, 0)
    for bad in (np.zeros((0, 0)), np.zeros((65, 65)), np.zeros((3, 4)), np.zeros(5)):
        with pytest.raises(ValueError):
            sup.perman_complex_exact(bad, cpu=True)


def test_range_entry_arguments(sup):
    a = X.as_array(X.random_gauss(9, 22))
    chunks = T.chunk_count(sup, 9)
    for g in (3, 4, -1):
        _einval(sup, lambda: sup.perman_complex_exact_range(a, 0, 1, group=g, cpu=True), f"group = {g}")
    _einval(sup, lambda: sup.perman_complex_exact_range(a, 0, 1, cpu=True, cap=1), "cap = 1 but this walk has")
    for c0, c1 in ((0, chunks + 1), (2, 1)):
        _einval(sup, lambda: sup.perman_complex_exact_range(a, c0, c1, cpu=True), "c0 <= c1 <=")
    for w in (32, -1):
        _einval(sup, lambda: sup.perman_complex_exact_range(a, 0, 1, cpu=True, walk_log2=w), "walk_log2")
    for c in (0, chunks):  # an empty range: zeros
        r = sup.perman_complex_exact_range(a, c, c, cpu=True)
        assert r["primes"] and not any(r["re"]) and not any(r["im"])


def test_c_abi_checks(sup):
    lib = sup._lib.load()
    last = lambda: lib.sup_last_error().decode()  # noqa: E731
    buf = (C.c_double * (2 * 65 * 65))()
    re, im = C.create_string_buffer(640), C.create_string_buffer(640)
    pr, rr, ri = (C.c_uint64 * 64)(), (C.c_uint64 * 64)(), (C.c_uint64 * 64)()
    k = C.c_int(0)
    for n in (0, 65, -1):
        for on_cpu in (0, 1):
            assert lib.sup_perman_complex_exact(buf, n, None, on_cpu, re, im, 640, None) == -1
            assert "outside [1, 64]" in last()
            assert lib.sup_perman_complex_exact_range(buf, n, 0, 1, None, on_cpu, 0, pr, rr, ri, 64, C.byref(k),
                                                      None) == -1
    for args in ((None, 2, None, 1, re, im, 640, None), (buf, 2, None, 1, None, im, 640, None),
                 (buf, 2, None, 1, re, None, 640, None)):
        assert lib.sup_perman_complex_exact(*args) == -1 and "null" in last()
    for args in ((None, pr, rr, ri, C.byref(k)), (buf, None, rr, ri, C.byref(k)), (buf, pr, None, ri, C.byref(k)),
                 (buf, pr, rr, None, C.byref(k)), (buf, pr, rr, ri, None)):
        assert lib.sup_perman_complex_exact_range(args[0], 2, 0, 1, None, 1, 0, args[1], args[2], args[3], 64,
                                                  args[4], None) == -1 and "null" in last()
    # a short buffer: the needed length in the message; one that just fits
    a = X.as_array(X.const_matrix(8, (3, 4))[0])
    want = X.const_matrix(8, (3, 4))[1]
    need = max(len(str(want[0])), len(str(want[1]))) + 1
    assert lib.sup_perman_complex_exact(a.ctypes.data, 8, None, 1, re, im, need - 1, None) == -1
    assert f"needs {need} bytes" in last()
    assert lib.sup_perman_complex_exact(a.ctypes.data, 8, None, 1, re, im, need, None) == 0
    assert (int(re.value), int(im.value)) == want


def test_device_cap_before_the_device(sup):
    """on_cpu = 0: the input limits first, then the cap (SUP_EUNSUPPORTED on any
    machine), then the device (SUP_ENODEV here: never a CPU fallback)."""
    cap = sup.COMPLEX_EXACT_MAX_DEVICE_N
    assert 1 <= cap <= 64
    small = X.as_array(X.random_gauss(4, 23))
    if cap < 64:
        big = X.as_array(X.instance(cap + 1))
        for call in (lambda: sup.perman_complex_exact(big), lambda: sup.perman_complex_exact_range(big, 0, 1)):
            with pytest.raises(sup.SupError) as e:
                call()
            assert e.value.code == -7 and str(cap) in str(e.value)
        bad = big.copy()
        bad[0, 0] = 0.5  # an input error wins over the cap
        _einval(sup, lambda: sup.perman_complex_exact(bad), "not an integer")
        # the host twin serves it
        L, m, c0, c1 = X.instance_range(sup, cap + 1)
        r = sup.perman_complex_exact_range(big, c0, c1, cpu=True, walk_log2=X.WALK_LOG2)
        assert X.residues_match(r, X.instance_truth(sup, cap + 1))
    if sup.device_count() == 0:
        for call in (lambda: sup.perman_complex_exact(small), lambda: sup.perman_complex_exact_range(small, 0, 1)):
            with pytest.raises(sup.SupError) as e:
                call()
            assert e.value.code == -2
    else:
        assert sup.perman_complex_exact(small) == sup.perman_complex_exact(small, cpu=True)


# ---- judging the floating walks ---------------------------------------------------------------------------------

@pytest.mark.parametrize("n,seed", [(14, 51), (16, 52)])
def test_floating_walks_against_the_exact_permanent(sup, n, seed):
    """Entries in {-1, 0, 1} + {-1, 0, 1} i.  The double-double walk within
    test_complex_quad.py's bound 2 factor 2^-103 B per part, the fp64 walk
    within test_complex.py's max(e_np, 2^-52) (2^m + n) S, both measured from
    the exact integers."""
    a = gauss_int_case(n, seed)
    er, ei = sup.perman_complex_exact(a, cpu=True)
    truth = (Fraction(er), Fraction(ei))
    q = _parts(sup.perman_complex_quad(a, cpu=True))
    tol = _whole_tol(sup, a)
    dq = [abs(q[p] - truth[p]) for p in (0, 1)]
    v_np, scale = np_ryser(a)
    e_np = err_over_scale(v_np, truth, scale)
    m = sup.layout(n)[1]
    e_walk = err_over_scale(sup.perman_complex(a, cpu=True), truth, scale)
    print(f"n={n} exact {er} {ei} dd err {float(dq[0]):.3e} {float(dq[1]):.3e} tol {float(tol):.3e} "
          f"fp64 e_walk {e_walk:.3e} e_np {e_np:.3e} bound {walk_bound(e_np, m, n):.3e}")
    assert dq[0] <= tol and dq[1] <= tol
    assert e_walk <= walk_bound(e_np, m, n)


# ---- CLI ------------------------------------------------------------------------------------------------------------

def _mtx(tmp_path, A):
    n = len(A)
    ent = [(i + 1, j + 1, float(A[i][j][0]), float(A[i][j][1])) for i in range(n) for j in range(n)]
    return write_mtx(tmp_path / "m.mtx", "general", n, ent)


def test_cli_complex_exact_cpu(sup, tmp_path):
    A, want = X.const_matrix(9, (2, -1))
    path = _mtx(tmp_path, A)
    for extra in ([], ["--complex"]):  # --complex beside it changes nothing
        r = subprocess.run([perman_exe(sup), "-f", path, "--complex-exact", "-c", "-t", "3"] + extra,
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        line = [l for l in r.stdout.splitlines() if l.startswith("Permanent (exact):")][0].split()
        assert (int(line[2]), int(line[3])) == want
        res = [l for l in r.stdout.splitlines() if l.startswith("Result: cpu_perman64_complex_exact")][0].split()
        assert float(res[2]) == pytest.approx(float(want[0]), rel=1e-5)
        assert float(res[3]) == pytest.approx(float(want[1]), rel=1e-5)


@pytest.mark.parametrize("opt", [["-s"], ["-o"], ["-u", "2"], ["-E"], ["-q"], ["-a"], ["-b"], ["-i"], ["-r", "1"],
                                 ["--complex-quad"]])
def test_cli_complex_exact_refused_pairs(sup, tmp_path, opt):
    path = write_mtx(tmp_path / "m.mtx", "general", 2, [(1, 1, 1.0, 0.0), (2, 2, 1.0, 1.0)])
    r = subprocess.run([perman_exe(sup), "-f", path, "--complex-exact", "-c"] + opt, capture_output=True, text=True)
    assert r.returncode == 1
    assert "--complex-exact" in r.stderr and opt[0] in r.stderr


def test_cli_non_integer_file(sup, tmp_path):
    path = write_mtx(tmp_path / "m.mtx", "general", 2, [(1, 1, 1.0, 0.0), (2, 2, 1.5, 1.0), (1, 2, 1.0, 0.0),
                                                         (2, 1, 2.0, 0.0)])
    r = subprocess.run([perman_exe(sup), "-f", path, "--complex-exact", "-c"], capture_output=True, text=True)
    assert r.returncode == 1
    assert "row 1, column 1, Re part" in r.stderr and "not an integer" in r.stderr
