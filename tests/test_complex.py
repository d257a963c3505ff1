"""Complex-matrix permanents on host threads (cplx.cpp, the host twin of
walk_cplx.hip, through perman_complex(cpu=True)), the complex MatrixMarket
reader and the CLI's --complex.

The reference cannot compute complex permanents, so truth is computed here by
exact arithmetic: every fp64 input is a dyadic rational, so the matrix times a
power of two is a matrix of Gaussian integers whose permanent Ryser's formula
gives exactly in Python integers.
"""
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

PHASES = (1, 1j, -1, -1j)


def exact_perm(a):
    """Exact permanent of a complex128 matrix as (Fraction re, Fraction im):
    Ryser over Python integers on 2^k A (k: the entries' largest dyadic
    denominator), Gray-code order (exact, so the order is immaterial)."""
    a = np.asarray(a, dtype=np.complex128)
    n = a.shape[0]
    fr = [[(Fraction(float(z.real)), Fraction(float(z.imag))) for z in row] for row in a]
    den = max(max(p.denominator for z in row for p in z) for row in fr)
    B = [[(int(z[0] * den), int(z[1] * den)) for z in row] for row in fr]
    sr, si = [0] * n, [0] * n  # row sums over the current subset
    tr = ti = 0
    for g in range(1, 1 << n):
        c = (g & -g).bit_length() - 1
        s = 1 if ((g ^ (g >> 1)) >> c) & 1 else -1
        for i in range(n):
            sr[i] += s * B[i][c][0]
            si[i] += s * B[i][c][1]
        pr, pi = 1, 0
        for i in range(n):
            pr, pi = pr * sr[i] - pi * si[i], pr * si[i] + pi * sr[i]
        if (n - bin(g ^ (g >> 1)).count("1")) & 1:
            pr, pi = -pr, -pi
        tr += pr
        ti += pi
    return Fraction(tr, den ** n), Fraction(ti, den ** n)


def np_ryser(a):
    """The yardstick: plain complex128 Ryser in the Nijenhuis-Wilf form, each
    x(S) formed from scratch by a column-subset sum (no Gray accumulation).
    Returns (value, S = sum over subsets of |prod_j x_j|)."""
    a = np.asarray(a, dtype=np.complex128)
    n = a.shape[0]
    x0 = a[:, n - 1] - a.sum(axis=1) / 2
    total, scale = 0j, 0.0
    for s in range(1 << (n - 1)):
        cols = [c for c in range(n - 1) if (s >> c) & 1]
        x = x0 + a[:, cols].sum(axis=1) if cols else x0
        t = np.prod(x)
        total += -t if len(cols) & 1 else t
        scale += abs(t)
    return complex(total) * (4 * (n & 1) - 2), scale


def err_over_scale(v, truth, scale):
    dr, di = Fraction(v.real) - truth[0], Fraction(v.imag) - truth[1]
    return float(dr * dr + di * di) ** 0.5 / scale


_CASES = {}


def random_case(n, seed):
    """(matrix, exact truth, S, e_np), computed once per (n, seed)."""
    if (n, seed) not in _CASES:
        rng = np.random.default_rng(seed)
        a = rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))
        truth = exact_perm(a)
        v, scale = np_ryser(a)
        _CASES[(n, seed)] = (a, truth, scale, err_over_scale(v, truth, scale))
    return _CASES[(n, seed)]


def gauss_int_case(n, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(-1, 2, (n, n)) + 1j * rng.integers(-1, 2, (n, n))


def as_complex(truth):
    assert truth[0].denominator == 1 and truth[1].denominator == 1
    return complex(int(truth[0]), int(truth[1]))


# ---- (a) closed forms and exact cases -------------------------------------

def test_n1_n2_closed_forms(sup):
    assert sup.perman_complex([[3 - 2j]], cpu=True) == 3 - 2j
    a = np.array([[1 + 2j, 3 - 1j], [-2 + 0.5j, 0.25 + 4j]])
    # (1+2i)(0.25+4i) + (3-i)(-2+0.5i): every product and sum exact in fp64
    assert sup.perman_complex(a, cpu=True) == (-7.75 + 4.5j) + (-5.5 + 3.5j)


def test_diagonal_matrix(sup):
    d = [1 + 1j, 2 - 1j, -3 + 0.5j, 0.5j, 4 + 0j]
    want = 1 + 0j
    for z in d:
        want *= z  # small dyadic values: exact
    assert want == 3 - 19j
    tr, ti = exact_perm(np.diag(d))
    assert want == complex(float(tr), float(ti))
    assert sup.perman_complex(np.diag(d), cpu=True) == want


def test_permutation_times_unit_phases(sup):
    rng = np.random.default_rng(11)
    n = 7
    perm = rng.permutation(n)
    ph = rng.integers(0, 4, n)
    a = np.zeros((n, n), dtype=np.complex128)
    want = 1 + 0j
    for i in range(n):
        a[i, perm[i]] = PHASES[ph[i]]
        want *= PHASES[ph[i]]
    assert sup.perman_complex(a, cpu=True) == want


@pytest.mark.parametrize("n,seed", [(3, 1), (6, 2), (8, 3)])
def test_gaussian_integer_matrices_exact(sup, n, seed):
    """Entries in {-1,0,1} + i{-1,0,1}: the walk's result equals the exact
    Gaussian-integer permanent.  Every intermediate is exactly representable:
    x_j(S) = (sum_c +-a_jc) / 2 has half-integer parts of magnitude <= n / 2,
    so 2 x_j is a Gaussian integer with |2 x_j| <= sqrt(2) n; a product of k
    factors times 2^k is a Gaussian integer of modulus <= (sqrt(2) n)^k, at
    most (sqrt(2) 8)^8 = 2.7e8 at n = 8.  In cx_mul each real product has a
    numerator <= |a| |b| <= 2.7e8 and each fma result one <= 2 |a| |b| < 2^30
    over a power-of-two denominator: exact.  Terms are multiples of 2^-n;
    the accumulator, the lane butterfly and the chunk tree add at most
    2^(n-1) = 128 of them: numerators <= 128 * 2.7e8 = 3.5e10 < 2^53, so every
    sum is exact, and the final factor +-2 is exact."""
    a = gauss_int_case(n, seed)
    want = as_complex(exact_perm(a))
    assert sup.perman_complex(a, cpu=True) == want
    assert sup.perman_complex(a, cpu=True, threads=1, walk_log2=1) == want


# ---- (b) random complex matrices -------------------------------------------

def walk_bound(e_np, m, n):
    return max(e_np, 2.0 ** -52) * (2 ** m + n)


@pytest.mark.parametrize("n,seed", [(4, 21), (9, 22), (12, 23)])
def test_random_complex_against_exact_truth(sup, n, seed):
    """|walk - T| / S <= max(e_np, 2^-52) (2^m + n): the walk accumulates x
    over up to 2^m + n additions where the from-scratch complex128 Ryser makes
    n.  Measured (complex walk): e_np 3.6e-16 / 2.1e-16 / 2.7e-16,
    walk 2.8e-16 / 2.3e-16 / 8.6e-17 at n = 4 / 9 / 12."""
    a, truth, scale, e_np = random_case(n, seed)
    m = sup.layout(n)[1]
    v, st = sup.perman_complex(a, cpu=True, return_stats=True)
    assert st["walk_bits"] == m and st["lane_bits"] == sup.layout(n)[0]
    assert st["gray_steps"] == 1 << (n - 1) and st["est_ops_per_step"] == 6 * n and st["devices_used"] == 0
    e_walk = err_over_scale(v, truth, scale)
    print(f"n={n} m={m} e_np={e_np:.3e} e_walk={e_walk:.3e} bound={walk_bound(e_np, m, n):.3e}")
    assert e_walk <= walk_bound(e_np, m, n)


# ---- (c) real input ---------------------------------------------------------

@pytest.mark.parametrize("n,seed", [(10, 31), (16, 32)])
def test_real_input(sup, n, seed):
    a = np.random.default_rng(seed).standard_normal((n, n))
    v = sup.perman_complex(a, cpu=True)
    assert v.imag == 0.0  # exactly +-0
    want = sup.perman_cpu(a, "dense_plain")
    print(f"n={n} complex walk {v.real!r} dense_plain {want!r} equal bits {v.real == want}")
    assert abs(v.real - want) <= 1e-10 * abs(want)


# ---- (d) determinism --------------------------------------------------------

def test_thread_count_changes_no_bit(sup):
    a = random_case(14, 41)[0]
    v1 = sup.perman_complex(a, cpu=True, threads=1)
    assert v1 == sup.perman_complex(a, cpu=True, threads=3) == sup.perman_complex(a, cpu=True, threads=16)


@pytest.mark.parametrize("k", [1, 3])
def test_aligned_ranges_fold_to_the_whole(sup, k):
    """n = 14 has 2 wave-chunks in the default layout (k = 1 splits those);
    walk_log2 = 4 gives the 8 that k = 3 needs, so both walk lengths are run."""
    n = 14
    a = random_case(n, 41)[0]
    L, m, h = sup.layout(n)
    w = 0 if h >= k else 4
    chunks = 1 << (h if w == 0 else n - 1 - L - w)
    step = chunks >> k
    assert step >= 1
    parts = [sup.perman_complex_range(a, i * step, (i + 1) * step, cpu=True, threads=4, walk_log2=w)
             for i in range(1 << k)]
    while len(parts) > 1:
        parts = [complex(parts[i].real + parts[i + 1].real, parts[i].imag + parts[i + 1].imag)
                 for i in range(0, len(parts), 2)]
    f = 4 * (n & 1) - 2
    assert complex(f * parts[0].real, f * parts[0].imag) == sup.perman_complex(a, cpu=True, walk_log2=w)


@pytest.mark.parametrize("walk_log2", [0, 4])
def test_walk_length_within_the_bound(sup, walk_log2):
    n = 14
    a, truth, scale, e_np = random_case(n, 41)
    v, st = sup.perman_complex(a, cpu=True, walk_log2=walk_log2, return_stats=True)
    m = walk_log2 or sup.layout(n)[1]
    assert st["walk_bits"] == m
    e_walk = err_over_scale(v, truth, scale)
    print(f"n={n} m={m} e_np={e_np:.3e} e_walk={e_walk:.3e}")
    assert e_walk <= walk_bound(e_np, m, n)


# ---- (e) reader --------------------------------------------------------------

def write_mtx(path, symmetry, n, entries, field="complex", fmt="coordinate", comments=()):
    with open(path, "w") as f:
        f.write(f"%%MatrixMarket matrix {fmt} {field} {symmetry}\n")
        for c in comments:
            f.write(f"% {c}\n")
        f.write(f"{n} {n} {len(entries)}\n")
        for e in entries:
            f.write(" ".join(repr(v) if isinstance(v, float) else str(v) for v in e) + "\n")
    return str(path)


def test_read_general_round_trip_with_comments(sup, tmp_path):
    rng = np.random.default_rng(51)
    n = 5
    a = rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))
    a[1, 3] = 0
    ent = [(i + 1, j + 1, float(a[i, j].real), float(a[i, j].imag)) for i in range(n) for j in range(n) if a[i, j]]
    m, nz = sup.read_mtx_complex(write_mtx(tmp_path / "g.mtx", "general", n, ent, comments=("a comment", "another")))
    assert m.dtype == np.complex128 and nz == len(ent)
    assert np.array_equal(m, a)


def test_read_symmetric_and_hermitian(sup, tmp_path):
    ent = [(1, 1, 2.0, 0.0), (2, 1, 1.5, -0.5), (3, 1, 0.0, 2.0), (3, 3, -1.0, 0.0)]
    s, _ = sup.read_mtx_complex(write_mtx(tmp_path / "s.mtx", "symmetric", 3, ent))
    h, _ = sup.read_mtx_complex(write_mtx(tmp_path / "h.mtx", "hermitian", 3, ent))
    lower = np.array([[2, 0, 0], [1.5 - 0.5j, 0, 0], [2j, 0, -1]])
    off = lower - np.diag(np.diag(lower))
    assert np.array_equal(s, lower + off.T)
    assert np.array_equal(h, lower + off.conj().T)
    assert np.array_equal(h, h.conj().T)


def test_read_later_duplicates_win(sup, tmp_path):
    ent = [(1, 2, 1.0, 1.0), (2, 2, 5.0, 0.0), (1, 2, -3.0, 0.25)]
    m, nz = sup.read_mtx_complex(write_mtx(tmp_path / "d.mtx", "general", 2, ent))
    assert nz == 3 and m[0, 1] == -3 + 0.25j and m[1, 1] == 5


def test_read_rejected_forms(sup, tmp_path):
    ok = [(1, 1, 1.0, 0.0), (2, 1, 0.5, 0.5)]
    bad = {
        "skew": write_mtx(tmp_path / "k.mtx", "skew-symmetric", 2, ok),
        "real": write_mtx(tmp_path / "r.mtx", "general", 2, [(1, 1, 1.0)], field="real"),
        "pattern": write_mtx(tmp_path / "p.mtx", "general", 2, [(1, 1)], field="pattern"),
        "array": write_mtx(tmp_path / "a.mtx", "general", 2, ok, fmt="array"),
        "range": write_mtx(tmp_path / "o.mtx", "general", 2, [(3, 1, 1.0, 0.0)]),
        "hermitian diagonal": write_mtx(tmp_path / "hd.mtx", "hermitian", 2, [(1, 1, 1.0, 0.5)]),
        "too large": write_mtx(tmp_path / "l.mtx", "general", 65, ok),
    }
    with open(tmp_path / "ns.mtx", "w") as f:
        f.write("%%MatrixMarket matrix coordinate complex general\n2 3 1\n1 1 1.0 0.0\n")
    bad["non-square"] = str(tmp_path / "ns.mtx")
    with open(tmp_path / "t.mtx", "w") as f:
        f.write("%%MatrixMarket matrix coordinate complex general\n2 2 3\n1 1 1.0 0.0\n2 2 1.0\n")
    bad["truncated"] = str(tmp_path / "t.mtx")
    bad["missing"] = str(tmp_path / "no_such_file.mtx")
    for what, path in bad.items():
        with pytest.raises(sup.SupError) as e:
            sup.read_mtx_complex(path)
        assert e.value.code == -6, what


def test_real_reader_still_refuses_complex(sup, tmp_path):
    path = write_mtx(tmp_path / "c.mtx", "general", 2, [(1, 1, 1.0, 0.0), (2, 2, 1.0, 1.0)])
    assert sup.read_mtx_complex(path)[0][1, 1] == 1 + 1j
    with pytest.raises(sup.SupError) as e:
        sup.read_mtx(path)
    assert e.value.code == -6
    with pytest.raises(sup.SupError):
        sup.read_matrix(path)


# ---- (f) argument checks -----------------------------------------------------

def test_argument_checks(sup):
    import ctypes as C
    lib = sup._lib.load()
    re, im = C.c_double(), C.c_double()
    buf = (C.c_double * (2 * 65 * 65))()
    for n in (0, 65, -1):  # the C ABI's own check (the Python wrapper refuses these first)
        assert lib.sup_perman_complex(buf, n, None, 1, C.byref(re), C.byref(im), None) == -1
        assert lib.sup_perman_complex_range(buf, n, 0, 1, None, 1, C.byref(re), C.byref(im), None) == -1
    assert lib.sup_perman_complex(None, 2, None, 1, C.byref(re), C.byref(im), None) == -1
    assert lib.sup_perman_complex(buf, 2, None, 1, None, C.byref(im), None) == -1
    for bad in (np.zeros((0, 0)), np.zeros((65, 65)), np.zeros((3, 4)), np.zeros(5)):
        with pytest.raises(ValueError):
            sup.perman_complex(bad, cpu=True)
        with pytest.raises(ValueError):
            sup.perman_complex_range(bad, 0, 1, cpu=True)
    a = random_case(9, 22)[0]
    chunks = 1 << sup.layout(9)[2]
    assert sup.perman_complex_range(a, chunks, chunks, cpu=True) == 0  # empty range
    for c0, c1 in ((0, chunks + 1), (2, 1)):
        with pytest.raises(sup.SupError) as e:
            sup.perman_complex_range(a, c0, c1, cpu=True)
        assert e.value.code == -1
    with pytest.raises(sup.SupError) as e:
        sup.perman_complex(a, cpu=True, walk_log2=32)
    assert e.value.code == -1


def test_no_device_is_an_error_not_a_cpu_fallback(sup):
    a = random_case(4, 21)[0]
    if sup.device_count() == 0:
        for call in (lambda: sup.perman_complex(a), lambda: sup.perman_complex_range(a, 0, 1)):
            with pytest.raises(sup.SupError) as e:
                call()
            assert e.value.code == -2
    else:  # a box with a device: the device walk, the host twin's bits
        assert sup.perman_complex(a) == sup.perman_complex(a, cpu=True)


# ---- (g) CLI -------------------------------------------------------------------

def perman_exe(sup):
    return os.path.join(os.path.dirname(sup.__file__), "bin", "perman")


def test_cli_complex_cpu(sup, tmp_path):
    n = 9
    a = random_case(n, 22)[0]
    ent = [(i + 1, j + 1, float(a[i, j].real), float(a[i, j].imag)) for i in range(n) for j in range(n)]
    path = write_mtx(tmp_path / "m.mtx", "general", n, ent)
    r = subprocess.run([perman_exe(sup), "-f", path, "--complex", "-c", "-t", "3"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    line = [l for l in r.stdout.splitlines() if l.startswith("Permanent:")][0].split()
    assert complex(float(line[1]), float(line[2])) == sup.perman_complex(a, cpu=True)
    assert "cpu_perman64_complex" in r.stdout
    # without --complex a complex file is still refused
    assert subprocess.run([perman_exe(sup), "-f", path, "-c"], capture_output=True, text=True).returncode == 1


@pytest.mark.parametrize("opt", [["-s"], ["-o"], ["-u", "2"], ["-E"], ["-q"], ["-a"], ["-b"], ["-i"], ["-r", "1"]])
def test_cli_complex_refused_pairs(sup, tmp_path, opt):
    path = write_mtx(tmp_path / "m.mtx", "general", 2, [(1, 1, 1.0, 0.0), (2, 2, 1.0, 1.0)])
    r = subprocess.run([perman_exe(sup), "-f", path, "--complex", "-c"] + opt, capture_output=True, text=True)
    assert r.returncode == 1
    assert "--complex" in r.stderr and opt[0] in r.stderr
