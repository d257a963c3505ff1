"""Torontonians on host threads (sup_torontonian, sup_torontonian_range,
sup_torontonian_plan through superman_amd): closed forms that
hold with equality, single-mode squeezing, random dyadic matrices against an
exact truth (Gaussian-integer determinants by fraction-free elimination, the
square roots in 60-digit decimals) under the power-trace tests' rule
error / S <= 8 max(e_np, n 2^-52), the structure of the sum (cut, order of the
list, threads, ranges), every error, the plan and the CLI."""
import itertools
import math
import subprocess
from decimal import Decimal, getcontext

import numpy as np
import pytest

EPS = 2.0 ** -52
getcontext().prec = 60


def fbits(v):
    return np.atleast_1d(np.asarray(v, dtype=np.float64)).view(np.uint64)


# ---- matrices ---------------------------------------------------------------------------

def dyadic_O(M, seed):
    """A 2M x 2M Hermitian matrix of dyadic entries (denominator 2^10) whose
    Gershgorin row sums sum_j |O_ij| lie in [0.5, 0.9]: small off-diagonal
    entries, and a diagonal that brings every row to about 0.7."""
    rng = np.random.default_rng(seed)
    N = 2 * M
    k = max(1, min(200, int(0.3 * 1024 / ((N - 1) * math.sqrt(2))))) if N > 1 else 1
    re, im = rng.integers(-k, k + 1, (N, N)), rng.integers(-k, k + 1, (N, N))
    A = np.tril(re + 1j * im, -1)
    A = A + A.conj().T
    off = np.abs(A).sum(1) / 1024
    diag = np.floor((0.7 - off) * 1024)
    O = (A + np.diag(diag)) / 1024
    sums = np.abs(O).sum(1)
    assert np.all(sums >= 0.5) and np.all(sums <= 0.9) and np.all(O * 1024 == np.round(O * 1024))
    return O


def rows_of(modes, M, z):
    return [int(modes[b]) + h * M for b in range(len(modes) - 1, -1, -1) if (z >> b) & 1 for h in (0, 1)]


# ---- exact truth ------------------------------------------------------------------------

def gdiv(a, b):
    """a / b in the Gaussian integers, exact."""
    n = b[0] * b[0] + b[1] * b[1]
    re, im = a[0] * b[0] + a[1] * b[1], a[1] * b[0] - a[0] * b[1]
    assert re % n == 0 and im % n == 0
    return (re // n, im // n)


def gdet(A):
    """The determinant of a matrix of Gaussian integers (pairs), fraction-free."""
    n = len(A)
    A = [row[:] for row in A]
    prev, sign = (1, 0), 1
    for k in range(n - 1):
        if A[k][k] == (0, 0):
            p = next((i for i in range(k + 1, n) if A[i][k] != (0, 0)), None)
            if p is None:
                return (0, 0)
            A[k], A[p], sign = A[p], A[k], -sign
        akk = A[k][k]
        for i in range(k + 1, n):
            aik = A[i][k]
            for j in range(k + 1, n):
                x, y = A[i][j], A[k][j]
                t = (x[0] * akk[0] - x[1] * akk[1] - aik[0] * y[0] + aik[1] * y[1],
                     x[0] * akk[1] + x[1] * akk[0] - aik[0] * y[1] - aik[1] * y[0])
                A[i][j] = gdiv(t, prev)
        prev = akk
    d = A[n - 1][n - 1] if n else (1, 0)
    return (sign * d[0], sign * d[1])


def truth(O, modes):
    """(tor, S = sum_z f(z)) as Decimals, exact up to the 60-digit square roots."""
    M, n = O.shape[0] // 2, len(modes)
    Oi = np.round(O * 1024)
    tor, S = Decimal(0), Decimal(0)
    for z in range(1 << n):
        r = rows_of(modes, M, z)
        A = [[((1024 if i == j else 0) - int(Oi[i, j].real), -int(Oi[i, j].imag) if i != j else 0) for j in r] for i in r]
        d = gdet(A)
        assert d[1] == 0 and d[0] > 0
        f = 1 / (Decimal(d[0]) / Decimal(1024) ** len(r)).sqrt()
        tor += f if (n - bin(z).count("1")) % 2 == 0 else -f
        S += f
    return tor, S


def tor_np(O, modes, zs=None):
    """The numpy restatement: np.linalg.cholesky per subset, math.fsum over z."""
    M, n = O.shape[0] // 2, len(modes)
    terms = []
    for z in (range(1 << n) if zs is None else zs):
        r = rows_of(modes, M, z)
        f = 1.0
        if r:
            Oz = O[np.ix_(r, r)]
            Oz = np.tril(Oz, -1) + np.tril(Oz, -1).conj().T + np.diag(np.diag(Oz).real)
            f = 1.0 / float(np.prod(np.diag(np.linalg.cholesky(np.eye(len(r)) - Oz)).real))
        terms.append(f if (n - bin(z).count("1")) % 2 == 0 else -f)
    return math.fsum(terms), math.fsum(abs(t) for t in terms)


# ---- closed forms that hold with equality ------------------------------------------------

@pytest.mark.parametrize("n", range(1, 23))
def test_three_to_the_n_with_equality(sup, n):
    assert sup.torontonian(np.diag([0.75] * (2 * n)), cpu=True) == 3.0 ** n


@pytest.mark.parametrize("n", range(1, 13))
def test_mixed_powers_of_four_with_equality(sup, n):
    e = np.random.default_rng(n).integers(1, 3, n)
    O = np.diag(np.tile(1.0 - 4.0 ** -e, 2))
    assert sup.torontonian(O, cpu=True) == float(np.prod(4.0 ** e - 1.0))
    perm = np.random.default_rng(100 + n).permutation(n)
    assert sup.torontonian_batch(O, perm, cpu=True) == float(np.prod(4.0 ** e - 1.0))


@pytest.mark.parametrize("n", [1, 2, 5, 9, 14])
def test_zero_matrix_gives_exactly_zero(sup, n):
    v = sup.torontonian(np.zeros((2 * n, 2 * n)), cpu=True)
    assert v == 0.0


@pytest.mark.parametrize("n", range(2, 13))
def test_single_mode_squeezing(sup, n):
    rng = np.random.default_rng(700 + n)
    a = rng.uniform(0.1, 0.5, n)
    b = rng.uniform(0.05, 0.3, n) * np.exp(2j * np.pi * rng.uniform(size=n))
    O = np.zeros((2 * n, 2 * n), dtype=complex)
    for i in range(n):
        O[i, i] = O[i + n, i + n] = a[i]
        O[i, i + n], O[i + n, i] = b[i], np.conj(b[i])
    f = 1.0 / np.sqrt((1.0 - a) ** 2 - np.abs(b) ** 2)
    want, S = float(np.prod(f - 1.0)), float(np.prod(f + 1.0))
    v = sup.torontonian(O, cpu=True)
    v_np, _ = tor_np(O, np.arange(n))
    e, e_np = abs(v - want) / S, abs(v_np - want) / S
    # the closed form itself is rounded: 3 operations per factor and the product
    bound = 8 * max(e_np, n * EPS)
    print(f"squeezing n={n} e={e:.3e} e_np={e_np:.3e} bound={bound:.3e}")
    assert e <= bound


# ---- random matrices against the exact truth ---------------------------------------------

@pytest.mark.parametrize("n", range(1, 11))
def test_random_dyadic_against_exact_truth(sup, n):
    O = dyadic_O(n + 2, 900 + n)
    modes = np.random.default_rng(n).permutation(n + 2)[:n]
    t, S = truth(O, modes)
    v = sup.torontonian_batch(O, modes, cpu=True)
    v_np, _ = tor_np(O, modes)
    e, e_np = float(abs(Decimal(v) - t) / S), float(abs(Decimal(v_np) - t) / S)
    bound = 8 * max(e_np, n * EPS)
    print(f"random n={n} e={e:.3e} e_np={e_np:.3e} bound={bound:.3e} S/|tor|={float(S / abs(t)):.3e}")
    assert e <= bound


# ---- structure -----------------------------------------------------------------------------

@pytest.mark.parametrize("n", [3, 6, 9, 11])
def test_bits_do_not_depend_on_the_cut(sup, monkeypatch, n):
    """TOR_TWIN_TAIL = W: every subset from nothing with the low W positions
    masked in place (the kernel's form); 0: the compact form without reuse.
    The default keeps the rows two consecutive subsets share."""
    O = dyadic_O(n + 1, 1100 + n)
    modes = np.random.default_rng(n).permutation(n + 1)[:n]
    want = sup.torontonian_batch(O, modes, cpu=True)
    for tail in (0, 1, 4, 5, n):
        monkeypatch.setenv("TOR_TWIN_TAIL", str(tail))
        assert fbits(sup.torontonian_batch(O, modes, cpu=True)) == fbits(want), tail
        monkeypatch.delenv("TOR_TWIN_TAIL")


def test_masked_rows_with_signed_zeros(sup, monkeypatch):
    """Decoupled modes give accumulators that are exactly zero, of either sign:
    the masked form may flip such a sign (tor.hpp) and no result may notice."""
    O = np.zeros((12, 12), dtype=complex)
    for i, (a, b) in enumerate([(0.25, 0.125j), (0.5, -0.25), (0.375, 0.0), (0.25, -0.125 - 0.125j), (0.0, 0.0),
                                (0.5, 0.25j)]):
        O[i, i] = O[i + 6, i + 6] = a
        O[i, i + 6], O[i + 6, i] = b, np.conj(b)
    O[1, 0] = O[0, 1] = -0.0625
    want = sup.torontonian(O, cpu=True)
    for tail in (0, 4, 6):
        monkeypatch.setenv("TOR_TWIN_TAIL", str(tail))
        assert fbits(sup.torontonian(O, cpu=True)) == fbits(want)
        monkeypatch.delenv("TOR_TWIN_TAIL")


def test_permuting_a_list_keeps_the_value(sup):
    O = dyadic_O(9, 1200)
    modes = np.arange(9)
    v = sup.torontonian_batch(O, modes, cpu=True)
    _, S = tor_np(O, modes)
    seen = {int(fbits(v)[0])}
    for seed in range(4):
        w = sup.torontonian_batch(O, np.random.default_rng(seed).permutation(9), cpu=True)
        assert abs(w - v) <= 16 * 9 * EPS * S
        seen.add(int(fbits(w)[0]))
    assert len(seen) > 1  # the order of the list is part of the operation order


def batch_case(count, n, M, seed):
    rng = np.random.default_rng(seed)
    return dyadic_O(M, seed), np.stack([rng.permutation(M)[:n] for _ in range(count)])


def test_batch_of_65_on_1_and_16_threads(sup):
    O, modes = batch_case(65, 8, 12, 1300)
    one = sup.torontonian_batch(O, modes, cpu=True, threads=1)
    many, st = sup.torontonian_batch(O, modes, cpu=True, threads=16, return_stats=True)
    assert np.array_equal(fbits(one), fbits(many))
    assert st["leaves"] == 65 and st["visited_steps"] == 65 * 256 and st["gray_steps"] == 65 * 256
    for k in (0, 33, 64):
        assert fbits(sup.torontonian_batch(O, modes[k], cpu=True)) == fbits(one[k])
    assert abs(one[7] - tor_np(O, modes[7])[0]) <= 64 * EPS * tor_np(O, modes[7])[1]


# ---- the range entry -----------------------------------------------------------------------

def tree(parts):
    """fock_fold's pairwise tree over a power-of-two run of partials."""
    parts = list(parts)
    while len(parts) > 1:
        parts = [parts[i] + parts[i + 1] for i in range(0, len(parts), 2)]
    return parts[0]


@pytest.mark.parametrize("n", [5, 11, 13])
def test_range_entry(sup, n):
    O = dyadic_O(n, 1400 + n)
    modes = np.random.default_rng(n).permutation(n)
    whole = sup.torontonian_batch(O, modes, cpu=True)
    full, st = sup.torontonian_range(O, modes, 0, 2 ** n, cpu=True, return_stats=True)
    assert fbits(full) == fbits(whole) and st["visited_steps"] == 2 ** n
    L = 2 ** max(6, min(n, 9), n - 15)  # a wave-chunk
    chunks = max(1, 2 ** n // L)
    singles = [sup.torontonian_range(O, modes, c * L, min(2 ** n, (c + 1) * L), cpu=True) for c in range(chunks)]
    assert fbits(tree(singles)) == fbits(whole)
    if chunks >= 4:
        halves = [sup.torontonian_range(O, modes, h * 2 ** n // 2, (h + 1) * 2 ** n // 2, cpu=True) for h in (0, 1)]
        assert fbits(halves[0] + halves[1]) == fbits(whole)
        assert fbits(halves[0]) == fbits(tree(singles[:chunks // 2]))
    # a cut inside a chunk agrees to rounding
    _, S = tor_np(O, modes)
    cut = 2 ** n // 2 + 3
    parts = sup.torontonian_range(O, modes, 0, cut, cpu=True) + sup.torontonian_range(O, modes, cut, 2 ** n, cpu=True)
    assert abs(parts - whole) <= 8 * n * EPS * S
    assert sup.torontonian_range(O, modes, 7, 7, cpu=True) == 0.0
    one = sup.torontonian_range(O, modes, 3, 4, cpu=True)  # z = 3 alone: positions 0 and 1
    assert abs(one - tor_np(O, modes, [3])[0]) <= 16 * EPS * abs(one)


@pytest.mark.parametrize("z0,z1", [(2 ** 32 - 128, 2 ** 32), (0, 128)])
def test_range_entry_at_32_modes(sup, z0, z1):
    O = dyadic_O(32, 1500)
    modes = np.random.default_rng(32).permutation(32)
    v, st = sup.torontonian_range(O, modes, z0, z1, cpu=True, return_stats=True)
    v_np, S = tor_np(O, modes, range(z0, z1))
    print(f"n=32 z in [{z0}, {z1}): |v - v_np| / S = {abs(v - v_np) / S:.3e}")
    assert abs(v - v_np) <= 8 * 32 * EPS * S
    assert st["visited_steps"] == 128 and st["gray_steps"] == 2 ** 32


# ---- errors, NaN, the cap, the plan, the CLI -----------------------------------------------

def test_errors(sup):
    O = dyadic_O(4, 1600)
    with pytest.raises(sup.SupError, match=r"outside \[0, 4\)"):
        sup.torontonian_batch(O, [0, 4], cpu=True)
    with pytest.raises(sup.SupError, match=r"outside \[0, 4\)"):
        sup.torontonian_batch(O, [[0, 1], [-1, 2]], cpu=True)
    with pytest.raises(sup.SupError, match=r"names mode 2 at positions 0 and 2.*distinct"):
        sup.torontonian_batch(O, [2, 1, 2], cpu=True)
    with pytest.raises(sup.SupError, match=r"n = 33 outside \[1, 32\]"):
        sup.torontonian(np.zeros((66, 66)), cpu=True)
    with pytest.raises(sup.SupError, match=r"outside 0 <= z_begin <= z_end <= 2\^3"):
        sup.torontonian_range(O, [0, 1, 2], 0, 9, cpu=True)
    with pytest.raises(sup.SupError, match=r"outside 0 <= z_begin <= z_end"):
        sup.torontonian_range(O, [0, 1, 2], 5, 4, cpu=True)
    with pytest.raises(ValueError):
        sup.torontonian(np.zeros((3, 3)), cpu=True)
    with pytest.raises(ValueError):
        sup.torontonian_range(O, [[0, 1]], 0, 1, cpu=True)
    lib = sup._lib.load()
    out = np.zeros(1)
    m = np.zeros(1, dtype=np.int32)
    Oc = np.ascontiguousarray(O)
    for args in ((None, 4, m.ctypes.data, 1, 1, None, 1, out.ctypes.data, None),
                 (Oc.ctypes.data, 4, None, 1, 1, None, 1, out.ctypes.data, None),
                 (Oc.ctypes.data, 4, m.ctypes.data, 1, 1, None, 1, None, None)):
        assert lib.sup_torontonian(*args) == -1  # SUP_EINVAL
        assert b"null pointer" in lib.sup_last_error()
    assert lib.sup_torontonian(Oc.ctypes.data, 4, m.ctypes.data, 0, 1, None, 1, out.ctypes.data, None) == -1


def test_not_positive_definite_gives_nan(sup):
    assert math.isnan(sup.torontonian(2.0 * np.eye(2), cpu=True))
    O = dyadic_O(5, 1700)
    O[3, 3] = 1.5
    v = sup.torontonian_batch(O, [[0, 1, 2], [4, 3, 0]], cpu=True)
    assert not math.isnan(v[0]) and math.isnan(v[1])


def test_hermitian_to_rounding_is_not_refused(sup):
    """Only the lower triangle and the real parts of the diagonal are read."""
    O = dyadic_O(6, 1800)
    v = sup.torontonian(O, cpu=True)
    noisy = O + np.triu(np.full(O.shape, 1e-3 + 2e-3j), 1) + 1e-3j * np.eye(12)
    assert fbits(sup.torontonian(noisy, cpu=True)) == fbits(v)


def test_the_device_cap_and_no_device(sup):
    assert sup.TORONTONIAN_MAX_DEVICE_N == 32  # every n the entry takes: nothing lies above the cap
    if sup.device_count() == 0:
        with pytest.raises(sup.SupError, match="SUP_ENODEV"):
            sup.torontonian(np.zeros((4, 4)))


def census(n, W=5):
    R = 2 * W
    tail = sum(sum(8 * c + 2 for c in range(r)) + 4 * r + 3 for r in range(R)) + 1
    H = n - W
    if H <= 0:
        return 0.0, float(tail)
    num = den = 0.0
    for j in range(H):
        wj = 2.0 ** -(j + 1) if j + 1 < H else 2.0 ** -j
        U = H - 1 - j
        for u in range(U + 1):
            w = wj * math.comb(U, u) / 2.0 ** U
            P = 2 * (u + 1)
            ops = sum(8 * i * (i - 1) / 2 + 6 * i + 3 for i in (P - 2, P - 1)) + R * (8 * (2 * P - 3) + 4) + W * (R + 1) * 8 * P
            num, den = num + w * ops, den + w
    return num / den / 2 ** W, float(tail)


def test_plan(sup):
    for n in (1, 4, 5, 12, 32):
        subsets, ops = sup.torontonian_plan(n)
        assert subsets == 2 ** n
        assert ops == pytest.approx(sum(census(n)), rel=1e-12)
    st = sup.torontonian(np.zeros((20, 20)), cpu=True, return_stats=True)[1]
    assert st["est_ops_per_step"] == sup.torontonian_plan(10)[1]
    # the reuse against a fresh factor per subset, (2k)^3 / 6 multiply-adds of 8 operations
    plain = sum(math.comb(32, k) / 2.0 ** 32 * 8 * (2 * k) ** 3 / 6 for k in range(33))
    assert sup.torontonian_plan(32)[1] < plain / 20
    for n in (0, 33):
        with pytest.raises(sup.SupError, match=r"outside \[1, 32\]"):
            sup.torontonian_plan(n)


def run_cli(sup, *args):
    return subprocess.run([sup._lib.PERMAN_BIN, *args], capture_output=True, text=True, timeout=120)


def test_cli_on_host_threads(sup, tmp_path):
    O = dyadic_O(6, 1900)
    path = tmp_path / "o12.mtx"
    with open(path, "w") as f:
        f.write("%%MatrixMarket matrix coordinate complex hermitian\n12 12 78\n")
        for i, j in itertools.product(range(12), repeat=2):
            if j <= i:
                f.write(f"{i + 1} {j + 1} {float(O[i, j].real)!r} {float(O[i, j].imag)!r}\n")
    for extra, want in (((), sup.torontonian(O, cpu=True)),
                        (("--modes", "0,3,5"), sup.torontonian_batch(O, [0, 3, 5], cpu=True)),
                        (("--modes", "4"), sup.torontonian_batch(O, [4], cpu=True))):
        r = run_cli(sup, "-f", str(path), "--torontonian", "-c", *extra)
        assert r.returncode == 0, r.stderr
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("Torontonian: ")]
        assert len(line) == 1 and "cpu_torontonian64" in r.stdout
        assert float(line[0].split()[1]) == want, (extra, line, want)
    r = run_cli(sup, "-f", str(path), "--torontonian", "-c", "--modes", "0,0")
    assert r.returncode != 0 and "distinct" in r.stderr
    r = run_cli(sup, "-f", str(path), "--torontonian", "-c", "--modes", "0,6")
    assert r.returncode == 1 and "--modes takes" in r.stderr
    r = run_cli(sup, "-f", str(path), "--modes", "0,1", "-c")
    assert r.returncode == 1 and "--modes goes with --torontonian" in r.stderr
    r = run_cli(sup, "-f", str(path), "--torontonian", "--hafnian", "-c")
    assert r.returncode == 1 and "does not combine with --hafnian" in r.stderr
