"""Loop torontonians on host threads (sup_loop_torontonian, its range and plan
entries, sup_ltor_exp and the threshold-detection layer through superman_amd;
DESIGN.md §8l): the exponential against 60-digit references, gamma = 0 against
the torontonian's bits, the closed form of decoupled modes, random dyadic
matrices against an exact truth (bordered Gaussian-integer determinants, exp
and sqrt in 60-digit decimals) under the rule error / S <= 8 max(e_np,
n 2^-52 (1 + x_max)), the structure of the sum (cut, order of the list,
threads, ranges), every error, the plan, the CLI, and the probabilities of all
click patterns of a displaced state summing to one."""
import itertools
import math
import subprocess
from decimal import Decimal, getcontext

import mpmath
import numpy as np
import pytest

from test_torontonian import EPS, batch_case, dyadic_O, fbits, gdet, rows_of

try:
    from scipy.linalg import solve_triangular
except ImportError:  # the same substitution, by numpy's general solver
    def solve_triangular(L, b, lower=True):
        return np.linalg.solve(L, b)

getcontext().prec = 60


# ---- the exponential -----------------------------------------------------------------------

def test_ltor_exp_within_one_ulp(sup):
    """At least 10^5 seeded arguments over the four ranges against mpmath; the
    ulp is that of the true value's binade."""
    mpmath.mp.prec = 200
    rng = np.random.default_rng(2400)
    worst = 0.0
    for lo, hi in ((0.0, 40.0), (0.0, 709.0), (-1.0, 1.0), (-700.0, 0.0)):
        x = rng.uniform(lo, hi, 26000)
        y = sup.ltor_exp(x)
        w = 0.0
        for xi, yi in zip(x, y):
            t = mpmath.exp(mpmath.mpf(float(xi)))
            ulp = mpmath.ldexp(mpmath.mpf(1), mpmath.frexp(t)[1] - 53)  # t = m 2^e, 1/2 <= m < 1
            w = max(w, float(abs(mpmath.mpf(float(yi)) - t) / ulp))
        print(f"ltor_exp on [{lo}, {hi}]: worst error {w:.3f} ulp")
        worst = max(worst, w)
    assert worst <= 1.0


def test_ltor_exp_exact_cases(sup):
    assert fbits(sup.ltor_exp(0.0)) == fbits(1.0) and fbits(sup.ltor_exp(-0.0)) == fbits(1.0)
    assert math.isnan(sup.ltor_exp(float("nan")))
    assert sup.ltor_exp(710.0) == math.inf and sup.ltor_exp(1e300) == math.inf and sup.ltor_exp(math.inf) == math.inf
    assert fbits(sup.ltor_exp(-746.0)) == fbits(0.0) and fbits(sup.ltor_exp(-1e300)) == fbits(0.0)
    assert fbits(sup.ltor_exp(-math.inf)) == fbits(0.0)
    assert sup.ltor_exp(-745.0) == 5e-324  # the last product rounds into the subnormals once
    assert abs(sup.ltor_exp(709.7) / math.exp(709.7) - 1.0) <= 2 * EPS
    v = sup.ltor_exp(np.array([[0.0, 1.0], [-1.0, 2.0]]))
    assert v.shape == (2, 2) and abs(v[0, 1] - math.e) <= 4 * EPS


# ---- gamma = 0 -------------------------------------------------------------------------------

@pytest.mark.parametrize("n", range(1, 13))
def test_gamma_zero_has_the_torontonians_bits(sup, n):
    O = dyadic_O(n + 1, 2500 + n)
    zero = np.zeros(2 * (n + 1))
    assert fbits(sup.loop_torontonian(O, zero, cpu=True)) == fbits(sup.torontonian(O, cpu=True))
    modes = np.stack([np.random.default_rng(s).permutation(n + 1)[:n] for s in range(3)])
    assert np.array_equal(fbits(sup.loop_torontonian_batch(O, 0.0, modes, cpu=True)),
                          fbits(sup.torontonian_batch(O, modes, cpu=True)))
    for z0, z1 in ((0, 2 ** n), (1, 2 ** n - 1), (2 ** n // 2, 2 ** n)):
        assert fbits(sup.loop_torontonian_range(O, zero, modes[0], z0, z1, cpu=True)) == \
            fbits(sup.torontonian_range(O, modes[0], z0, z1, cpu=True))


# ---- decoupled modes -------------------------------------------------------------------------

def decoupled_case(n, seed):
    """O = diag(a_i on rows i and i + n), gamma arbitrary, the full list's
    exponent x = 4.  ltor = prod (g_i - 1); sum_z f(z) = prod (g_i + 1).  The
    bound of the test is relative to prod g_i while the rounding of a signed
    sum scales with sum_z f(z), so a_i in [0.90, 0.97] keeps g_i >= 10 and the
    two within 1.1^n of each other."""
    rng = np.random.default_rng(seed)
    a = rng.uniform(0.90, 0.97, n)
    gamma = rng.normal(size=2 * n) + 1j * rng.normal(size=2 * n)
    x = 0.5 * (np.abs(gamma[:n]) ** 2 + np.abs(gamma[n:]) ** 2) / (1.0 - a)
    gamma = gamma * math.sqrt(4.0 / x.sum())
    x = x * 4.0 / x.sum()
    g = [mpmath.exp(mpmath.mpf(float(0.5 * (abs(gamma[i]) ** 2 + abs(gamma[i + n]) ** 2))) / (1 - mpmath.mpf(float(a[i]))))
         / (1 - mpmath.mpf(float(a[i]))) for i in range(n)]
    return np.diag(np.tile(a, 2)), gamma, g, float(x.sum())


@pytest.mark.parametrize("n", range(1, 23))
def test_decoupled_modes_closed_form(sup, n):
    mpmath.mp.prec = 200
    O, gamma, g, xmax = decoupled_case(n, 2600 + n)
    want, scale = mpmath.fprod(gi - 1 for gi in g), mpmath.fprod(g)
    v = sup.loop_torontonian(O, gamma, cpu=True)
    e = float(abs(mpmath.mpf(v) - want) / scale)
    bound = n * EPS * (1.0 + xmax)
    print(f"decoupled n={n} e={e:.3e} bound={bound:.3e}")
    assert e <= bound


# ---- random matrices against the exact truth -------------------------------------------------

def dyadic_gamma(O, seed):
    """A dyadic vector (denominator 2^10) scaled so that the whole matrix's
    exponent 1/2 gamma^H (I - O)^-1 gamma is about 4."""
    rng = np.random.default_rng(seed)
    N = O.shape[0]
    g = rng.normal(size=N) + 1j * rng.normal(size=N)
    x = 0.5 * (g.conj() @ np.linalg.solve(np.eye(N) - O, g)).real
    g = np.round(g * math.sqrt(4.0 / x) * 1024) / 1024
    return g


def ltruth(O, gamma, modes):
    """(ltor, S = sum_z f(z), x_max) as Decimals: q = gamma_z^H M_z^-1 gamma_z =
    -det [[M_z, gamma_z], [gamma_z^H, 0]] / det M_z from Gaussian-integer
    determinants, exact up to the 60-digit exp and sqrt."""
    M, n = O.shape[0] // 2, len(modes)
    Oi, gi = np.round(O * 1024), np.round(gamma * 1024)
    ltor, S, xmax = Decimal(0), Decimal(0), Decimal(0)
    for z in range(1 << n):
        r = rows_of(modes, M, z)
        m = len(r)
        f = Decimal(1)
        if m:
            A = [[((1024 if i == j else 0) - int(Oi[i, j].real), -int(Oi[i, j].imag) if i != j else 0) for j in r] for i in r]
            B = [A[k] + [(int(gi[r[k]].real), int(gi[r[k]].imag))] for k in range(m)]
            B.append([(int(gi[j].real), -int(gi[j].imag)) for j in r] + [(0, 0)])
            dA, dB = gdet(A), gdet(B)
            assert dA[1] == 0 and dA[0] > 0 and dB[1] == 0 and dB[0] <= 0
            x = Decimal(-dB[0]) / (Decimal(1024) * Decimal(dA[0])) / 2
            xmax = max(xmax, x)
            f = x.exp() / (Decimal(dA[0]) / Decimal(1024) ** m).sqrt()
        ltor += f if (n - bin(z).count("1")) % 2 == 0 else -f
        S += f
    return ltor, S, xmax


def ltor_np(O, gamma, modes, zs=None):
    """The numpy restatement: np.linalg.cholesky and a triangular solve per
    subset, math.exp, math.fsum over z.  (value, sum of |terms|)."""
    M, n = O.shape[0] // 2, len(modes)
    terms = []
    for z in (range(1 << n) if zs is None else zs):
        r = rows_of(modes, M, z)
        f = 1.0
        if r:
            Oz = O[np.ix_(r, r)]
            Oz = np.tril(Oz, -1) + np.tril(Oz, -1).conj().T + np.diag(np.diag(Oz).real)
            L = np.linalg.cholesky(np.eye(len(r)) - Oz)
            y = solve_triangular(L, gamma[r], lower=True)
            f = math.exp(0.5 * float(np.sum(np.abs(y) ** 2))) / float(np.prod(np.diag(L).real))
        terms.append(f if (n - bin(z).count("1")) % 2 == 0 else -f)
    return math.fsum(terms), math.fsum(abs(t) for t in terms)


@pytest.mark.parametrize("n", range(1, 11))
def test_random_dyadic_against_exact_truth(sup, n):
    O = dyadic_O(n + 2, 2700 + n)
    gamma = dyadic_gamma(O, 2750 + n)
    modes = np.random.default_rng(n).permutation(n + 2)[:n]
    t, S, xmax = ltruth(O, gamma, modes)
    v = sup.loop_torontonian_batch(O, gamma, modes, cpu=True)
    v_np, _ = ltor_np(O, gamma, modes)
    e, e_np = float(abs(Decimal(v) - t) / S), float(abs(Decimal(v_np) - t) / S)
    bound = 8 * max(e_np, n * EPS * (1.0 + float(xmax)))
    print(f"random n={n} e={e:.3e} e_np={e_np:.3e} bound={bound:.3e} x_max={float(xmax):.3f} S/|ltor|={float(S / abs(t)):.3e}")
    assert e <= bound


# ---- structure -------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [3, 6, 9, 11])
def test_bits_do_not_depend_on_the_cut(sup, monkeypatch, n):
    """LTOR_TWIN_TAIL = W: every subset from nothing with the low W positions
    masked in place (the kernel's form); 0: the compact form without reuse."""
    O = dyadic_O(n + 1, 2800 + n)
    gamma = dyadic_gamma(O, 2850 + n)
    modes = np.random.default_rng(n).permutation(n + 1)[:n]
    want = sup.loop_torontonian_batch(O, gamma, modes, cpu=True)
    assert fbits(want) != fbits(sup.torontonian_batch(O, modes, cpu=True))
    for tail in (0, 1, 4, 5, n):
        monkeypatch.setenv("LTOR_TWIN_TAIL", str(tail))
        assert fbits(sup.loop_torontonian_batch(O, gamma, modes, cpu=True)) == fbits(want), tail
        monkeypatch.delenv("LTOR_TWIN_TAIL")


def test_masked_rows_with_signed_zeros(sup, monkeypatch):
    """Decoupled modes (and entries of gamma that are zero, of either sign)
    give accumulators that are exactly zero, of either sign: the masked form
    may flip such a sign and no result may notice."""
    O = np.zeros((12, 12), dtype=complex)
    for i, (a, b) in enumerate([(0.25, 0.125j), (0.5, -0.25), (0.375, 0.0), (0.25, -0.125 - 0.125j), (0.0, 0.0),
                                (0.5, 0.25j)]):
        O[i, i] = O[i + 6, i + 6] = a
        O[i, i + 6], O[i + 6, i] = b, np.conj(b)
    O[1, 0] = O[0, 1] = -0.0625
    gamma = np.array([0.5, -0.25j, 0.0, complex(-0.0, 0.125), 0.375, -0.5 + 0.25j,
                      complex(0.0, -0.0), 0.25, -0.125, 0.0, 0.0625j, complex(-0.0, -0.0)])
    want = sup.loop_torontonian(O, gamma, cpu=True)
    for tail in (0, 1, 4, 5, 6):
        monkeypatch.setenv("LTOR_TWIN_TAIL", str(tail))
        assert fbits(sup.loop_torontonian(O, gamma, cpu=True)) == fbits(want), tail
        monkeypatch.delenv("LTOR_TWIN_TAIL")


def test_permuting_a_list_keeps_the_value(sup):
    O = dyadic_O(9, 2900)
    gamma = dyadic_gamma(O, 2901)
    v = sup.loop_torontonian_batch(O, gamma, np.arange(9), cpu=True)
    _, S = ltor_np(O, gamma, np.arange(9))
    seen = {int(fbits(v)[0])}
    for seed in range(4):
        w = sup.loop_torontonian_batch(O, gamma, np.random.default_rng(seed).permutation(9), cpu=True)
        assert abs(w - v) <= 16 * 9 * EPS * (1.0 + 4.0) * S
        seen.add(int(fbits(w)[0]))
    assert len(seen) > 1  # the order of the list is part of the operation order


def test_batch_of_65_on_1_and_16_threads(sup):
    O, modes = batch_case(65, 8, 12, 3000)
    gamma = dyadic_gamma(O, 3001)
    one = sup.loop_torontonian_batch(O, gamma, modes, cpu=True, threads=1)
    many, st = sup.loop_torontonian_batch(O, gamma, modes, cpu=True, threads=16, return_stats=True)
    assert np.array_equal(fbits(one), fbits(many))
    assert st["leaves"] == 65 and st["visited_steps"] == 65 * 256 and st["gray_steps"] == 65 * 256
    for k in (0, 33, 64):
        assert fbits(sup.loop_torontonian_batch(O, gamma, modes[k], cpu=True)) == fbits(one[k])
    v_np, S = ltor_np(O, gamma, modes[7])
    assert abs(one[7] - v_np) <= 64 * EPS * (1.0 + 4.0) * S


# ---- the range entry -------------------------------------------------------------------------

def tree(parts):
    """fock_fold's pairwise tree over a power-of-two run of partials."""
    parts = list(parts)
    while len(parts) > 1:
        parts = [parts[i] + parts[i + 1] for i in range(0, len(parts), 2)]
    return parts[0]


@pytest.mark.parametrize("n", [5, 11, 13])
def test_range_entry(sup, n):
    O = dyadic_O(n, 3100 + n)
    gamma = dyadic_gamma(O, 3150 + n)
    modes = np.random.default_rng(n).permutation(n)
    whole = sup.loop_torontonian_batch(O, gamma, modes, cpu=True)
    full, st = sup.loop_torontonian_range(O, gamma, modes, 0, 2 ** n, cpu=True, return_stats=True)
    assert fbits(full) == fbits(whole) and st["visited_steps"] == 2 ** n
    L = 2 ** max(6, min(n, 9), n - 15)  # a wave-chunk
    chunks = max(1, 2 ** n // L)
    singles = [sup.loop_torontonian_range(O, gamma, modes, c * L, min(2 ** n, (c + 1) * L), cpu=True) for c in range(chunks)]
    assert fbits(tree(singles)) == fbits(whole)
    if chunks >= 4:
        halves = [sup.loop_torontonian_range(O, gamma, modes, h * 2 ** n // 2, (h + 1) * 2 ** n // 2, cpu=True) for h in (0, 1)]
        assert fbits(halves[0] + halves[1]) == fbits(whole)
        assert fbits(halves[0]) == fbits(tree(singles[:chunks // 2]))
        quarters = [sup.loop_torontonian_range(O, gamma, modes, k * 2 ** n // 4, (k + 1) * 2 ** n // 4, cpu=True) for k in range(4)]
        assert fbits((quarters[0] + quarters[1]) + (quarters[2] + quarters[3])) == fbits(whole)
    assert sup.loop_torontonian_range(O, gamma, modes, 7, 7, cpu=True) == 0.0
    one = sup.loop_torontonian_range(O, gamma, modes, 3, 4, cpu=True)  # z = 3 alone: positions 0 and 1
    assert abs(one - ltor_np(O, gamma, modes, [3])[0]) <= 16 * EPS * (1.0 + 4.0) * abs(one)


@pytest.mark.parametrize("z0,z1", [(2 ** 32 - 128, 2 ** 32), (0, 128)])
def test_range_entry_at_32_modes(sup, z0, z1):
    O = dyadic_O(32, 3200)
    gamma = dyadic_gamma(O, 3201)  # x <= 4 for every subset
    modes = np.random.default_rng(32).permutation(32)
    v, st = sup.loop_torontonian_range(O, gamma, modes, z0, z1, cpu=True, return_stats=True)
    v_np, S = ltor_np(O, gamma, modes, range(z0, z1))
    print(f"n=32 z in [{z0}, {z1}): |v - v_np| / S = {abs(v - v_np) / S:.3e}")
    assert abs(v - v_np) <= 8 * 32 * EPS * (1.0 + 4.0) * S
    assert st["visited_steps"] == 128 and st["gray_steps"] == 2 ** 32


# ---- errors, NaN, the cap, the plan, the CLI -------------------------------------------------

def test_errors(sup):
    O = dyadic_O(4, 3300)
    g = np.zeros(8, dtype=complex)
    with pytest.raises(sup.SupError, match=r"outside \[0, 4\)"):
        sup.loop_torontonian_batch(O, g, [0, 4], cpu=True)
    with pytest.raises(sup.SupError, match=r"outside \[0, 4\)"):
        sup.loop_torontonian_batch(O, g, [[0, 1], [-1, 2]], cpu=True)
    with pytest.raises(sup.SupError, match=r"names mode 2 at positions 0 and 2.*distinct"):
        sup.loop_torontonian_batch(O, g, [2, 1, 2], cpu=True)
    with pytest.raises(sup.SupError, match=r"n = 33 outside \[1, 32\]"):
        sup.loop_torontonian(np.zeros((66, 66)), np.zeros(66), cpu=True)
    with pytest.raises(sup.SupError, match=r"outside 0 <= z_begin <= z_end <= 2\^3"):
        sup.loop_torontonian_range(O, g, [0, 1, 2], 0, 9, cpu=True)
    with pytest.raises(sup.SupError, match=r"outside 0 <= z_begin <= z_end"):
        sup.loop_torontonian_range(O, g, [0, 1, 2], 5, 4, cpu=True)
    with pytest.raises(ValueError):
        sup.loop_torontonian(np.zeros((3, 3)), np.zeros(3), cpu=True)
    with pytest.raises(ValueError):
        sup.loop_torontonian(O, np.zeros(7), cpu=True)
    with pytest.raises(ValueError):
        sup.loop_torontonian_range(O, g, [[0, 1]], 0, 1, cpu=True)
    lib = sup._lib.load()
    out = np.zeros(1)
    m = np.zeros(1, dtype=np.int32)
    Oc = np.ascontiguousarray(O)
    for args in ((None, 4, g.ctypes.data, m.ctypes.data, 1, 1, None, 1, out.ctypes.data, None),
                 (Oc.ctypes.data, 4, None, m.ctypes.data, 1, 1, None, 1, out.ctypes.data, None),
                 (Oc.ctypes.data, 4, g.ctypes.data, None, 1, 1, None, 1, out.ctypes.data, None),
                 (Oc.ctypes.data, 4, g.ctypes.data, m.ctypes.data, 1, 1, None, 1, None, None)):
        assert lib.sup_loop_torontonian(*args) == -1  # SUP_EINVAL
        assert b"null pointer" in lib.sup_last_error()
    assert lib.sup_loop_torontonian_range(Oc.ctypes.data, 4, None, m.ctypes.data, 1, 0, 1, None, 1, out.ctypes.data, None) == -1
    assert lib.sup_loop_torontonian(Oc.ctypes.data, 4, g.ctypes.data, m.ctypes.data, 0, 1, None, 1, out.ctypes.data, None) == -1
    assert lib.sup_loop_torontonian(Oc.ctypes.data, 0, g.ctypes.data, m.ctypes.data, 1, 1, None, 1, out.ctypes.data, None) == -1
    assert lib.sup_ltor_exp_device(None, 3, out.ctypes.data, 0) == -1


def test_not_positive_definite_gives_nan(sup):
    assert math.isnan(sup.loop_torontonian(2.0 * np.eye(2), [0.5, 0.25j], cpu=True))
    O = dyadic_O(5, 3400)
    gamma = dyadic_gamma(O, 3401)
    O[3, 3] = 1.5
    v = sup.loop_torontonian_batch(O, gamma, [[0, 1, 2], [4, 3, 0]], cpu=True)
    assert not math.isnan(v[0]) and math.isnan(v[1])


def test_an_exponent_beyond_the_range_is_no_error(sup):
    v = sup.loop_torontonian(np.diag([0.5, 0.5]), [60.0, 0.0], cpu=True)  # exp(3600) - 1
    assert v == math.inf


def test_the_device_cap_and_no_device(sup):
    assert sup.LOOP_TORONTONIAN_MAX_DEVICE_N == 32  # every n the entry takes: nothing lies above the cap
    if sup.device_count() == 0:
        with pytest.raises(sup.SupError, match="SUP_ENODEV"):
            sup.loop_torontonian(np.zeros((4, 4)), np.zeros(4))
        with pytest.raises(sup.SupError, match="SUP_ENODEV"):
            sup.ltor_exp(np.zeros(3), device=True)


EXP_OPS = 34  # ltor.hpp kLtorExpOps: 1 product, 1 rint, 15 fmas (2 each), 2 scalings


def census(n, W=4):
    """ltor.hpp ltor_ops(n) restated (W = SUP_LTOR_W)."""
    R = 2 * W
    tail = sum(sum(8 * c + 2 for c in range(r)) + 4 * r + 3 for r in range(R)) + 1
    tail += sum(8 * c + 2 for c in range(R)) + 4 * R + 1 + EXP_OPS + 1
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
            ops = sum(8 * i * (i - 1) / 2 + 6 * i + 3 for i in (P - 2, P - 1)) + (R + 1) * (8 * (2 * P - 3) + 4)
            ops += W * (R + 1) * 8 * P + R * 8 * P + 4 * P
            num, den = num + w * ops, den + w
    return num / den / 2 ** W, float(tail)


def test_plan(sup):
    for n in (1, 4, 5, 12, 32):
        subsets, ops = sup.loop_torontonian_plan(n)
        assert subsets == 2 ** n
        assert ops == pytest.approx(sum(census(n)), rel=1e-12)
    st = sup.loop_torontonian(np.zeros((20, 20)), np.zeros(20), cpu=True, return_stats=True)[1]
    assert st["est_ops_per_step"] == sup.loop_torontonian_plan(10)[1]
    for n in (0, 33):
        with pytest.raises(sup.SupError, match=r"outside \[1, 32\]"):
            sup.loop_torontonian_plan(n)


def run_cli(sup, *args):
    return subprocess.run([sup._lib.PERMAN_BIN, *args], capture_output=True, text=True, timeout=120)


def test_cli_on_host_threads(sup, tmp_path):
    O = dyadic_O(6, 3500)
    gamma = dyadic_gamma(O, 3501)
    path, gpath, apath = tmp_path / "o12.mtx", tmp_path / "g12.mtx", tmp_path / "g12_array.mtx"
    with open(path, "w") as f:
        f.write("%%MatrixMarket matrix coordinate complex hermitian\n12 12 78\n")
        for i, j in itertools.product(range(12), repeat=2):
            if j <= i:
                f.write(f"{i + 1} {j + 1} {float(O[i, j].real)!r} {float(O[i, j].imag)!r}\n")
    with open(gpath, "w") as f:
        f.write("%%MatrixMarket matrix coordinate complex general\n12 1 12\n")
        for i in range(12):
            f.write(f"{i + 1} 1 {float(gamma[i].real)!r} {float(gamma[i].imag)!r}\n")
    with open(apath, "w") as f:
        f.write("%%MatrixMarket matrix array complex general\n12 1\n")
        for i in range(12):
            f.write(f"{float(gamma[i].real)!r} {float(gamma[i].imag)!r}\n")
    for gfile in (gpath, apath):
        for extra, want in (((), sup.loop_torontonian(O, gamma, cpu=True)),
                            (("--modes", "0,3,5"), sup.loop_torontonian_batch(O, gamma, [0, 3, 5], cpu=True)),
                            (("--modes", "4"), sup.loop_torontonian_batch(O, gamma, [4], cpu=True))):
            r = run_cli(sup, "-f", str(path), "--torontonian", "--loop", "--gamma", str(gfile), "-c", *extra)
            assert r.returncode == 0, r.stderr
            line = [ln for ln in r.stdout.splitlines() if ln.startswith("Loop torontonian: ")]
            assert len(line) == 1 and "cpu_loop_torontonian64" in r.stdout
            assert float(line[0].split()[2]) == want, (extra, line, want)
    r = run_cli(sup, "-f", str(path), "--torontonian", "--loop", "-c")
    assert r.returncode == 1 and "needs --gamma" in r.stderr
    r = run_cli(sup, "-f", str(path), "--torontonian", "--gamma", str(gpath), "-c")
    assert r.returncode == 1 and "--gamma goes with --torontonian --loop" in r.stderr
    r = run_cli(sup, "-f", str(path), "--gamma", str(gpath), "-c")
    assert r.returncode == 1 and "--gamma goes with --torontonian --loop" in r.stderr
    r = run_cli(sup, "-f", str(path), "--torontonian", "--loop", "--gamma", str(path), "-c")
    assert r.returncode == 1 and "12 x 1 vector" in r.stderr
    r = run_cli(sup, "-f", str(path), "--torontonian", "--loop", "--gamma", str(gpath), "-c", "--modes", "0,0")
    assert r.returncode != 0 and "distinct" in r.stderr
    r = run_cli(sup, "-f", str(path), "--torontonian", "-c")  # the plain torontonian is untouched
    assert r.returncode == 0 and "cpu_torontonian64" in r.stdout


# ---- threshold detection ---------------------------------------------------------------------

def random_state(M, seed, hbar=2.0):
    """A random symplectic (exp of a Hamiltonian matrix) applied to thermal
    noise, and a random mean, in xxpp ordering."""
    rng = np.random.default_rng(seed)
    A = rng.normal(size=(2 * M, 2 * M)) * 0.35
    A = (A + A.T) / 2
    J = np.block([[np.zeros((M, M)), np.eye(M)], [-np.eye(M), np.zeros((M, M))]])
    H = J @ A
    Sp, term = np.eye(2 * M), np.eye(2 * M)
    for k in range(1, 40):
        term = term @ H / k
        Sp = Sp + term
    assert np.allclose(Sp @ J @ Sp.T, J, atol=1e-12)
    nbar = rng.uniform(0.0, 0.5, M)
    cov = Sp @ np.diag(np.tile(hbar * (nbar + 0.5), 2)) @ Sp.T
    return rng.normal(size=2 * M) * math.sqrt(hbar) * 0.7, (cov + cov.T) / 2


def test_threshold_probabilities_sum_to_one(sup):
    mu, cov = random_state(4, 3600)
    pats = np.array(list(itertools.product((0, 1), repeat=4)))
    p = sup.threshold_detection_probs(mu, cov, pats, cpu=True)
    print("threshold probabilities:", p, "sum - 1 =", p.sum() - 1.0)
    assert p.shape == (16,) and np.all(p >= -1e-12) and abs(p.sum() - 1.0) <= 1e-10
    assert np.max(np.abs(mu)) > 0.1 and p.min() < 0.9 * p.max()
    for k in (0, 5, 15):
        assert sup.threshold_detection_prob(mu, cov, pats[k], cpu=True) == p[k]
    # the same state with hbar = 1 / 2: mu and cov rescaled with it
    q = sup.threshold_detection_probs(mu / 2.0, cov / 4.0, pats, hbar=0.5, cpu=True)
    assert np.max(np.abs(q - p)) <= 1e-13


def test_threshold_without_a_mean_is_the_torontonian_path(sup):
    _, cov = random_state(4, 3700)
    pats = np.array(list(itertools.product((0, 1), repeat=4)))
    p0 = sup.threshold_detection_probs(None, cov, pats, cpu=True)
    pz = sup.threshold_detection_probs(np.zeros(8), cov, pats, cpu=True)
    assert np.array_equal(fbits(p0), fbits(pz)) and abs(p0.sum() - 1.0) <= 1e-10
    O, gamma, pre = sup._threshold_setup(None, cov, 2.0)
    assert gamma is None
    assert fbits(p0[0b1011]) == fbits(pre * sup.torontonian_batch(O, [0, 2, 3], cpu=True))
    assert fbits(p0[0]) == fbits(pre)


def test_threshold_coherent_state_closed_form(sup):
    hbar = 2.0
    beta = np.array([0.3 + 0.4j, -0.8j, 0.0, 1.1 - 0.2j])
    mu = math.sqrt(2.0 * hbar) * np.concatenate([beta.real, beta.imag])
    cov = np.eye(8) * hbar / 2.0
    pats = np.array(list(itertools.product((0, 1), repeat=4)))
    p = sup.threshold_detection_probs(mu, cov, pats, hbar=hbar, cpu=True)
    e = np.exp(-np.abs(beta) ** 2)
    want = np.array([np.prod(np.where(s == 1, 1.0 - e, e)) for s in pats])
    assert np.max(np.abs(p - want)) <= 1e-13
    with pytest.raises(ValueError):
        sup.threshold_detection_probs(mu, cov, [[0, 1, 2, 0]], cpu=True)
    with pytest.raises(ValueError):
        sup.threshold_detection_probs(mu[:6], cov, pats, cpu=True)
