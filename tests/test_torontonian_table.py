"""Torontonian tables (ABI 25) on the host twin: the raw table
f(z), the subset Moebius transform, all 2^n (loop) torontonians of a list from
one walk, the click distribution and the sampler on it.  The device's bits
against these: test_gpu_torontonian_table.py."""
from __future__ import annotations

import ctypes as C
import itertools
import math
from decimal import Decimal

import numpy as np
import pytest

from test_loop_torontonian import dyadic_gamma, ltor_np, ltruth, random_state
from test_torontonian import EPS, dyadic_O, fbits, run_cli, tor_np, truth

U = 2.0 ** -53


def popcount(a):
    a = np.asarray(a, dtype=np.uint64)
    return sum((a >> np.uint64(b)) & np.uint64(1) for b in range(32)).astype(np.int64)


def butterfly(t, sign):
    """The stages b = 0 .. n-1 ascending on a copy: t[z] += sign t[z ^ (1 << b)]."""
    t = np.array(t, dtype=np.float64)
    for b in range(int(t.shape[0]).bit_length() - 1):
        v = t.reshape(-1, 2, 2 ** b)
        if sign < 0:
            v[:, 1, :] -= v[:, 0, :]
        else:
            v[:, 1, :] += v[:, 0, :]
    return t


def sublist(modes, mask):
    return [int(modes[b]) for b in range(len(modes)) if (mask >> b) & 1]


def table(sup, O, gamma, modes, **kw):
    if gamma is None:
        return sup.torontonian_table(O, modes, cpu=True, **kw)
    return sup.loop_torontonian_table(O, gamma, modes, cpu=True, **kw)


def per_pattern(sup, O, gamma, modes, masks):
    """The per-pattern entry on the sub-lists of the masks, one batch per size."""
    out = np.ones(len(masks))
    size = popcount(masks)
    for k in np.unique(size):
        if k == 0:
            continue  # the empty list: 1 by definition
        which = np.nonzero(size == k)[0]
        lists = np.array([sublist(modes, int(masks[i])) for i in which], dtype=np.int32)
        out[which] = (sup.torontonian_batch(O, lists, cpu=True) if gamma is None
                      else sup.loop_torontonian_batch(O, gamma, lists, cpu=True))
    return out


FORMS = ["tor", "ltor"]


def case(form, M, seed):
    O = dyadic_O(M, seed)
    return O, (dyadic_gamma(O, seed + 1) if form == "ltor" else None)


# ---- the definition --------------------------------------------------------------------------

@pytest.mark.parametrize("form", FORMS)
def test_raw_has_the_bits_of_the_one_subset_range(sup, form):
    n = 7
    O, gamma = case(form, 9, 4100)
    modes = np.random.default_rng(41).permutation(9)[:n]
    raw = table(sup, O, gamma, modes, transform=False)
    assert raw.shape == (1 << n,) and raw[0] == 1.0
    for z in range(1 << n):
        r = (sup.torontonian_range(O, modes, z, z + 1, cpu=True) if gamma is None
             else sup.loop_torontonian_range(O, gamma, modes, z, z + 1, cpu=True))
        sign = -1.0 if (n - bin(z).count("1")) & 1 else 1.0
        assert fbits(raw[z]) == fbits(sign * r), z


@pytest.mark.parametrize("n", range(1, 13))
def test_transform_has_the_bits_of_the_numpy_butterfly(sup, n):
    for form in FORMS:
        O, gamma = case(form, n + 1, 4200 + n)
        modes = np.random.default_rng(n).permutation(n + 1)[:n]
        raw = table(sup, O, gamma, modes, transform=False)
        tab = table(sup, O, gamma, modes)
        assert np.array_equal(fbits(tab), fbits(butterfly(raw, -1))) and tab[0] == 1.0
        assert np.array_equal(fbits(sup.subset_mobius(raw, cpu=True)), fbits(tab))


def int_mobius(v):
    t = [int(x) for x in v]
    n = len(t).bit_length() - 1
    for b in range(n):
        for z in range(len(t)):
            if (z >> b) & 1:
                t[z] -= t[z ^ (1 << b)]
    return t


def int_case(n):
    return np.random.default_rng(4300 + n).integers(-(2 ** 20) + 1, 2 ** 20, 1 << n).astype(np.float64)


@pytest.mark.parametrize("n", [0, 1, 5, 6, 7, 11, 12, 13, 18])
def test_subset_mobius_on_integers(sup, n):
    v = int_case(n)
    want = int_mobius(v)
    assert max(abs(x) for x in want) < 2 ** 53
    got = sup.subset_mobius(v, cpu=True)
    assert got.shape == v.shape and [int(x) for x in got] == want
    assert np.array_equal(sup.subset_mobius(v, cpu=True, threads=1), got)


@pytest.mark.parametrize("bits,passes", [("6,3", 3), ("6,2", 4), ("7,4", 3)])
def test_subset_mobius_with_forced_shapes(sup, monkeypatch, bits, passes):
    L, K = (int(x) for x in bits.split(","))
    assert 1 + -(-(12 - L) // K) == passes
    v = int_case(12)
    monkeypatch.setenv("SUP_MOBIUS_BITS", bits)
    assert [int(x) for x in sup.subset_mobius(v, cpu=True)] == int_mobius(v)


def test_a_shape_the_transform_was_not_compiled_for(sup, monkeypatch):
    assert (sup.MOBIUS_TILE_BITS, sup.MOBIUS_PASS_BITS) == (12, 6)
    for bad in ("5,3", "13,3", "8,0", "8,7", "8", "8,3,1", "x"):
        monkeypatch.setenv("SUP_MOBIUS_BITS", bad)
        with pytest.raises(sup.SupError, match="SUP_EINVAL.*SUP_MOBIUS_BITS"):
            sup.subset_mobius(np.zeros(4), cpu=True)
        with pytest.raises(sup.SupError, match="SUP_EINVAL.*SUP_MOBIUS_BITS"):
            sup.torontonian_table(np.zeros((4, 4)), cpu=True)
    monkeypatch.setenv("SUP_MOBIUS_BITS", "12,6")
    assert sup.subset_mobius(np.ones(4), cpu=True).tolist() == [1.0, 0.0, 0.0, 0.0]


def test_three_to_the_popcount_with_equality(sup):
    tab = sup.torontonian_table(np.diag([0.75] * 24), cpu=True)
    assert tab.shape == (4096,)
    assert np.array_equal(tab, 3.0 ** popcount(np.arange(4096)))


# ---- against the per-pattern entries -----------------------------------------------------------

@pytest.mark.parametrize("form", FORMS)
def test_against_the_per_pattern_entry(sup, form):
    """Both sides add the same bit-equal terms f(Z), Z in S: the table in a tree
    of depth |S|, the entry in one of depth <= 6 (wave butterfly) + 8 (the groups
    of a 2^9 chunk) + 7 (the fold) for |S| <= 16; each addition errs by at most
    2^-53 of a partial sum of absolute value <= zeta[S] = sum f(Z); factor 2 for
    the second order."""
    n = 10
    O, gamma = case(form, 12, 4242)
    modes = np.arange(n)
    raw = table(sup, O, gamma, modes, transform=False)
    tab, zeta = table(sup, O, gamma, modes), butterfly(raw, +1)
    size = popcount(np.arange(1 << n))
    masks = np.array([m for m in range(1 << n) if size[m] in (1, 2, 5, 9, 10) or m % 37 == 0])
    ref = per_pattern(sup, O, gamma, modes, masks)
    err = np.abs(tab[masks] - ref)
    bound = 2 * (size[masks] + 21) * U * zeta[masks]
    print(f"{form}: {len(masks)} masks, worst err / bound = {np.max(err / bound):.3e}")
    assert np.all(err <= bound)
    assert tab[0] == 1.0


@pytest.mark.parametrize("form", FORMS)
def test_against_exact_truth(sup, form):
    n = 6
    O, gamma = case(form, 8, 4400)
    modes = np.random.default_rng(44).permutation(8)[:n]
    tab = table(sup, O, gamma, modes)
    worst = 0.0
    for mask in range(1, 1 << n):
        s = sublist(modes, mask)
        if gamma is None:
            t, S = truth(O, s)
            v_np, scale = tor_np(O, s)[0], 1.0
        else:
            t, S, xmax = ltruth(O, gamma, s)
            v_np, scale = ltor_np(O, gamma, s)[0], 1.0 + float(xmax)
        e, e_np = float(abs(Decimal(float(tab[mask])) - t) / S), float(abs(Decimal(v_np) - t) / S)
        bound = 8 * max(e_np, len(s) * EPS * scale)
        worst = max(worst, e / bound)
        assert e <= bound, (mask, e, bound)
    print(f"{form}: worst e / bound = {worst:.3e}")


def test_nan_reaches_exactly_the_supersets(sup):
    O = dyadic_O(6, 4500)
    O[3, 3] = 1.5
    modes = np.array([4, 0, 3, 5, 1, 2])
    pos = 2  # the position of mode 3
    for gamma in (None, dyadic_gamma(dyadic_O(6, 4500), 4501)):
        for transform in (False, True):
            tab = table(sup, O, gamma, modes, transform=transform)
            has = ((np.arange(64) >> pos) & 1).astype(bool)
            assert np.array_equal(np.isnan(tab), has)


# ---- the click distribution --------------------------------------------------------------------

def state6():
    return random_state(6, 4600)


def np_distribution(sup, mu, cov, modes=None):
    """Every pattern's probability by the numpy restatement, per pattern."""
    mu_r, cov_r = sup._threshold_reduce(mu, cov, modes)
    O, gamma, pre = sup._threshold_setup(mu_r, cov_r, 2.0)
    n = O.shape[0] // 2
    return np.array([pre * ltor_np(O, gamma, sublist(range(n), m))[0] for m in range(1 << n)])


@pytest.fixture(scope="module")
def dist6(sup):
    mu, cov = state6()
    return sup.threshold_detection_distribution(mu, cov, cpu=True)


def test_distribution_against_the_per_pattern_probabilities(sup, dist6):
    mu, cov = state6()
    n = 6
    O, gamma, pre = sup._threshold_setup(mu, cov, 2.0)
    pats = (np.arange(64)[:, None] >> np.arange(n)[None, :]) & 1  # bit b = the click on mode b
    p = sup.threshold_detection_probs(mu, cov, pats, cpu=True)
    zeta = butterfly(sup.loop_torontonian_table(O, gamma, transform=False, cpu=True), +1)
    size = popcount(np.arange(64))
    bound = 2 * (size + 21) * U * zeta * pre
    err = np.abs(dist6 - p)
    print(f"distribution: worst err / bound = {np.max(err / bound):.3e}")
    assert dist6.shape == (64,) and np.all(err <= bound)
    assert fbits(dist6[0]) == fbits(pre)
    # the probabilities sum to one: the table's own bound, or numpy's inversion where that dominates
    total = abs(math.fsum(dist6) - 1.0)
    own = 64 * n * EPS * float(zeta.sum()) * pre
    total_np = abs(math.fsum(np_distribution(sup, mu, cov)) - 1.0)
    print(f"|sum p - 1| = {total:.3e}, table bound {own:.3e}, numpy restatement {total_np:.3e}")
    assert total <= max(own, 8 * total_np)
    assert np.all(dist6 > 0) and dist6.min() < 0.9 * dist6.max()


def test_marginals_are_consistent(sup, dist6):
    """The full distribution summed over two modes against the distribution of
    the other four alone.  The two sides go through different numpy inversions,
    so the yardstick is the same discrepancy of a pure-numpy evaluation."""
    mu, cov = state6()
    n, keep = 6, [0, 2, 3, 5]

    def marginal(p):
        out = np.zeros(16)
        for m in range(64):
            out[sum(((m >> b) & 1) << i for i, b in enumerate(keep))] += p[m]
        return out

    ours = np.max(np.abs(marginal(dist6) - sup.threshold_detection_distribution(mu, cov, modes=keep, cpu=True)))
    ref = np.max(np.abs(marginal(np_distribution(sup, mu, cov)) - np_distribution(sup, mu, cov, keep)))
    print(f"marginal discrepancy: ours {ours:.3e}, numpy {ref:.3e}")
    assert ours <= max(8 * ref, n * EPS)


def test_distribution_without_a_mean_and_with_modes(sup):
    _, cov = random_state(5, 4700)
    p0 = sup.threshold_detection_distribution(None, cov, cpu=True)
    pz = sup.threshold_detection_distribution(np.zeros(10), cov, cpu=True)
    assert np.array_equal(fbits(p0), fbits(pz)) and abs(p0.sum() - 1.0) <= 1e-10
    # bit b is the click on modes[b]
    mu, cov = random_state(4, 4701)
    a = sup.threshold_detection_distribution(mu, cov, modes=[0, 1, 2, 3], cpu=True)
    b = sup.threshold_detection_distribution(mu, cov, modes=[2, 0, 3, 1], cpu=True)
    perm = [sum(((m >> i) & 1) << q for i, q in enumerate([2, 0, 3, 1])) for m in range(16)]
    assert np.max(np.abs(b - a[perm])) <= 1e-13
    for bad in ([0, 0], [4], []):
        with pytest.raises(ValueError):
            sup.threshold_detection_distribution(mu, cov, modes=bad, cpu=True)


def test_sampler(sup, dist6):
    mu, cov = state6()
    N = 20000
    s = sup.threshold_detection_sample(mu, cov, N, 12345, cpu=True)
    assert s.shape == (N, 6) and s.dtype == np.uint8 and set(np.unique(s)) <= {0, 1}
    assert np.array_equal(s, sup.threshold_detection_sample(mu, cov, N, 12345, cpu=True))
    assert not np.array_equal(s, sup.threshold_detection_sample(mu, cov, N, 12346, cpu=True))
    freq = np.bincount((s.astype(np.int64) << np.arange(6)).sum(1), minlength=64) / N
    sigma = np.sqrt(dist6 * (1.0 - dist6) / N)
    print(f"sampler: worst |freq - p| / sigma = {np.max(np.abs(freq - dist6) / sigma):.2f}")
    assert np.all(np.abs(freq - dist6) <= 5 * sigma)


def test_a_decoupled_vacuum_mode_never_clicks(sup):
    mu5, cov5 = random_state(5, 4800)
    M = 6
    ix = np.concatenate([np.arange(5), M + np.arange(5)])
    mu, cov = np.zeros(2 * M), np.eye(2 * M)  # hbar = 2: the vacuum is the identity
    mu[ix] = mu5
    cov[np.ix_(ix, ix)] = cov5
    p = sup.threshold_detection_distribution(mu, cov, cpu=True)
    assert np.max(np.abs(p[32:])) <= 1e-15
    s = sup.threshold_detection_sample(mu, cov, 5000, 7, cpu=True)
    assert s.shape == (5000, 6) and not s[:, 5].any() and s[:, :5].any()


# ---- errors, stats, the CLI --------------------------------------------------------------------

def test_errors(sup):
    O = dyadic_O(4, 4900)
    g = np.zeros(8, dtype=np.complex128)
    for call in (lambda m: sup.torontonian_table(O, m, cpu=True), lambda m: sup.loop_torontonian_table(O, g, m, cpu=True)):
        with pytest.raises(sup.SupError, match=r"SUP_EINVAL.*outside \[0, 4\)"):
            call([0, 4])
        with pytest.raises(sup.SupError, match=r"SUP_EINVAL.*names mode 2 at positions 0 and 2.*distinct"):
            call([2, 1, 2])
        with pytest.raises(ValueError):
            call([[0, 1], [2, 3]])
    with pytest.raises(sup.SupError, match=r"SUP_EINVAL.*n = 33 outside \[1, 32\]"):
        sup.torontonian_table(np.zeros((66, 66)), cpu=True)
    for cpu in (True, False):  # above the cap on either path, before any device work
        with pytest.raises(sup.SupError, match=r"SUP_EUNSUPPORTED.*n = 29 above SUP_TORONTONIAN_TABLE_MAX_N = 28"):
            sup.torontonian_table(np.zeros((58, 58)), cpu=cpu)
        with pytest.raises(sup.SupError, match=r"SUP_EUNSUPPORTED.*n = 29 above"):
            sup.loop_torontonian_table(np.zeros((58, 58)), 0.0, cpu=cpu)
    assert sup.TORONTONIAN_TABLE_MAX_N == 28
    with pytest.raises(ValueError):
        sup.subset_mobius(np.zeros(6), cpu=True)
    lib = sup._lib.load()
    out, m = np.zeros(2), np.zeros(1, dtype=np.int32)
    Oc, gc = np.ascontiguousarray(O), np.ascontiguousarray(g)
    o, mm, oo, gg = Oc.ctypes.data, m.ctypes.data, out.ctypes.data, gc.ctypes.data
    for args in ((None, 4, mm, 1, 1, None, 1, oo, None), (o, 4, None, 1, 1, None, 1, oo, None),
                 (o, 4, mm, 1, 1, None, 1, None, None)):
        assert lib.sup_torontonian_table(*args) == -1 and b"null pointer" in lib.sup_last_error()
    for args in ((None, 4, gg, mm, 1, 1, None, 1, oo, None), (o, 4, None, mm, 1, 1, None, 1, oo, None),
                 (o, 4, gg, None, 1, 1, None, 1, oo, None), (o, 4, gg, mm, 1, 1, None, 1, None, None)):
        assert lib.sup_loop_torontonian_table(*args) == -1 and b"null pointer" in lib.sup_last_error()
    assert lib.sup_torontonian_table(o, 4, mm, 0, 1, None, 1, oo, None) == -1
    assert lib.sup_mobius_subsets(None, 3, None, 1) == -1 and b"null pointer" in lib.sup_last_error()
    for n in (-1, 29):
        assert lib.sup_mobius_subsets(oo, n, None, 1) == -1 and b"outside [0, 28]" in lib.sup_last_error()
    op = sup._opts(gpu_num=2)
    for on_cpu in (0, 1):
        assert lib.sup_torontonian_table(o, 4, mm, 1, 1, C.byref(op), on_cpu, oo, None) == -1
        assert b"gpu_num = 2" in lib.sup_last_error()
        assert lib.sup_loop_torontonian_table(o, 4, gg, mm, 1, 1, C.byref(op), on_cpu, oo, None) == -1
    if sup.device_count() == 0:
        with pytest.raises(sup.SupError, match="SUP_ENODEV"):
            sup.torontonian_table(np.zeros((4, 4)))
        with pytest.raises(sup.SupError, match="SUP_ENODEV"):
            sup.loop_torontonian_table(np.zeros((4, 4)), 0.0)
        with pytest.raises(sup.SupError, match="SUP_ENODEV"):
            sup.subset_mobius(np.zeros(4))


def test_stats(sup):
    for n in (3, 11):
        O = dyadic_O(n, 5000 + n)
        tab, st = sup.torontonian_table(O, cpu=True, return_stats=True)
        assert tab.shape == (1 << n,)
        assert st["leaves"] == 1 and st["gray_steps"] == st["visited_steps"] == 1 << n
        assert st["est_ops_per_step"] == sup.torontonian_plan(n)[1] + n / 2
        assert st["kernel_ms"] == 0.0 and st["wall_ms"] > 0.0 and st["devices_used"] == 0
        st = sup.loop_torontonian_table(O, 0.0, cpu=True, transform=False, return_stats=True)[1]
        assert st["est_ops_per_step"] == sup.loop_torontonian_plan(n)[1] + n / 2
        assert st["gray_steps"] == st["visited_steps"] == 1 << n


def test_gamma_zero_has_the_torontonian_tables_bits(sup):
    O = dyadic_O(8, 5100)
    for transform in (False, True):
        a = sup.torontonian_table(O, cpu=True, transform=transform)
        b = sup.loop_torontonian_table(O, 0.0, cpu=True, transform=transform)
        assert np.array_equal(fbits(a), fbits(b))
    assert np.array_equal(fbits(sup.torontonian_table(O, cpu=True, threads=1)), fbits(sup.torontonian_table(O, cpu=True)))


def test_cli_on_host_threads(sup, tmp_path):
    O = dyadic_O(6, 5200)
    gamma = dyadic_gamma(O, 5201)
    path, gpath = tmp_path / "o12.mtx", tmp_path / "g12.mtx"
    with open(path, "w") as f:
        f.write("%%MatrixMarket matrix coordinate complex hermitian\n12 12 78\n")
        for i, j in itertools.product(range(12), repeat=2):
            if j <= i:
                f.write(f"{i + 1} {j + 1} {float(O[i, j].real)!r} {float(O[i, j].imag)!r}\n")
    with open(gpath, "w") as f:
        f.write("%%MatrixMarket matrix coordinate complex general\n12 1 12\n")
        for i in range(12):
            f.write(f"{i + 1} 1 {float(gamma[i].real)!r} {float(gamma[i].imag)!r}\n")
    cases = (((), sup.torontonian_table(O, cpu=True)),
             (("--raw",), sup.torontonian_table(O, cpu=True, transform=False)),
             (("--modes", "5,0,3"), sup.torontonian_table(O, [5, 0, 3], cpu=True)),
             (("--loop", "--gamma", str(gpath)), sup.loop_torontonian_table(O, gamma, cpu=True)),
             (("--loop", "--gamma", str(gpath), "--raw", "--modes", "4,1"),
              sup.loop_torontonian_table(O, gamma, [4, 1], cpu=True, transform=False)))
    for extra, want in cases:
        r = run_cli(sup, "-f", str(path), "--torontonian", "--table", "-c", *extra)
        assert r.returncode == 0, r.stderr
        lines = [ln for ln in r.stdout.splitlines() if ln[:1].isdigit()]
        assert lines == [f"{mask} {v:.17e}" for mask, v in enumerate(want)], extra
        assert ("cpu_loop_torontonian_table64" if "--loop" in extra else "cpu_torontonian_table64") in r.stdout
    r = run_cli(sup, "-f", str(path), "--torontonian", "--raw", "-c")
    assert r.returncode == 1 and "--raw goes with --torontonian --table" in r.stderr
    r = run_cli(sup, "-f", str(path), "--table", "-c")
    assert r.returncode == 1 and "--table and --raw go with --torontonian" in r.stderr
    r = run_cli(sup, "-f", str(path), "--torontonian", "--table", "-c", "--modes", "1,1")
    assert r.returncode != 0 and "distinct" in r.stderr
    r = run_cli(sup, "-f", str(path), "--torontonian", "-c")  # the plain entry is untouched
    assert r.returncode == 0 and "cpu_torontonian64" in r.stdout
