"""Loop-hafnian tables (ABI 27) on the host twin: every entry
against exact integer truth and against the per-pattern Kan walk under a bound
derived from the recurrence, the bits against threads and the low kernel's
knob, the Fock-basis state vector, density matrix, photon-number distribution
and its sampler, and every error path of the C entry."""
import ctypes as C
import itertools
import math

import numpy as np
import pytest

from test_complex_batch import bits
from test_gbs import lossy, three_mode_state, two_mode_state

U = 2.0 ** -53


def patterns(dims):
    """Every n with n_i < dims[i], mode 0 fastest: the table's own order."""
    return [p[::-1] for p in itertools.product(*[range(d) for d in dims[::-1]])]


def sqrt_fact(p):
    return math.sqrt(float(math.prod(math.factorial(int(v)) for v in p)))


def bound(p, M, tabs):
    """|t(n) - truth| <= 2 N (M + 8) u tabs(n): per level of the recurrence p + 2
    accumulations and the roundings of s, the product and the scale are about
    (M + 8) u of the absolute sum, over N levels, doubled for second order; the
    table of (|A|, |zeta|) majorises every partial sum."""
    return 2.0 * sum(p) * (M + 8) * U * tabs[tuple(p)]


def abs_table(sup, A, mu, dims):
    return sup.loop_hafnian_table(np.abs(A), None if mu is None else np.abs(mu), dims, cpu=True).real


def gauss_int(rng, M):
    A = rng.integers(-2, 3, (M, M)) + 1j * rng.integers(-2, 3, (M, M))
    A = np.triu(A) + np.triu(A, 1).T
    return A, rng.integers(-2, 3, M) + 1j * rng.integers(-2, 3, M)


# ---- 1. exact truth ----------------------------------------------------------------------------

@pytest.mark.parametrize("dims", [(4, 4, 3), (3, 3, 3, 3, 3), (9, 9), (6, 5, 4, 3), (2,) * 10])
def test_against_exact_truth(sup, dims):
    M = len(dims)
    A, mu = gauss_int(np.random.default_rng(2700 + M), M)
    t = sup.loop_hafnian_table(A, mu, dims, cpu=True)
    tabs = abs_table(sup, A, mu, dims)
    assert t.shape == tuple(dims) and t.dtype == np.complex128
    by_total = {}
    for p in patterns(dims):
        by_total.setdefault(sum(p), []).append(p)
    worst = 0.0
    for N, pats in sorted(by_total.items()):
        assert N <= 64
        if N == 0:
            assert bits(t[pats[0]]).tolist() == bits(1.0 + 0.0j).tolist()
            continue
        idx = np.array([np.repeat(np.arange(M), p) for p in pats], dtype=np.int32)
        truth = sup.hafnian_exact_batch(A, idx, mu=mu, loop=True, cpu=True)
        for p, (re, im) in zip(pats, truth):
            f = sqrt_fact(p)
            err, b = abs(t[p] * f - complex(re, im)), bound(p, M, tabs) * f
            assert err <= b, (p, err, b)
            if b > 0:
                worst = max(worst, err / b)
    print(f"dims {dims}: worst |t - truth| / bound = {worst:.4f}")


# ---- 2. an independent algorithm: the per-pattern Kan walk ---------------------------------------

@pytest.mark.parametrize("loop", [True, False])
def test_against_the_per_pattern_walk(sup, loop):
    B, zeta, _ = sup.gbs_pure_state(*three_mode_state())
    mu = zeta if loop else None
    dims = (4, 4, 4)
    t = sup.loop_hafnian_table(B, mu, dims, cpu=True)
    tabs = abs_table(sup, B, mu, dims)
    pats = patterns(dims)
    lists = [np.repeat(np.arange(3), p) for p in pats]
    v = sup.loop_hafnian_each(B, (zeta if loop else np.zeros(3))[None, :], lists, mu_of=np.zeros(len(pats), np.int32),
                              cpu=True)
    worst = 0.0
    for k, p in enumerate(pats):
        f = sqrt_fact(p)
        err, b = abs(t[p] * f - v[k]), bound(p, 3, tabs) * f
        assert err <= b, (p, err, b)
        if b > 0:
            worst = max(worst, err / b)
        if not loop and sum(p) % 2:
            assert t[p] == 0
    print(f"loop={loop}: worst |t - each| / bound = {worst:.4f}")


# ---- 3. bits -------------------------------------------------------------------------------------

def dense_case(M, seed):
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((M, M)) + 1j * rng.standard_normal((M, M))
    return A + A.T, rng.standard_normal(M) + 1j * rng.standard_normal(M)


def test_threads_do_not_change_bits(sup):
    A, mu = dense_case(5, 2710)
    dims = (5, 6, 7, 8, 9)  # the slabs of the last modes are split over the threads
    one = sup.loop_hafnian_table(A, mu, dims, cpu=True, threads=1)
    many = sup.loop_hafnian_table(A, mu, dims, cpu=True, threads=16)
    assert np.array_equal(bits(one), bits(many))


def test_the_knob_does_not_change_bits(sup, monkeypatch):
    A, mu = dense_case(4, 2711)
    dims = (3, 4, 2, 5)
    want = sup.loop_hafnian_table(A, mu, dims, cpu=True)
    plan = sup.loop_hafnian_table_plan(dims)
    assert plan[0] == 120 and plan[1] == 1
    for low, launches in ((1, 1 + 2 + 3 + 1 + 4), (2, 11), (7, 1 + 3 + 1 + 4), (12, 1 + 1 + 4), (24, 1 + 4)):
        monkeypatch.setenv("SUP_LHAF_TABLE_LOW", str(low))
        assert np.array_equal(bits(sup.loop_hafnian_table(A, mu, dims, cpu=True)), bits(want))
        assert sup.loop_hafnian_table_plan(dims)[1] == launches


@pytest.mark.parametrize("dims", [(1,), (3,), (1, 1, 1), (5, 1, 4), (1, 6)])
def test_shapes_and_the_first_entry(sup, dims):
    A, mu = dense_case(len(dims), 2712)
    for m in (mu, None):
        t = sup.loop_hafnian_table(A, m, dims, cpu=True)
        assert t.shape == tuple(dims) and t.flags.f_contiguous
        assert bits(t.reshape(-1, order="F")[0]).tolist() == bits(1.0 + 0.0j).tolist()
    t = sup.loop_hafnian_table(A, mu, dims, cpu=True)
    for p in patterns(dims):  # the definition, on the gathered matrix
        if sum(p):
            want = sup.loop_hafnian_each(A, mu[None, :], [np.repeat(np.arange(len(dims)), p)], cpu=True)[0] / sqrt_fact(p)
            assert abs(t[p] - want) <= 1e-12 * max(abs(want), 1.0), p


def test_plan_counts_the_operations(sup):
    # one mode: entry c > 0 costs 6, and 6 more for the A_00 term when c > 1
    assert sup.loop_hafnian_table_plan((5,)) == (5, 1, (6 * 4 + 6 * 3) / 5)
    # (2, 2): entries 1 and 2 cost 6; entry 3 reads t[2 - e_0]: 12
    assert sup.loop_hafnian_table_plan((2, 2)) == (4, 1, 24 / 4)
    A, mu = dense_case(3, 2713)
    st = sup.loop_hafnian_table(A, mu, (4, 3, 3), cpu=True, return_stats=True)[1]
    e, _, ops = sup.loop_hafnian_table_plan((4, 3, 3))
    assert st["gray_steps"] == st["visited_steps"] == e == 36 and st["est_ops_per_step"] == ops
    assert st["leaves"] == 1 and st["devices_used"] == 0 and st["kernel_ms"] == 0
    assert sup.loop_hafnian_table_plan((65,) * 64)[0] == 2 ** 64 - 1  # saturates


# ---- 4. physics ----------------------------------------------------------------------------------

def test_a_pure_state_gives_psi_psi_dagger(sup):
    mu, cov = two_mode_state()
    dims = (5, 4)
    psi = sup.gbs_state_vector(mu, cov, dims, cpu=True)
    rho = sup.gbs_density_matrix(mu, cov, dims, cpu=True)
    assert psi.shape == dims and rho.shape == dims + dims
    want = psi[:, :, None, None] * np.conj(psi)[None, None, :, :]
    err = np.max(np.abs(rho - want))
    print(f"pure against mixed: max |rho - psi psi^dagger| = {err:.3e}")
    # measured 1.5e-16 on the twin (parts of order one); two decades above it
    assert err <= 2e-14
    with pytest.raises(ValueError, match="not pure"):
        sup.gbs_state_vector(*lossy(mu, cov, 0.8), dims, cpu=True)
    with pytest.raises(ValueError, match=r"12000\^2 = 144000000.*LHAF_TABLE_MAX_ENTRIES = 134217728"):
        sup.gbs_density_matrix(mu, cov, (120, 100), cpu=True)
    # an integer is a cutoff: photon numbers 0 .. cutoff on every mode
    assert sup.gbs_state_vector(mu, cov, 3, cpu=True).shape == (4, 4)


@pytest.mark.parametrize("eta", [1.0, 0.8])
def test_distribution_against_the_per_pattern_probabilities(sup, eta):
    mu, cov = two_mode_state()
    if eta < 1.0:
        mu, cov = lossy(mu, cov, eta)
    p = sup.pnr_detection_distribution(mu, cov, (5, 5), cpu=True)
    pats = np.array(patterns((5, 5)))
    want = sup.pnr_detection_probs(mu, cov, pats, cpu=True)
    err = max(abs(p[tuple(q)] - w) for q, w in zip(pats, want))
    print(f"eta = {eta}: max |p - pnr_detection_probs| = {err:.3e}, missing mass = {1.0 - p.sum():.3e}")
    assert p.shape == (5, 5) and err <= 1e-14  # probabilities below one, two algorithms at 1e-16 each
    assert p.sum() <= 1.0 + 1e-12 and 1.0 - p.sum() >= 0.0


def test_a_marginal_from_the_table_against_modes(sup):
    mu, cov = three_mode_state()
    full = sup.pnr_detection_distribution(mu, cov, (9, 9, 9), cpu=True)
    missing = 1.0 - full.sum()
    print(f"marginals: missing mass of the (9, 9, 9) table = {missing:.3e}")
    assert missing >= 0.0
    part = sup.pnr_detection_distribution(mu, cov, (9, 9), modes=[0, 1], cpu=True)
    # sum_{n_2 < 9} p(n_0, n_1, n_2) = p(n_0, n_1) - P(n_0, n_1, n_2 >= 9), and the last is within the missing mass
    assert part.shape == (9, 9) and np.max(np.abs(full.sum(2) - part)) <= missing + 1e-14
    one = sup.pnr_detection_distribution(mu, cov, 8, modes=[2], cpu=True)
    assert one.shape == (9,) and np.max(np.abs(full.sum((0, 1)) - one)) <= missing + 1e-14


def test_sampler(sup):
    mu, cov = lossy(*two_mode_state(), 0.8)
    N, dims = 40000, (5, 5)
    p = sup.pnr_detection_distribution(mu, cov, dims, cpu=True)
    s, missing = sup.pnr_detection_sample(mu, cov, N, 2026, dims, return_missing=True, cpu=True)
    assert s.shape == (N, 2) and s.dtype == np.int32 and s.min() >= 0 and s.max() <= 4
    assert missing == 1.0 - np.clip(p.reshape(-1, order="F"), 0.0, None).sum() and missing >= 0.0
    q = p / p.sum()
    freq = np.bincount(s[:, 0] + 5 * s[:, 1], minlength=25).reshape(dims, order="F") / N
    sigma = np.sqrt(q * (1.0 - q) / N)
    print(f"sampler: worst |freq - p| / sigma = {np.max(np.abs(freq - q) / sigma):.2f}")
    assert np.all(np.abs(freq - q) <= 5 * sigma)
    # pieces and seeds reproduce
    assert np.array_equal(s[:1000], sup.pnr_detection_sample(mu, cov, 1000, 2026, dims, cpu=True))
    assert np.array_equal(s, sup.pnr_detection_sample(mu, cov, N, 2026, dims, cpu=True))
    assert not np.array_equal(s, sup.pnr_detection_sample(mu, cov, N, 2027, dims, cpu=True))
    pure = sup.pnr_detection_sample(*two_mode_state(), 500, 3, 4, cpu=True)
    assert pure.shape == (500, 2) and pure.max() <= 4


# ---- 5. error paths, through the raw C entry --------------------------------------------------------

def raw(sup, A, mu, dims, M=None, op=None, cpu=1, null=()):
    lib = sup._lib.load()
    a = np.ascontiguousarray(A, dtype=np.complex128)
    m = None if mu is None else np.ascontiguousarray(mu, dtype=np.complex128)
    d = np.ascontiguousarray(dims, dtype=np.int32)
    out = np.full(4, 7.0)  # a refused call writes nothing
    ptr = {"A": a.ctypes.data, "dims": d.ctypes.data, "out": out.ctypes.data}
    for name in null:
        ptr[name] = None
    rc = lib.sup_loop_hafnian_table(ptr["A"], a.shape[0] if M is None else M, None if m is None else m.ctypes.data,
                                    ptr["dims"], None if op is None else C.byref(op), cpu, ptr["out"], None)
    assert np.all(out == 7.0)
    return rc, lib.sup_last_error().decode()


def test_errors(sup, monkeypatch):
    A, mu = dense_case(2, 2720)
    EINVAL, EUNSUPPORTED = -1, -7
    for name in ("A", "dims", "out"):
        assert raw(sup, A, mu, (2, 2), null=(name,)) == (EINVAL, "sup_loop_hafnian_table: null pointer")
    for M in (0, -1, 65):
        rc, msg = raw(sup, A, mu, (2, 2), M=M)
        assert rc == EINVAL and f"M = {M} outside [1, 64]" in msg
    for bad in (0, -3, 66):
        rc, msg = raw(sup, A, mu, (2, bad))
        assert rc == EINVAL and f"dims[1] = {bad} outside [1, 65]" in msg
    skew = A.copy()
    skew[1, 0] = np.nextafter(skew[1, 0].real, 9.0) + 1j * skew[1, 0].imag
    rc, msg = raw(sup, skew, mu, (2, 2))
    assert rc == EINVAL and "A[0][1] and A[1][0] differ: A must be symmetric bit for bit" in msg
    op = sup._opts(gpu_num=2)
    for cpu in (0, 1):
        rc, msg = raw(sup, A, mu, (2, 2), op=op, cpu=cpu)
        assert rc == EINVAL and "gpu_num = 2: a table is one device's" in msg
    for knob in ("0", "4097", "-1", "12x", "x"):
        monkeypatch.setenv("SUP_LHAF_TABLE_LOW", knob)
        rc, msg = raw(sup, A, mu, (2, 2))
        assert rc == EINVAL and f"SUP_LHAF_TABLE_LOW={knob}: expected E with 1 <= E <= 4096" in msg
        with pytest.raises(sup.SupError, match="SUP_EINVAL.*SUP_LHAF_TABLE_LOW"):
            sup.loop_hafnian_table_plan((2, 2))
    monkeypatch.delenv("SUP_LHAF_TABLE_LOW")
    big, mub = dense_case(5, 2721)
    over = (65, 65, 65, 65, 8)
    for cpu in (0, 1):  # above the cap on either path, before any device work
        rc, msg = raw(sup, big, mub, over, cpu=cpu)
        assert rc == EUNSUPPORTED and "prod dims = 142805000 above SUP_LHAF_TABLE_MAX_ENTRIES = 134217728" in msg
        with pytest.raises(sup.SupError, match=r"SUP_EUNSUPPORTED.*prod dims = 142805000 above"):
            sup.loop_hafnian_table(big, mub, over, cpu=bool(cpu))
    rc, msg = raw(sup, np.zeros((64, 64)), None, (65,) * 64)
    assert rc == EUNSUPPORTED and "prod dims at least 2^64 above SUP_LHAF_TABLE_MAX_ENTRIES = 134217728" in msg
    assert sup.LHAF_TABLE_MAX_ENTRIES == 1 << 27 and sup.loop_hafnian_table_plan((2,) * 27)[0] == 1 << 27
    lib = sup._lib.load()
    assert lib.sup_loop_hafnian_table_plan(None, 2, None, None, None) == EINVAL and b"null pointer" in lib.sup_last_error()
    with pytest.raises(sup.SupError, match=r"SUP_EINVAL.*dims\[0\] = 66 outside \[1, 65\]"):
        sup.loop_hafnian_table_plan((66,))
    with pytest.raises(ValueError):
        sup.loop_hafnian_table(A, mu, (2, 2, 2), cpu=True)
    with pytest.raises(ValueError):
        sup.loop_hafnian_table(A, mu[:1], (2, 2), cpu=True)
    if sup.device_count() == 0:
        rc, msg = raw(sup, A, mu, (2, 2), cpu=0)
        assert rc == -2 and "device" in msg  # SUP_ENODEV: no CPU fallback
        with pytest.raises(sup.SupError, match="SUP_ENODEV"):
            sup.loop_hafnian_table(A, mu, (2, 2))
