"""PNR Gaussian boson sampling on ragged loop hafnians (ABI 26)
on the host twin: the each-entry's bits against the single-order entry, the
probabilities against closed forms, the pure (order N) against the general
(order 2N) formula, the sums over each click pattern against the threshold
table, and the chain-rule sampler's behaviour and statistics."""
import itertools
import math

import numpy as np
import pytest

from test_complex_batch import bits

HBAR = 2.0


# ---- Gaussian states in xxpp ordering, vacuum = hbar / 2, built with numpy ----

def gaussian_state(r, U, alpha, hbar=HBAR):
    """Squeezers r_i on the vacuum, the passive unitary U, then displacements
    alpha_i: (mu, cov)."""
    r, alpha = np.asarray(r, float), np.asarray(alpha, complex)
    M = r.size
    S = np.diag(np.concatenate([np.exp(-r), np.exp(r)]))
    U = np.eye(M) if U is None else np.asarray(U, complex)
    P = np.block([[U.real, -U.imag], [U.imag, U.real]])
    S = P @ S
    cov = (hbar / 2.0) * S @ S.T
    mu = np.sqrt(2.0 * hbar) * np.concatenate([alpha.real, alpha.imag])
    return mu, (cov + cov.T) / 2.0


def lossy(mu, cov, eta, hbar=HBAR):
    """Every mode through a loss channel of transmission eta: a mixed state."""
    return np.sqrt(eta) * mu, eta * cov + (1.0 - eta) * (hbar / 2.0) * np.eye(cov.shape[0])


def random_unitary(M, seed):
    rng = np.random.default_rng(seed)
    q, rr = np.linalg.qr(rng.standard_normal((M, M)) + 1j * rng.standard_normal((M, M)))
    return q * (np.diag(rr) / np.abs(np.diag(rr)))[None, :]


def three_mode_state():
    return gaussian_state([0.11, -0.08, 0.1], random_unitary(3, 26), [0.12 + 0.05j, -0.08 + 0.1j, 0.05 - 0.12j])


def two_mode_state():
    bs = np.array([[1.0, 1.0], [1.0, -1.0]]) / np.sqrt(2.0)
    return gaussian_state([0.35, 0.25], bs, [0.3 + 0.2j, -0.25 + 0.35j])


def all_patterns(M, top):
    return np.array(list(itertools.product(range(top + 1), repeat=M)), dtype=np.int64)


# ---- 1. the each-entry: the bits of the single-order entry ---------------------

def each_case(seed=2600, M=7, nmu=5):
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((M, M)) + 1j * rng.standard_normal((M, M))
    A = A + A.T
    mus = rng.standard_normal((nmu, M)) + 1j * rng.standard_normal((nmu, M))
    return A, mus, rng


def ragged_lists(rng, M, orders):
    """One list per order: collision patterns vary with the position."""
    return [rng.integers(0, (2, 3, M, 1)[k % 4] if n > 12 else M, n) for k, n in enumerate(orders)]


def test_each_entry_has_the_bits_of_the_single_order_entry(sup):
    A, mus, rng = each_case()
    orders = [0, 1, 2, 3, 7, 8, 16, 17, 3, 0, 8, 17, 2, 16, 1, 7]
    lists = ragged_lists(rng, 7, orders)
    lists[6] = np.array([0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 0, 1])  # 16 with seven distinct values
    mu_of = [k % 5 for k in range(len(orders))]
    v, st = sup.loop_hafnian_each(A, mus, lists, mu_of=mu_of, cpu=True, return_stats=True)
    terms = 0
    for k, l in enumerate(lists):
        if len(l) == 0:
            assert bits(v[k]).tolist() == bits(1.0 + 0.0j).tolist()  # exactly 1 + 0i
            continue
        want = sup.hafnian_batch(A, l, mu=mus[mu_of[k]], loop=True, cpu=True)
        assert bits(v[k]).tolist() == bits(want).tolist(), (k, len(l))
        terms += sup.hafnian_plan(l)
    assert st["visited_steps"] == terms and st["leaves"] == len(lists) and st["est_ops_per_step"] > 0
    assert st["gray_steps"] == sum(1 << (n - 1) for n in orders if n)
    # the whole matrix at its own diagonal: loop_hafnian's bits
    whole = sup.loop_hafnian_each(A, np.diag(A)[None, :], [np.arange(7)], cpu=True)
    assert bits(whole[0]).tolist() == bits(sup.loop_hafnian(A, cpu=True)).tolist()
    # mu_of = None: item k reads row k
    v5 = sup.loop_hafnian_each(A, mus, lists[2:7], cpu=True)
    for k in range(5):
        assert bits(v5[k]).tolist() == bits(sup.hafnian_batch(A, lists[2 + k], mu=mus[k], loop=True, cpu=True)).tolist()


def test_each_entry_shares_one_row_among_items_and_threads_do_not_change_bits(sup):
    A, mus, rng = each_case(2601)
    orders = [(0, 1, 2, 3, 7, 8, 16, 17)[k % 8] for k in range(65)]
    lists = ragged_lists(rng, 7, orders)
    mu_of = [3] * 60 + [0, 1, 2, 4, 3]
    one = sup.loop_hafnian_each(A, mus, lists, mu_of=mu_of, cpu=True, threads=1)
    many = sup.loop_hafnian_each(A, mus, lists, mu_of=mu_of, cpu=True, threads=16)
    assert np.array_equal(bits(one), bits(many))
    for k in (1, 9, 15, 62):
        assert bits(one[k]).tolist() == bits(sup.hafnian_batch(A, lists[k], mu=mus[mu_of[k]], loop=True, cpu=True)).tolist()
    assert all(bits(one[k]).tolist() == bits(1.0 + 0.0j).tolist() for k in range(0, 65, 8))
    assert sup.loop_hafnian_each(A, mus, [], cpu=True).shape == (0,)


def raw_each(sup, A, mus, mu_of, idx, stride, n, count, cpu=1, null=()):
    """sup_loop_hafnian_complex_each as C sees it: (rc, message)."""
    lib = sup._lib.load()
    a = np.ascontiguousarray(A, dtype=np.complex128)
    m = np.ascontiguousarray(mus, dtype=np.complex128)
    i32 = np.ascontiguousarray(idx, dtype=np.int32)
    n32 = np.ascontiguousarray(n, dtype=np.int32)
    of = None if mu_of is None else np.ascontiguousarray(mu_of, dtype=np.int32)
    out = np.zeros(2 * max(count, 1))
    ptr = {"A": a.ctypes.data, "mu": m.ctypes.data, "idx": i32.ctypes.data, "n": n32.ctypes.data,
           "out": out.ctypes.data}
    for name in null:
        ptr[name] = None
    rc = lib.sup_loop_hafnian_complex_each(ptr["A"], a.shape[0], ptr["mu"], m.shape[0],
                                           None if of is None else of.ctypes.data, ptr["idx"], stride, ptr["n"],
                                           count, None, cpu, ptr["out"], None)
    return rc, lib.sup_last_error().decode()


def test_each_entry_errors(sup):
    A, mus, _ = each_case(2602)
    idx = np.array([[0, 1, 2, 3], [4, 5, 6, 0]])
    ok = dict(mu_of=[0, 4], idx=idx, stride=4, n=[4, 3], count=2)
    assert raw_each(sup, A, mus, **ok)[0] == 0
    for name in ("A", "mu", "idx", "n", "out"):
        rc, msg = raw_each(sup, A, mus, null=(name,), **ok)
        assert rc == -1 and "null" in msg, name
    bad = A.copy()
    bad[2, 5] = np.nextafter(bad[2, 5].real, 9.0) + 1j * bad[2, 5].imag  # one ulp
    rc, msg = raw_each(sup, bad, mus, **ok)
    assert rc == -1 and "symmetric" in msg and "[2][5]" in msg
    rc, msg = raw_each(sup, A, mus, **{**ok, "stride": 3, "idx": idx[:, :3]})
    assert rc == -1 and "stride = 3" in msg and "k = 0" in msg
    for v in (-1, 65):
        wide = np.zeros((2, 65), np.int32)
        rc, msg = raw_each(sup, A, mus, **{**ok, "idx": wide, "stride": 65, "n": [4, v]})
        assert rc == -1 and "n[k = 1]" in msg and "[0, 64]" in msg
    for v in (-1, 5):
        rc, msg = raw_each(sup, A, mus, **{**ok, "mu_of": [0, v]})
        assert rc == -1 and "mu_of[k = 1]" in msg and "[0, 5)" in msg
    rc, msg = raw_each(sup, A, mus[:1], **{**ok, "mu_of": None})  # row k = 1 of one row
    assert rc == -1 and "mu_of[k = 1]" in msg
    for v in (-1, 7):
        j = idx.copy()
        j[1, 2] = v
        rc, msg = raw_each(sup, A, mus, **{**ok, "idx": j})
        assert rc == -1 and "idx[k = 1][position 2]" in msg
    j = idx.copy()
    j[1, 3] = 99  # past n[1] = 3: not read
    assert raw_each(sup, A, mus, **{**ok, "idx": j})[0] == 0
    with pytest.raises(sup.SupError) as e:
        sup.loop_hafnian_each(A, mus, [[0, 1], [7]], cpu=True)
    assert e.value.code == -1
    with pytest.raises(ValueError):
        sup.loop_hafnian_each(A, mus, [np.zeros(65, int)], cpu=True)


def test_each_entry_refuses_more_than_2_24_wave_chunks_before_any_work(sup):
    rng = np.random.default_rng(4)
    A = rng.standard_normal((42, 42)) + 0j
    A = A + A.T
    with pytest.raises(sup.SupError) as e:
        sup.loop_hafnian_each(A, np.zeros((1, 42)), [[0, 1], np.arange(42)], mu_of=[0, 0], cpu=True)
    assert e.value.code == -7 and "k = 1" in str(e.value)


def test_each_entry_without_a_device_is_an_error_not_a_cpu_fallback(sup):
    A, mus, rng = each_case(2603)
    lists = ragged_lists(rng, 7, [0, 3, 8, 5])
    if sup.device_count() == 0:
        with pytest.raises(sup.SupError) as e:
            sup.loop_hafnian_each(A, mus, lists)
        assert e.value.code == -2
        with pytest.raises(sup.SupError) as e:
            sup.gbs_sample_chain(np.zeros((1, 1)), np.zeros(1), np.zeros((2, 1)), 1)
        assert e.value.code == -2
    else:
        assert np.array_equal(bits(sup.loop_hafnian_each(A, mus, lists)), bits(sup.loop_hafnian_each(A, mus, lists, cpu=True)))


# ---- 2. probabilities: closed forms --------------------------------------------

def test_single_mode_squeezed_vacuum(sup):
    r = 0.6
    _, cov = gaussian_state([r], None, [0])
    p = sup.pnr_detection_probs(None, cov, np.arange(13)[:, None], cpu=True)
    for k in range(7):
        want = math.tanh(r) ** (2 * k) * math.factorial(2 * k) / (4 ** k * math.factorial(k) ** 2 * math.cosh(r))
        assert abs(p[2 * k] - want) <= 1e-14, (k, p[2 * k], want)
    assert (p[1::2] == 0.0).all()  # odd photon numbers: exactly zero
    assert sup.pnr_detection_prob(None, cov, [4], cpu=True) == p[4]


def test_coherent_state_is_poisson(sup):
    alpha = np.array([0.7 - 0.4j, -0.3 + 0.9j])
    mu, cov = gaussian_state([0, 0], None, alpha)
    pat = all_patterns(2, 6)
    p = sup.pnr_detection_probs(mu, cov, pat, cpu=True)
    a2 = np.abs(alpha) ** 2
    for q, n in zip(p, pat):
        want = np.prod([math.exp(-a2[i]) * a2[i] ** int(n[i]) / math.factorial(int(n[i])) for i in range(2)])
        assert abs(q - want) <= 1e-14 * max(want, 1e-3), (n, q, want)


def test_two_mode_squeezed_vacuum(sup):
    r = 0.5
    bs = np.array([[1.0, 1.0], [1.0, -1.0]]) / np.sqrt(2.0)
    _, cov = gaussian_state([r, -r], bs, [0, 0])
    lam = math.tanh(r)
    pat = all_patterns(2, 5)
    p = sup.pnr_detection_probs(None, cov, pat, cpu=True)
    for q, n in zip(p, pat):
        want = (1 - lam ** 2) * lam ** (2 * int(n[0])) if n[0] == n[1] else 0.0
        assert abs(q - want) <= 1e-14, (n, q, want)


# ---- 3. the pure (order N) and the general (order 2N) formula agree -------------

def mixed_path_probs(sup, mu, cov, pat):
    """The order-2N formula of pnr_detection_probs restated on hafnian_batch, one
    pattern per call, for states the function itself would send down the pure
    path."""
    O, gamma, pre = sup._threshold_setup(mu, cov, HBAR)
    M = O.shape[0] // 2
    Abar = np.concatenate([O[M:], O[:M]])
    Abar = (Abar + Abar.T) / 2.0
    out = np.zeros(len(pat))
    for k, n in enumerate(pat):
        if n.sum() == 0:
            out[k] = pre
            continue
        idx = np.repeat(np.concatenate([np.arange(M), np.arange(M) + M]), np.concatenate([n, n]))
        v = sup.hafnian_batch(Abar, idx, mu=np.conj(gamma), loop=True, cpu=True)
        out[k] = pre * v.real / np.prod([math.factorial(int(x)) for x in n])
    return out


def test_pure_and_general_formula_agree(sup):
    """Measured on the host twin: the largest difference over the 64 patterns
    is 2.1e-16 (probabilities up to 0.94); the bound is two decades above it.
    The opposite conjugation convention differs by 2.9e-3 on this state."""
    mu, cov = three_mode_state()
    pat = all_patterns(3, 3)
    pure = sup.pnr_detection_probs(mu, cov, pat, cpu=True)
    B, zeta, p0 = sup.gbs_pure_state(mu, cov)  # the pure path is the one taken
    lists = [np.repeat(np.arange(3), n) for n in pat]
    v = sup.loop_hafnian_each(B, zeta[None, :], lists, mu_of=np.zeros(64, int), cpu=True)
    fac = np.array([np.prod([math.factorial(int(x)) for x in n]) for n in pat])
    assert np.array_equal(pure[1:], (p0 * (v.real * v.real + v.imag * v.imag) / fac)[1:]) and pure[0] == p0
    general = mixed_path_probs(sup, mu, cov, pat)
    d = np.abs(pure - general).max()
    print(f"pure vs general: max |difference| = {d:.3e}, largest p = {pure.max():.3f}")
    assert d <= 2.1e-14
    wrong = sup.loop_hafnian_each(B, np.conj(zeta)[None, :], lists, mu_of=np.zeros(64, int), cpu=True)
    assert np.abs(p0 * np.abs(wrong) ** 2 / fac - general).max() > 1e-4  # the check has teeth
    # a mixed state takes the order-2N path by itself
    ml, cl = lossy(mu, cov, 0.8)
    with pytest.raises(ValueError):
        sup.gbs_pure_state(ml, cl)
    assert np.array_equal(sup.pnr_detection_probs(ml, cl, pat[:9], cpu=True), mixed_path_probs(sup, ml, cl, pat[:9]))


# ---- 4. against the threshold table --------------------------------------------

@pytest.mark.parametrize("eta", [1.0, 0.8])
def test_sums_over_click_patterns_match_the_threshold_table(sup, eta):
    """eta = 1: the pure path; eta = 0.8: the same state after loss, mixed."""
    mu, cov = three_mode_state()
    if eta < 1.0:
        mu, cov = lossy(mu, cov, eta)
    cutoff = 7
    pat = all_patterns(3, cutoff)
    p = sup.pnr_detection_probs(mu, cov, pat, cpu=True, threads=16)
    missing = 1.0 - p.sum()
    table = sup.threshold_detection_distribution(mu, cov, cpu=True)
    print(f"eta = {eta}: missing = {missing:.3e}")
    assert -1e-12 <= missing < 1e-8
    click = ((pat > 0) * (1 << np.arange(3))[None, :]).sum(1)
    for c in range(8):
        s = p[click == c].sum()
        assert table[c] - missing - 1e-12 <= s <= table[c] + 1e-12, (c, s, table[c])


# ---- 5. the sampler ------------------------------------------------------------

def test_sampler_vacuum_and_cutoff_zero_give_zeros(sup):
    _, vac = gaussian_state([0, 0, 0], None, [0, 0, 0])
    assert (sup.gbs_sample(None, vac, 50, 1, cpu=True) == 0).all()
    mu, cov = three_mode_state()
    s, st = sup.gbs_sample(mu, cov, 50, 1, cutoff=0, cpu=True, return_stats=True)
    assert s.shape == (50, 3) and s.dtype == np.int32 and (s == 0).all()
    assert st["leaves"] == 50 and st["failed"] == 0
    assert sup.gbs_sample(mu, cov, 0, 1, cpu=True).shape == (0, 3)
    with pytest.raises(ValueError):
        sup.gbs_sample(*lossy(mu, cov, 0.9), 4, 1, cpu=True)


def test_sampler_pieces_with_sample0_are_the_whole_run(sup):
    mu, cov = three_mode_state()
    whole, st = sup.gbs_sample(mu, cov, 97, 5, cutoff=4, cpu=True, return_stats=True)
    assert whole.max() >= 1 and whole.min() >= 0 and st["visited_steps"] > 0
    assert np.array_equal(whole, sup.gbs_sample(mu, cov, 97, 5, cutoff=4, cpu=True, threads=1))
    a = 33
    head = sup.gbs_sample(mu, cov, a, 5, cutoff=4, cpu=True)
    tail = sup.gbs_sample(mu, cov, 97 - a, 5, cutoff=4, sample0=a, cpu=True)
    assert np.array_equal(np.concatenate([head, tail]), whole)
    assert not np.array_equal(whole, sup.gbs_sample(mu, cov, 97, 6, cutoff=4, cpu=True))


def test_sampler_chain_errors(sup):
    B = np.array([[0.1, 0.2], [0.2, 0.3]], complex)
    z, het = np.zeros(2), np.zeros((3, 2))
    assert (sup.gbs_sample_chain(B, z, het, 1, cutoff=3, cpu=True) >= 0).all()
    bad = B.copy()
    bad[0, 1] = 0.25
    for kw in (dict(B=bad), dict(cutoff=-1), dict(cutoff=65)):
        args = dict(B=B, zeta=z, het=het, seed=1, cutoff=3, cpu=True)
        args.update(kw)
        with pytest.raises(sup.SupError) as e:
            sup.gbs_sample_chain(**args)
        assert e.value.code == -1
    with pytest.raises(sup.SupError) as e:
        sup.gbs_sample_chain(np.zeros((65, 65)), np.zeros(65), np.zeros((1, 65)), 1, cpu=True)
    assert e.value.code == -1
    # weights that overflow: the sample is marked, not drawn
    s, st = sup.gbs_sample_chain(np.array([[0.5]]), np.array([1e200]), np.zeros((2, 1)), 1, cutoff=4, cpu=True,
                                 return_stats=True)
    assert (s == -1).all() and st["failed"] == 2


def within_five_sigma(counts, p, n):
    sigma = np.sqrt(n * p * (1.0 - p))
    z = np.abs(counts - n * p) / sigma
    return z


def test_sampler_single_mode_follows_the_truncated_law(sup):
    mu, cov = gaussian_state([0.5], None, [0.4 + 0.3j])
    cutoff, n = 6, 20000
    s = sup.gbs_sample(mu, cov, n, 11, cutoff=cutoff, cpu=True)
    p = sup.pnr_detection_probs(mu, cov, np.arange(cutoff + 1)[:, None], cpu=True)
    p = p / p.sum()
    assert s.min() >= 0 and s.max() <= cutoff
    z = within_five_sigma(np.bincount(s[:, 0], minlength=cutoff + 1), p, n)
    print("M = 1: sigmas", np.round(z, 2))
    assert z.max() <= 5.0


def test_sampler_statistics_two_modes(sup):
    """r = 0.35, 0.25, a balanced beamsplitter, |alpha| = 0.36 and 0.43, cutoff
    7, 40,000 samples: each of the nine cells n1, n2 <= 2 within 5 binomial
    sigma of pnr_detection_probs (a correct sampler fails with probability below
    1e-5).  The committed seed sits at 2.2 sigma on the host twin."""
    mu, cov = two_mode_state()
    n = 40000
    s = sup.gbs_sample(mu, cov, n, 2026, cutoff=7, cpu=True, threads=16)
    assert s.min() >= 0
    pat = all_patterns(2, 2)
    p = sup.pnr_detection_probs(mu, cov, pat, cpu=True)
    counts = np.array([((s[:, 0] == a) & (s[:, 1] == b)).sum() for a, b in pat])
    z = within_five_sigma(counts, p, n)
    print("two modes: sigmas", np.round(z, 2), "p", np.round(p, 4))
    assert z.max() <= 5.0
