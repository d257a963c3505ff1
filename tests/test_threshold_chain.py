"""The threshold-detector chain-rule sampler on ragged loop torontonians (ABI 28,
DESIGN.md §8p) on the host twin: the each-entry's bits against the single-order
entry, every error, the conventions against threshold_detection_probs, the
sampler's weights against a numpy restatement, its identities and its law."""
import itertools

import numpy as np
import pytest

from test_gbs import gaussian_state, lossy, random_unitary

HBAR = 2.0


def dbits(v):
    return np.ascontiguousarray(np.asarray(v, dtype=np.float64)).view(np.uint64)


# ---- 1. the each-entry: the bits of the single-order entry ---------------------

# no walk (0); padded below the tail width W = 4 (1, 3); the tail alone (4: no
# position of the list is a prefix position); one 64-group (5, 6); two groups
# (7); one 512-chunk (9); two chunks to fold (10); eight (12)
ORDERS = [0, 1, 3, 4, 5, 6, 7, 9, 10, 12]


def each_case(seed=2800, M=13, ngamma=5):
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((2 * M, 2 * M)) + 1j * rng.standard_normal((2 * M, 2 * M))
    H = A @ A.conj().T
    O = 0.45 * H / np.linalg.norm(H, 2)  # I - O_z positive definite for every z
    gammas = 0.3 * (rng.standard_normal((ngamma, 2 * M)) + 1j * rng.standard_normal((ngamma, 2 * M)))
    return O, gammas, rng


def ragged_lists(rng, M, orders):
    return [rng.permutation(M)[:n] for n in orders]


@pytest.mark.parametrize("slab", [None, "1", "3"])
@pytest.mark.parametrize("threads", [1, 16])
def test_each_entry_has_the_bits_of_the_single_order_entry(sup, monkeypatch, slab, threads):
    O, gammas, rng = each_case()
    orders = ORDERS + ORDERS[::-1]
    lists = ragged_lists(rng, 13, orders)
    if slab is not None:
        monkeypatch.setenv("SUP_LTOR_EACH_SLAB", slab)  # read at every call
    # shared rows: five rows among twenty items; own rows: item k reads row k
    shared = [(3 * k) % 5 for k in range(len(orders))]
    own = np.concatenate([gammas] * 4)
    for rows, gamma_of in ((gammas, shared), (own, None)):
        v, st = sup.loop_torontonian_each(O, rows, lists, gamma_of=gamma_of, cpu=True, threads=threads, return_stats=True)
        assert v.shape == (len(orders),) and np.isfinite(v).all()
        for k, l in enumerate(lists):
            if len(l) == 0:
                assert dbits(v[k]).tolist() == dbits(1.0).tolist()  # exactly 1.0
                continue
            g = rows[k if gamma_of is None else gamma_of[k]]
            want = sup.loop_torontonian_batch(O, g, l, cpu=True)
            assert dbits(v[k]).tolist() == dbits(want).tolist(), (k, len(l))
        walking = [n for n in orders if n]
        assert st["leaves"] == len(orders)
        assert st["gray_steps"] == st["visited_steps"] == sum(1 << n for n in walking)
        ops = sum((1 << n) * sup.loop_torontonian_plan(n)[1] for n in walking) / sum(1 << n for n in walking)
        assert abs(st["est_ops_per_step"] - ops) <= 1e-12 * ops
    assert sup.loop_torontonian_each(O, gammas, [], cpu=True).shape == (0,)
    # a single row given as a vector
    one = sup.loop_torontonian_each(O, gammas[2], [lists[5]], cpu=True)
    assert dbits(one[0]).tolist() == dbits(sup.loop_torontonian_batch(O, gammas[2], lists[5], cpu=True)).tolist()


def raw_each(sup, O, gammas, gamma_of, modes, stride, n, count, cpu=1, null=(), M=None):
    """sup_loop_torontonian_each as C sees it: (rc, message)."""
    lib = sup._lib.load()
    o = np.ascontiguousarray(O, dtype=np.complex128)
    g = np.ascontiguousarray(gammas, dtype=np.complex128)
    i32 = np.ascontiguousarray(modes, dtype=np.int32)
    n32 = np.ascontiguousarray(n, dtype=np.int32)
    of = None if gamma_of is None else np.ascontiguousarray(gamma_of, dtype=np.int32)
    out = np.zeros(max(count, 1))
    ptr = {"O": o.ctypes.data, "gamma": g.ctypes.data, "modes": i32.ctypes.data, "n": n32.ctypes.data, "out": out.ctypes.data}
    for name in null:
        ptr[name] = None
    rc = lib.sup_loop_torontonian_each(ptr["O"], o.shape[0] // 2 if M is None else M, ptr["gamma"], g.shape[0],
                                       None if of is None else of.ctypes.data, ptr["modes"], stride, ptr["n"], count,
                                       None, cpu, ptr["out"], None)
    return rc, lib.sup_last_error().decode(), out


def test_each_entry_errors(sup, monkeypatch):
    O, gammas, _ = each_case(2801)
    modes = np.array([[0, 1, 2, 3], [4, 5, 6, 0]])
    ok = dict(gamma_of=[0, 4], modes=modes, stride=4, n=[4, 3], count=2)
    assert raw_each(sup, O, gammas, **ok)[0] == 0
    for name in ("O", "gamma", "modes", "n", "out"):
        rc, msg, _ = raw_each(sup, O, gammas, null=(name,), **ok)
        assert rc == -1 and "null" in msg, name
    rc, msg, _ = raw_each(sup, O, gammas, M=0, **ok)
    assert rc == -1 and "M = 0" in msg
    rc, msg, _ = raw_each(sup, O, gammas, **{**ok, "stride": 3, "modes": modes[:, :3]})
    assert rc == -1 and "stride = 3" in msg and "k = 0" in msg
    for v in (-1, 33):
        wide = np.tile(np.arange(13), 3)[None, :33].repeat(2, 0)
        rc, msg, _ = raw_each(sup, O, gammas, **{**ok, "modes": wide, "stride": 33, "n": [4, v]})
        assert rc == -1 and "n[k = 1]" in msg and "[0, 32]" in msg
    for v in (-1, 5):
        rc, msg, _ = raw_each(sup, O, gammas, **{**ok, "gamma_of": [0, v]})
        assert rc == -1 and "gamma_of[k = 1]" in msg and "[0, 5)" in msg
    rc, msg, _ = raw_each(sup, O, gammas[:1], **{**ok, "gamma_of": None})  # row k = 1 of one row
    assert rc == -1 and "gamma_of[k = 1]" in msg
    for v in (-1, 13):
        j = modes.copy()
        j[1, 2] = v
        rc, msg, _ = raw_each(sup, O, gammas, **{**ok, "modes": j})
        assert rc == -1 and "modes[k = 1][position 2]" in msg
    j = modes.copy()
    j[0, 3] = 1  # mode 1 twice in list 0
    rc, msg, _ = raw_each(sup, O, gammas, **{**ok, "modes": j})
    assert rc == -1 and "k = 0" in msg and "distinct" in msg and "positions 1 and 3" in msg
    j = modes.copy()
    j[1, 3] = 99  # past n[1] = 3: not read, and a repeat there is none
    assert raw_each(sup, O, gammas, **{**ok, "modes": j})[0] == 0
    for knob in ("0", "-2", "three", "2x", ""):
        monkeypatch.setenv("SUP_LTOR_EACH_SLAB", knob)
        rc, msg, out = raw_each(sup, O, gammas, **ok)
        assert rc == -1 and "SUP_LTOR_EACH_SLAB" in msg, knob
        assert (out == 0).all()  # before any work
    monkeypatch.delenv("SUP_LTOR_EACH_SLAB")
    # every error comes before any work: an item of order 0 ahead of the bad one is not written
    rc, msg, out = raw_each(sup, O, gammas, **{**ok, "n": [0, 5]})
    assert rc == -1 and (out == 0).all()
    with pytest.raises(sup.SupError) as e:
        sup.loop_torontonian_each(O, gammas, [[0, 1], [13]], cpu=True)
    assert e.value.code == -1
    with pytest.raises(ValueError):
        sup.loop_torontonian_each(O, gammas[:, :5], [[0]], cpu=True)


def test_each_entry_without_a_device_is_an_error_not_a_cpu_fallback(sup):
    O, gammas, rng = each_case(2802)
    lists = ragged_lists(rng, 13, [0, 3, 7, 5])
    if sup.device_count() == 0:
        with pytest.raises(sup.SupError) as e:
            sup.loop_torontonian_each(O, gammas, lists)
        assert e.value.code == -2
        with pytest.raises(sup.SupError) as e:
            sup.threshold_sample_chain(np.zeros((1, 1)), np.zeros(1), np.zeros((2, 1)), 1)
        assert e.value.code == -2
    else:
        assert np.array_equal(dbits(sup.loop_torontonian_each(O, gammas, lists)),
                              dbits(sup.loop_torontonian_each(O, gammas, lists, cpu=True)))


# ---- 2. the conventions ---------------------------------------------------------

def three_mode_state():
    """Pure, displaced, every click pattern likely."""
    return gaussian_state([0.55, -0.4, 0.5], random_unitary(3, 28), [0.35 + 0.2j, -0.3 + 0.4j, 0.25 - 0.45j])


def chain_setup(sup, mu, cov):
    """(O, gamma, p0) of the sampler's own setup: O from B, gamma = (zeta, conj zeta)."""
    B, zeta, p0 = sup.gbs_pure_state(mu, cov)
    M = B.shape[0]
    O = np.zeros((2 * M, 2 * M), complex)
    O[:M, M:], O[M:, :M] = B, B.conj()
    return B, zeta, p0, O, np.concatenate([zeta, zeta.conj()])


def test_conventions_match_threshold_detection_probs(sup):
    """p0 loop_torontonian_each(O from B, (zeta, conj zeta)) over all 8 patterns
    against threshold_detection_probs, which differs only by the rounding of the
    setup (its O keeps the rounding of I - Q^-1 in the diagonal blocks, its
    gamma is Q^-1 alpha whole).  Measured on the host twin: the largest
    difference is 3.2e-16 (probabilities up to 0.48); the bound is two decades
    above it."""
    mu, cov = three_mode_state()
    B, zeta, p0, O, gamma = chain_setup(sup, mu, cov)
    pat = np.array(list(itertools.product((0, 1), repeat=3)))
    lists = [np.nonzero(p)[0] for p in pat]
    got = p0 * sup.loop_torontonian_each(O, gamma, lists, gamma_of=np.zeros(8, int), cpu=True)
    want = sup.threshold_detection_probs(mu, cov, pat, cpu=True)
    d = np.abs(got - want).max()
    print(f"each vs threshold_detection_probs: max |difference| = {d:.3e}, largest p = {want.max():.3f}, sum = {got.sum():.16f}")
    assert d <= 3.2e-14
    assert want.min() > 0.005  # every pattern matters
    # the other conjugation is another state: the check has teeth
    wrong = p0 * sup.loop_torontonian_each(O, np.concatenate([zeta.conj(), zeta]), lists, gamma_of=np.zeros(8, int), cpu=True)
    assert np.abs(wrong - want).max() > 1e-3


# ---- 3. the weights -------------------------------------------------------------

def ltor_restated(O, gamma, modes):
    """(ltor, sum_Z f(Z)) of the list by a dense solve per subset."""
    M = O.shape[0] // 2
    modes = np.asarray(modes, int)
    total, scale = 0.0, 0.0
    for r in range(len(modes) + 1):
        for Z in itertools.combinations(range(len(modes)), r):
            ix = np.concatenate([modes[list(Z)], modes[list(Z)] + M]).astype(int)
            if ix.size == 0:
                f = 1.0
            else:
                Mz = np.eye(ix.size) - O[np.ix_(ix, ix)]
                g = gamma[ix]
                f = (np.exp(0.5 * (g.conj() @ np.linalg.solve(Mz, g)).real) / np.sqrt(np.linalg.det(Mz).real))
            total += (-1.0) ** (len(modes) - r) * f
            scale += f
    return total, scale


def four_mode_state():
    return gaussian_state([0.5, -0.45, 0.4, 0.55], random_unitary(4, 29),
                          [0.3 + 0.2j, -0.25 + 0.3j, 0.2 - 0.35j, -0.3 - 0.1j])


def test_weights_are_the_restated_conditional_loop_torontonians(sup):
    """M = 4, 64 samples.  The weights of return_weights against the formulas
    restated in numpy (z by a matrix product, a dense solve per subset), relative
    to sum_Z f(Z).  The yardstick is the parent's single-order entry fed the
    same lists and the same numpy gamma against the same restatement: measured
    on the host twin 2.04e-16; the sampler's weights, whose z differs from
    numpy's by rounding only, measured 2.04e-16 too.  The bound is 100 times the
    yardstick's figure."""
    mu, cov = four_mode_state()
    B, zeta, p0 = sup.gbs_pure_state(mu, cov)
    M, ns = 4, 64
    het = sup._gbs_heterodyne(mu, cov, M, ns, 31, HBAR, 0)
    out, w = sup.threshold_sample_chain(B, zeta, het, 31, return_weights=True, cpu=True)
    assert out.shape == (ns, M) and w.shape == (ns, M, 2) and set(np.unique(out)) == {0, 1}
    O = np.zeros((2 * M, 2 * M), complex)
    O[:M, M:], O[M:, :M] = B, B.conj()
    worst, yard = 0.0, 0.0
    for s in range(ns):
        for k in range(M):
            z = zeta[:k + 1] + B[:k + 1, k + 1:] @ het[s, k + 1:].conj()
            gamma = np.zeros(2 * M, complex)
            gamma[:k + 1], gamma[M:M + k + 1] = z, z.conj()
            C = [i for i in range(k) if out[s, i] == 1]  # the prefix the sampler itself drew
            for c, lst in enumerate((C, C + [k])):
                want, scale = ltor_restated(O, gamma, lst)
                worst = max(worst, abs(w[s, k, c] - max(want, 0.0)) / scale)
                if lst:
                    yard = max(yard, abs(sup.loop_torontonian_batch(O, gamma, lst, cpu=True) - want) / scale)
    print(f"weights vs restatement: {worst:.3e} of sum f; the single-order entry vs the same: {yard:.3e}")
    assert worst <= 100 * 2.04e-16
    assert (w >= 0).all() and not np.signbit(w).any()


# ---- 4. the sampler's identities ------------------------------------------------

def test_sampler_vacuum_gives_zeros_and_mixed_states_raise(sup):
    _, vac = gaussian_state([0, 0, 0], None, [0, 0, 0])
    s, st = sup.threshold_sample(None, vac, 50, 1, cpu=True, return_stats=True)
    assert s.shape == (50, 3) and s.dtype == np.int32 and (s == 0).all()
    assert st["leaves"] == 50 and st["failed"] == 0
    mu, cov = three_mode_state()
    assert sup.threshold_sample(mu, cov, 0, 1, cpu=True).shape == (0, 3)
    with pytest.raises(ValueError):
        sup.threshold_sample(*lossy(mu, cov, 0.9), 4, 1, cpu=True)


def test_sampler_pieces_with_sample0_are_the_whole_run(sup):
    mu, cov = three_mode_state()
    whole, st = sup.threshold_sample(mu, cov, 97, 5, cpu=True, return_stats=True)
    assert set(np.unique(whole)) == {0, 1} and st["visited_steps"] > 0
    assert st["each_ms"] > 0 and st["host_ms"] > 0 and st["kernel_ms"] == 0
    assert np.array_equal(whole, sup.threshold_sample(mu, cov, 97, 5, cpu=True, threads=1))  # 16 threads and 1
    a = 33
    head = sup.threshold_sample(mu, cov, a, 5, cpu=True)
    tail = sup.threshold_sample(mu, cov, 97 - a, 5, sample0=a, cpu=True)
    assert np.array_equal(np.concatenate([head, tail]), whole)
    assert not np.array_equal(whole, sup.threshold_sample(mu, cov, 97, 6, cpu=True))
    # the heterodyne outcomes are gbs_sample's: the helper did not change them
    B, zeta, _ = sup.gbs_pure_state(mu, cov)
    het = sup._gbs_heterodyne(mu, cov, 3, 20, 9, HBAR, 4)
    assert np.array_equal(sup.gbs_sample(mu, cov, 20, 9, cutoff=3, sample0=4, cpu=True),
                          sup.gbs_sample_chain(B, zeta, het, 9, cutoff=3, sample0=4, cpu=True))


def test_sampler_chain_errors_and_failed_samples(sup):
    B = np.array([[0.1, 0.2], [0.2, 0.3]], complex)
    z, het = np.zeros(2), np.zeros((3, 2))
    assert (sup.threshold_sample_chain(B, z, het, 1, cpu=True) >= 0).all()
    bad = B.copy()
    bad[0, 1] = 0.25
    with pytest.raises(sup.SupError) as e:
        sup.threshold_sample_chain(bad, z, het, 1, cpu=True)
    assert e.value.code == -1 and "symmetric" in str(e.value)
    with pytest.raises(sup.SupError) as e:
        sup.threshold_sample_chain(np.zeros((65, 65)), np.zeros(65), np.zeros((1, 65)), 1, cpu=True)
    assert e.value.code == -1
    # a NaN in zeta_0: -1 from mode 0 on, counted; the other samples are drawn
    zs = np.zeros((3, 2), complex)
    zs[1, 0] = np.nan
    s, w, st = sup.threshold_sample_chain(B, zs, het, 1, cpu=True, return_weights=True, return_stats=True)
    assert (s[1] == -1).all() and (s[[0, 2]] >= 0).all() and st["failed"] == 1
    assert w[1, 0, 0] == 1.0 and np.isnan(w[1, 0, 1]) and (w[1, 1] == 0).all()


# ---- 5. the sampler's law -------------------------------------------------------

def test_sampler_follows_the_exact_distribution(sup):
    """3 modes, 20,000 samples against threshold_detection_distribution: chi^2
    over the 8 patterns (every expected count is above 20 on this state, so no
    cell is merged; the merge is there for other states), (chi^2 - dof) /
    sqrt(2 dof) <= 5.  The committed seed sits at -0.9 on the host twin
    (200,000 samples of another seed: +0.07)."""
    mu, cov = three_mode_state()
    n = 20000
    s = sup.threshold_sample(mu, cov, n, 1, cpu=True, threads=16)
    assert set(np.unique(s)) == {0, 1}
    p = sup.threshold_detection_distribution(mu, cov, cpu=True)  # bit b of the index: mode b
    counts = np.bincount((s * (1 << np.arange(3))[None, :]).sum(1), minlength=8).astype(float)
    exp = n * p
    small = exp < 20.0  # cells with an expected count below 20 are merged into one
    if small.any():
        counts = np.concatenate([counts[~small], [counts[small].sum()]])
        exp = np.concatenate([exp[~small], [exp[small].sum()]])
    dof = exp.size - 1
    chi2 = ((counts - exp) ** 2 / exp).sum()
    z = (chi2 - dof) / np.sqrt(2.0 * dof)
    print(f"chi^2 = {chi2:.2f} on {dof} degrees of freedom: {z:+.2f} sigma; p = {np.round(p, 4)}")
    assert z <= 5.0
