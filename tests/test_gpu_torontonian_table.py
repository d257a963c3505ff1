"""Torontonian tables on the GPU (the table forms of walk_tor.hip and
walk_ltor.hip, then mobius.hip): bit for bit the host twin, raw and
transformed, at the smallest shapes where the kernels can go wrong (fewer
positions than tail bits, the first prefixes, more than one chunk, every pass
count of the transform and a ragged last pass), one table of 2^20, and the
distribution and the sampler on it.  Bits are compared as uint64."""
import numpy as np
import pytest

from test_loop_torontonian import dyadic_gamma, random_state
from test_torontonian import dyadic_O, fbits
from test_torontonian_table import U, int_case, int_mobius

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def need_gpu(sup):
    if sup.device_count() < 1:
        pytest.fail("no HIP device visible: -m gpu tests must run on the MI355X box")


def same_bits(a, b):
    """uint64 equality; a NaN is a NaN (its payload is not compared)."""
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(fbits(a[~na]), fbits(b[~nb]))


def both(sup, O, gamma, modes, **kw):
    if gamma is None:
        return sup.torontonian_table(O, modes, **kw), sup.torontonian_table(O, modes, cpu=True, **kw)
    return sup.loop_torontonian_table(O, gamma, modes, **kw), sup.loop_torontonian_table(O, gamma, modes, cpu=True, **kw)


@pytest.mark.parametrize("n", [1, 2, 4, 5, 6, 7, 9, 10, 12, 16])
def test_gpu_table_bits_are_the_twins(sup, n):
    O = dyadic_O(18, 9000 + n)
    modes = np.random.default_rng(n).permutation(18)[:n]
    for gamma in (None, dyadic_gamma(O, 9050 + n)):
        for transform in (False, True):
            dev, host = both(sup, O, gamma, modes, transform=transform)
            assert dev.shape == (1 << n,) and same_bits(dev, host), (n, gamma is None, transform)
    tab, st = sup.torontonian_table(O, modes, return_stats=True)
    assert st["devices_used"] == 1 and st["kernel_ms"] > 0 and st["grid"] >= 1 and st["leaves"] == 1
    assert st["gray_steps"] == st["visited_steps"] == 1 << n
    assert st["est_ops_per_step"] == sup.torontonian_plan(n)[1] + n / 2


@pytest.mark.parametrize("group", [1, 64])
def test_gpu_table_bits_do_not_depend_on_the_queue_group(sup, monkeypatch, group):
    n = 12
    O = dyadic_O(14, 9100)
    gamma = dyadic_gamma(O, 9101)
    modes = np.random.default_rng(91).permutation(14)[:n]
    want = [sup.torontonian_table(O, modes, cpu=True), sup.loop_torontonian_table(O, gamma, modes, cpu=True)]
    monkeypatch.setenv("SUP_WALK_GROUP", str(group))
    assert same_bits(sup.torontonian_table(O, modes), want[0])
    assert same_bits(sup.loop_torontonian_table(O, gamma, modes), want[1])


def test_gpu_nan_reaches_exactly_the_supersets(sup):
    O = dyadic_O(8, 9200)
    O[3, 3] = 1.5
    modes = np.array([4, 0, 3, 5, 1, 2, 7, 6])
    dev, host = both(sup, O, None, modes)
    assert same_bits(dev, host) and np.array_equal(np.isnan(dev), ((np.arange(256) >> 2) & 1).astype(bool))


def int64_mobius(v):
    t = np.asarray(v).astype(np.int64)
    for b in range(int(t.shape[0]).bit_length() - 1):
        w = t.reshape(-1, 2, 2 ** b)
        w[:, 1, :] -= w[:, 0, :]
    return t


def mobius_sizes(sup):
    L, K = sup.MOBIUS_TILE_BITS, sup.MOBIUS_PASS_BITS
    sizes = {0, 1, L - 1, L, L + 1, L + K, L + K + 1}
    passes = lambda n: 1 if n <= L else 1 + -(-(n - L) // K)
    for p in range(2, passes(24) + 1):  # the smallest n <= 24 of each further pass count
        sizes.add(min(n for n in range(25) if passes(n) == p))
    return sorted(sizes)


def test_gpu_subset_mobius_on_integers(sup):
    v12 = int_case(12)
    assert int64_mobius(v12).tolist() == int_mobius(v12)  # the exact reference against Python's own integers
    for n in mobius_sizes(sup):
        v = int_case(n)
        want = int64_mobius(v)
        assert np.max(np.abs(want)) < 2 ** 53
        got = sup.subset_mobius(v)
        assert got.shape == v.shape and np.array_equal(got.astype(np.int64), want) and np.array_equal(got, np.rint(got)), n


@pytest.mark.parametrize("bits,passes", [("6,3", 3), ("6,2", 4), ("7,4", 3), ("8,3", 3), ("10,1", 3)])
def test_gpu_subset_mobius_with_forced_shapes(sup, monkeypatch, bits, passes):
    """Three and four passes at n = 12, ragged last passes (7,4: 4 + 1 bits; 8,3: 3 + 1)."""
    L, K = (int(x) for x in bits.split(","))
    assert 1 + -(-(12 - L) // K) == passes
    v = int_case(12)
    monkeypatch.setenv("SUP_MOBIUS_BITS", bits)
    assert np.array_equal(sup.subset_mobius(v).astype(np.int64), int64_mobius(v))
    O = dyadic_O(12, 9300)
    assert same_bits(sup.torontonian_table(O), sup.torontonian_table(O, cpu=True))


def test_gpu_table_of_twenty_modes(sup):
    n = 20
    O = dyadic_O(n, 9400)
    raw, host_raw = both(sup, O, None, np.arange(n), transform=False)
    assert same_bits(raw, host_raw)
    tab = sup.torontonian_table(O)
    assert same_bits(tab, sup.subset_mobius(host_raw, cpu=True))
    full = sup.torontonian(O)
    zeta = float(np.sum(raw))
    err, bound = abs(tab[-1] - full), 2 * (n + 21) * U * zeta
    print(f"n = 20: |table[full] - torontonian| = {err:.3e}, bound {bound:.3e}")
    assert err <= bound


def test_gpu_distribution_and_sampler_are_the_twins(sup):
    mu, cov = random_state(6, 4600)
    p = sup.threshold_detection_distribution(mu, cov)
    assert same_bits(p, sup.threshold_detection_distribution(mu, cov, cpu=True))
    p0 = sup.threshold_detection_distribution(None, cov, modes=[4, 1, 2])
    assert same_bits(p0, sup.threshold_detection_distribution(None, cov, modes=[4, 1, 2], cpu=True))
    s = sup.threshold_detection_sample(mu, cov, 20000, 12345)
    assert np.array_equal(s, sup.threshold_detection_sample(mu, cov, 20000, 12345, cpu=True))
