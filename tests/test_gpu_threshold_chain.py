"""The ragged loop torontonian batch and the threshold-detector sampler on the
GPU (walk_ltore in walk_ltor.hip through sup_loop_torontonian_each and
sup_threshold_sample): bit for bit the host twin, with chunks of different
orders next to each other in one queue, across queue groups, slab boundaries
and logical devices; the smallest order whose chunks grow with n against the
single-order kernel; a pivot that is not positive; and the sampler's samples
and weights identical to the host twin's."""
import numpy as np
import pytest

from test_gbs import gaussian_state, random_unitary
from test_threshold_chain import dbits

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def need_gpu(sup):
    if sup.device_count() < 1:
        pytest.fail("no HIP device visible: -m gpu tests must run on the MI355X box")


# one-chunk items between many-chunk ones (13: 16 chunks, 16: 128), order 0 among them
ORDERS = [16, 0, 1, 13, 4, 5, 10, 6, 7, 9, 10, 0, 13, 1, 16, 5, 9, 4, 7, 6]
_REF = {}


def hermitian(rng, M, scale):
    A = rng.standard_normal((2 * M, 2 * M)) + 1j * rng.standard_normal((2 * M, 2 * M))
    H = A @ A.conj().T
    return scale * H / np.linalg.norm(H, 2)


def each_case(sup):
    """(O, gammas, lists, gamma_of, the host twin's result), computed once."""
    if "each" not in _REF:
        rng = np.random.default_rng(2828)
        M = 20
        O = hermitian(rng, M, 0.45)
        gammas = 0.25 * (rng.standard_normal((5, 2 * M)) + 1j * rng.standard_normal((5, 2 * M)))
        lists = [rng.permutation(M)[:n] for n in ORDERS]
        gamma_of = [(3 * k) % 5 for k in range(len(ORDERS))]
        want = sup.loop_torontonian_each(O, gammas, lists, gamma_of=gamma_of, cpu=True, threads=16)
        _REF["each"] = (O, gammas, lists, gamma_of, want)
    return _REF["each"]


def test_gpu_each_entry_bit_equal_to_host_twin(sup):
    O, gammas, lists, gamma_of, want = each_case(sup)
    assert sorted(set(ORDERS)) == [0, 1, 4, 5, 6, 7, 9, 10, 13, 16]
    v, st = sup.loop_torontonian_each(O, gammas, lists, gamma_of=gamma_of, return_stats=True)
    assert np.array_equal(dbits(v), dbits(want))
    assert np.isfinite(v).all() and (v != 0).all()
    for k, l in enumerate(lists):  # and the bits are the single-order kernel's
        if len(l) in (1, 4, 5, 9, 13):
            assert dbits(v[k]).tolist() == dbits(sup.loop_torontonian_batch(O, gammas[gamma_of[k]], l)).tolist(), k
        if len(l) == 0:
            assert dbits(v[k]).tolist() == dbits(1.0).tolist()
    assert st["devices_used"] == 1 and st["leaves"] == len(ORDERS)
    assert st["visited_steps"] == st["gray_steps"] == sum(1 << n for n in ORDERS if n)
    assert st["kernel_ms"] > 0 and st["wall_ms"] >= st["kernel_ms"] and st["grid"] >= 1
    assert st["est_ops_per_step"] > 0
    # gamma_of = None: item k reads row k
    own = sup.loop_torontonian_each(O, gammas, lists[2:7])
    assert np.array_equal(dbits(own), dbits(sup.loop_torontonian_each(O, gammas, lists[2:7], cpu=True)))


@pytest.mark.parametrize("group", ["1", "4", "64"])
def test_gpu_each_entry_in_queue_groups(sup, monkeypatch, group):
    """Tickets of `group` slots: wave-chunks of different order share a ticket."""
    O, gammas, lists, gamma_of, want = each_case(sup)
    monkeypatch.setenv("SUP_WALK_GROUP", group)  # read at every call
    assert np.array_equal(dbits(sup.loop_torontonian_each(O, gammas, lists, gamma_of=gamma_of)), dbits(want))


@pytest.mark.parametrize("slab", ["1", "3"])
def test_gpu_each_entry_slab_boundaries(sup, monkeypatch, slab):
    """Slabs of 1 and 3 items: every slab sends up its own rows of gamma."""
    O, gammas, lists, gamma_of, want = each_case(sup)
    monkeypatch.setenv("SUP_LTOR_EACH_SLAB", slab)  # read at every call
    assert np.array_equal(dbits(sup.loop_torontonian_each(O, gammas, lists, gamma_of=gamma_of)), dbits(want))


def test_gpu_each_entry_logical_devices_take_contiguous_ranges(sup, monkeypatch):
    O, gammas, lists, gamma_of, want = each_case(sup)
    monkeypatch.setenv("SUP_DEVICE_MAP", "0,0,0")
    assert sup.device_count() == 3
    for G in (2, 3):
        v, st = sup.loop_torontonian_each(O, gammas, lists, gamma_of=gamma_of, gpu_num=G, return_stats=True)
        assert np.array_equal(dbits(v), dbits(want)) and st["devices_used"] == G
    monkeypatch.delenv("SUP_DEVICE_MAP")


def test_gpu_order_25_has_the_single_order_kernels_bits(sup):
    """n = 25 is the smallest order with a chunk of 2^(n - 15) subsets; the
    single-order kernel on the device is the reference (a twin run takes
    seconds)."""
    rng = np.random.default_rng(2825)
    M = 25
    O = hermitian(rng, M, 0.3)
    gamma = 0.15 * (rng.standard_normal(2 * M) + 1j * rng.standard_normal(2 * M))
    l = rng.permutation(M)
    v, st = sup.loop_torontonian_each(O, gamma, [l, l[:3]], gamma_of=[0, 0], return_stats=True)
    want = sup.loop_torontonian_batch(O, gamma, l)
    assert np.isfinite(want) and want != 0
    assert dbits(v[0]).tolist() == dbits(want).tolist()
    assert dbits(v[1]).tolist() == dbits(sup.loop_torontonian_batch(O, gamma, l[:3])).tolist()
    assert st["visited_steps"] == (1 << 25) + 8


def test_gpu_non_positive_pivot_is_nan_in_that_item_only(sup):
    O, gammas, lists, gamma_of, want = each_case(sup)
    bad = O.copy()
    bad[7, 7] = 1.5  # 1 - O[7][7] < 0: every list with mode 7 meets a pivot that is not positive
    v = sup.loop_torontonian_each(bad, gammas, lists, gamma_of=gamma_of)
    has = np.array([7 in l.tolist() for l in lists])
    assert has.any() and (~has).any()
    assert np.isnan(v[has]).all()
    assert np.array_equal(dbits(v[~has]), dbits(want[~has]))  # the others keep their bits


def test_gpu_sampler_draws_the_host_twins_samples(sup):
    """256 samples, M = 6; and M = 1."""
    mu, cov = gaussian_state([0.5, -0.45, 0.4, 0.55, -0.35, 0.6], random_unitary(6, 28),
                             [0.3 + 0.2j, -0.25 + 0.3j, 0.2 - 0.35j, -0.3 - 0.1j, 0.15 + 0.25j, -0.2 + 0.1j])
    dev, wd, st = sup.threshold_sample(mu, cov, 256, 77, return_weights=True, return_stats=True)
    cpu, wc = sup.threshold_sample(mu, cov, 256, 77, return_weights=True, cpu=True)
    assert np.array_equal(dev, cpu) and np.array_equal(dbits(wd), dbits(wc))
    assert set(np.unique(dev)) == {0, 1} and len({tuple(r) for r in dev.tolist()}) > 20
    assert st["devices_used"] == 1 and st["kernel_ms"] > 0 and st["visited_steps"] > 0 and st["failed"] == 0
    assert st["each_ms"] > 0 and st["host_ms"] > 0
    mu1, cov1 = gaussian_state([0.5], None, [0.4 + 0.3j])
    one, w1 = sup.threshold_sample(mu1, cov1, 256, 78, return_weights=True)
    c1, wc1 = sup.threshold_sample(mu1, cov1, 256, 78, return_weights=True, cpu=True)
    assert np.array_equal(one, c1) and np.array_equal(dbits(w1), dbits(wc1)) and set(np.unique(one)) == {0, 1}
