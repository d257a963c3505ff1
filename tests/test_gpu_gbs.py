"""The ragged loop-hafnian batch and the PNR sampler on the GPU (walk_lhafe.hip
through sup_loop_hafnian_complex_each and sup_gbs_sample): bit for bit the host
twin, with orders of both parities next to each other in one queue, across
queue groups, slab boundaries and logical devices; and the sampler's samples
identical to the host twin's.  Bits are compared as uint64 pairs."""
import numpy as np
import pytest

from test_complex_batch import bits
from test_gbs import gaussian_state, random_unitary
from test_hafnian import walk_shape

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def need_gpu(sup):
    if sup.device_count() < 1:
        pytest.fail("no HIP device visible: -m gpu tests must run on the MI355X box")


def ones(n):
    return (1,) * n


# (multiplicities, (T, Tw, H)) in the order of the call: odd and even orders sit
# next to each other, one-chunk items between many-chunk ones, order 0 among them
ITEMS = [
    (ones(17), (1 << 16, 1024, 64)),           # odd: the final multiply by r
    ((4, 4, 4, 4), (500, 4, 125)),             # 16: Tw = 4, 61 valid lanes in the second chunk
    ((1,), (1, 1, 1)),                         # 1: r alone
    ((1, 1), (2, 1, 2)),                       # 2: two valid lanes
    ((), None),                                # 0: exactly 1, nothing walked
    (ones(18), (1 << 17, 1024, 128)),          # 18: ten walk digits
    ((5, 4, 4, 4), (600, 6, 100)),             # 17 with repeats: 36 valid lanes in the second chunk
    (ones(22), (1 << 21, 1024, 2048)),         # 22: 11 high digits, the chunk-start quadratic form
    ((6,), (6, 1, 6)),                         # 6: one odd-radix digit
    ((16, 16, 16, 16), (78608, 272, 289)),     # 64: four groups of sixteen, m = 32
    ((1,), (1, 1, 1)),
    ((6, 6, 4), (196, 1, 196)),                # 16: Tw = 1, 4 chunks
    ((2,), (2, 1, 2)),                         # 2: one value twice
    ((), None),
    ((4, 4, 4, 4, 2), (1250, 5, 250)),         # 18: Tw = 5
    ((2,) * 9, (13122, 162, 81)),              # 18: Tw = 162
    ((3, 3), (12, 1, 12)),                     # 6
    (ones(17), (1 << 16, 1024, 64)),
]
_REF = {}


def each_case(sup):
    """(A, mus, lists, mu_of, the host twin's result), computed once."""
    if "each" not in _REF:
        rng = np.random.default_rng(2626)
        M = 24
        A = rng.standard_normal((M, M)) + 1j * rng.standard_normal((M, M))
        A = (A + A.T) / 4.0
        mus = (rng.standard_normal((5, M)) + 1j * rng.standard_normal((5, M))) / 2.0
        lists = [np.repeat(rng.choice(M, len(s), replace=False), s).astype(np.int64) for s, _ in ITEMS]
        mu_of = [(3 * k) % 5 for k in range(len(ITEMS))]
        want = sup.loop_hafnian_each(A, mus, lists, mu_of=mu_of, cpu=True, threads=16)
        _REF["each"] = (A, mus, lists, mu_of, want)
    return _REF["each"]


def test_gpu_each_entry_bit_equal_to_host_twin(sup):
    A, mus, lists, mu_of, want = each_case(sup)
    for l, (s, shape) in zip(lists, ITEMS):
        if shape is not None:
            assert walk_shape(l)[:3] == shape, s  # the shapes are what the comments say
    assert sorted({len(l) for l in lists}) == [0, 1, 2, 6, 16, 17, 18, 22, 64]
    v, st = sup.loop_hafnian_each(A, mus, lists, mu_of=mu_of, return_stats=True)
    assert np.array_equal(bits(v), bits(want))
    assert np.isfinite(v).all() and (v != 0).all()
    for k, l in enumerate(lists):  # and the twin's bits are the single-order entry's
        if len(l) in (1, 2, 6, 16, 17):
            assert bits(v[k]).tolist() == bits(sup.hafnian_batch(A, l, mu=mus[mu_of[k]], loop=True)).tolist(), k
        if len(l) == 0:
            assert bits(v[k]).tolist() == bits(1.0 + 0.0j).tolist()
    assert st["devices_used"] == 1 and st["leaves"] == len(ITEMS)
    assert st["visited_steps"] == sum(shape[0] for _, shape in ITEMS if shape)
    assert st["kernel_ms"] > 0 and st["wall_ms"] >= st["kernel_ms"] and st["grid"] >= 1
    assert st["est_ops_per_step"] > 0


@pytest.mark.parametrize("group", ["4", "64"])
def test_gpu_each_entry_in_queue_groups(sup, monkeypatch, group):
    """Tickets of `group` chunks: wave-chunks of different order share a ticket."""
    A, mus, lists, mu_of, want = each_case(sup)
    monkeypatch.setenv("SUP_WALK_GROUP", group)  # read at every call
    assert np.array_equal(bits(sup.loop_hafnian_each(A, mus, lists, mu_of=mu_of)), bits(want))


@pytest.mark.parametrize("slab", ["1", "3"])
def test_gpu_each_entry_slab_boundaries(sup, monkeypatch, slab):
    """Slabs of 1 and 3 items: every slab sends up its own rows of mu."""
    A, mus, lists, mu_of, want = each_case(sup)
    monkeypatch.setenv("SUP_HAFNIAN_SLAB", slab)  # read at every call
    assert np.array_equal(bits(sup.loop_hafnian_each(A, mus, lists, mu_of=mu_of)), bits(want))
    assert np.array_equal(bits(sup.loop_hafnian_each(A, mus, lists, mu_of=mu_of, cpu=True)), bits(want))


def test_gpu_each_entry_logical_devices_take_contiguous_ranges(sup, monkeypatch):
    A, mus, lists, mu_of, want = each_case(sup)
    monkeypatch.setenv("SUP_DEVICE_MAP", "0,0,0")
    assert sup.device_count() == 3
    for G in (2, 3):
        v, st = sup.loop_hafnian_each(A, mus, lists, mu_of=mu_of, gpu_num=G, return_stats=True)
        assert np.array_equal(bits(v), bits(want)) and st["devices_used"] == G
    monkeypatch.delenv("SUP_DEVICE_MAP")


def test_gpu_sampler_draws_the_host_twins_samples(sup):
    """256 samples, M = 4, cutoff 5; and M = 1."""
    mu, cov = gaussian_state([0.4, -0.3, 0.35, 0.25], random_unitary(4, 27),
                             [0.3 + 0.1j, -0.2 + 0.25j, 0.1 - 0.3j, 0.25 + 0.2j])
    dev, st = sup.gbs_sample(mu, cov, 256, 77, cutoff=5, return_stats=True)
    cpu = sup.gbs_sample(mu, cov, 256, 77, cutoff=5, cpu=True)
    assert np.array_equal(dev, cpu)
    assert dev.min() >= 0 and dev.max() >= 2 and len({tuple(r) for r in dev.tolist()}) > 20
    assert st["devices_used"] == 1 and st["kernel_ms"] > 0 and st["visited_steps"] > 0 and st["failed"] == 0
    assert st["each_ms"] > 0 and st["host_ms"] > 0
    mu1, cov1 = gaussian_state([0.5], None, [0.4 + 0.3j])
    one = sup.gbs_sample(mu1, cov1, 256, 78, cutoff=6)
    assert np.array_equal(one, sup.gbs_sample(mu1, cov1, 256, 78, cutoff=6, cpu=True)) and one.max() >= 2
