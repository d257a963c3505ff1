"""The hafnian walk on the GPU (walk_haf.hip through sup_hafnian_complex and
sup_loop_hafnian_complex): bit for bit the host twin, at the smallest shapes
where the kernel can go wrong, and the twin's anchors (exact Gaussian integers,
the rank-one closed form).  Bits are compared as uint64 pairs."""
import numpy as np
import pytest

from test_complex_batch import bits
from test_hafnian import (err, exact_entries, hetero_lists, kan_haf, rank_one_bound, rank_one_haf_case,
                          rank_one_scale, sym_gauss_int, walk_shape)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def need_gpu(sup):
    if sup.device_count() < 1:
        pytest.fail("no HIP device visible: -m gpu tests must run on the MI355X box")


def ones(n):
    return (1,) * n


# name -> (n, [multiplicities], [(T, Tw, H)] the shapes are chosen for, the forms run)
SHAPES = {
    # H = 2: two valid lanes; idx (0, 1) and (0, 0)
    "n2": (2, [(1, 1), (2,)], [(2, 1, 2), (2, 1, 2)], (False, True)),
    # one odd-radix digit
    "n6_one_group": (6, [(6,)], [(6, 1, 6)], (False, True)),
    # Tw = 1: 4 chunks with 4 valid lanes in the last; Tw = 4 with 61 valid lanes in the second chunk
    "n16_no_walk": (16, [(6, 6, 4), (4, 4, 4, 4)], [(196, 1, 196), (500, 4, 125)], (False, True)),
    # odd Tw = 5; Tw = 162 (H = 81); Tw = 2^10 (ten walk digits, H = 128)
    "n18_walks": (18, [(4, 4, 4, 4, 2), (2,) * 9, ones(18)],
                  [(1250, 5, 250), (13122, 162, 81), (1 << 17, 1024, 128)], (False, True)),
    # 11 high digits: the chunk-start quadratic form
    "n22_distinct": (22, [ones(22)], [(1 << 21, 1024, 2048)], (False, True)),
    # odd n: the loop form only
    "n17_loop_odd": (17, [ones(17)], [(1 << 16, 1024, 64)], (True,)),
}
_REF = {}


def shape_case(name):
    n, patterns, _, _ = SHAPES[name]
    rng = np.random.default_rng(7000 + n)
    M = 24
    A = rng.standard_normal((M, M)) + 1j * rng.standard_normal((M, M))
    A = A + A.T
    mu = rng.standard_normal(M) + 1j * rng.standard_normal(M)
    idx = np.stack([np.repeat(rng.choice(M, len(s), replace=False), s) for s in patterns])
    return A, mu, idx


def case(sup, name, loop):
    """(A, mu, idx, GPU result on one device, its stats), computed once per shape and form."""
    if (name, loop) not in _REF:
        A, mu, idx = shape_case(name)
        v, st = sup.hafnian_batch(A, idx, mu=mu, loop=loop, return_stats=True)
        _REF[(name, loop)] = (A, mu, idx, v, st)
    return _REF[(name, loop)]


@pytest.mark.parametrize("name,loop", [(name, loop) for name in SHAPES for loop in SHAPES[name][3]])
def test_gpu_bit_equal_to_host_twin(sup, name, loop):
    A, mu, idx, v, st = case(sup, name, loop)
    n, _, want, _ = SHAPES[name]
    assert [walk_shape(idx[k])[:3] for k in range(len(want))] == want  # the shapes are what the comment says
    assert sup.hafnian_plan(idx).tolist() == [w[0] for w in want]
    assert np.array_equal(bits(v), bits(sup.hafnian_batch(A, idx, mu=mu, loop=loop, cpu=True, threads=16)))
    one = np.array([sup.hafnian_batch(A, idx[k], mu=mu, loop=loop) for k in range(len(want))])
    assert np.array_equal(bits(v), bits(one))
    assert np.isfinite(v).all() and (v != 0).all()
    assert st["devices_used"] == 1 and st["leaves"] == len(want)
    assert st["visited_steps"] == sum(w[0] for w in want) and st["gray_steps"] == len(want) << (n - 1)
    assert st["kernel_ms"] > 0 and st["wall_ms"] >= st["kernel_ms"] and st["grid"] >= 1
    assert st["est_ops_per_step"] > 0


@pytest.mark.parametrize("loop", [False, True])
def test_gpu_n64_m32_longest_power_and_rank_one_closed_form(sup, loop):
    """(16, 16, 16, 16): Tw = 272, H = 289 (5 chunks, 33 valid lanes in the
    last), m = 32.  The bound is test_hafnian.test_rank_one_closed_form's."""
    n, mult = 64, (16, 16, 16, 16)
    A, mu, u, idx, truth = rank_one_haf_case(n, mult, loop, 600 + n)
    assert walk_shape(idx)[:3] == (78608, 272, 289)
    v, st = sup.hafnian_batch(A, idx, mu=mu, loop=loop, return_stats=True)
    c = sup.hafnian_batch(A, idx, mu=mu, loop=loop, cpu=True, threads=16)
    assert bits(v).tolist() == bits(c).tolist() and st["visited_steps"] == 78608
    bound = rank_one_bound(n, 272, 4, loop)
    e = err(v, truth) / rank_one_scale(n, idx, u, mu, loop)
    print(f"n64 loop={loop} e/S={e:.3e} bound={bound:.3e}")
    assert e <= bound


def hetero_case(n, count, seed):
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((12, 12)) + 1j * rng.standard_normal((12, 12))
    A = A + A.T
    mu = rng.standard_normal(12) + 1j * rng.standard_normal(12)
    return A, mu, hetero_lists(n, count, seed)


@pytest.mark.parametrize("group", ["4", "64"])
@pytest.mark.parametrize("loop", [False, True])
def test_gpu_heterogeneous_batch_in_queue_groups(sup, monkeypatch, group, loop):
    """Tickets of `group` chunks: one-chunk and many-chunk matrices share queue
    groups and the last group is partial."""
    A, mu, idx = hetero_case(14, 65, 414)
    want = sup.hafnian_batch(A, idx, mu=mu, loop=loop, cpu=True, threads=16)
    monkeypatch.setenv("SUP_WALK_GROUP", group)  # read at every call
    assert np.array_equal(bits(sup.hafnian_batch(A, idx, mu=mu, loop=loop)), bits(want))


@pytest.mark.parametrize("slab", ["1", "3"])
def test_gpu_slab_boundaries(sup, monkeypatch, slab):
    A, mu, idx = hetero_case(12, 7, 812)
    for loop in (False, True):
        whole = sup.hafnian_batch(A, idx, mu=mu, loop=loop)
        monkeypatch.setenv("SUP_HAFNIAN_SLAB", slab)  # read at every call
        assert np.array_equal(bits(sup.hafnian_batch(A, idx, mu=mu, loop=loop)), bits(whole))
        monkeypatch.delenv("SUP_HAFNIAN_SLAB")
        assert np.array_equal(bits(whole), bits(sup.hafnian_batch(A, idx, mu=mu, loop=loop, cpu=True, threads=16)))


def test_gpu_logical_devices_take_contiguous_ranges(sup, monkeypatch):
    A, mu, idx = hetero_case(10, 9, 910)
    for loop in (False, True):
        one, s1 = sup.hafnian_batch(A, idx, mu=mu, loop=loop, return_stats=True)
        assert s1["devices_used"] == 1
        monkeypatch.setenv("SUP_DEVICE_MAP", "0,0,0")
        assert sup.device_count() == 3
        for G in (2, 3):
            v, st = sup.hafnian_batch(A, idx, mu=mu, loop=loop, gpu_num=G, return_stats=True)
            assert np.array_equal(bits(v), bits(one)) and st["devices_used"] == G
        monkeypatch.delenv("SUP_DEVICE_MAP")


def test_gpu_gaussian_integers_round_to_the_exact_integer(sup):
    A = sym_gauss_int(16, 316)
    truth = kan_haf(exact_entries(A), range(16))
    v = sup.hafnian(A)
    assert err(v, truth) < 0.5
    assert bits(v).tolist() == bits(sup.hafnian(A, cpu=True)).tolist()
