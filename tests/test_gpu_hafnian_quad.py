"""The double-double hafnian walk on the GPU (walk_hafdd.hip through
sup_hafnian_complex_quad and sup_loop_hafnian_complex_quad): all four doubles of
every result bit for bit the host twin's, at the smallest shapes where the
kernel can go wrong (test_gpu_hafnian.py's, asserted), the two lists whose
weights pass 2^53, and the twin's anchor (exact Gaussian integers).  Nothing
above 2^21 states per matrix."""
from fractions import Fraction

import numpy as np
import pytest

from test_gpu_hafnian import SHAPES, hetero_case, shape_case
from test_hafnian import rank_one_haf_case, sym_dyadic, sym_gauss_int, walk_shape

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def need_gpu(sup):
    if sup.device_count() < 1:
        pytest.fail("no HIP device visible: -m gpu tests must run on the MI355X box")


def qbits(v):
    return np.ascontiguousarray(np.asarray(v, dtype=np.float64)).view(np.uint64)


_REF = {}


def case(sup, name, loop):
    """(A, mu, idx, GPU result on one device, its stats), computed once per shape and form."""
    if (name, loop) not in _REF:
        A, mu, idx = shape_case(name)
        v, st = sup.hafnian_quad_batch(A, idx, mu=mu, loop=loop, return_stats=True)
        _REF[(name, loop)] = (A, mu, idx, v, st)
    return _REF[(name, loop)]


@pytest.mark.parametrize("name,loop", [(name, loop) for name in SHAPES for loop in SHAPES[name][3]])
def test_gpu_bit_equal_to_host_twin(sup, name, loop):
    """n = 2 and 6 (W = 0, partly filled wave), 16 and 18 (W <= 4 with repeats
    and the W > 4 branch), 17 (loop, odd), 22 (11 high digits)."""
    A, mu, idx, v, st = case(sup, name, loop)
    n, _, want, _ = SHAPES[name]
    assert [walk_shape(idx[k])[:3] for k in range(len(want))] == want  # the shapes are what the comment says
    assert v.shape == (len(want), 4)
    assert np.array_equal(qbits(v), qbits(sup.hafnian_quad_batch(A, idx, mu=mu, loop=loop, cpu=True, threads=16)))
    one = np.array([np.ravel(sup.hafnian_quad_batch(A, idx[k], mu=mu, loop=loop)) for k in range(len(want))])
    assert np.array_equal(qbits(v), qbits(one))
    assert np.isfinite(v).all() and (v[:, 0] != 0).all() and (v[:, 2] != 0).all()
    assert (v[:, 0] + v[:, 1] == v[:, 0]).all() and (v[:, 2] + v[:, 3] == v[:, 2]).all()  # normalised pairs
    # the hi words are the fp64 walk's value to its own accuracy
    f = sup.hafnian_batch(A, idx, mu=mu, loop=loop, cpu=True)
    assert np.allclose(v[:, 0] + 1j * v[:, 2], f, rtol=1e-6, atol=0)
    assert st["devices_used"] == 1 and st["leaves"] == len(want)
    assert st["visited_steps"] == sum(w[0] for w in want) and st["gray_steps"] == len(want) << (n - 1)
    assert st["kernel_ms"] > 0 and st["wall_ms"] >= st["kernel_ms"] and st["grid"] >= 1
    _, cst = sup.hafnian_quad_batch(A, idx, mu=mu, loop=loop, cpu=True, return_stats=True)
    assert st["est_ops_per_step"] == cst["est_ops_per_step"] > 100


@pytest.mark.parametrize("loop", [False, True])
def test_gpu_n12_with_repeats(sup, loop):
    """(3, 3, 3, 3) and (2) x 6 at n = 12: W <= 4 and W > 4 with odd radices."""
    A = sym_dyadic(6, 52)
    mu = np.diag(sym_dyadic(6, 53))
    idx = np.stack([np.repeat(np.arange(4), 3), np.repeat(np.arange(6), 2)])
    assert [walk_shape(i)[:3] for i in idx] == [(192, 3, 64), (486, 6, 81)]
    v = sup.hafnian_quad_batch(A, idx, mu=mu, loop=loop)
    assert np.array_equal(qbits(v), qbits(sup.hafnian_quad_batch(A, idx, mu=mu, loop=loop, cpu=True)))


@pytest.mark.parametrize("loop", [False, True])
def test_gpu_n64_m32_longest_power(sup, loop):
    """(16, 16, 16, 16): Tw = 272, H = 289 (5 chunks, 33 valid lanes in the last), m = 32."""
    A, mu, u, idx, truth = rank_one_haf_case(64, (16, 16, 16, 16), loop, 664)
    assert walk_shape(idx)[:3] == (78608, 272, 289)
    v, st = sup.hafnian_quad_batch(A, idx, mu=mu, loop=loop, return_stats=True)
    c = sup.hafnian_quad_batch(A, idx, mu=mu, loop=loop, cpu=True, threads=16)
    assert qbits(np.ravel(v)).tolist() == qbits(np.ravel(c)).tolist() and st["visited_steps"] == 78608


@pytest.mark.parametrize("idx,shape,loop", [([0] * 57 + list(range(1, 8)), (3712, 58, 64), False),
                                            ([0] * 62 + [1, 1], (126, 1, 126), False),
                                            ([0] * 57 + list(range(1, 8)), (3712, 58, 64), True),
                                            ([0] * 57 + list(range(1, 7)), (1856, 1, 1856), True),
                                            ([0] * 61 + [1, 1], (124, 1, 124), True)])
def test_gpu_weights_beyond_2_53(sup, idx, shape, loop):
    """C(57, 28) in the step program (n = 64, both forms), C(62, 31), C(61, 30) and
    at n = 63 C(57, 28) in the high-digit table: no list of order 63 walks a digit
    of radix 58 (H >= 64 would need seven more indices)."""
    assert walk_shape(idx)[:3] == shape
    A = sym_dyadic(8, 58)
    v = sup.hafnian_quad_batch(A, idx, loop=loop)
    assert qbits(np.ravel(v)).tolist() == qbits(np.ravel(sup.hafnian_quad_batch(A, idx, loop=loop, cpu=True))).tolist()
    assert v[0][0] != 0 and v[1][0] != 0


@pytest.mark.parametrize("group", ["4", "64"])
@pytest.mark.parametrize("loop", [False, True])
def test_gpu_heterogeneous_batch_in_queue_groups(sup, monkeypatch, group, loop):
    A, mu, idx = hetero_case(14, 65, 414)
    want = sup.hafnian_quad_batch(A, idx, mu=mu, loop=loop, cpu=True, threads=16)
    monkeypatch.setenv("SUP_WALK_GROUP", group)  # read at every call
    assert np.array_equal(qbits(sup.hafnian_quad_batch(A, idx, mu=mu, loop=loop)), qbits(want))


@pytest.mark.parametrize("slab", ["1", "3"])
def test_gpu_slab_boundaries(sup, monkeypatch, slab):
    A, mu, idx = hetero_case(12, 7, 812)
    for loop in (False, True):
        whole = sup.hafnian_quad_batch(A, idx, mu=mu, loop=loop)
        monkeypatch.setenv("SUP_HAFNIAN_SLAB", slab)  # read at every call
        assert np.array_equal(qbits(sup.hafnian_quad_batch(A, idx, mu=mu, loop=loop)), qbits(whole))
        monkeypatch.delenv("SUP_HAFNIAN_SLAB")
        assert np.array_equal(qbits(whole), qbits(sup.hafnian_quad_batch(A, idx, mu=mu, loop=loop, cpu=True, threads=16)))


def test_gpu_logical_devices_take_contiguous_ranges(sup, monkeypatch):
    A, mu, idx = hetero_case(10, 9, 910)
    for loop in (False, True):
        one, s1 = sup.hafnian_quad_batch(A, idx, mu=mu, loop=loop, return_stats=True)
        assert s1["devices_used"] == 1
        monkeypatch.setenv("SUP_DEVICE_MAP", "0,0,0")
        assert sup.device_count() == 3
        for G in (2, 3):
            v, st = sup.hafnian_quad_batch(A, idx, mu=mu, loop=loop, gpu_num=G, return_stats=True)
            assert np.array_equal(qbits(v), qbits(one)) and st["devices_used"] == G
        monkeypatch.delenv("SUP_DEVICE_MAP")


def test_gpu_gaussian_integers_round_to_the_exact_integer(sup):
    A = sym_gauss_int(16, 316)
    for loop in (False, True):
        (rh, rl), (ih, il) = sup.hafnian_quad_batch(A, np.arange(16), loop=loop)
        want = (sup.loop_hafnian_exact if loop else sup.hafnian_exact)(A, cpu=True)
        assert (round(Fraction(rh) + Fraction(rl)), round(Fraction(ih) + Fraction(il))) == tuple(want)
