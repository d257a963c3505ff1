"""Loop-hafnian tables on the GPU (lhaftab.hip): bit for bit the host twin at
the smallest shapes where the two kernels can go wrong (one entry, modes of one
value, slabs below a wave, with a ragged second wave, with a ragged second
work-group, many work-groups), the hand-over from the low kernel to the slab
launches at every mode and inside a mode's slabs, one table of 2^21 entries,
where a NaN goes, the stats, and the state vector, distribution and sampler on
it.  Bits are compared as uint64."""
import numpy as np
import pytest

from test_gbs import lossy, three_mode_state, two_mode_state
from test_lhaf_table import dense_case

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def need_gpu(sup):
    if sup.device_count() < 1:
        pytest.fail("no HIP device visible: -m gpu tests must run on the MI355X box")


def same_bits(a, b):
    """uint64 equality of the parts; a NaN is a NaN (its payload is not compared)."""
    a = np.ascontiguousarray(a.reshape(-1, order="F")).view(np.float64)
    b = np.ascontiguousarray(b.reshape(-1, order="F")).view(np.float64)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint64), b[~nb].view(np.uint64))


# dims, and a knob value inside a slab of the mode the default tile would take whole
SHAPES = [((1,), 1), ((2,), 1), ((3,), 2), ((1, 1, 1), 1), ((2, 2), 3), ((5, 1, 4), 7), ((1, 6), 4),
          ((4, 4, 4), 40),      # slabs of 16: less than a wave
          ((9, 9, 3), 100),     # slabs of 81: a ragged second wave
          ((17, 17, 2), 300),   # a slab of 289: a ragged second work-group
          ((7,) * 6, 1000)]     # slabs of 16,807


@pytest.mark.parametrize("dims,inside", SHAPES, ids=[str(s[0]) for s in SHAPES])
def test_gpu_bits_are_the_twins(sup, monkeypatch, dims, inside):
    A, mu = dense_case(len(dims), 2750 + len(dims) + dims[0])
    for m in (mu, None):
        want = sup.loop_hafnian_table(A, m, dims, cpu=True)
        for low in (1, inside, None):
            if low is None:
                monkeypatch.delenv("SUP_LHAF_TABLE_LOW", raising=False)
            else:
                monkeypatch.setenv("SUP_LHAF_TABLE_LOW", str(low))
            got, st = sup.loop_hafnian_table(A, m, dims, return_stats=True)
            assert got.shape == tuple(dims) and same_bits(got, want), (dims, m is None, low)
            assert st["launches"] == sup.loop_hafnian_table_plan(dims)[1]


def test_gpu_a_table_of_two_million_entries(sup):
    A, mu = dense_case(7, 2760)
    A, mu = A / 4.0, mu / 4.0  # the entries stay of order one
    dims = (8,) * 7
    got, st = sup.loop_hafnian_table(A, mu, dims, return_stats=True)
    assert same_bits(got, sup.loop_hafnian_table(A, mu, dims, cpu=True))
    e, launches, ops = sup.loop_hafnian_table_plan(dims)
    assert e == 2097152 and launches == 1 + 3 * 7
    assert st["devices_used"] == 1 and st["kernel_ms"] > 0 and st["leaves"] == 1 and st["launches"] == launches
    assert st["gray_steps"] == st["visited_steps"] == e and st["est_ops_per_step"] == ops
    assert st["grid"] == 8 ** 6 // 256


def test_gpu_nan_reaches_exactly_the_entries_that_read_it(sup, monkeypatch):
    A, mu = dense_case(3, 2761)
    mu[1] = complex(np.nan, 0.0)
    dims = (3, 4, 3)
    host = sup.loop_hafnian_table(A, mu, dims, cpu=True)
    # zeta_1 enters at the entries whose highest occupied mode is 1; every entry with
    # n_1 > 0 reads one of them, and an entry with n_1 = 0 reads only such entries
    want = np.zeros(dims, bool)
    want[:, 1:, :] = True
    assert np.array_equal(np.isnan(host.real) | np.isnan(host.imag), want)
    for low in (1, 5, None):
        if low is not None:
            monkeypatch.setenv("SUP_LHAF_TABLE_LOW", str(low))
        else:
            monkeypatch.delenv("SUP_LHAF_TABLE_LOW")
        assert same_bits(sup.loop_hafnian_table(A, mu, dims), host)


def test_gpu_state_vector_distribution_and_sampler(sup):
    mu, cov = three_mode_state()
    psi = sup.gbs_state_vector(mu, cov, (5, 6, 7))
    assert same_bits(psi, sup.gbs_state_vector(mu, cov, (5, 6, 7), cpu=True))
    for m, c in (two_mode_state(), lossy(*two_mode_state(), 0.8)):
        p = sup.pnr_detection_distribution(m, c, (6, 5))
        assert np.array_equal(p.view(np.uint64), sup.pnr_detection_distribution(m, c, (6, 5), cpu=True).view(np.uint64))
        s = sup.pnr_detection_sample(m, c, 20000, 2027, (6, 5))
        assert s.shape == (20000, 2) and np.array_equal(s, sup.pnr_detection_sample(m, c, 20000, 2027, (6, 5), cpu=True))
