"""The batched complex walk on the GPU (walk_cplxb.hip, cplx_batch.hip through
sup_perman_complex_batch / sup_perman_complex_submatrices): result k has the
bits of the host twin and of perman_complex on matrix k alone, for any slab
size and device count.  Bits are compared as uint64 pairs."""
import numpy as np
import pytest

from test_complex import as_complex, exact_perm, gauss_int_case
from test_complex_batch import batch_of, bits, repeated_indices

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def need_gpu(sup):
    if sup.device_count() < 1:
        pytest.fail("no HIP device visible: -m gpu tests must run on the MI355X box")


_REF = {}


def case(sup, n, count):
    """(matrices, GPU batch result on one device, its stats), computed once per shape."""
    if (n, count) not in _REF:
        mats = batch_of(n, count, 7000 + 100 * n + count)
        v, st = sup.perman_complex_batch(mats, return_stats=True)
        _REF[(n, count)] = (mats, v, st)
    return _REF[(n, count)]


# (7, 4): L = 6, no walk bits, T = 1; (8, 3): m = 1, only the odd tail step;
# (13, 65): one chunk per matrix, count no multiple of the queue's group;
# (17, 9): first N with two SGPR pieces per plane; (20, 8): 2^7 chunks per
# matrix, the fold tree has depth; n < 7: invalid lanes.
SHAPES = [(1, 5), (2, 3), (5, 65), (7, 4), (8, 3), (13, 65), (17, 9), (20, 8), (24, 2)]


@pytest.mark.parametrize("n,count", SHAPES)
def test_gpu_batch_bit_equal_to_host_twin_and_gpu_loop(sup, n, count):
    mats, v, st = case(sup, n, count)
    assert v.shape == (count,) and st["devices_used"] == 1
    assert np.array_equal(bits(v), bits(sup.perman_complex_batch(mats, cpu=True, threads=16)))
    one = np.array([sup.perman_complex(a) for a in mats], dtype=np.complex128)
    assert np.array_equal(bits(v), bits(one))


@pytest.mark.parametrize("n,count", [(13, 10), (20, 7)])
def test_gpu_batch_slab_boundary(sup, monkeypatch, n, count):
    mats = batch_of(n, count, 9000 + n)
    whole = sup.perman_complex_batch(mats)
    monkeypatch.setenv("SUP_CPLX_BATCH_SLAB", "3")  # read at every call
    slabbed = sup.perman_complex_batch(mats)
    assert np.array_equal(bits(slabbed), bits(whole))
    assert np.array_equal(bits(whole), bits(sup.perman_complex_batch(mats, cpu=True, threads=16)))


def test_gpu_submatrices_bit_equal_to_host_twin(sup, monkeypatch):
    rng = np.random.default_rng(12)
    U = rng.standard_normal((16, 16)) + 1j * rng.standard_normal((16, 16))
    rows, cols = repeated_indices(rng, 33, 12, 16, 16)
    v = sup.perman_complex_submatrices(U, rows, cols)
    assert np.array_equal(bits(v), bits(sup.perman_complex_submatrices(U, rows, cols, cpu=True, threads=16)))
    gathered = np.stack([U[np.ix_(rows[k], cols[k])] for k in range(33)])
    assert np.array_equal(bits(v), bits(sup.perman_complex_batch(gathered)))
    monkeypatch.setenv("SUP_CPLX_BATCH_SLAB", "5")  # the index lists of a later slab
    assert np.array_equal(bits(v), bits(sup.perman_complex_submatrices(U, rows, cols)))


def test_gpu_submatrices_exact_gaussian_integers(sup):
    rng = np.random.default_rng(48)
    U = gauss_int_case(10, 9)
    rows, cols = repeated_indices(rng, 6, 8, 10, 10)
    got = sup.perman_complex_submatrices(U, rows, cols)
    for k in range(6):
        assert got[k] == as_complex(exact_perm(U[np.ix_(rows[k], cols[k])])), k


@pytest.mark.parametrize("n,count", [(13, 65), (20, 8), (24, 2), (5, 1)])
def test_gpu_batch_multi_device(sup, n, count):
    mats = batch_of(n, count, 7000 + 100 * n + count)
    v = case(sup, n, count)[1] if (n, count) in SHAPES else sup.perman_complex_batch(mats)
    nd = sup.device_count()
    vd, sd = sup.perman_complex_batch(mats, gpu_num=nd, return_stats=True)
    assert np.array_equal(bits(vd), bits(v))
    assert sd["devices_used"] == min(nd, count)


def test_gpu_batch_order_33_runs_the_single_matrix_walk(sup):
    mats = batch_of(33, 2, 33)
    v, st = sup.perman_complex_batch(mats, return_stats=True)
    one = np.array([sup.perman_complex(a) for a in mats], dtype=np.complex128)
    assert np.array_equal(bits(v), bits(one))
    assert st["leaves"] == 2 and st["gray_steps"] == 2 << 32 and st["kernel_ms"] > 0


@pytest.mark.parametrize("n,count", [(5, 65), (13, 65), (20, 8)])
def test_gpu_batch_stats(sup, n, count):
    _, _, st = case(sup, n, count)
    L, m, _ = sup.layout(n)
    assert st["leaves"] == count and st["gray_steps"] == count << (n - 1)
    assert st["kernel_ms"] > 0 and st["wall_ms"] >= st["kernel_ms"] and st["grid"] >= 1
    assert st["lane_bits"] == L and st["walk_bits"] == m and st["est_ops_per_step"] == 6 * n


def test_gpu_batch_walk_bits(sup):
    mats = batch_of(16, 6, 160)
    v, st = sup.perman_complex_batch(mats, walk_log2=2, return_stats=True)
    assert st["walk_bits"] == 2
    assert np.array_equal(bits(v), bits(sup.perman_complex_batch(mats, cpu=True, threads=16, walk_log2=2)))


def test_gpu_batch_nan_stays_in_its_own_result(sup):
    mats, clean, _ = case(sup, 13, 65)
    dirty = mats.copy()
    dirty[31, 5, 12] = complex(1.0, np.nan)
    dirty[64, 0, 3] = complex(np.inf, 0.0)
    got = sup.perman_complex_batch(dirty)
    keep = [k for k in range(65) if k not in (31, 64)]
    assert np.array_equal(bits(got[keep]), bits(clean[keep]))
    assert not np.isfinite(got[31]) and not np.isfinite(got[64])
