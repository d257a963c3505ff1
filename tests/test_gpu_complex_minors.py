"""The one-walk permanent minors on the GPU (walk_cplxm.hip, cplx_minors.hip
through sup_perman_complex_minors / _minors_range): result (k, j) has the bits
of the host twin for any slab size, queue group and device count.  Bits are
compared as uint64 pairs."""
import numpy as np
import pytest

from test_complex import as_complex, exact_perm, gauss_int_case
from test_complex_batch import bits
from test_complex_minors import batch_B, minors_of, via_lists

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def need_gpu(sup):
    if sup.device_count() < 1:
        pytest.fail("no HIP device visible: -m gpu tests must run on the MI355X box")


_REF = {}


def case(sup, n, count):
    """(matrices, host twin's result), computed once per shape."""
    if (n, count) not in _REF:
        Bs = batch_B(n, count, 8000 + 100 * n + count)
        _REF[(n, count)] = (Bs, via_lists(sup, Bs, cpu=True, threads=16))
    return _REF[(n, count)]


# n <= 7: invalid lanes; 8: L = 6 and no walk bits; 9: m = 1, only the odd tail
# step; 14: one chunk per matrix; 15: two chunks, the first fold; 17: the first
# N with two SGPR pieces per plane; 21: fold depth 7; 22: the first N on one
# wave per SIMD.
@pytest.mark.parametrize("n", range(2, 25))
def test_gpu_minors_bit_equal_to_host_twin(sup, n):
    Bs, want = case(sup, n, 3)
    got, st = via_lists(sup, Bs, return_stats=True)
    assert got.shape == (3, n) and st["devices_used"] == 1
    assert np.array_equal(bits(got), bits(want))


@pytest.mark.parametrize("n", range(25, 33))
def test_gpu_minors_range_register_heaviest_instances(sup, n):
    """walk_log2 = 10: the first 64 and the last 64 wave-chunks of the plan."""
    B = batch_B(n, 1, 8800 + n)[0]
    chunks = 1 << (n - 2 - 6 - 10)
    for c0, c1 in ((0, 64), (chunks - 64, chunks)):
        got, st = sup.perman_complex_minors_range(B, c0, c1, walk_log2=10, return_stats=True)
        want = sup.perman_complex_minors_range(B, c0, c1, walk_log2=10, cpu=True, threads=16)
        assert st["walk_bits"] == 10 and st["gray_steps"] == 64 << 16 and st["devices_used"] == 1
        assert np.array_equal(bits(got), bits(want)), (c0, c1)


@pytest.mark.parametrize("n", [6, 14])
def test_gpu_minors_count_65(sup, n):
    """Matrix boundaries inside and across queue groups, a count that is no
    multiple of the group."""
    Bs, want = case(sup, n, 65)
    assert np.array_equal(bits(via_lists(sup, Bs)), bits(want))


@pytest.mark.parametrize("group", ["4", "64"])
@pytest.mark.parametrize("n,count", [(6, 65), (15, 3), (21, 3)])
def test_gpu_minors_forced_queue_group(sup, monkeypatch, n, count, group):
    Bs, want = case(sup, n, count)
    monkeypatch.setenv("SUP_WALK_GROUP", group)  # read at every call
    assert np.array_equal(bits(via_lists(sup, Bs)), bits(want))


@pytest.mark.parametrize("slab", ["1", "3"])
@pytest.mark.parametrize("n", [14, 21])
def test_gpu_minors_slabs(sup, monkeypatch, n, slab):
    """Slabs of 1 and 3 on count 7: the index lists of a later slab."""
    Bs, want = case(sup, n, 7)
    monkeypatch.setenv("SUP_CPLX_MINORS_SLAB", slab)  # read at every call
    assert np.array_equal(bits(via_lists(sup, Bs)), bits(want))


def test_gpu_minors_repeated_indices(sup):
    rng = np.random.default_rng(12)
    U = rng.standard_normal((16, 16)) + 1j * rng.standard_normal((16, 16))
    n, count = 12, 33
    rows = rng.integers(0, 16, (count, n))
    cols = rng.integers(0, 16, (count, n - 1))
    rows[:, -1] = rows[:, 0]
    cols[:, 1] = cols[:, 0]
    got = sup.perman_complex_minors_submatrices(U, rows, cols)
    assert np.array_equal(bits(got), bits(sup.perman_complex_minors_submatrices(U, rows, cols, cpu=True)))


@pytest.mark.parametrize("n,count", [(14, 65), (21, 7), (5, 1)])
def test_gpu_minors_multi_device(sup, n, count):
    Bs, want = case(sup, n, count)
    nd = sup.device_count()
    got, st = via_lists(sup, Bs, gpu_num=nd, return_stats=True)
    assert np.array_equal(bits(got), bits(want))
    assert st["devices_used"] == min(nd, count)


def test_gpu_minors_exact_gaussian_integers(sup):
    B = gauss_int_case(8, 5)[:, :7]
    want = [as_complex(exact_perm(a)) for a in minors_of(B)]
    assert np.array_equal(sup.perman_complex_minors(B), want)


def test_gpu_minors_nan_stays_in_its_own_matrix(sup):
    Bs, clean = case(sup, 14, 65)
    dirty = Bs.copy()
    dirty[31, 5, 12] = complex(1.0, np.nan)
    dirty[64, 0, 3] = complex(np.inf, 0.0)
    got = via_lists(sup, dirty)
    keep = [k for k in range(65) if k not in (31, 64)]
    assert np.array_equal(bits(got[keep]), bits(clean[keep]))
    assert not np.isfinite(np.delete(got[31], 5)).any() and not np.isfinite(np.delete(got[64], 0)).any()
    # the minor without the poisoned row never reads it
    assert np.array_equal(bits(got[31, 5]), bits(clean[31, 5]))


@pytest.mark.parametrize("n,count", [(6, 65), (14, 65), (21, 7)])
def test_gpu_minors_stats(sup, n, count):
    Bs, _ = case(sup, n, count)
    _, st = via_lists(sup, Bs, return_stats=True)
    L, m, _ = sup.layout(n - 1)
    assert st["leaves"] == count * n and st["gray_steps"] == count << (n - 2)
    assert st["kernel_ms"] > 0 and st["wall_ms"] >= st["kernel_ms"] and st["grid"] >= 1
    assert st["lane_bits"] == L and st["walk_bits"] == m and st["est_ops_per_step"] == 16 * n - 24


def test_gpu_minors_walk_bits(sup):
    Bs = batch_B(17, 6, 170)
    got, st = via_lists(sup, Bs, walk_log2=2, return_stats=True)
    assert st["walk_bits"] == 2
    assert np.array_equal(bits(got), bits(via_lists(sup, Bs, cpu=True, threads=16, walk_log2=2)))


def test_gpu_minors_33_rows_run_the_single_matrix_walk(sup):
    B = batch_B(33, 1, 33)[0]
    got, st = sup.perman_complex_minors(B, return_stats=True)
    one = np.array([sup.perman_complex(a) for a in minors_of(B)], dtype=np.complex128)
    assert np.array_equal(bits(got), bits(one))
    assert st["leaves"] == 33 and st["gray_steps"] == 33 << 31 and st["kernel_ms"] > 0
