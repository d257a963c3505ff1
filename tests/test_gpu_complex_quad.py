"""The complex double-double walk on the GPU, instance by instance
(walk_cplxdd.hip through sup_perman_complex_quad and its range entry): every
walk_cplxdd<N>, N = 1 ... COMPLEX_QUAD_MAX_DEVICE_N, runs on at most eight
wave-chunks and returns the host twin's four doubles bit for bit, and at a
spread of orders the exact rational sum of complex_range_truth.py within the
derived bound (test_complex_quad.py).  Then whole matrices, device counts,
walk lengths, the cap, NaN and the stats."""
import math

import numpy as np
import pytest

import range_truth as T
from test_complex_quad import check_range, random_matrix, range_case

pytestmark = pytest.mark.gpu

CAP = 40
TRUTH_N = set(range(1, 14)) | {17, 24, 31, 32, 33, CAP}


@pytest.fixture(scope="module", autouse=True)
def need_gpu(sup):
    if sup.device_count() < 1:
        pytest.fail("no HIP device visible: -m gpu tests must run on the MI355X box")
    assert sup.COMPLEX_QUAD_MAX_DEVICE_N == CAP


@pytest.mark.parametrize("n", range(1, CAP + 1))
def test_every_order_every_instance(sup, n):
    a, c0, c1, L, m, h = range_case(sup, n)
    assert c1 - c0 <= 8
    v, st = sup.perman_complex_quad_range(a, c0, c1, walk_log2=3, return_stats=True)
    assert st["devices_used"] == 1 and st["kernel_ms"] > 0 and st["grid"] >= 1
    assert st["lane_bits"] == L and st["walk_bits"] == m and st["est_ops_per_step"] == 86 * n - 28
    host = sup.perman_complex_quad_range(a, c0, c1, cpu=True, threads=8, walk_log2=3)
    assert v == host, (n, v, host)
    assert all(math.isfinite(x) for p in v for x in p) and v[0][0] != 0.0
    if n in TRUTH_N:
        check_range(a, v, c0, c1, L, m, h, who="gpu ")


@pytest.mark.parametrize("n", [1, 2])
def test_single_lane_orders_whole(sup, n):
    """N = 1 has one valid lane, N = 2 two: the other lanes add zeros."""
    a = random_matrix(n)
    assert sup.perman_complex_quad(a) == sup.perman_complex_quad(a, cpu=True)
    assert sup.perman_complex_quad([[3 - 2j]]) == ((3.0, 0.0), (-2.0, 0.0))


@pytest.mark.parametrize("n", [7, 8, 14, 18, 22])
def test_whole_matrices(sup, n):
    a = random_matrix(n)
    v, st = sup.perman_complex_quad(a, return_stats=True)
    assert st["devices_used"] == 1 and st["kernel_ms"] > 0 and st["gray_steps"] == 1 << (n - 1)
    assert v == sup.perman_complex_quad(a, cpu=True, threads=16)


def test_all_devices_same_bits(sup):
    n = 18
    a = random_matrix(n)
    ndev = sup.device_count()
    v, st = sup.perman_complex_quad(a, gpu_num=ndev, return_stats=True)
    assert st["devices_used"] == min(ndev, T.chunk_count(sup, n)) and st["kernel_ms"] > 0
    assert v == sup.perman_complex_quad(a) == sup.perman_complex_quad(a, cpu=True, threads=16)
    last = ndev - 1
    assert sup.perman_complex_quad(a, device_id=last) == v


@pytest.mark.parametrize("n,walk_log2", [(12, 1), (26, 1), (16, 6), (26, 6)])
def test_walk_lengths(sup, n, walk_log2):
    a = random_matrix(n)
    chunks = T.chunk_count(sup, n, walk_log2)
    c0 = T.scattered_start(chunks)
    c1 = min(chunks, c0 + 8)
    v, st = sup.perman_complex_quad_range(a, c0, c1, walk_log2=walk_log2, return_stats=True)
    assert st["walk_bits"] == min(walk_log2, n - 1 - st["lane_bits"])
    assert v == sup.perman_complex_quad_range(a, c0, c1, cpu=True, threads=8, walk_log2=walk_log2)


def test_above_the_cap_is_unsupported(sup):
    big = random_matrix(CAP + 1)
    for call in (lambda: sup.perman_complex_quad(big), lambda: sup.perman_complex_quad_range(big, 0, 1)):
        with pytest.raises(sup.SupError) as e:
            call()
        assert e.value.code == -7 and str(CAP) in str(e.value)


def test_nan_propagates(sup):
    a = random_matrix(9).copy()
    a[3, 4] = complex(float("nan"), 1.0)
    (re, im) = sup.perman_complex_quad(a)
    assert math.isnan(re[0]) and math.isnan(im[0])


def test_empty_range_and_stats(sup):
    n = 13
    a = random_matrix(n)
    assert sup.perman_complex_quad_range(a, 3, 3, walk_log2=2) == ((0.0, 0.0), (0.0, 0.0))
    v, st = sup.perman_complex_quad(a, return_stats=True)
    L, m, h = sup.layout(n)
    assert st["devices_used"] == 1 and st["kernel_ms"] > 0 and st["wall_ms"] >= st["kernel_ms"]
    assert st["lane_bits"] == L and st["walk_bits"] == m and st["grid"] >= 1
    assert st["gray_steps"] == 1 << (n - 1) and st["est_ops_per_step"] == 86 * n - 28
