"""The exact hafnian walk on the GPU (walk_hafexact.hip through
sup_hafnian_complex_exact): the device's integers == the host twin's == one
matrix per call, at the smallest shapes where the kernel can go wrong (those of
test_gpu_hafnian.py), against the restatement and the closed forms, over one,
two and three launches, queue groups, slabs and logical devices.  Every
comparison of the entry is == on Python ints."""
import math

import numpy as np
import pytest

from test_complex_fock import cmul
from test_gpu_hafnian import SHAPES
from test_hafnian import err, hetero_lists, rank_one_bound, sym_gauss_int, walk_shape
from test_hafnian_exact import BIG, dfact, kan_exact, kan_scale_distinct, sym_gauss
from test_hafnian_powertrace import EPS, np_sum

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def need_gpu(sup):
    if sup.device_count() < 1:
        pytest.fail("no HIP device visible: -m gpu tests must run on the MI355X box")


def shape_case(name):
    n, patterns, _, _ = SHAPES[name]
    rng = np.random.default_rng(7000 + n)
    A, mu = sym_gauss(24, 7100 + n)
    idx = np.stack([np.repeat(rng.choice(24, len(s), replace=False), s) for s in patterns])
    return A, mu, idx


@pytest.mark.parametrize("name,loop", [(name, loop) for name in SHAPES for loop in SHAPES[name][3]])
def test_gpu_equals_host_twin(sup, name, loop):
    A, mu, idx = shape_case(name)
    n, _, want, _ = SHAPES[name]
    assert [walk_shape(idx[k])[:3] for k in range(len(want))] == want
    v, st = sup.hafnian_exact_batch(A, idx, mu=mu, loop=loop, return_stats=True)
    c, sc = sup.hafnian_exact_batch(A, idx, mu=mu, loop=loop, cpu=True, threads=16, return_stats=True)
    assert v == c
    assert v == [sup.hafnian_exact_batch(A, idx[k], mu=mu, loop=loop) for k in range(len(want))]
    if n <= 16:
        assert v == [kan_exact(A, idx[k], mu if loop else None) for k in range(len(want))]
    assert st["devices_used"] == 1 and st["leaves"] == len(want)
    assert st["visited_steps"] == sum(w[0] for w in want) and st["gray_steps"] == len(want) << (n - 1)
    assert st["kernel_ms"] > 0 and st["wall_ms"] >= st["kernel_ms"] and st["grid"] >= 1
    assert st["est_ops_per_step"] > 0 and st["est_ops_per_step"] == sc["est_ops_per_step"]
    assert st["seg_cached_bits"] == sc["seg_cached_bits"] >= 1


@pytest.mark.parametrize("loop", [False, True])
def test_gpu_n64_five_chunks_rank_one_closed_form(sup, loop):
    """(16, 16, 16, 16): 78,608 states, Tw = 272, H = 289 (5 chunks, 33 valid
    lanes in the last), m = 32.  A = u u^T, mu = c u: haf = 63!! prod u_idx,
    lhaf = prod u_idx sum_j n! / (2^j j! (n-2j)!) c^(n-2j)."""
    n = 64
    rng = np.random.default_rng(64)
    u = np.array([1 + 2j, -2 + 1j, 3j, -1 - 1j])
    cc = (2, -1)
    idx = np.repeat(np.arange(4), 16)
    rng.shuffle(idx[1:])
    assert walk_shape(idx)[:3] == (78608, 272, 289)
    prod = (1, 0)
    for i in idx:
        prod = cmul(prod, (int(u[i].real), int(u[i].imag)))
    if loop:
        s = (0, 0)
        for j in range(n // 2 + 1):
            coef = math.factorial(n) // (2 ** j * math.factorial(j) * math.factorial(n - 2 * j))
            p = (1, 0)
            for _ in range(n - 2 * j):
                p = cmul(p, cc)
            s = (s[0] + coef * p[0], s[1] + coef * p[1])
        want = cmul(prod, s)
    else:
        want = (dfact(63) * prod[0], dfact(63) * prod[1])
    v, st = sup.hafnian_exact_batch(np.outer(u, u), idx, mu=complex(*cc) * u, loop=loop, return_stats=True)
    assert v == want and st["visited_steps"] == 78608
    assert v == sup.hafnian_exact_batch(np.outer(u, u), idx, mu=complex(*cc) * u, loop=loop, cpu=True)


def test_gpu_weights_above_2_53_and_one_mode(sup):
    A, mu = sym_gauss(8, 53)
    for idx in (np.repeat([0, 1], 32), np.array([0] * 57 + list(range(1, 8)))):
        for loop in (False, True):
            v = sup.hafnian_exact_batch(A, idx, mu=mu, loop=loop)
            assert v == sup.hafnian_exact_batch(A, idx, mu=mu, loop=loop, cpu=True)
            assert v == kan_exact(A, idx, mu if loop else None)
    one = np.ones((1, 1))
    assert sup.hafnian_exact_batch(one, [0] * 64) == (dfact(63), 0)
    a = [1, 1]
    for k in range(2, 65):
        a.append(a[-1] + (k - 1) * a[-2])
    assert sup.hafnian_exact_batch(one, [0] * 64, mu=[1], loop=True) == (a[64], 0)


def test_gpu_one_two_and_three_launches(sup):
    """One launch (5 primes), a partly filled second launch (10 primes) and
    three launches (18 primes), with entries +-(2^31 - 1)(1 + i)."""
    rng = np.random.default_rng(12)
    sg = rng.choice([-1, 1], (6, 6))
    sg = np.triu(sg) + np.triu(sg, 1).T
    A = sg * (BIG * (1 + 1j))
    mu = np.diag(A).copy()
    i12 = [0] * 3 + [1] * 3 + [2] * 3 + [3] * 3
    for idx, loop, primes, launches in ((list(range(6)), False, 5, 1), (i12, False, 10, 2), (i12, True, 18, 3)):
        v, st = sup.hafnian_exact_batch(A, idx, mu=mu, loop=loop, return_stats=True)
        assert (st["seg_cached_bits"], st["seg_pair_bits"]) == (primes, launches)
        assert v == sup.hafnian_exact_batch(A, idx, mu=mu, loop=loop, cpu=True)
        assert v == kan_exact(A, idx, mu if loop else None)


def hetero_case(n, count, seed):
    A, mu = sym_gauss(12, seed)
    return A, mu, hetero_lists(n, count, seed)


@pytest.mark.parametrize("group", ["4", "64"])
@pytest.mark.parametrize("loop", [False, True])
def test_gpu_heterogeneous_batch_in_queue_groups(sup, monkeypatch, group, loop):
    A, mu, idx = hetero_case(14, 65, 414)
    want = sup.hafnian_exact_batch(A, idx, mu=mu, loop=loop, cpu=True, threads=16)
    monkeypatch.setenv("SUP_WALK_GROUP", group)  # read at every call
    assert sup.hafnian_exact_batch(A, idx, mu=mu, loop=loop) == want


@pytest.mark.parametrize("slab", ["1", "3"])
def test_gpu_slab_boundaries(sup, monkeypatch, slab):
    A, mu, idx = hetero_case(12, 7, 812)
    for loop in (False, True):
        whole = sup.hafnian_exact_batch(A, idx, mu=mu, loop=loop)
        monkeypatch.setenv("SUP_HAFNIAN_SLAB", slab)  # read at every call
        assert sup.hafnian_exact_batch(A, idx, mu=mu, loop=loop) == whole
        monkeypatch.delenv("SUP_HAFNIAN_SLAB")
        assert whole == sup.hafnian_exact_batch(A, idx, mu=mu, loop=loop, cpu=True, threads=16)


def test_gpu_logical_devices_take_contiguous_ranges(sup, monkeypatch):
    A, mu, idx = hetero_case(10, 9, 910)
    for loop in (False, True):
        one, s1 = sup.hafnian_exact_batch(A, idx, mu=mu, loop=loop, return_stats=True)
        assert s1["devices_used"] == 1
        monkeypatch.setenv("SUP_DEVICE_MAP", "0,0,0")
        assert sup.device_count() == 3
        for G in (2, 3):
            v, st = sup.hafnian_exact_batch(A, idx, mu=mu, loop=loop, gpu_num=G, return_stats=True)
            assert v == one and st["devices_used"] == G
        monkeypatch.delenv("SUP_DEVICE_MAP")


def test_gpu_last_device(sup):
    A, mu, idx = hetero_case(8, 5, 77)
    last = sup.device_count() - 1
    v, st = sup.hafnian_exact_batch(A, idx, mu=mu, loop=True, device_id=last, return_stats=True)
    assert v == sup.hafnian_exact_batch(A, idx, mu=mu, loop=True, cpu=True) and st["devices_used"] == 1


def test_gpu_floating_entries_against_the_device_exact_integers(sup):
    """The device's fp64 hafnian and power-trace hafnian at n = 22 within their
    own tests' bounds of the device's exact integers."""
    n = 22
    A = sym_gauss_int(n, 300 + n)
    idx = np.arange(n)
    truth = sup.hafnian_exact(A)
    assert truth == sup.hafnian_exact(A, cpu=True)
    T, Tw, H, K = walk_shape(idx)
    e = err(sup.hafnian(A), truth) / kan_scale_distinct(A, None, n, False)
    print(f"kan n={n} error/S={e:.3e} bound={rank_one_bound(n, Tw, K, False):.3e}")
    assert e <= rank_one_bound(n, Tw, K, False)
    v_np, S = np_sum(A, idx, None)
    e, e_np = err(sup.hafnian_powertrace(A), truth) / S, err(v_np, truth) / S
    print(f"powertrace n={n} error/S={e:.3e} numpy restatement {e_np:.3e}")
    assert e <= 8 * max(e_np, n * EPS)
