"""The loop torontonian kernel on the GPU (walk_ltor.hip through
sup_loop_torontonian and the range entry): the exponential's bits against the
host's, bit for bit the host twin at the smallest shapes where the kernel can
go wrong (fewer positions than tail bits, the first prefixes, the pausing step,
more than one chunk), the range entry at the cap, and one closed form with no
twin.  Bits are compared as uint64."""
import math

import mpmath
import numpy as np
import pytest

from test_loop_torontonian import decoupled_case, dyadic_gamma, ltor_np
from test_torontonian import EPS, batch_case, dyadic_O, fbits

pytestmark = pytest.mark.gpu

W = 4  # ltor.hpp kLtorW (SUP_LTOR_W): the tail positions of a lane


@pytest.fixture(scope="module", autouse=True)
def need_gpu(sup):
    if sup.device_count() < 1:
        pytest.fail("no HIP device visible: -m gpu tests must run on the MI355X box")


def test_gpu_ltor_exp_has_the_hosts_bits(sup):
    rng = np.random.default_rng(8000)
    x = np.concatenate([rng.uniform(0, 40, 25000), rng.uniform(0, 709, 25000), rng.uniform(-1, 1, 25000),
                        rng.uniform(-700, 0, 25000), rng.uniform(-760, -700, 500), rng.uniform(709, 712, 500),
                        [0.0, -0.0, math.nan, 710.0, -746.0, -745.0, 709.7, math.inf, -math.inf, 1e300, -1e300,
                         5e-324, -5e-324, 711.0, -750.0]])
    dev, host = sup.ltor_exp(x, device=True), sup.ltor_exp(x)
    nan = np.isnan(host)
    assert np.array_equal(np.isnan(dev), nan) and nan.sum() == 1  # a NaN is a NaN: its payload is not compared
    assert np.array_equal(fbits(dev[~nan]), fbits(host[~nan]))
    edge = dict(zip(x[-15:].tolist(), dev[-15:].tolist()))
    assert fbits(edge[0.0]) == fbits(1.0) and edge[710.0] == math.inf and fbits(edge[-746.0]) == fbits(0.0)
    assert fbits(dev[-14]) == fbits(1.0)  # exp(-0)


@pytest.mark.parametrize("n", sorted({1, 2, 3, W - 1, W, W + 1, W + 2, 8, 12, 16}))
def test_gpu_bits_are_the_twins(sup, n):
    O = dyadic_O(18, 8100 + n)
    gamma = dyadic_gamma(O, 8150 + n)
    modes = np.random.default_rng(n).permutation(18)[:n]
    v, st = sup.loop_torontonian_batch(O, gamma, modes, return_stats=True)
    want = sup.loop_torontonian_batch(O, gamma, modes, cpu=True, threads=16)
    assert fbits(v) == fbits(want), (v, want)
    assert fbits(v) != fbits(sup.torontonian_batch(O, modes, cpu=True, threads=16))
    assert st["devices_used"] == 1 and st["kernel_ms"] > 0 and st["visited_steps"] == 2 ** n
    assert st["gray_steps"] == 2 ** n and st["leaves"] == 1 and st["grid"] >= 1
    assert st["est_ops_per_step"] == sup.loop_torontonian_plan(n)[1]


def test_gpu_batch_of_nine_lists(sup):
    O, modes = batch_case(9, 10, 16, 8200)
    gamma = dyadic_gamma(O, 8201)
    v = sup.loop_torontonian_batch(O, gamma, modes)
    assert np.array_equal(fbits(v), fbits(sup.loop_torontonian_batch(O, gamma, modes, cpu=True, threads=16)))
    for k in (0, 5):
        assert fbits(sup.loop_torontonian_batch(O, gamma, modes[k])) == fbits(v[k])


def test_gpu_gamma_zero_has_the_torontonians_bits(sup):
    O = dyadic_O(12, 8300)
    v = sup.loop_torontonian(O, np.zeros(24))
    assert fbits(v) == fbits(sup.torontonian(O)) and fbits(v) == fbits(sup.torontonian(O, cpu=True))


def test_gpu_range_entry_at_the_cap(sup):
    """[2^cap - 128, 2^cap): every position selected, the longest prefix; [0,
    128): none; ranges inside a chunk and across chunks (a chunk is 2^17 z)."""
    cap = sup.LOOP_TORONTONIAN_MAX_DEVICE_N
    O = dyadic_O(cap, 8400)
    gamma = dyadic_gamma(O, 8401)
    modes = np.random.default_rng(cap).permutation(cap)
    L = 2 ** (cap - 15)
    for z0, z1 in ((2 ** cap - 128, 2 ** cap), (0, 128), (5 * L + 37, 5 * L + 37 + 100), (3 * L - 70, 3 * L + 90),
                   (2 ** cap - L - 64, 2 ** cap - L + 64)):
        v, st = sup.loop_torontonian_range(O, gamma, modes, z0, z1, return_stats=True)
        want = sup.loop_torontonian_range(O, gamma, modes, z0, z1, cpu=True)
        assert fbits(v) == fbits(want), (z0, z1, v, want)
        assert st["visited_steps"] == z1 - z0
    v_np, S = ltor_np(O, gamma, modes, range(2 ** cap - 128, 2 ** cap))
    # the whole matrix's exponent is 4 (dyadic_gamma), a subset's is no larger
    assert abs(sup.loop_torontonian_range(O, gamma, modes, 2 ** cap - 128, 2 ** cap) - v_np) <= 8 * cap * EPS * (1.0 + 4.0) * S


@pytest.mark.parametrize("group", ["1", "64"])
def test_gpu_queue_groups_keep_the_bits(sup, monkeypatch, group):
    O, modes = batch_case(65, 8, 12, 8500)
    gamma = dyadic_gamma(O, 8501)
    want = sup.loop_torontonian_batch(O, gamma, modes, cpu=True, threads=16)
    monkeypatch.setenv("SUP_WALK_GROUP", group)  # read at every call
    assert np.array_equal(fbits(sup.loop_torontonian_batch(O, gamma, modes)), fbits(want))
    monkeypatch.delenv("SUP_WALK_GROUP")
    O = dyadic_O(13, 8502)  # one list of 16 chunks
    gamma = dyadic_gamma(O, 8503)
    monkeypatch.setenv("SUP_WALK_GROUP", group)
    v = sup.loop_torontonian(O, gamma)
    monkeypatch.delenv("SUP_WALK_GROUP")
    assert fbits(v) == fbits(sup.loop_torontonian(O, gamma, cpu=True))


def test_gpu_logical_devices_take_contiguous_ranges(sup, monkeypatch):
    O, modes = batch_case(9, 10, 14, 8600)
    gamma = dyadic_gamma(O, 8601)
    one, s1 = sup.loop_torontonian_batch(O, gamma, modes, return_stats=True)
    assert s1["devices_used"] == 1
    monkeypatch.setenv("SUP_DEVICE_MAP", "0,0,0")
    assert sup.device_count() == 3
    for G in (2, 3):
        v, st = sup.loop_torontonian_batch(O, gamma, modes, gpu_num=G, return_stats=True)
        assert np.array_equal(fbits(v), fbits(one)) and st["devices_used"] == G
    monkeypatch.delenv("SUP_DEVICE_MAP")


def test_gpu_not_positive_definite_gives_nan(sup):
    assert math.isnan(sup.loop_torontonian(2.0 * np.eye(2), [0.5, 0.25j]))
    O = dyadic_O(8, 8700)
    gamma = dyadic_gamma(O, 8701)
    O[3, 3] = 1.5  # in the prefix of the second list, in the tail of the third
    v = sup.loop_torontonian_batch(O, gamma, [[0, 1, 2, 4, 5, 6], [4, 5, 6, 7, 0, 3], [3, 5, 6, 7, 0, 1]])
    assert not math.isnan(v[0]) and math.isnan(v[1]) and math.isnan(v[2])


def test_gpu_decoupled_modes_at_22(sup):
    mpmath.mp.prec = 200
    O, gamma, g, xmax = decoupled_case(22, 2622)
    want, scale = mpmath.fprod(gi - 1 for gi in g), mpmath.fprod(g)
    v = sup.loop_torontonian(O, gamma)
    e = float(abs(mpmath.mpf(v) - want) / scale)
    print(f"decoupled n=22 on the device: e={e:.3e} bound={22 * EPS * (1.0 + xmax):.3e}")
    assert e <= 22 * EPS * (1.0 + xmax)
