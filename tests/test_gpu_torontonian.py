"""The torontonian kernel on the GPU (walk_tor.hip through sup_torontonian and
the range entry): bit for bit the host twin at the smallest shapes where the
kernel can go wrong (fewer positions than tail bits, the first prefixes, more
than one chunk), the range entry at the cap, and one closed form with no twin.
Bits are compared as uint64."""
import math

import numpy as np
import pytest

from test_torontonian import EPS, batch_case, dyadic_O, fbits, tor_np

pytestmark = pytest.mark.gpu

W = 5  # tor.hpp kTorW: the tail positions of a lane


@pytest.fixture(scope="module", autouse=True)
def need_gpu(sup):
    if sup.device_count() < 1:
        pytest.fail("no HIP device visible: -m gpu tests must run on the MI355X box")


@pytest.mark.parametrize("n", [1, 2, 3, W, W + 1, W + 2, 8, 12, 16])
def test_gpu_bits_are_the_twins(sup, n):
    O = dyadic_O(18, 7000 + n)
    modes = np.random.default_rng(n).permutation(18)[:n]
    v, st = sup.torontonian_batch(O, modes, return_stats=True)
    want = sup.torontonian_batch(O, modes, cpu=True, threads=16)
    assert fbits(v) == fbits(want), (v, want)
    assert st["devices_used"] == 1 and st["kernel_ms"] > 0 and st["visited_steps"] == 2 ** n
    assert st["est_ops_per_step"] == sup.torontonian_plan(n)[1]


def test_gpu_batch_of_nine_lists(sup):
    O, modes = batch_case(9, 10, 16, 7100)
    v = sup.torontonian_batch(O, modes)
    assert np.array_equal(fbits(v), fbits(sup.torontonian_batch(O, modes, cpu=True, threads=16)))
    for k in (0, 5):
        assert fbits(sup.torontonian_batch(O, modes[k])) == fbits(v[k])


def test_gpu_range_entry_at_the_cap(sup):
    """[2^cap - 128, 2^cap): every position selected, the longest prefix; [0,
    128): none; ranges inside a chunk and across chunks (a chunk is 2^17 z)."""
    cap = sup.TORONTONIAN_MAX_DEVICE_N
    O = dyadic_O(cap, 7200)
    modes = np.random.default_rng(cap).permutation(cap)
    L = 2 ** (cap - 15)
    for z0, z1 in ((2 ** cap - 128, 2 ** cap), (0, 128), (5 * L + 37, 5 * L + 37 + 100), (3 * L - 70, 3 * L + 90),
                   (2 ** cap - L - 64, 2 ** cap - L + 64)):
        v, st = sup.torontonian_range(O, modes, z0, z1, return_stats=True)
        want = sup.torontonian_range(O, modes, z0, z1, cpu=True)
        assert fbits(v) == fbits(want), (z0, z1, v, want)
        assert st["visited_steps"] == z1 - z0
    v_np, S = tor_np(O, modes, range(2 ** cap - 128, 2 ** cap))
    assert abs(sup.torontonian_range(O, modes, 2 ** cap - 128, 2 ** cap) - v_np) <= 8 * cap * EPS * S


def test_gpu_three_to_the_22_with_equality(sup):
    assert sup.torontonian(np.diag([0.75] * 44)) == 3.0 ** 22


@pytest.mark.parametrize("group", ["1", "64"])
def test_gpu_queue_groups_keep_the_bits(sup, monkeypatch, group):
    O, modes = batch_case(65, 8, 12, 7300)
    want = sup.torontonian_batch(O, modes, cpu=True, threads=16)
    monkeypatch.setenv("SUP_WALK_GROUP", group)  # read at every call
    assert np.array_equal(fbits(sup.torontonian_batch(O, modes)), fbits(want))
    monkeypatch.delenv("SUP_WALK_GROUP")
    O = dyadic_O(13, 7301)  # one list of 16 chunks
    monkeypatch.setenv("SUP_WALK_GROUP", group)
    v = sup.torontonian(O)
    monkeypatch.delenv("SUP_WALK_GROUP")
    assert fbits(v) == fbits(sup.torontonian(O, cpu=True))


def test_gpu_logical_devices_take_contiguous_ranges(sup, monkeypatch):
    O, modes = batch_case(9, 10, 14, 7400)
    one, s1 = sup.torontonian_batch(O, modes, return_stats=True)
    assert s1["devices_used"] == 1
    monkeypatch.setenv("SUP_DEVICE_MAP", "0,0,0")
    assert sup.device_count() == 3
    for G in (2, 3):
        v, st = sup.torontonian_batch(O, modes, gpu_num=G, return_stats=True)
        assert np.array_equal(fbits(v), fbits(one)) and st["devices_used"] == G
    monkeypatch.delenv("SUP_DEVICE_MAP")


def test_gpu_not_positive_definite_gives_nan(sup):
    assert math.isnan(sup.torontonian(2.0 * np.eye(2)))
    O = dyadic_O(8, 7500)
    O[3, 3] = 1.5  # in the prefix of the second list, in the tail of the third
    v = sup.torontonian_batch(O, [[0, 1, 2, 4, 5, 6], [4, 5, 6, 7, 0, 3], [3, 5, 6, 7, 0, 1]])
    assert not math.isnan(v[0]) and math.isnan(v[1]) and math.isnan(v[2])
