"""The power-trace hafnian kernel on the GPU (walk_hafpt.hip through
sup_hafnian_complex_pt, sup_loop_hafnian_complex_pt and the range entry): bit
for bit the host twin at the smallest shapes where the kernel can go wrong,
every column-count instantiation through the range entry, and one order the
Kan walk cannot serve in test time against its closed form.  Bits are compared
as uint64 pairs."""
import math
from fractions import Fraction

import numpy as np
import pytest

from test_complex_batch import bits
from test_hafnian_powertrace import EPS, cmul, err

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def need_gpu(sup):
    if sup.device_count() < 1:
        pytest.fail("no HIP device visible: -m gpu tests must run on the MI355X box")


def sym_case(M, seed):
    rng = np.random.default_rng(seed)
    A = (rng.standard_normal((M, M)) + 1j * rng.standard_normal((M, M))) / math.sqrt(M)
    return A + A.T, rng.standard_normal(M) + 1j * rng.standard_normal(M)


# n -> the forms run: 1, 2, .. 12 pairs (one, two and three 8-column blocks, the
# 32-column kernel), odd n (the virtual index)
WHOLE = [(2, (False, True)), (4, (False, True)), (6, (False, True)), (8, (False, True)), (10, (False, True)),
         (16, (False, True)), (17, (True,)), (18, (False, True)), (24, (False, True))]


@pytest.mark.parametrize("n,loop", [(n, loop) for n, forms in WHOLE for loop in forms])
def test_gpu_bits_are_the_twins(sup, n, loop):
    A, mu = sym_case(26, 5000 + n)
    idx = np.random.default_rng(n).choice(26, n, replace=False)
    v, st = sup.hafnian_powertrace_batch(A, idx, mu=mu, loop=loop, return_stats=True)
    want = sup.hafnian_powertrace_batch(A, idx, mu=mu, loop=loop, cpu=True, threads=16)
    assert bits(v).tolist() == bits(want).tolist()
    assert st["devices_used"] == 1 and st["kernel_ms"] > 0 and st["visited_steps"] == 2 ** ((n + 1) // 2) - 1


def repeats_case():
    A, mu = sym_case(5, 5100)
    rng = np.random.default_rng(12)
    idx = np.stack([np.sort(rng.integers(0, (1, 2, 3, 5)[k % 4], 12)) for k in range(9)])  # k % 4 == 0: one mode 12 times
    idx[1] = np.repeat(np.arange(3), (6, 4, 2))
    return A, mu, idx


@pytest.mark.parametrize("loop", [False, True])
def test_gpu_batch_with_repeats(sup, loop):
    A, mu, idx = repeats_case()
    v = sup.hafnian_powertrace_batch(A, idx, mu=mu, loop=loop)
    assert np.array_equal(bits(v), bits(sup.hafnian_powertrace_batch(A, idx, mu=mu, loop=loop, cpu=True, threads=16)))
    for k in (0, 5):
        assert bits(sup.hafnian_powertrace_batch(A, idx[k], mu=mu, loop=loop)).tolist() == bits(v[k]).tolist()


def kpad(z):
    return 8 * ((2 * z.bit_length() + 7) // 8)


@pytest.mark.parametrize("loop", [False, True])
def test_gpu_every_column_count_through_the_range_entry(sup, loop):
    """64 consecutive subsets from z = 2^p - 1, p = 4, 8, .., 28, and the last
    64 subsets, at the largest order the device serves: every instantiation
    (8, 16, .., 64 columns) runs, with 2 to 62 rows."""
    cap = sup.HAFNIAN_PT_MAX_DEVICE_N
    n = min(64, cap) & ~1
    m = n // 2
    A, mu = sym_case(n, 5200)
    idx = np.arange(n)
    starts = [2 ** p - 1 for p in (4, 8, 12, 16, 20, 24, 28)] + [2 ** m - 64]
    seen = set()
    for z0 in starts:
        seen |= {kpad(z) for z in range(z0, z0 + 64)}
        v, st = sup.hafnian_powertrace_range(A, idx, z0, z0 + 64, mu=mu, loop=loop, return_stats=True)
        want = sup.hafnian_powertrace_range(A, idx, z0, z0 + 64, mu=mu, loop=loop, cpu=True, threads=16)
        assert bits(v).tolist() == bits(want).tolist(), z0
        assert st["visited_steps"] == 64
    assert seen == set(range(8, 65, 8))
    if cap < 64:  # above the cap the device refuses and the twin serves the range
        A64, mu64 = sym_case(64, 5264)
        z0 = 2 ** 32 - 64
        with pytest.raises(sup.SupError, match="above the device cap") as e:
            sup.hafnian_powertrace_range(A64, np.arange(64), z0, z0 + 64, mu=mu64, loop=loop)
        assert e.value.code == -7
        v = sup.hafnian_powertrace_range(A64, np.arange(64), z0, z0 + 8, mu=mu64, loop=loop, cpu=True, threads=16)
        assert np.isfinite(v.real) and np.isfinite(v.imag) and v != 0


def test_gpu_unaligned_ranges_and_wide_chunks(sup):
    """n = 40 (m = 20): four subsets per wave-chunk; ranges that start and end
    inside a chunk, and one that spans three."""
    A, mu = sym_case(40, 5300)
    idx = np.arange(40)
    for z0, z1 in ((0, 3), (5, 7), (2 ** 20 - 9, 2 ** 20), (1021, 1031)):
        for loop in (False, True):
            v = sup.hafnian_powertrace_range(A, idx, z0, z1, mu=mu, loop=loop)
            want = sup.hafnian_powertrace_range(A, idx, z0, z1, mu=mu, loop=loop, cpu=True, threads=16)
            assert bits(v).tolist() == bits(want).tolist(), (z0, z1, loop)


@pytest.mark.parametrize("group", ["1", "64"])
def test_gpu_queue_groups_keep_the_bits(sup, monkeypatch, group):
    A, mu = sym_case(14, 5400)
    idx = np.random.default_rng(14).integers(0, 14, (65, 14))
    for loop in (False, True):
        want = sup.hafnian_powertrace_batch(A, idx, mu=mu, loop=loop, cpu=True, threads=16)
        monkeypatch.setenv("SUP_WALK_GROUP", group)  # read at every call
        assert np.array_equal(bits(sup.hafnian_powertrace_batch(A, idx, mu=mu, loop=loop)), bits(want))
        monkeypatch.delenv("SUP_WALK_GROUP")


def test_gpu_logical_devices_take_contiguous_ranges(sup, monkeypatch):
    A, mu = sym_case(10, 5500)
    idx = np.random.default_rng(10).integers(0, 10, (9, 10))
    for loop in (False, True):
        one, s1 = sup.hafnian_powertrace_batch(A, idx, mu=mu, loop=loop, return_stats=True)
        assert s1["devices_used"] == 1
        monkeypatch.setenv("SUP_DEVICE_MAP", "0,0,0")
        assert sup.device_count() == 3
        for G in (2, 3):
            v, st = sup.hafnian_powertrace_batch(A, idx, mu=mu, loop=loop, gpu_num=G, return_stats=True)
            assert np.array_equal(bits(v), bits(one)) and st["devices_used"] == G
        monkeypatch.delenv("SUP_DEVICE_MAP")


def test_gpu_above_the_cap_is_unsupported(sup):
    cap = sup.HAFNIAN_PT_MAX_DEVICE_N
    assert 50 <= cap < 64
    A = np.ones((cap + 1, cap + 1), dtype=np.complex128)
    for loop in (False, True):
        with pytest.raises(sup.SupError, match=f"SUP_HAFNIAN_PT_MAX_DEVICE_N = {cap}") as e:
            sup.hafnian_powertrace_batch(A, np.arange(cap + 1), loop=loop)
        assert e.value.code == -7


def test_gpu_rank_one_order_36(sup):
    """A = u u^T, 36 distinct indices, 2^18 subsets: haf = 35!! prod u_i.  Here
    tr (N_z X)^j = s_z^j with s_z = 2 sum_{b in z} u_2b u_2b+1, so f(z) =
    C(2m, m) / 4^m s_z^m and S = sum_z |f(z)| has a closed form too.  u has 8-bit
    dyadic parts, so A is exactly u u^T.  Bound: the host tests' 8 n 2^-52 S,
    scaled by n (the sum over 2^18 subsets is pairwise, the powers reach
    degree 18).  The host twin needs 16 threads for several seconds at this
    order and is not run; its bits are compared up to n = 24 above."""
    n, m = 36, 18
    rng = np.random.default_rng(36)
    ur, ui = rng.integers(-255, 256, n), rng.integers(-255, 256, n)
    u = (ur + 1j * ui) / 256
    A = np.outer(u, u)
    assert np.array_equal(A, A.T)
    prod = (Fraction(1), Fraction(0))
    for a, b in zip(ur, ui):
        prod = cmul(prod, (Fraction(int(a), 256), Fraction(int(b), 256)))
    dfact = math.prod(range(n - 1, 0, -2))
    truth = (dfact * prod[0], dfact * prod[1])
    pair = 2 * u[0::2] * u[1::2]
    z = np.arange(1, 2 ** m, dtype=np.int64)
    s = np.zeros(z.shape, dtype=np.complex128)
    for b in range(m):
        s += np.where((z >> b) & 1, pair[b], 0)
    S = float(np.sum(np.abs(s) ** m)) * math.comb(2 * m, m) / 4.0 ** m
    v, st = sup.hafnian_powertrace(A, return_stats=True)
    e = err(v, truth) / S
    print(f"n=36 rank one: e={e:.3e} bound={8 * n * n * EPS:.3e} S/|haf|={S / abs(v):.1f} kernel_ms={st['kernel_ms']:.2f}")
    assert e <= 8 * n * n * EPS
    assert st["visited_steps"] == 2 ** m - 1
