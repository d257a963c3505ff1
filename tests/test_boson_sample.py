"""The exact boson sampler (sup_boson_sample; Clifford & Clifford 2018,
algorithm A, on the one-walk minors): the host twin, which draws the same
samples as the device path bit for bit."""
import itertools
import math

import numpy as np
import pytest

from test_complex import np_ryser

CHI2_34_1M = 88.38  # the 1 - 1e-6 quantile of chi^2 with 34 degrees of freedom


def haar_unitary(M, seed):
    """QR of a standard-normal complex M x M, columns multiplied by the unit
    phases of diag(R)."""
    rng = np.random.default_rng(seed)
    z = rng.standard_normal((M, M)) + 1j * rng.standard_normal((M, M))
    q, r = np.linalg.qr(z)
    d = np.diag(r)
    return q * (d / np.abs(d))


_DIST = {}


def outcome_distribution(M=5, inputs=(0, 2, 3), seed=2024):
    """(U, {sorted outcome: P}) with P(z) = |per U[z, inputs]|^2 / prod z_m!,
    computed once."""
    key = (M, tuple(inputs), seed)
    if key not in _DIST:
        U = haar_unitary(M, seed)
        P = {}
        for z in itertools.combinations_with_replacement(range(M), len(inputs)):
            mult = math.prod(math.factorial(z.count(m)) for m in set(z))
            P[z] = abs(np_ryser(U[np.ix_(list(z), list(inputs))])[0]) ** 2 / mult
        _DIST[key] = (U, P)
    return _DIST[key]


def chi_square(samples, P):
    counts = {z: 0 for z in P}
    for row in samples:
        counts[tuple(int(v) for v in row)] += 1
    n = len(samples)
    return sum((counts[z] - n * P[z]) ** 2 / (n * P[z]) for z in P)


def test_distribution_setup_is_sound():
    _, P = outcome_distribution()
    assert len(P) == 35
    assert abs(sum(P.values()) - 1.0) <= 1e-12
    assert 20000 * min(P.values()) >= 5
    print(f"min P = {min(P.values()):.3e}")


def test_single_photon_counts(sup):
    """n = 1, M = 4: the outcome is mode i with probability |U[i][input]|^2.
    Pearson chi^2 with 3 degrees of freedom stays below its 1 - 1e-6 quantile
    30.66 (a correct sampler fails a given seed with probability 1e-6)."""
    U = haar_unitary(4, 7)
    s = sup.boson_sample(U, [2], 20000, seed=3, cpu=True)
    assert s.shape == (20000, 1) and s.dtype == np.int32
    p = np.abs(U[:, 2]) ** 2
    counts = np.bincount(s[:, 0], minlength=4)
    chi2 = float(((counts - 20000 * p) ** 2 / (20000 * p)).sum())
    print(f"counts {counts.tolist()} expected {(20000 * p).round(1).tolist()} chi2 {chi2:.2f}")
    assert chi2 < 30.66


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_outcome_distribution_chi_square(sup, seed):
    U, P = outcome_distribution()
    s = sup.boson_sample(U, [0, 2, 3], 20000, seed=seed, cpu=True)
    chi2 = chi_square(s, P)
    print(f"seed {seed}: chi2 = {chi2:.1f} over 35 cells (threshold {CHI2_34_1M})")
    assert chi2 < CHI2_34_1M


def test_sample_depends_on_its_index_only(sup):
    U, _ = outcome_distribution()
    a = sup.boson_sample(U, [0, 2, 3], 100, seed=9, cpu=True, threads=1)
    b = sup.boson_sample(U, [0, 2, 3], 1000, seed=9, cpu=True, threads=16)
    assert np.array_equal(a, b[:100])
    assert np.array_equal(b, sup.boson_sample(U, [0, 2, 3], 1000, seed=9, cpu=True, threads=1))
    assert not np.array_equal(b, sup.boson_sample(U, [0, 2, 3], 1000, seed=10, cpu=True))
    # the order of the input list is part of the shuffle's start, not of the distribution: still valid rows
    assert sup.boson_sample(U, [3, 0, 2], 10, seed=9, cpu=True).shape == (10, 3)


def test_rows_sorted_and_in_range(sup):
    U = haar_unitary(8, 11)
    s, st = sup.boson_sample(U, [1, 4, 5, 7, 0], 300, seed=5, cpu=True, return_stats=True)
    assert s.shape == (300, 5)
    assert (np.diff(s, axis=1) >= 0).all() and s.min() >= 0 and s.max() < 8
    assert st["leaves"] == 300 and st["devices_used"] == 0
    assert st["gray_steps"] == 300 * sum(1 << (k - 2) for k in range(2, 6))
    assert sup.boson_sample(U, [1, 4], 0, cpu=True).shape == (0, 2)


def test_argument_errors(sup):
    U = haar_unitary(6, 13)
    with pytest.raises(sup.SupError, match=r"inputs\[position 2\] = 1 repeats position 0") as e:
        sup.boson_sample(U, [1, 3, 1], 10, cpu=True)
    assert e.value.code == -1
    with pytest.raises(sup.SupError, match=r"inputs\[position 1\] = 6 outside \[0, 6\)") as e:
        sup.boson_sample(U, [0, 6], 10, cpu=True)
    assert e.value.code == -1
    with pytest.raises(sup.SupError, match=r"inputs\[position 0\] = -1 outside") as e:
        sup.boson_sample(U, [-1, 2], 10, cpu=True)
    assert e.value.code == -1
    bad = U.copy()
    bad[2, 3] += 1e-6
    with pytest.raises(sup.SupError, match="not orthonormal") as e:
        sup.boson_sample(bad, [3, 4], 10, cpu=True)
    assert e.value.code == -1
    sup.boson_sample(bad, [0, 1], 10, cpu=True)  # only the used columns are checked
    with pytest.raises(sup.SupError, match="n = 33") as e:
        sup.boson_sample(np.eye(40), list(range(33)), 1, cpu=True)
    assert e.value.code == -7
    with pytest.raises(ValueError, match="square"):
        sup.boson_sample(np.ones((3, 4)), [0], 1, cpu=True)
    import ctypes as C
    lib = sup._lib.load()
    u = np.ascontiguousarray(U)
    ins = np.array([0, 1], dtype=np.int32)
    out = (C.c_int32 * 4)()
    assert lib.sup_boson_sample(None, 6, ins.ctypes.data, 2, 2, 0, None, 1, out, None) == -1
    assert lib.sup_boson_sample(u.ctypes.data, 6, None, 2, 2, 0, None, 1, out, None) == -1
    assert lib.sup_boson_sample(u.ctypes.data, 6, ins.ctypes.data, 2, 2, 0, None, 1, None, None) == -1
    assert lib.sup_boson_sample(u.ctypes.data, 6, ins.ctypes.data, 0, 2, 0, None, 1, out, None) == -1
    assert lib.sup_boson_sample(u.ctypes.data, 0, ins.ctypes.data, 2, 2, 0, None, 1, out, None) == -1


def test_no_device_is_an_error_not_a_cpu_fallback(sup):
    U, _ = outcome_distribution()
    if sup.device_count() == 0:
        with pytest.raises(sup.SupError) as e:
            sup.boson_sample(U, [0, 2, 3], 4)
        assert e.value.code == -2
    else:  # a box with a device: the host twin's samples
        assert np.array_equal(sup.boson_sample(U, [0, 2, 3], 4), sup.boson_sample(U, [0, 2, 3], 4, cpu=True))
