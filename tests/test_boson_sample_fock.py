"""The exact boson sampler on the collision-aware one-walk minors
(sup_boson_sample_fock, boson_sample(collision_aware=True)): the host twin,
which draws the same samples as the device path bit for bit.  Everything but
the per-stage minors call is sup_boson_sample's.

The walks here are tiny: stage k has k - 2 <= 3 free columns, so T <= 8,
Tw = 1, H = T (one wave-chunk per matrix)."""
import ctypes as C

import numpy as np
import pytest

from test_boson_sample import CHI2_34_1M, chi_square, haar_unitary, outcome_distribution


def test_sample_depends_on_its_index_only(sup):
    """M = 5, n = 3: T <= 2, Tw = 1, H = T."""
    U, _ = outcome_distribution()
    kw = dict(cpu=True, collision_aware=True)
    a = sup.boson_sample(U, [0, 2, 3], 100, seed=9, threads=1, **kw)
    b = sup.boson_sample(U, [0, 2, 3], 1000, seed=9, threads=16, **kw)
    assert np.array_equal(a, b[:100])
    assert np.array_equal(b, sup.boson_sample(U, [0, 2, 3], 1000, seed=9, threads=1, **kw))
    assert np.array_equal(b, sup.boson_sample(U, [0, 2, 3], 1000, seed=9, threads=5, **kw))
    assert not np.array_equal(b, sup.boson_sample(U, [0, 2, 3], 1000, seed=10, **kw))


def test_rows_sorted_and_stats(sup):
    """M = 8, n = 5: T <= 8, Tw = 1, H = T.  gray_steps stays nominal,
    visited_steps sums the stages' terms: below it once photons collide."""
    U = haar_unitary(8, 11)
    s, st = sup.boson_sample(U, [1, 4, 5, 7, 0], 300, seed=5, cpu=True, return_stats=True, collision_aware=True)
    assert s.shape == (300, 5) and s.dtype == np.int32
    assert (np.diff(s, axis=1) >= 0).all() and s.min() >= 0 and s.max() < 8
    assert st["leaves"] == 300 and st["devices_used"] == 0
    nominal = 300 * sum(1 << (k - 2) for k in range(2, 6))
    assert st["gray_steps"] == nominal and 300 * 4 <= st["visited_steps"] < nominal
    assert st["est_ops_per_step"] == 16 * 5 - 20
    assert (np.diff(s, axis=1) == 0).any()  # some photons did collide
    assert sup.boson_sample(U, [1, 4], 0, cpu=True, collision_aware=True).shape == (0, 2)
    # a single photon: no minors walk at all
    one, st1 = sup.boson_sample(U, [3], 50, seed=1, cpu=True, return_stats=True, collision_aware=True)
    assert np.array_equal(one, sup.boson_sample(U, [3], 50, seed=1, cpu=True))
    assert st1["gray_steps"] == 0 and st1["visited_steps"] == 0


def test_argument_errors(sup):
    U = haar_unitary(6, 13)
    kw = dict(cpu=True, collision_aware=True)
    with pytest.raises(sup.SupError, match=r"sup_boson_sample_fock: inputs\[position 2\] = 1 repeats position 0") as e:
        sup.boson_sample(U, [1, 3, 1], 10, **kw)
    assert e.value.code == -1
    with pytest.raises(sup.SupError, match=r"inputs\[position 1\] = 6 outside \[0, 6\)") as e:
        sup.boson_sample(U, [0, 6], 10, **kw)
    assert e.value.code == -1
    with pytest.raises(sup.SupError, match=r"inputs\[position 0\] = -1 outside") as e:
        sup.boson_sample(U, [-1, 2], 10, **kw)
    assert e.value.code == -1
    bad = U.copy()
    bad[2, 3] += 1e-6
    with pytest.raises(sup.SupError, match="not orthonormal") as e:
        sup.boson_sample(bad, [3, 4], 10, **kw)
    assert e.value.code == -1
    sup.boson_sample(bad, [0, 1], 10, **kw)  # only the used columns are checked
    with pytest.raises(sup.SupError, match="n = 33") as e:
        sup.boson_sample(np.eye(40), list(range(33)), 1, **kw)
    assert e.value.code == -7
    with pytest.raises(ValueError, match="square"):
        sup.boson_sample(np.ones((3, 4)), [0], 1, **kw)
    lib = sup._lib.load()
    u = np.ascontiguousarray(U)
    ins = np.array([0, 1], dtype=np.int32)
    out = (C.c_int32 * 4)()
    call = lib.sup_boson_sample_fock
    assert call(None, 6, ins.ctypes.data, 2, 2, 0, None, 1, out, None) == -1
    assert call(u.ctypes.data, 6, None, 2, 2, 0, None, 1, out, None) == -1
    assert call(u.ctypes.data, 6, ins.ctypes.data, 2, 2, 0, None, 1, None, None) == -1
    assert call(u.ctypes.data, 6, ins.ctypes.data, 0, 2, 0, None, 1, out, None) == -1
    assert call(u.ctypes.data, 0, ins.ctypes.data, 2, 2, 0, None, 1, out, None) == -1


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_outcome_distribution_chi_square(sup, seed):
    """test_boson_sample's test on the new entry: M = 5, inputs [0, 2, 3], 20000
    samples, Pearson chi^2 over the 35 outcomes below the same quantile
    (T <= 2, Tw = 1, H = T)."""
    U, P = outcome_distribution()
    s = sup.boson_sample(U, [0, 2, 3], 20000, seed=seed, cpu=True, collision_aware=True)
    chi2 = chi_square(s, P)
    print(f"seed {seed}: chi2 = {chi2:.1f} over 35 cells (threshold {CHI2_34_1M})")
    assert chi2 < CHI2_34_1M


def test_all_rows_equal_the_one_walk_sampler(sup):
    """M = 8, n = 5, 500 samples, one seed: every row equals boson_sample's.
    Only the last bits of the weights differ between the two minors entries, so
    a draw could move only where u sum(w) lies within rounding of a running
    sum, on the order of 1e-9 per run; this seed was confirmed on the host twin
    to give equality (T <= 8, Tw = 1, H = T)."""
    U = haar_unitary(8, 11)
    a = sup.boson_sample(U, [1, 4, 5, 7, 0], 500, seed=5, cpu=True)
    b = sup.boson_sample(U, [1, 4, 5, 7, 0], 500, seed=5, cpu=True, collision_aware=True)
    assert np.array_equal(a, b)
    # and the old entry is still its own: the switch changes nothing there
    assert np.array_equal(a, sup.boson_sample(U, [1, 4, 5, 7, 0], 500, seed=5, cpu=True, collision_aware=False))


def test_no_device_is_an_error_not_a_cpu_fallback(sup):
    U, _ = outcome_distribution()
    if sup.device_count() == 0:
        with pytest.raises(sup.SupError) as e:
            sup.boson_sample(U, [0, 2, 3], 4, collision_aware=True)
        assert e.value.code == -2
    else:  # a box with a device: the host twin's samples
        assert np.array_equal(sup.boson_sample(U, [0, 2, 3], 4, collision_aware=True),
                              sup.boson_sample(U, [0, 2, 3], 4, cpu=True, collision_aware=True))
