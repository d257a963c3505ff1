"""Batched complex permanents on host threads (cplx.cpp cplx_perman_batch
through perman_complex_batch / perman_complex_submatrices with cpu=True).

The contract: result k has the bits of perman_complex of matrix k alone (for
the submatrix form, of the gathered matrix) with the same walk bits, for any
thread count.  Bits are compared as uint64 pairs, so NaN payloads and signed
zeros count.
"""
import math

import numpy as np
import pytest

from test_complex import as_complex, exact_perm, gauss_int_case, random_case


def bits(v):
    return np.ascontiguousarray(np.asarray(v, dtype=np.complex128)).view(np.uint64)


def batch_of(n, count, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((count, n, n)) + 1j * rng.standard_normal((count, n, n))


def loop(sup, mats, **kw):
    return np.array([sup.perman_complex(a, cpu=True, **kw) for a in mats], dtype=np.complex128)


def repeated_indices(rng, count, n, R, C):
    """Index lists with collisions: every list repeats at least one entry."""
    rows = rng.integers(0, R, (count, n))
    cols = rng.integers(0, C, (count, n))
    rows[:, -1] = rows[:, 0]
    cols[:, 1] = cols[:, 0]
    return rows, cols


@pytest.mark.parametrize("count", [1, 3, 65])
@pytest.mark.parametrize("n", [1, 2, 5, 7, 8, 13])
def test_batch_bit_equal_to_loop(sup, n, count):
    mats = batch_of(n, count, 1000 * n + count)
    got = sup.perman_complex_batch(mats, cpu=True)
    assert got.dtype == np.complex128 and got.shape == (count,)
    assert np.array_equal(bits(got), bits(loop(sup, mats)))


def test_batch_bit_equal_with_walk_bits(sup):
    mats = batch_of(13, 5, 77)
    got, st = sup.perman_complex_batch(mats, cpu=True, walk_log2=3, return_stats=True)
    assert st["walk_bits"] == 3 and st["lane_bits"] == 6
    assert np.array_equal(bits(got), bits(loop(sup, mats, walk_log2=3)))
    # the walk bits are part of the result's definition: the default layout's chunks differ
    assert st["leaves"] == 5 and st["gray_steps"] == 5 << 12 and st["est_ops_per_step"] == 6 * 13


def test_batch_agrees_with_exact_truth(sup):
    a, truth, scale, _ = random_case(8, 1)
    v = sup.perman_complex_batch(np.stack([a, a]), cpu=True)
    assert v[0] == v[1] == sup.perman_complex(a, cpu=True)
    assert abs(v[0] - complex(float(truth[0]), float(truth[1]))) <= 1e-12 * scale


def test_submatrices_equal_batch_of_gathered(sup):
    rng = np.random.default_rng(5)
    U = rng.standard_normal((9, 11)) + 1j * rng.standard_normal((9, 11))
    rows, cols = repeated_indices(rng, 17, 6, 9, 11)
    gathered = np.stack([U[np.ix_(rows[k], cols[k])] for k in range(17)])
    got = sup.perman_complex_submatrices(U, rows, cols, cpu=True)
    assert got.shape == (17,)
    assert np.array_equal(bits(got), bits(sup.perman_complex_batch(gathered, cpu=True)))
    assert np.array_equal(bits(got), bits(loop(sup, gathered)))


@pytest.mark.parametrize("n", [3, 6, 8])
def test_submatrices_exact_gaussian_integers(sup, n):
    rng = np.random.default_rng(40 + n)
    U = gauss_int_case(10, 9)
    rows, cols = repeated_indices(rng, 6, n, 10, 10)
    got = sup.perman_complex_submatrices(U, rows, cols, cpu=True)
    for k in range(6):
        assert got[k] == as_complex(exact_perm(U[np.ix_(rows[k], cols[k])])), k


@pytest.mark.parametrize("n", [2, 5, 8])
def test_submatrices_of_ones_with_equal_rows_give_factorial(sup, n):
    U = np.ones((4, 12), dtype=np.complex128)
    rows = np.zeros((3, n), dtype=np.int64)  # every row the same row of U
    rows[1, : n // 2] = 3
    cols = np.tile(np.arange(n), (3, 1))
    cols[2] = 7  # and every column the same column
    got = sup.perman_complex_submatrices(U, rows, cols, cpu=True)
    assert np.array_equal(got, np.full(3, complex(math.factorial(n), 0.0)))


def test_empty_batch(sup):
    v, st = sup.perman_complex_batch(np.zeros((0, 5, 5), dtype=np.complex128), cpu=True, return_stats=True)
    assert v.shape == (0,) and v.dtype == np.complex128
    assert st["leaves"] == 0 and st["gray_steps"] == 0
    U = np.ones((3, 3), dtype=np.complex128)
    w = sup.perman_complex_submatrices(U, np.zeros((0, 2), dtype=np.int32), np.zeros((0, 2), dtype=np.int32), cpu=True)
    assert w.shape == (0,)


def test_argument_errors(sup):
    with pytest.raises(ValueError, match="count, n, n"):
        sup.perman_complex_batch(np.zeros((3, 4, 5)), cpu=True)
    with pytest.raises(ValueError, match="outside"):
        sup.perman_complex_batch(np.zeros((1, 65, 65)), cpu=True)
    with pytest.raises(sup.SupError, match="walk_log2 = 40") as e:
        sup.perman_complex_batch(np.ones((2, 4, 4)), cpu=True, walk_log2=40)
    assert e.value.code == -1
    U = np.ones((3, 4), dtype=np.complex128)
    with pytest.raises(ValueError, match="shape"):
        sup.perman_complex_submatrices(U, np.zeros((2, 3), dtype=int), np.zeros((2, 4), dtype=int), cpu=True)
    with pytest.raises(ValueError, match="integer"):
        sup.perman_complex_submatrices(U, np.zeros((2, 3)), np.zeros((2, 3)), cpu=True)


def test_index_errors_name_the_offender(sup):
    U = np.ones((3, 4), dtype=np.complex128)
    rows = np.zeros((5, 2), dtype=np.int32)
    cols = np.zeros((5, 2), dtype=np.int32)
    bad = rows.copy()
    bad[3, 1] = 3  # R = 3
    with pytest.raises(sup.SupError, match=r"rows\[k = 3\]\[position 1\] = 3 outside \[0, 3\)") as e:
        sup.perman_complex_submatrices(U, bad, cols, cpu=True)
    assert e.value.code == -1
    bad = cols.copy()
    bad[4, 0] = -1
    with pytest.raises(sup.SupError, match=r"cols\[k = 4\]\[position 0\] = -1 outside \[0, 4\)"):
        sup.perman_complex_submatrices(U, rows, bad, cpu=True)


def test_c_abi_null_and_range_errors(sup):
    import ctypes as C

    lib = sup._lib.load()
    out = (C.c_double * 4)()
    m = np.ones(2 * 2 * 4)
    assert lib.sup_perman_complex_batch(None, 2, 2, None, 1, out, None) == -1
    assert lib.sup_perman_complex_batch(m.ctypes.data, 2, 2, None, 1, None, None) == -1
    assert lib.sup_perman_complex_batch(m.ctypes.data, 0, 2, None, 1, out, None) == -1
    assert lib.sup_perman_complex_batch(m.ctypes.data, 65, 0, None, 1, out, None) == -1
    idx = np.zeros(4, dtype=np.int32)
    for R, Cc in ((0, 2), (2, 0)):
        assert lib.sup_perman_complex_submatrices(m.ctypes.data, R, Cc, idx.ctypes.data, idx.ctypes.data, 2, 2, None,
                                                  1, out, None) == -1
    assert lib.sup_perman_complex_submatrices(m.ctypes.data, 2, 2, None, idx.ctypes.data, 2, 2, None, 1, out,
                                              None) == -1
    # count == 0 writes nothing
    out[0] = 7.0
    assert lib.sup_perman_complex_batch(m.ctypes.data, 2, 0, None, 1, out, None) == 0 and out[0] == 7.0


def test_nan_stays_in_its_own_result(sup):
    mats = batch_of(7, 9, 31)
    clean = sup.perman_complex_batch(mats, cpu=True)
    dirty = mats.copy()
    dirty[4, 2, 3] = complex(np.nan, 1.0)
    dirty[6, 0, 0] = complex(0.0, np.inf)
    got = sup.perman_complex_batch(dirty, cpu=True)
    keep = [k for k in range(9) if k not in (4, 6)]
    assert np.array_equal(bits(got[keep]), bits(clean[keep]))
    assert not np.isfinite(got[4]) and not np.isfinite(got[6])
    assert np.array_equal(bits(got[[4, 6]]), bits(loop(sup, dirty[[4, 6]])))


@pytest.mark.parametrize("n,count", [(8, 40), (13, 3)])
def test_thread_count_changes_no_bit(sup, n, count):
    mats = batch_of(n, count, 5 * n)
    one = sup.perman_complex_batch(mats, cpu=True, threads=1)
    assert np.array_equal(bits(one), bits(sup.perman_complex_batch(mats, cpu=True, threads=16)))
