"""The collision-aware complex walk on the GPU (walk_cplxf.hip, cplx_fock.hip
through sup_perman_complex_fock): bit for bit the host twin, at the smallest
shapes where the kernel can go wrong, and the twin's anchors (exact Gaussian
integers, the rank-one closed form).  Bits are compared as uint64 pairs."""
import math

import numpy as np
import pytest

from test_complex import as_complex, err_over_scale, exact_perm, gauss_int_case
from test_complex_batch import bits
from test_complex_fock import fock_bound, hetero_batch, plan, rank_one_case

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def need_gpu(sup):
    if sup.device_count() < 1:
        pytest.fail("no HIP device visible: -m gpu tests must run on the MI355X box")


def pattern_batch(n, patterns, seed):
    """One (rows, cols) pair per (rows multiplicities, cols multiplicities), the
    groups in the order given (the order of first appearance orders the digits)."""
    rng = np.random.default_rng(seed)
    U = rng.standard_normal((n + 3, n + 2)) + 1j * rng.standard_normal((n + 3, n + 2))
    rows = np.stack([np.repeat(rng.choice(n + 3, len(rm), replace=False), rm) for rm, _ in patterns])
    cols = np.stack([np.repeat(rng.choice(n + 2, len(cm), replace=False), cm) for _, cm in patterns])
    return U, rows, cols


def ones(n):
    return (1,) * n


# name -> (n, [(rows multiplicities, cols multiplicities)], the (T, side, Tw, H) the shapes are chosen for)
SHAPES = {
    "n1_T1": (1, [((1,), (1,))] * 3, [(1, 0, 1, 1)] * 3),
    # one odd-radix digit: five equal columns, t' = 4
    "n5_one_group": (5, [(ones(5), (5,)), ((5,), ones(5))], [(5, 0, 1, 5), (5, 1, 1, 5)]),
    # Tw = 1 with H < 64 and H = 125 (two chunks, 61 valid lanes in the second)
    "n13_no_walk": (13, [(ones(13), (6, 6, 1)), (ones(13), (4, 4, 4, 1)), ((4, 4, 4, 1), ones(13))],
                    [(49, 0, 1, 49), (125, 0, 1, 125), (125, 1, 1, 125)]),
    # odd Tw = 5 (H = 125), Tw = 81 (H = 81), Tw = 2^10 (H = 64), one group (T = 17), side 1 with 4 chunks
    "n17_walks": (17, [(ones(17), (4, 4, 4, 4, 1)), (ones(17), (2,) * 8 + (1,)), (ones(17), ones(17)),
                       (ones(17), (17,)), ((6, 6, 5), ones(17))],
                  [(625, 0, 5, 125), (6561, 0, 81, 81), (1 << 16, 0, 1024, 64), (17, 0, 1, 17), (245, 1, 1, 245)]),
    # chunk counts 3, 5 and 6 in the fold next to one-chunk matrices; even Tw = 16 with H = 64
    "n18_folds": (18, [(ones(18), (4, 5, 5, 3, 1)), (ones(18), (18,)), (ones(18), (6, 6, 5, 1)),
                       ((9, 9), ones(18)), ((6, 6, 6), ones(18)), (ones(18), (3, 3, 3, 3, 3, 2, 1))],
                  [(720, 0, 5, 144), (18, 0, 1, 18), (294, 0, 1, 294), (90, 1, 1, 90), (294, 1, 1, 294),
                   (3072, 0, 16, 192)]),
}
_REF = {}


def case(sup, name):
    """(U, rows, cols, GPU result on one device, its stats), computed once per shape."""
    if name not in _REF:
        n, patterns, _ = SHAPES[name]
        U, rows, cols = pattern_batch(n, patterns, 5000 + n)
        v, st = sup.perman_complex_fock(U, rows, cols, return_stats=True)
        _REF[name] = (U, rows, cols, v, st)
    return _REF[name]


@pytest.mark.parametrize("name", list(SHAPES))
def test_gpu_bit_equal_to_host_twin(sup, name):
    U, rows, cols, v, st = case(sup, name)
    want = SHAPES[name][2]
    assert [plan(rows[k], cols[k]) for k in range(len(want))] == want  # the shapes are what the comment says
    assert np.array_equal(bits(v), bits(sup.perman_complex_fock(U, rows, cols, cpu=True, threads=16)))
    one = np.array([sup.perman_complex_fock(U, rows[k], cols[k]) for k in range(len(want))])
    assert np.array_equal(bits(v), bits(one))
    assert st["devices_used"] == 1 and st["leaves"] == len(want)
    assert st["visited_steps"] == sum(w[0] for w in want) and st["gray_steps"] == len(want) << (SHAPES[name][0] - 1)
    assert st["kernel_ms"] > 0 and st["wall_ms"] >= st["kernel_ms"] and st["grid"] >= 1
    assert st["est_ops_per_step"] == 6 * SHAPES[name][0]


@pytest.mark.parametrize("group", ["4", "64"])
def test_gpu_one_chunk_matrix_beside_many_chunk_matrix_in_one_queue_group(sup, monkeypatch, group):
    """Tickets of `group` chunks: the one-chunk and the 3-, 5- and 6-chunk
    matrices of n18_folds share queue groups, and the last group is partial."""
    U, rows, cols, v, _ = case(sup, "n18_folds")
    monkeypatch.setenv("SUP_WALK_GROUP", group)  # read at every call
    assert np.array_equal(bits(v), bits(sup.perman_complex_fock(U, rows, cols)))


@pytest.mark.parametrize("n", [6, 9, 13])
def test_gpu_heterogeneous_batch(sup, n):
    U, rows, cols = hetero_batch(n, 65, 800 + n)
    v = sup.perman_complex_fock(U, rows, cols)
    assert np.array_equal(bits(v), bits(sup.perman_complex_fock(U, rows, cols, cpu=True, threads=16)))


@pytest.mark.parametrize("slab", ["1", "3"])
def test_gpu_slab_boundaries(sup, monkeypatch, slab):
    U, rows, cols = hetero_batch(12, 7, 812)
    whole = sup.perman_complex_fock(U, rows, cols)
    monkeypatch.setenv("SUP_CPLX_FOCK_SLAB", slab)  # read at every call
    assert np.array_equal(bits(sup.perman_complex_fock(U, rows, cols)), bits(whole))
    assert np.array_equal(bits(whole), bits(sup.perman_complex_fock(U, rows, cols, cpu=True, threads=16)))


def test_gpu_exact_gaussian_integers(sup):
    rng = np.random.default_rng(48)
    U = gauss_int_case(6, 9)
    rows = rng.integers(0, 3, (8, 8))
    cols = rng.integers(0, 6, (8, 8))
    got = sup.perman_complex_fock(U, rows, cols)
    for k in range(8):
        assert got[k] == as_complex(exact_perm(U[np.ix_(rows[k], cols[k])])), k


# the piece fences of the column update: one piece up to 16 rows, a piece per
# plane up to 32, two passes of two pieces above; n = 64 is an instance asked
# for one wave per SIMD
@pytest.mark.parametrize("n,mult", [(16, (5, 5, 5, 1)), (17, (4, 4, 4, 4, 1)), (32, (8, 8, 8, 7, 1)),
                                    (33, (8, 8, 8, 8, 1)), (48, (12, 12, 12, 11, 1)), (49, (12, 12, 12, 12, 1)),
                                    (64, (16, 16, 16, 15, 1))])
def test_gpu_rank_one_closed_form(sup, n, mult):
    U, rows, cols, truth, scale = rank_one_case(n, mult, 700 + n)
    T, side, Tw, H = plan(rows, cols)
    v, st = sup.perman_complex_fock(U, rows, cols, return_stats=True)
    assert st["visited_steps"] == T == math.prod(t + 1 for t in mult[:-1])
    assert bits(v).tolist() == bits(sup.perman_complex_fock(U, rows, cols, cpu=True, threads=16)).tolist()
    e = err_over_scale(v, truth, scale)
    print(f"n={n} mult={mult} T={T} Tw={Tw} H={H} e_fock={e:.3e} bound={fock_bound(0.0, Tw, n):.3e}")
    assert e <= fock_bound(0.0, Tw, n)


def test_gpu_multi_device(sup):
    """gpu_num logical devices take contiguous ranges of matrices: the same bits."""
    U, rows, cols, v, _ = case(sup, "n17_walks")
    nd = sup.device_count()
    vd, sd = sup.perman_complex_fock(U, rows, cols, gpu_num=nd, return_stats=True)
    assert np.array_equal(bits(vd), bits(v))
    assert sd["devices_used"] == min(nd, len(v))
    if nd >= 2:
        v2, s2 = sup.perman_complex_fock(U, rows, cols, gpu_num=2, return_stats=True)
        assert np.array_equal(bits(v2), bits(v)) and s2["devices_used"] == 2


def test_gpu_nan_stays_in_the_results_that_gather_it(sup):
    U, rows, cols = hetero_batch(13, 65, 813)
    clean = sup.perman_complex_fock(U, rows, cols)
    dirty = U.copy()
    dirty[1, 1] = complex(1.0, np.nan)
    got = sup.perman_complex_fock(dirty, rows, cols)
    hit = np.array([1 in rows[k] and 1 in cols[k] for k in range(65)])
    assert hit.any() and not hit.all()
    assert np.array_equal(bits(got[~hit]), bits(clean[~hit]))
    assert not np.isfinite(got[hit]).any()
