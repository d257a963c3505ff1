"""The collision-aware one-walk minors on the GPU (walk_cplxfm.hip and
cplx_fock.hip's prepare and fold through sup_perman_complex_fock_minors):
result (k, j) has the bits of the host twin for any slab size, queue group
and device count.  Every comparison is device against host twin, bit for bit,
as uint64 pairs.  (T, Tw, H) by test_complex_fock.layout's restatement of the
rule; every docstring states its own."""
import numpy as np
import pytest

from test_complex_batch import bits
from test_complex_fock import groups, layout

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def need_gpu(sup):
    if sup.device_count() < 1:
        pytest.fail("no HIP device visible: -m gpu tests must run on the MI355X box")


_U = {}


def unitary():
    """One 32 x 32 complex matrix for every case."""
    if not _U:
        rng = np.random.default_rng(1700)
        _U[0] = rng.standard_normal((32, 32)) + 1j * rng.standard_normal((32, 32))
    return _U[0]


def lists(n, mults, seed):
    """One (rows, cols) pair per multiplicity vector in `mults` (each sums to
    n - 1, in order of first appearance): n distinct rows, random distinct
    column values."""
    rng = np.random.default_rng(seed)
    rows = np.array([rng.permutation(32)[:n] for _ in mults])
    cols = np.array([np.repeat(rng.choice(32, size=len(m), replace=False), m) for m in mults]).reshape(len(mults), n - 1)
    return rows, cols


def fours(q):
    """q columns in groups of four, the remainder as a smaller last group."""
    return (4,) * (q // 4) + ((q % 4,) if q % 4 else ())


_REF = {}


def both(sup, key, rows, cols, **kw):
    """(device result, host twin's result); the twin's computed once per key."""
    if key not in _REF:
        _REF[key] = sup.perman_complex_fock_minors_submatrices(unitary(), rows, cols, cpu=True, threads=16)
    return sup.perman_complex_fock_minors_submatrices(unitary(), rows, cols, **kw), _REF[key]


@pytest.mark.parametrize("n", range(2, 33))
def test_gpu_bit_equal_to_host_twin_in_groups_of_four(sup, n):
    """Count 3, the q columns in groups of four.  (T, Tw, H): n <= 15: Tw = 1,
    H = T = 1, 2, 3, 4, 5, 10, 15, 20, 25, 50, 75, 100, 125, 250; n = 16: (375,
    5, 75); 17: (500, 4, 125); 18: (625, 5, 125); 19: (1250, 5, 250); 20: (1875,
    25, 75); 21: (2500, 20, 125); 22: (3125, 25, 125); 23: (6250, 25, 250); 24:
    (9375, 125, 75); 25: (12500, 100, 125); 26: (15625, 125, 125); 27: (31250,
    125, 250); 28: (46875, 625, 75); 29: (62500, 500, 125); 30: (78125, 625,
    125); 31: (156250, 625, 250); 32: (234375, 625, 375)."""
    rows, cols = lists(n, [fours(n - 1)] * 3, 9000 + n)
    got, want = both(sup, ("fours", n), rows, cols, return_stats=True)
    got, st = got
    assert got.shape == (3, n) and st["devices_used"] == 1
    assert st["visited_steps"] == 3 * layout(groups(cols[0]))[0] and st["est_ops_per_step"] == 16 * n - 20
    assert np.array_equal(bits(got), bits(want))


# name: (n, multiplicity vectors)
SHAPES = {
    "all_distinct_18": (18, [(1,) * 17] * 2),                  # T = 2^16, Tw = 2^10, H = 64
    "t_is_one": (2, [(1,)] * 5),                               # T = 1: no walk, no digit
    "one_odd_radix_digit": (4, [(3,)] * 3),                    # T = 3 = H, Tw = 1
    "tw1_odd_and_even": (6, [(5,), (4, 1), (3, 2), (2, 2, 1)]),  # T = 5, 5, 8, 9; Tw = 1, H = T < 64
    "two_chunks_h125": (17, [(4, 4, 4, 4)] * 3),               # T = 500, Tw = 4, H = 125: two chunks, the second 61 lanes
    # chunks 1..6 in one call (H = 16, 66, 132, 196, 264, 324 at Tw = 1), next to
    # (4,4,4,4) (Tw = 4, H = 125) and all distinct (T = 2^15, Tw = 512, H = 64)
    "fold_counts": (17, [(16,), (10, 6), (3, 3, 10), (1,) * 16, (4, 6, 6), (10, 1, 1, 2, 1, 1), (16,),
                         (8, 2, 3, 2, 1), (4, 4, 4, 4), (10, 6)]),
    "count_7": (13, [(4, 4, 4), (12,), (1,) * 12, (6, 6), (2,) * 6, (3, 3, 3, 3), (11, 1)]),
}


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_gpu_layout_paths(sup, name):
    """(T, Tw, H) per shape: the comments at SHAPES; checked here against the rule."""
    n, mults = SHAPES[name]
    rows, cols = lists(n, mults, 9100 + n)
    if name == "all_distinct_18":
        assert layout(groups(cols[0])) == (1 << 16, 1 << 10, 64)
    if name == "two_chunks_h125":
        assert layout(groups(cols[0])) == (500, 4, 125)
    if name == "fold_counts":
        assert sorted({(layout(groups(c))[2] + 63) // 64 for c in cols}) == [1, 2, 3, 4, 5, 6]
    got, want = both(sup, name, rows, cols)
    assert np.array_equal(bits(got), bits(want))


@pytest.mark.parametrize("group", ["4", "64"])
@pytest.mark.parametrize("name", ["fold_counts", "tw1_odd_and_even", "all_distinct_18"])
def test_gpu_forced_queue_group(sup, monkeypatch, name, group):
    """(T, Tw, H): the comments at SHAPES."""
    n, mults = SHAPES[name]
    rows, cols = lists(n, mults, 9100 + n)
    monkeypatch.setenv("SUP_WALK_GROUP", group)  # read at every call
    got, want = both(sup, name, rows, cols)
    assert np.array_equal(bits(got), bits(want))


@pytest.mark.parametrize("slab", ["1", "3"])
def test_gpu_slabs_of_1_and_3_on_count_7(sup, monkeypatch, slab):
    """n = 13, seven patterns: (T, Tw, H) = (100, 1, 100), (12, 1, 12), (2^11, 32,
    64), (42, 1, 42), (486, 6, 81), (192, 3, 64), (12, 1, 12)."""
    n, mults = SHAPES["count_7"]
    rows, cols = lists(n, mults, 9100 + n)
    monkeypatch.setenv("SUP_CPLX_FOCK_MINORS_SLAB", slab)  # read at every call
    got, want = both(sup, "count_7", rows, cols)
    assert np.array_equal(bits(got), bits(want))


@pytest.mark.parametrize("name", ["fold_counts", "count_7", "t_is_one"])
def test_gpu_all_devices(sup, name):
    """(T, Tw, H): the comments at SHAPES."""
    n, mults = SHAPES[name]
    rows, cols = lists(n, mults, 9100 + n)
    nd = sup.device_count()
    got, want = both(sup, name, rows, cols, gpu_num=nd, return_stats=True)
    got, st = got
    assert np.array_equal(bits(got), bits(want))
    assert st["devices_used"] == min(nd, len(mults))


def test_gpu_nan_stays_in_its_own_matrix(sup):
    """n = 17, the fold_counts patterns (chunks 1..6; Tw = 1, 4, 512).  The
    minor without the poisoned row keeps its clean bits."""
    n, mults = SHAPES["fold_counts"]
    rows, cols = lists(n, mults, 9100 + n)
    U = unitary()
    # a private copy of U's rows for matrix 4: rows 32.. of a taller U, poisoned in one place
    tall = np.concatenate([U, U], axis=0)
    clean = sup.perman_complex_fock_minors_submatrices(tall, rows, cols, cpu=True, threads=16)
    assert np.array_equal(bits(clean), bits(sup.perman_complex_fock_minors_submatrices(U, rows, cols, cpu=True)))
    r2 = rows.copy()
    r2[4] += 32
    tall[r2[4, 5], cols[4, 0]] = complex(1.0, np.nan)
    got = sup.perman_complex_fock_minors_submatrices(tall, r2, cols)
    keep = [k for k in range(len(mults)) if k != 4]
    assert np.array_equal(bits(got[keep]), bits(clean[keep]))
    assert not np.isfinite(np.delete(got[4], 5)).any()
    assert np.array_equal(bits(got[4, 5]), bits(clean[4, 5]))


@pytest.mark.parametrize("name", ["fold_counts", "count_7", "all_distinct_18"])
def test_gpu_stats(sup, name):
    """visited_steps = sum of the plan entry's T; (T, Tw, H): the comments at SHAPES."""
    n, mults = SHAPES[name]
    rows, cols = lists(n, mults, 9100 + n)
    (_, st), _ = both(sup, name, rows, cols, return_stats=True)
    assert st["visited_steps"] == int(sup.perman_complex_fock_minors_plan(cols).sum())
    assert st["est_ops_per_step"] == 16 * n - 20
    assert st["leaves"] == len(mults) * n and st["gray_steps"] == len(mults) << (n - 2)
    assert st["kernel_ms"] > 0 and st["wall_ms"] >= st["kernel_ms"] and st["grid"] >= 1
