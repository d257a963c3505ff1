"""Specialised high-bit steps of the segmented walk (jit.cpp Gen::hi_loop:
the kernel's outer q loop unrolled by 2^u, SUP_JIT_HI forces u) and the op
census of the generated code (sup_plan_census).

No device: the census classes add up to est_ops_per_step exactly and do not
grow with u, every u's kernel compiles for gfx950 (the clamp cases too), and
the host twin, which restates no u, stays bit-equal to the oracle's mirror.
On the GPU: the permanents of u = 0..3 are bit-equal to each other and to the
mirror, on a real matrix and on an integer matrix whose plan skips chunks
(equal visited counts), and two shards at u = 2 sum to the one-launch value.

n = 28 with SUP_JIT_B=3 has 8 walk bits: 16 blocks of 2^3 pair steps per
wave-chunk, so walk bits b+1 .. b+4 all occur and u = 3 leaves a generic step."""
import struct

import numpy as np
import pytest

from conftest import fixture_path

N = 28


def _real():
    rng = np.random.default_rng(281)
    a = np.where(rng.random((N, N)) < 0.5, rng.random((N, N)) * 5, 0.0)
    a[np.arange(N), rng.permutation(N)] = 1.0 + rng.random(N)
    return a


def _int():
    """Integer entries in -3..3, d = 0.3: rows untouched by the walk are exactly
    zero in every lane of about half the wave-chunks, which the kernel skips."""
    rng = np.random.default_rng(47)
    mask = rng.random((N, N)) < 0.3
    mask[np.arange(N), rng.permutation(N)] = True
    a = np.where(mask, rng.integers(-3, 4, (N, N)), 0).astype(np.float64)
    a[(a == 0) & mask] = 1.0
    return a


def _bits(v):
    return struct.pack("<d", v)  # == treats -0.0 and +0.0 alike; the bytes do not


def _total(cen):
    t = 0.0
    for v in cen["classes"].values():  # index order, as the library adds them
        t += v
    return t


@pytest.fixture(scope="module")
def mirror(sup, orc):
    """The oracle mirror's permanents of the two n = 28 matrices (b = 3), once."""
    mp = pytest.MonkeyPatch()
    mp.setenv("SUP_JIT_B", "3")
    try:
        return {"real": orc.engine_perman_as(sup, _real(), "seg", threads=16),
                "int": orc.engine_perman_as(sup, _int(), "seg", threads=16)}
    finally:
        mp.undo()


def test_census_sums_to_est_ops_n28(sup, monkeypatch):
    monkeypatch.setenv("SUP_JIT_B", "3")
    a = _real()
    totals = []
    for u in (0, 1, 2, 3):
        monkeypatch.setenv("SUP_JIT_HI", str(u))
        info, cen = sup.plan_info(a, "seg"), sup.plan_census(a, "seg")
        assert info["m"] == 8 and info["pair_bits"] == 3 and cen["hi_bits"] == u
        assert list(cen["classes"]) == list(sup.CENSUS_CLASSES)
        assert all(v >= 0.0 for v in cen["classes"].values()) and cen["chunk_start"] > 0.0
        assert _total(cen) == info["est_ops_per_step"], u
        hi = cen["classes"]["hi_adds"] + cen["classes"]["hi_copies"] + cen["classes"]["hi_forms"]
        assert (hi > 0.0) == (u > 0)
        totals.append(info["est_ops_per_step"])
    # non-increasing in u (and the walk order, layout and cached bits never move)
    assert all(totals[i + 1] <= totals[i] for i in range(3)), totals
    assert totals[3] < totals[0]


def test_census_bench_plan(sup, tmp_path, monkeypatch):
    """The bench matrix's plan (budget pinned: no compiler check): the classes
    add up exactly and the total does not grow with u (0, the 1 the plan takes
    on MI355X, and 3; each u is a fresh walk-order search of ~3 s)."""
    monkeypatch.setenv("SUP_JIT_CACHE_DIR", str(tmp_path))
    monkeypatch.setenv("SUP_JIT_BUDGET", "190")
    a, _, _ = sup.read_matrix(fixture_path("double__40_0.50_0"))
    totals, maps = [], []
    for u in (0, 1, 3):
        monkeypatch.setenv("SUP_JIT_HI", str(u))
        info, cen = sup.plan_info(a, "dense", jit=1), sup.plan_census(a, "dense", jit=1)
        assert info["kind"] == "seg" and cen["hi_bits"] == u
        assert _total(cen) == info["est_ops_per_step"], u
        totals.append(info["est_ops_per_step"])
        maps.append((info["colmap"].tolist(), info["m"], info["cached"], info["pair_bits"]))
    assert all(totals[i + 1] <= totals[i] for i in range(2)), totals
    assert all(m == maps[0] for m in maps)


def test_census_of_other_walks_is_zero(sup):
    cen = sup.plan_census(_real(), "dense", jit=-1)
    assert cen["hi_bits"] == 0 and _total(cen) == 0.0 and cen["chunk_start"] == 0.0


@pytest.mark.parametrize("b,u,want", [(3, 0, 0), (3, 1, 1), (3, 2, 2), (3, 3, 3),
                                      (4, 3, 3),   # m - 1 - b == u: the generic step never runs
                                      (6, 3, 1)])  # m - 1 - b < u: clamped
def test_generated_kernel_compiles_for_each_u(sup, tmp_path, monkeypatch, b, u, want):
    monkeypatch.setenv("SUP_JIT_CACHE_DIR", str(tmp_path))
    monkeypatch.setenv("SUP_JIT_B", str(b))
    monkeypatch.setenv("SUP_JIT_HI", str(u))
    a = _real()
    assert sup.plan_info(a, "seg")["m"] == 8
    assert sup.plan_census(a, "seg")["hi_bits"] == want
    info = sup.prepare(a, "seg")
    assert info["kind"] == "seg" and info["compile_ms"] > 0.0
    assert len(list(tmp_path.glob("seg_*.co"))) == 1


def test_plan_key_follows_u(sup, monkeypatch):
    monkeypatch.setenv("SUP_JIT_B", "3")
    a = _real()
    keys = set()
    for u in (0, 1, 2, 3):
        monkeypatch.setenv("SUP_JIT_HI", str(u))
        keys.add(sup.plan_key(a, "seg"))
    assert len(keys) == 4


def test_negative_zero_start_keeps_plain_loop(sup, monkeypatch):
    """A start value of -0 (a -0.0 in the last column of a row that sums to
    zero): adding a +0 would turn it into +0, so the steps that leave such adds
    out are not generated."""
    monkeypatch.setenv("SUP_JIT_B", "3")
    monkeypatch.setenv("SUP_JIT_HI", "2")
    a = _int()
    a[5, :] = 0.0
    a[5, 0], a[5, 1], a[5, N - 1] = 2.0, -2.0, -0.0
    assert sup.plan_census(a, "seg")["hi_bits"] == 0
    a[5, N - 1] = 0.0
    assert sup.plan_census(a, "seg")["hi_bits"] == 2


def test_host_twin_does_not_depend_on_u(sup, mirror, monkeypatch):
    monkeypatch.setenv("SUP_JIT_B", "3")
    a = _real()
    for u in (0, 3):
        monkeypatch.setenv("SUP_JIT_HI", str(u))
        assert _bits(sup.perman_cpu(a, "seg", threads=16)) == _bits(mirror["real"]), u


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["real", "int"])
def test_gpu_every_u_bit_equal(sup, mirror, monkeypatch, which):
    if sup.device_count() < 1:
        pytest.fail("no HIP device visible: -m gpu tests must run on the MI355X box")
    monkeypatch.setenv("SUP_JIT_B", "3")
    a = _real() if which == "real" else _int()
    got, visited = [], []
    for u in (0, 1, 2, 3):
        monkeypatch.setenv("SUP_JIT_HI", str(u))
        assert sup.plan_census(a, "seg")["hi_bits"] == u
        v, st = sup.perman(a, algo=4, kernel="seg", return_stats=True)
        assert st["walk_kind"] == 3 and st["gray_steps"] == 2 ** (N - 1)
        got.append(_bits(v))
        visited.append(st["visited_steps"])
    assert got == [_bits(mirror[which])] * 4, (which, got)
    assert len(set(visited)) == 1
    if which == "real":
        assert visited[0] == 2 ** (N - 1)
    else:  # the plan skips chunks
        assert 0 < visited[0] < 2 ** (N - 1)


@pytest.mark.gpu
def test_gpu_two_shards_at_u2(sup, monkeypatch):
    """Shards are runs of whole wave-chunks and q restarts at 0 in each chunk,
    so a shard boundary never falls inside an unrolled body."""
    if sup.device_count() < 1:
        pytest.fail("no HIP device visible: -m gpu tests must run on the MI355X box")
    monkeypatch.setenv("SUP_JIT_B", "3")
    monkeypatch.setenv("SUP_JIT_HI", "2")
    a = _real()
    full = sup.perman_shard(a, 0, 1, kernel="seg")
    parts = [sup.perman_shard(a, r, 2, kernel="seg") for r in range(2)]
    assert _bits(parts[0] + parts[1]) == _bits(full)
    monkeypatch.setenv("SUP_JIT_HI", "0")
    assert _bits(sup.perman_shard(a, 0, 1, kernel="seg")) == _bits(full)
