"""The double-double walk on the GPU, instance by instance (walk_dd.hip through
sup_perman_quad_range): every walk_dd<N> and walk_dd_blocked<N>, N = 1 ... 64
(the one-wave-per-SIMD orders above 40 included), runs on eight wave-chunks
and returns the host twin's (hi, lo) bit for bit, and at a spread of orders the
exact rational sum of range_truth.py within the derived double-double bound
(test_quad_range.py).  Then chunk ends in rows >= 32, the planner's reported
choice and device selection.  The last test asserts that the module launched
every instance."""
import os
from contextlib import contextmanager
from fractions import Fraction

import numpy as np
import pytest

import range_truth as T

pytestmark = pytest.mark.gpu

FORMS = (1, 2)
TRUTH_N = set(range(1, 14)) | {17, 31, 32, 33, 40, 41, 48, 56, 63, 64}
EPS = Fraction(1, 1 << 103)
# (N, form) of every device launch of this module (in-process only)
LEDGER = set()


@pytest.fixture(scope="module", autouse=True)
def need_gpu(sup):
    if sup.device_count() < 1:
        pytest.fail("no HIP device visible: -m gpu tests must run on the MI355X box")


def _device(sup, a, c0, c1, **kw):
    v, info = sup.perman_quad_range(a, c0, c1, **kw)
    assert info["devices_used"] == 1 and (c0 == c1 or info["kernel_ms"] > 0)
    LEDGER.add((len(a), info["walk_kind"] + 1))
    return v, info


def _both(sup, a, c0, c1, form, **kw):
    v, info = _device(sup, a, c0, c1, form=form, **kw)
    host, hi = sup.perman_quad_range(a, c0, c1, cpu=True, form=form, **kw)
    assert info["walk_kind"] == form - 1 == hi["walk_kind"] and info["colmap"] == hi["colmap"]
    assert v == host, (len(a), form, v, host)
    return v, info


def _tol(a, info, c0, c1):
    n = len(a)
    h = n - 1 - info["L"] - info["m"]
    return T.dd_factor(n, info["m"], h) * EPS * T.dd_bound(a, T.subsets(info["L"], info["m"], c0, c1))


@pytest.mark.parametrize("n", range(1, 65))
def test_every_order_every_instance(sup, n):
    """The integer matrix of test_gpu_exact_range.py with one row scaled by 0.1,
    so the low words are live; the truth is the integer sum times the double 0.1."""
    ai = T.sparse_int_matrix(n, 300 + n)
    a = ai.astype(np.float64)
    a[n // 2] *= 0.1
    chunks = T.chunk_count(sup, n, 6)
    c0 = 0 if n <= 20 else T.scattered_start(chunks)
    c1 = min(c0 + 8, chunks)
    m = min(6, n - 1 - sup.layout(n)[0])
    truth = {}
    for form in FORMS:
        if form == 2 and m == 0:
            with pytest.raises(sup.SupError, match="form 2"):
                sup.perman_quad_range(a, c0, c1, walk_log2=6, form=2)
            continue
        v, info = _both(sup, a, c0, c1, form, walk_log2=6)
        assert info["m"] == m and info["gray_steps"] == (c1 - c0) << (info["L"] + m)
        if n in TRUTH_N:
            assert T.subsets(info["L"], m, c0, c1) <= 1 << 15
            key = tuple(info["colmap"])
            if key not in truth:
                truth[key] = Fraction(0.1) * Fraction(T.range_sum(T.doubled(ai), info["colmap"], info["L"], m, c0, c1),
                                                      1 << n)
            assert abs(Fraction(v[0]) + Fraction(v[1]) - truth[key]) <= _tol(a, info, c0, c1), form


def test_chunk_ends_in_high_rows(sup):
    """Chunk-end rows 32..35 (the high word of the zero-row mask): a range in
    which some chunks end at their first state and some are walked."""
    ai = T.chunk_end_matrix()
    a = ai.astype(np.float64)
    chunks = T.chunk_count(sup, 36, 6)
    for form in FORMS:
        _, info = sup.perman_quad_range(a, 0, 0, cpu=True, walk_log2=6, form=form)
        rows = T.chunk_end_rows(ai, info)
        assert rows[-4:] == [32, 33, 34, 35]
        c0, ended = T.mixed_window(ai, info, [32, 33, 34, 35], T.scattered_start(chunks, 1 << 16))
        assert ended == T.ended_chunks(ai, info, c0, c0 + 8, rows)  # rows below 32 hold odd values: never zero
        v, info = _both(sup, a, c0, c0 + 8, form, walk_log2=6)
        truth = Fraction(T.range_sum(T.doubled(ai), info["colmap"], 6, 6, c0, c0 + 8), 1 << 36)
        assert truth != 0 and abs(Fraction(v[0]) + Fraction(v[1]) - truth) <= _tol(a, info, c0, c0 + 8)
        for i, e in enumerate(ended):
            if e:
                assert _device(sup, a, c0 + i, c0 + i + 1, walk_log2=6, form=form)[0] == (0.0, 0.0)


def test_planner_choice_is_reported(sup):
    rng = np.random.default_rng(24)
    n = 24
    a = np.where(rng.random((n, n)) < 0.12, rng.integers(1, 4, (n, n)), 0).astype(np.int32)
    a[np.arange(n), rng.permutation(n)] = 1
    for cpu in (False, True):
        got, st = sup.perman_quad(a, cpu=cpu, return_stats=True)
        assert st["walk_kind"] == 1 and 0 < st["est_ops_per_step"] < 16 * n + 13, st
        assert (st["lane_bits"], st["walk_bits"]) == sup.layout(n)[:2]
        _, st1 = sup.perman_quad(np.ones((20, 20)), cpu=cpu, return_stats=True)
        assert st1["walk_kind"] == 0 and st1["est_ops_per_step"] == 16 * 20 + 13, st1
    # form 0 of the range entry is that planner: the whole range scaled is the whole call
    v, info = _device(sup, a, 0, T.chunk_count(sup, n))
    assert info["walk_kind"] == 1 and (-2.0 * v[0], -2.0 * v[1]) == got
    assert Fraction(got[0]) + Fraction(got[1]) == sup.perman_exact(a)


@contextmanager
def device_map(spec):
    old = os.environ.get("SUP_DEVICE_MAP")
    os.environ["SUP_DEVICE_MAP"] = spec
    try:
        yield
    finally:
        if old is None:
            del os.environ["SUP_DEVICE_MAP"]
        else:
            os.environ["SUP_DEVICE_MAP"] = old


def test_device_selection(sup):
    """The range entries run on one device, sup_opts.device_id: every visible
    device, and a second logical device on GPU 0, return the same bits."""
    a = T.sparse_int_matrix(21, 321) * 0.1
    want, _ = sup.perman_quad_range(a, 5, 13, cpu=True, walk_log2=6)
    for d in range(sup.device_count()):
        assert _device(sup, a, 5, 13, walk_log2=6, device_id=d)[0] == want
    with device_map("0,0"):
        assert sup.device_count() == 2
        assert _device(sup, a, 5, 13, walk_log2=6, device_id=1)[0] == want
        with pytest.raises(sup.SupError, match="device_id"):
            sup.perman_quad_range(a, 5, 13, walk_log2=6, device_id=2)


def test_every_instance_was_launched(sup):
    """Runs last: the launches above cover walk_dd<N> and walk_dd_blocked<N>
    for every N, but for the blocked kernel at N <= 7, which has no walk bits
    and is refused."""
    want = {(n, form) for n in range(1, 65) for form in FORMS if not (form == 2 and n <= 7)}
    assert len(want) == 128 - 7
    assert want - LEDGER == set()
