"""The fp64 walks on the GPU, instance by instance (walk_dense.hip,
walk_sparse.hip, walk_skip.hip and walk_lds.hip through sup_partial): every
walk_dense<N>, walk_sparse<N>, walk_skip<N> and walk_lds<N>, N = 2 ... 64, runs
on windows of eight wave-chunks of two matrices (fp64_range_truth.py: integers
in {-1, 1, 2}, and dyadic k / 8) and returns

* the bits of the oracle's mirror of the engine schedule (plain dense,
  prefix-blocked, SkipPer; the LDS walk returns the plain dense walk's bits),
* a value within F 2^-53 S of the exact sum in Python integers, S the exact sum
  of |term| (the derivation: fp64_range_truth.py; soundness without a GPU:
  test_fp64_range.py).

The integer flavour's negative entries are taken by every kernel as they are.
The segmented walk (a hiprtc compile per pattern) runs at a spread of orders;
then chunk ends of the prefix-blocked walk in rows >= 32.  The last tests assert
that the module launched every instance and print the worst |err| / (2^-53 S)
per kernel."""
import numpy as np
import pytest

import fp64_range_truth as R
import range_truth as T

pytestmark = pytest.mark.gpu

# (N, walk_kind) of every device launch of this module (in-process only)
LEDGER = set()
# kernel -> (worst ratio, (n, flavour, window)) on the device; "mirror ...": the CPU mirror on the same inputs
WORST = {}


@pytest.fixture(scope="module", autouse=True)
def need_gpu(sup):
    if sup.device_count() < 1:
        pytest.fail("no HIP device visible: -m gpu tests must run on the MI355X box")


def _partial(sup, a, n, c0, c1, kernel, kind):
    """sup_partial over the window's Gray indices: the kernel and the layout
    that were asked for ran on one device."""
    s, e = R.gray_range(n, c0, c1)
    L, m, _ = R.layout(n)
    v, st = sup.partial(a, s, e, kernel=kernel, walk_log2=R.WALK_LOG2, return_stats=True)
    assert st["walk_kind"] == kind and st["gray_steps"] == (c1 - c0) << (L + m) == e - s, (kernel, st)
    assert (st["lane_bits"], st["walk_bits"]) == (L, m) and st["devices_used"] == 1 and st["kernel_ms"] > 0
    LEDGER.add((n, st["walk_kind"]))
    return v, st


@pytest.mark.parametrize("n", range(1, 65))
def test_every_order_every_instance(sup, orc, n):
    if n == 1:  # no flippable column, no range: the permanent is the entry
        for _, make in R.FLAVOURS:
            a = make(1)
            for kernel, _ in R.KERNELS:
                assert sup.perman(a, kernel=kernel) == a[0, 0] != 0
        return
    L, m, _ = R.layout(n)
    for flavour, _ in R.FLAVOURS:
        for c0, c1 in R.windows(n):
            a, total, scale = R.truth(n, flavour, c0, c1)
            where = (n, flavour, (c0, c1))
            got = {}
            for kernel, kind in R.KERNELS:
                got[kernel], _ = _partial(sup, a, n, c0, c1, kernel, kind)
                if kernel in R.MIRROR:
                    mir, _ = orc.engine_range(a, R.MIRROR[kernel], c0, c1, L, m, None, 16)
                    R.note("mirror " + kernel, R.ratio(mir, total, scale), where, WORST)
                    assert got[kernel] == mir, (kernel, where, got[kernel], mir)
                else:
                    assert got[kernel] == got["dense_plain"], (kernel, where)
                R.note(kernel, R.ratio(got[kernel], total, scale), where, WORST)
                assert R.within(got[kernel], total, scale, n), (kernel, where, got[kernel], float(total))


def _scattered_window(n):
    chunks = R.layout(n)[2]
    c0 = T.scattered_start(chunks, R.WINDOW)
    return c0, min(c0 + R.WINDOW, chunks)


@pytest.mark.parametrize("n", R.SEG_ORDERS)
def test_segmented_walk_spread(sup, orc, n):
    """The pattern-specialised walk on the dyadic flavour's scattered window:
    the bits of the mirror run with the plan's reported cached and pair bits,
    within the tolerance of the truth."""
    L, m, _ = R.layout(n)
    c0, c1 = _scattered_window(n)
    a, total, scale = R.truth(n, "dyadic", c0, c1)
    got, st = _partial(sup, a, n, c0, c1, "seg", 3)
    mir, _ = orc.engine_range(a, "seg", c0, c1, L, m, None, 16, st["seg_cached_bits"], st["seg_pair_bits"])
    assert got == mir, (n, got, mir, st["seg_cached_bits"], st["seg_pair_bits"])
    R.note("seg", R.ratio(got, total, scale), (n, "dyadic", (c0, c1)), WORST)
    assert R.within(got, total, scale, n), (n, got, float(total))


def _chunk_end_case():
    """T.chunk_end_matrix() under sup_partial's identity column map: the
    chunk-end rows are those no column below L + m = 12 touches; a window of
    eight chunks of which some end at their first state and some are walked."""
    ai = T.chunk_end_matrix()
    n = len(ai)
    L, m, chunks = R.layout(n)
    info = {"colmap": list(range(n - 1)), "L": L, "m": m}
    rows = T.chunk_end_rows(ai, info)
    assert rows and rows[-4:] == [32, 33, 34, 35]
    c0, ended = T.mixed_window(ai, info, [32, 33, 34, 35], T.scattered_start(chunks, 1 << 16))
    assert ended == T.ended_chunks(ai, info, c0, c0 + 8, rows)  # rows below 32 hold odd values: never zero
    assert any(ended) and not all(ended)
    return ai.astype(np.float64), n, c0, ended


def test_chunk_ends_in_high_rows(sup, orc):
    """Chunk-end rows 32..35 (the high word of the zero-row mask) in the
    prefix-blocked fp64 walk: the window's partial is the mirror's and within
    the tolerance of the truth, and each ended chunk alone is exactly 0.0."""
    a, n, c0, ended = _chunk_end_case()
    L, m, _ = R.layout(n)
    got, _ = _partial(sup, a, n, c0, c0 + 8, "sparse", 1)
    mir, _ = orc.engine_range(a, "sparse", c0, c0 + 8, L, m, None, 16)
    assert got == mir
    total, scale = R.range_sum_abs_float(a, list(range(n - 1)), L, m, c0, c0 + 8)
    assert total != 0 and R.within(got, total, scale, n)
    R.note("sparse", R.ratio(got, total, scale), (n, "chunk ends", (c0, c0 + 8)), WORST)
    for i, e in enumerate(ended):
        if e:
            assert _partial(sup, a, n, c0 + i, c0 + i + 1, "sparse", 1)[0] == 0.0


def test_chunk_ends_visited_steps(sup):
    """The window's visited_steps counts only the chunks that were walked (7
    of its 8 chunks end, 1 is walked), and so does each chunk's alone.  An
    ended chunk and a chunk walked over its exact-zero terms return the same
    0.0: this count, which walk_sparse<N> takes where a chunk ends, is what
    shows that rows >= 32 of the chunk-end mask ended their chunks."""
    a, n, c0, ended = _chunk_end_case()
    L, m, _ = R.layout(n)
    _, st = _partial(sup, a, n, c0, c0 + 8, "sparse", 1)
    print("visited_steps", st["visited_steps"], "walked chunks", ended.count(False), "of", len(ended))
    assert st["visited_steps"] == ended.count(False) << (L + m)
    for i, e in enumerate(ended):
        _, st = _partial(sup, a, n, c0 + i, c0 + i + 1, "sparse", 1)
        assert st["visited_steps"] == (0 if e else 1 << (L + m)), (i, e, st["visited_steps"])


def test_every_instance_was_launched(sup):
    """Runs last: the launches above cover walk_dense<N>, walk_sparse<N>,
    walk_skip<N> and walk_lds<N> for every N in 2 ... 64 (N = 1 has no range)."""
    want = {(n, kind) for n in range(2, 65) for _, kind in R.KERNELS}
    assert len(want) == 252
    assert want - LEDGER == set()
    assert {(n, 3) for n in R.SEG_ORDERS} <= LEDGER


def test_print_worst_ratios(capsys):
    assert all(0.0 <= ratio <= R.factor(64) for ratio, _ in WORST.values())
    with capsys.disabled():
        print()
        for kind, (ratio, where) in sorted(WORST.items()):
            print(f"fp64 range, GPU, {kind}: worst |err| / (2^-53 S) = {ratio:.3f} at (n, flavour, window) = {where}")
