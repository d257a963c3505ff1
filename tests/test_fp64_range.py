"""The truth and the tolerance of the per-order fp64 tests, shown sound without
a GPU: for every order 2 ... 64, both matrix flavours and the windows of
fp64_range_truth.py, the oracle's mirrors of the plain dense, prefix-blocked
and SkipPer walks (orc.engine_range, the sums the kernels return bit for bit)
and the complex walk's host twin lie within F 2^-53 S of the exact sum.  Once
per kind the reference's own chunk helpers, restated in the oracle, land on the
same truth: that pins the Gray index, sign and p0 conventions.  The last test
prints the worst |err| / (2^-53 S) per kind.

The integer flavour holds negative entries; sup_partial and the mirrors take
them for every kernel, so no |a| is needed for the prefix-blocked and SkipPer
walks."""
from fractions import Fraction

import pytest

import complex_range_truth as CT
import fp64_range_truth as R

THREADS = 8
# kind -> (worst ratio, (n, flavour, window)); filled by the tests below
WORST = {}


def complex_within(got, tr, ti, scale, n):
    L, m, chunks = R.layout(n)
    tol = CT.factor(n, m, chunks.bit_length() - 1) * R.EPS * scale
    return abs(Fraction(got.real) - tr) <= tol and abs(Fraction(got.imag) - ti) <= tol


def complex_ratio(got, tr, ti, scale):
    return max(R.ratio(got.real, tr, scale), R.ratio(got.imag, ti, scale))


def test_truth_helpers_agree_with_range_truth():
    """The second accumulator changes nothing in the first; S >= |sum|."""
    import range_truth as T
    for n in (2, 9, 14, 17):
        L, m, _ = R.layout(n)
        cm = list(range(n - 1))
        for flavour, make in R.FLAVOURS:
            for c0, c1 in R.windows(n):
                total, scale = R.range_sum_abs_float(make(n), cm, L, m, c0, c1)
                assert total == T.range_sum_float(make(n), cm, L, m, c0, c1) and scale >= abs(total) and scale > 0
        a = R.complex_matrix(n)
        for c0, c1 in R.windows(n):
            tr, ti, scale = CT.range_sum_abs_float(a, L, m, c0, c1)
            assert (tr, ti) == CT.range_sum_float(a, L, m, c0, c1) and scale >= abs(tr) + abs(ti) and scale > 0


def test_windows():
    assert R.windows(13) == [(0, 1)] and R.windows(16) == [(0, 8)] and R.windows(17) == [(0, 8), (8, 16)]
    w = R.windows(64)
    assert w[0] == (0, 8) and w[2] == ((1 << 51) - 8, 1 << 51) and w[0][1] < w[1][0] < w[1][1] < w[2][0]
    for n in range(2, 65):
        L, m, chunks = R.layout(n)
        assert all(0 <= c0 < c1 <= chunks and ((c1 - c0) << (L + m)) <= 1 << 15 for c0, c1 in R.windows(n))
        assert R.factor(n) * float(R.EPS) < 5e-13


@pytest.mark.parametrize("n", range(2, 65))
def test_mirrors_within_tolerance_of_truth(orc, n):
    L, m, _ = R.layout(n)
    for flavour, _ in R.FLAVOURS:
        for c0, c1 in R.windows(n):
            a, total, scale = R.truth(n, flavour, c0, c1)
            for kind in ("dense", "sparse", "skip"):
                got, _ = orc.engine_range(a, kind, c0, c1, L, m, None, THREADS)
                R.note(kind, R.ratio(got, total, scale), (n, flavour, (c0, c1)), WORST)
                assert R.within(got, total, scale, n), (kind, flavour, (c0, c1), got, float(total))


@pytest.mark.parametrize("n", range(2, 65))
def test_complex_twin_within_tolerance_of_truth(sup, n):
    L, m, _ = R.layout(n)
    a = R.complex_matrix(n)
    for c0, c1 in R.windows(n):
        tr, ti, scale = CT.range_sum_abs_float(a, L, m, c0, c1)
        got, st = sup.perman_complex_range(a, c0, c1, cpu=True, threads=THREADS, walk_log2=R.WALK_LOG2,
                                           return_stats=True)
        assert (st["lane_bits"], st["walk_bits"], st["gray_steps"]) == (L, m, (c1 - c0) << (L + m))
        R.note("complex twin", complex_ratio(got, tr, ti, scale), (n, "complex", (c0, c1)), WORST)
        assert complex_within(got, tr, ti, scale, n), ((c0, c1), got, float(tr), float(ti))


@pytest.mark.parametrize("kind", ["dense", "sparse", "skip"])
def test_reference_helpers_land_on_the_truth(orc, kind):
    """The reference's chunk helpers over the Gray indices [s, e) of a window
    (they leave index 0, the p0 term, to their caller).  They add their terms
    one after another and the sparse ones keep the product incrementally, so a
    term passes at most n^2 + 2n roundings of its own and 4 per Gray step of
    the range: F_ref = n^2 + 2n + 4 (e - s), below 2e-11 S where a wrong term
    is 2^-15 S."""
    fn = {"dense": orc.ref_dense_partial, "sparse": orc.ref_sparse_partial, "skip": orc.ref_skip_partial}[kind]
    for n in (9, 16, 22):
        for flavour, _ in R.FLAVOURS:
            for c0, c1 in R.windows(n):
                a, total, scale = R.truth(n, flavour, c0, c1)
                s, e = R.gray_range(n, c0, c1)
                got = Fraction(fn(a, max(s, 1), e, 1))
                if s == 0:
                    got += Fraction(orc.nw_start(a)[1])
                f_ref = n * n + 2 * n + 4 * (e - s)
                assert f_ref * R.EPS < Fraction(1, 1 << 20) * Fraction(1, 1 << 15)
                assert abs(got - total) <= f_ref * R.EPS * scale, (n, flavour, (c0, c1))
                # and the engine's mirror of the same range is the same sum
                L, m, _ = R.layout(n)
                mir, _ = orc.engine_range(a, kind, c0, c1, L, m, None, THREADS)
                assert R.within(mir, total, scale, n)


def test_print_worst_ratios(capsys):
    """Runs last: the worst |err| / (2^-53 S) per kind over the tests above."""
    assert all(0.0 <= ratio <= CT.factor(64, 6, 51) for ratio, _ in WORST.values())
    with capsys.disabled():
        print()
        for kind, (ratio, where) in sorted(WORST.items()):
            print(f"fp64 range, CPU, {kind}: worst |err| / (2^-53 S) = {ratio:.3f} at (n, flavour, window) = {where}")
