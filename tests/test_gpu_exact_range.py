"""The residue walk on the GPU, instance by instance (walk_exact.hip through
sup_perman_exact_range): every walk_exact<N, G> and walk_exact_blocked<N, G>,
N = 1 ... 64, G = 1, 2, 4, runs on eight wave-chunks and returns the host
twin's residues (the twin always runs a G = 1 chain, so the grouped products,
their tails and the block chains are checked against another operation
order), and at a spread of orders the Python-integer sum of range_truth.py.
Then the edges: the exactness budget G xbits + pbits <= 51 driven to its limit
for each G, the 256-step accumulator fold, chunk ends in rows >= 32, the
planner's reported choice, and device selection.  The last test asserts that
the module launched every instance."""
import os
from contextlib import contextmanager

import numpy as np
import pytest

import range_truth as T

pytestmark = pytest.mark.gpu

FORMS = (1, 2)
GROUPS = (1, 2, 4)
TRUTH_N = set(range(1, 14)) | {17, 31, 32, 33, 40, 41, 48, 56, 63, 64}
# (N, form, G) of every device launch of this module (in-process only)
LEDGER = set()


@pytest.fixture(scope="module", autouse=True)
def need_gpu(sup):
    if sup.device_count() < 1:
        pytest.fail("no HIP device visible: -m gpu tests must run on the MI355X box")


def _device(sup, a, c0, c1, **kw):
    res, info = sup.perman_exact_range(a, c0, c1, **kw)
    assert info["devices_used"] == 1 and (c0 == c1 or info["kernel_ms"] > 0)
    LEDGER.add((len(a), info["walk_kind"] + 1, info["G"]))
    return res, info


def _both(sup, a, c0, c1, form, group, **kw):
    """Device and host twin: same primes (all of them), same residues, the
    kernel and G that were asked for."""
    res, info = _device(sup, a, c0, c1, form=form, group=group, **kw)
    host, hi = sup.perman_exact_range(a, c0, c1, cpu=True, form=form, group=group, **kw)
    assert (info["walk_kind"], info["G"]) == (form - 1, group) == (hi["walk_kind"], hi["G"])
    assert info["primes"] == hi["primes"] and info["colmap"] == hi["colmap"]
    assert len(res) == len(info["primes"]) and res == host, (len(a), form, group)
    return res, info


def _prime_count(a, group):
    """Primes the walk of `a` needs with groups of `group` rows (include/superman.h)."""
    rowabs = np.abs(np.asarray(a, dtype=np.int64)).sum(1)
    pbits = min(42, 51 - group * int(rowabs.max()).bit_length())
    need = len(a) - 1 + float(np.log2(rowabs.astype(np.float64)).sum()) + 3
    return pbits, int(np.ceil(need / pbits))  # primes just below 2^pbits: a lower bound, exact unless need is at a multiple


@pytest.mark.parametrize("n", range(1, 65))
def test_every_order_every_instance(sup, n):
    a = T.sparse_int_matrix(n, 300 + n)
    chunks = T.chunk_count(sup, n, 6)
    c0 = 0 if n <= 20 else T.scattered_start(chunks)
    c1 = min(c0 + 8, chunks)
    m = min(6, n - 1 - sup.layout(n)[0])
    truth = {}
    for form in FORMS:
        if form == 2 and m == 0:
            with pytest.raises(sup.SupError, match="form 2"):
                sup.perman_exact_range(a, c0, c1, walk_log2=6, form=2)
            continue
        for group in GROUPS:
            res, info = _both(sup, a, c0, c1, form, group, walk_log2=6)
            assert info["m"] == m and info["gray_steps"] == (c1 - c0) << (info["L"] + m)
            pbits, count = _prime_count(a, group)
            assert all(p.bit_length() == pbits for p in info["primes"]) and count <= len(res) <= count + 1
            if n in TRUTH_N:
                assert T.subsets(info["L"], m, c0, c1) <= 1 << 15
                key = tuple(info["colmap"])
                if key not in truth:
                    truth[key] = T.range_sum(T.doubled(a), info["colmap"], info["L"], m, c0, c1)
                assert res == [truth[key] % p for p in info["primes"]], (form, group)


def _edge_matrix(n, xbits, alternating):
    """Every row sum of |a| is 2^xbits - 1: the largest the budget of that xbits allows."""
    total = (1 << xbits) - 1
    a = np.full((n, n), total // n, np.int64)
    a[:, 0] += total - (total // n) * n
    assert (np.abs(a).sum(1) == total).all() and int(total).bit_length() == xbits
    if alternating:
        a *= (-1) ** np.add.outer(np.arange(n), np.arange(n))
    return a.astype(np.int32)


@pytest.mark.parametrize("n", [8, 11])
@pytest.mark.parametrize("group,xbits,pbits", [(1, 31, 20), (2, 15, 21), (4, 7, 23)])
@pytest.mark.parametrize("alternating", [False, True])
def test_exactness_edge(sup, n, group, xbits, pbits, alternating):
    """G xbits + pbits = 51 exactly, |X_j| reaching the row sum (one sign) so a
    group product reaches 2^(G xbits): whole permanents against Python integers."""
    a = _edge_matrix(n, xbits, alternating)
    want = T.permanent([[int(v) for v in row] for row in a])
    chunks = T.chunk_count(sup, n)
    sign = 1 if n & 1 else -1
    for form in FORMS:
        res, info = _both(sup, a, 0, chunks, form, group)
        assert all(p.bit_length() == pbits for p in info["primes"])
        if group == 1:
            assert len(info["primes"]) > 8  # 13 primes at n = 8, 18 at n = 11: two or three launches of up to 8
        total = T.crt_signed(res, info["primes"])
        assert total % (1 << (n - 1)) == 0 and sign * (total >> (n - 1)) == want
    got, st = sup.perman_exact(a, return_stats=True)
    assert got == want and st["devices_used"] == 1
    LEDGER.add((n, st["walk_kind"] + 1, st["seg_pair_bits"]))
    # one step past the edge: this G is refused, another one still gives the truth
    b = _edge_matrix(n, xbits + 1, alternating) if xbits < 31 else None
    if b is None:  # a row sum of 2^31 leaves no G at all
        b64 = a.astype(np.float64)
        b64[:, 1] += np.sign(b64[:, 1])
        with pytest.raises(sup.SupError, match="xbits = 32") as e:
            sup.perman_exact_range(b64, 0, chunks, group=1)
        assert e.value.code == -1
        with pytest.raises(sup.SupError, match="below 2\\^31") as e:
            sup.perman_exact(b64)
        assert e.value.code == -7
        return
    with pytest.raises(sup.SupError, match=f"xbits = {xbits + 1}") as e:
        sup.perman_exact_range(b, 0, chunks, group=group)
    assert e.value.code == -1
    got, st = sup.perman_exact(b, return_stats=True)
    assert got == T.permanent([[int(v) for v in row] for row in b]) and 1 <= st["seg_pair_bits"] < group


@pytest.mark.parametrize("walk_log2", [9, 10])
def test_accumulator_fold(sup, walk_log2):
    """T = 2^m >= 512 steps per lane with 42-bit primes: the fold at every 256th
    step runs (the default layouts reach m >= 9 only from n = 29 on).  n = 17
    has two chunks at m = 9 and one at m = 10: the whole range."""
    n = 17
    a = T.sparse_int_matrix(n, 317)
    chunks = T.chunk_count(sup, n, walk_log2)
    assert chunks == 1 << (10 - walk_log2)
    for form in FORMS:
        res, info = _both(sup, a, 0, min(4, chunks), form, 1, walk_log2=walk_log2)
        assert info["m"] == walk_log2 and all(p.bit_length() == 42 for p in info["primes"])
        if walk_log2 == 9:
            one, _ = _both(sup, a, 1, 2, form, 1, walk_log2=9)
            assert T.subsets(6, 9, 1, 2) == 1 << 15
            truth = T.range_sum(T.doubled(a), info["colmap"], 6, 9, 1, 2)
            assert one == [truth % p for p in info["primes"]]


def test_chunk_ends_in_high_rows(sup):
    """Chunk-end rows 32..35 (the high word of the zero-row mask): a range in
    which some chunks end at their first state and some are walked."""
    a = T.chunk_end_matrix()
    chunks = T.chunk_count(sup, 36, 6)
    for form in FORMS:
        _, info = sup.perman_exact_range(a, 0, 0, cpu=True, walk_log2=6, form=form)
        rows = T.chunk_end_rows(a, info)
        assert rows[-4:] == [32, 33, 34, 35]
        c0, ended = T.mixed_window(a, info, [32, 33, 34, 35], T.scattered_start(chunks, 1 << 16))
        assert ended == T.ended_chunks(a, info, c0, c0 + 8, rows)  # rows below 32 hold odd values: never zero
        for group in GROUPS:
            res, info = _both(sup, a, c0, c0 + 8, form, group, walk_log2=6)
            truth = T.range_sum(T.doubled(a), info["colmap"], 6, 6, c0, c0 + 8)
            assert res == [truth % p for p in info["primes"]]
            # the ended chunks alone sum to zero, the others do not all
            for i, e in enumerate(ended):
                if e:
                    one, _ = _device(sup, a, c0 + i, c0 + i + 1, walk_log2=6, form=form, group=group)
                    assert one == [0] * len(one)
        assert truth != 0


def test_planner_choice_is_reported(sup):
    rng = np.random.default_rng(24)
    n = 24
    a = np.where(rng.random((n, n)) < 0.12, rng.integers(1, 4, (n, n)), 0).astype(np.int32)
    a[np.arange(n), rng.permutation(n)] = 1
    for cpu in (False, True):
        got, st = sup.perman_exact(a, cpu=cpu, return_stats=True)
        assert st["walk_kind"] == 1 and st["seg_pair_bits"] in GROUPS, st
        assert (st["lane_bits"], st["walk_bits"]) == sup.layout(n)[:2]
        ones, st1 = sup.perman_exact(np.ones((20, 20), np.int32), cpu=cpu, return_stats=True)
        assert st1["walk_kind"] == 0 and st1["seg_pair_bits"] in GROUPS, st1
    # form 0 of the range entry is that planner
    chunks = T.chunk_count(sup, n)
    res, info = _device(sup, a, 0, chunks)
    assert info["walk_kind"] == 1 and info["G"] == st["seg_pair_bits"]
    total = T.crt_signed(res, info["primes"])
    assert -(total >> (n - 1)) == got


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
    device, and a second logical device on GPU 0, return the same residues."""
    a = T.sparse_int_matrix(21, 321)
    want, _ = sup.perman_exact_range(a, 5, 13, cpu=True, walk_log2=6)
    for d in range(sup.device_count()):
        assert _device(sup, a, 5, 13, walk_log2=6, device_id=d)[0] == want
    with device_map("0,0"):
        assert sup.device_count() == 2
        assert _device(sup, a, 5, 13, walk_log2=6, device_id=1)[0] == want
        with pytest.raises(sup.SupError, match="device_id"):
            sup.perman_exact_range(a, 5, 13, walk_log2=6, device_id=2)


def test_every_instance_was_launched(sup):
    """Runs last: the launches above cover walk_exact<N, G> and
    walk_exact_blocked<N, G> for every N and G, but for the blocked kernel at
    N <= 7, which has no walk bits and is refused."""
    want = {(n, form, g) for n in range(1, 65) for form in FORMS for g in GROUPS if not (form == 2 and n <= 7)}
    assert len(want) == 384 - 21
    assert want - LEDGER == set()
