"""sup_perman_exact_range on host threads (the host twin cpu_exact_range
behind exact.cpp's planner, prime selection and both plan forms), against
plain Python integers (range_truth.py): no GPU, no oracle.

* the whole range, joined by a CRT written here, is the permanent: the sign
  convention, Garner and the big-integer code of sup_perman_exact checked from
  outside;
* range algebra: residues of disjoint ranges add modulo p;
* ranges high in the chunk space of n = 33 ... 64 equal the Python sum;
* every refusal."""
import ctypes as C

import numpy as np
import pytest

import range_truth as T

FORMS = (1, 2)


def _ints(a):
    return [[int(v) for v in row] for row in a]


@pytest.mark.parametrize("n", range(1, 11))
def test_whole_range_is_the_permanent(sup, n):
    """T = the whole range of 2A; perm = (4(n&1) - 2) T / 2^n, i.e. the signed
    T shifted by n - 1 (not (4(n&1) - 2) T / 2^(n-1), which counts the factor
    2 twice; n = 1 decides it: T = a)."""
    rng = np.random.default_rng(40 + n)
    a = rng.integers(-3, 4, (n, n)).astype(np.int32)
    want = T.permanent(_ints(a))
    assert sup.perman_exact(a, cpu=True, threads=3) == want
    chunks = T.chunk_count(sup, n)
    for form in (0, 1, 2):
        for group in (0, 1, 2, 4):
            if form == 2 and sup.layout(n)[1] == 0:
                continue
            res, info = sup.perman_exact_range(a, 0, chunks, cpu=True, threads=1 + group, form=form, group=group)
            assert len(res) == len(info["primes"]) >= 1 and all(0 <= r < p for r, p in zip(res, info["primes"]))
            assert group == 0 or info["G"] == group
            assert form == 0 or info["walk_kind"] == form - 1
            assert (info["L"], info["m"]) == sup.layout(n)[:2] and info["gray_steps"] == 1 << (n - 1)
            assert sorted(info["colmap"]) == list(range(n - 1))
            total = T.crt_signed(res, info["primes"])
            assert total % (1 << (n - 1)) == 0
            assert (total >> (n - 1)) * (1 if n & 1 else -1) == want, (form, group)
            # and the sum itself, subset by subset
            assert total == T.range_sum(T.doubled(a), info["colmap"], info["L"], info["m"], 0, chunks)


@pytest.mark.parametrize("n", [16, 19])
@pytest.mark.parametrize("walk_log2", [0, 1, 4])
def test_range_algebra(sup, n, walk_log2):
    a = T.sparse_int_matrix(n, 100 + n)
    chunks = T.chunk_count(sup, n, walk_log2)
    for form in FORMS:
        whole, info = sup.perman_exact_range(a, 0, chunks, cpu=True, walk_log2=walk_log2, form=form)
        primes = info["primes"]
        assert info["m"] == (walk_log2 or sup.layout(n)[1])
        for pieces in (2, 4, 8):
            step = chunks // pieces
            acc = [0] * len(primes)
            for i in range(pieces):
                r, pi = sup.perman_exact_range(a, i * step, (i + 1) * step, cpu=True, threads=1 + i,
                                               walk_log2=walk_log2, form=form)
                assert pi["primes"] == primes and pi["colmap"] == info["colmap"]
                acc = [(x + y) % p for x, y, p in zip(acc, r, primes)]
            assert acc == whole, (form, pieces)
        # an unaligned split at 3 and 11 (where the plan has fewer chunks, at its end)
        cuts = [0, min(3, chunks), min(11, chunks), chunks]
        acc = [0] * len(primes)
        for lo, hi in zip(cuts, cuts[1:]):
            r, _ = sup.perman_exact_range(a, lo, hi, cpu=True, walk_log2=walk_log2, form=form)
            acc = [(x + y) % p for x, y, p in zip(acc, r, primes)]
        assert acc == whole, form
    # both forms and every group: the same integer (primes differ with G)
    want = T.crt_signed(whole, primes)
    for group in (1, 2, 4):
        r, gi = sup.perman_exact_range(a, 0, chunks, cpu=True, walk_log2=walk_log2, group=group)
        assert T.crt_signed(r, gi["primes"]) == want


@pytest.mark.parametrize("n", [33, 41, 57, 63, 64])
def test_truth_by_range_at_large_n(sup, n):
    a = T.sparse_int_matrix(n, 200 + n)
    chunks = T.chunk_count(sup, n, 4)
    c0 = T.scattered_start(chunks)
    assert c0 >> (n - 1 - 6 - 4 - 3) != 0  # the top bits of the chunk index are in play
    truth = {}
    for form in FORMS:
        res, info = sup.perman_exact_range(a, c0, c0 + 8, cpu=True, walk_log2=4, form=form)
        assert (info["L"], info["m"], info["walk_kind"]) == (6, 4, form - 1)
        assert info["gray_steps"] == 8 << 10 == T.subsets(6, 4, c0, c0 + 8)
        key = tuple(info["colmap"])
        if key not in truth:
            truth[key] = T.range_sum(T.doubled(a), info["colmap"], 6, 4, c0, c0 + 8)
        assert res == [truth[key] % p for p in info["primes"]], form


def test_primes_follow_the_group(sup):
    """pbits = min(42, 51 - G xbits); the largest primes below 2^pbits, enough
    of them for 2^(n-1) prod_j rowabs_j (+ 3 bits)."""
    a = T.sparse_int_matrix(12, 7)
    xbits = int(np.abs(a).sum(1).max()).bit_length()
    need = 11 + sum(np.log2(np.abs(a).sum(1))) + 3
    for group in (1, 2, 4):
        _, info = sup.perman_exact_range(a, 0, 1, cpu=True, group=group)
        pbits = min(42, 51 - group * xbits)
        pr = info["primes"]
        assert all(p.bit_length() == pbits for p in pr) and pr == sorted(pr, reverse=True)
        assert sum(np.log2(p) for p in pr) >= need > sum(np.log2(p) for p in pr[:-1])


def test_errors(sup):
    lib = sup._lib.load()
    a = T.sparse_int_matrix(9, 1)
    chunks = T.chunk_count(sup, 9)

    def refused(match, *args, **kw):
        with pytest.raises(sup.SupError, match=match) as e:
            sup.perman_exact_range(*args, cpu=True, **kw)
        assert e.value.code == -1

    refused("c0 <= c1", a, 2, 1)
    refused("c0 <= c1", a, 0, chunks + 1)
    refused("walk_log2", a, 0, 1, walk_log2=32)
    refused("walk_log2", a, 0, 1, walk_log2=-1)
    refused("form", a, 0, 1, form=3)
    refused("group", a, 0, 1, group=3)
    refused("cap", a, 0, 1, cap=0)
    refused("integers", a + 0.5, 0, 1)
    for n in range(1, 8):  # no walk bits at n <= 7: the blocked kernel has nothing to walk
        refused("form 2", T.sparse_int_matrix(n, n), 0, 1, form=2)
    # an infeasible group: a row sum of 2^16 - 1 (xbits 16) leaves G = 2 primes of 51 - 32 = 19 bits
    big = np.full((4, 4), (1 << 14) - 1, np.int32)
    big[0, 0] += 3
    refused("xbits = 16", big, 0, 1, group=2)
    refused("xbits = 16", big, 0, 1, group=4)
    for group in (0, 1):
        res, info = sup.perman_exact_range(big, 0, 1, cpu=True, group=group)
        assert info["G"] == 1 and info["primes"][0].bit_length() == 35 and len(info["primes"]) >= 2
        refused("cap", big, 0, 1, group=group, cap=len(info["primes"]) - 1)
        assert T.crt_signed(res, info["primes"]) == -8 * T.permanent(_ints(big))  # n = 4, one chunk: -2^(n-1) perm
    # an empty range: zeros, every prime listed
    res, info = sup.perman_exact_range(a, 1, 1, cpu=True)
    assert res == [0] * len(info["primes"]) and info["gray_steps"] == 0
    # the C entry's own checks
    buf = np.ascontiguousarray(a)
    pr, rs = (C.c_uint64 * 128)(), (C.c_uint64 * 128)()
    npr = C.c_int(0)

    def raw(mat=buf.ctypes.data, n=9, c0=0, c1=1, primes=pr, residues=rs, cap=128, nprimes=C.byref(npr)):
        return lib.sup_perman_exact_range(mat, 0, n, c0, c1, None, 1, 0, 0, primes, residues, cap, nprimes, None, None)

    assert raw() == 0 and npr.value >= 1
    assert raw(mat=None) == -1 and raw(primes=None) == -1 and raw(residues=None) == -1 and raw(nprimes=None) == -1
    assert raw(n=0) == -1 and raw(n=65) == -1 and raw(n=-1) == -1
    assert raw(cap=npr.value - 1) == -1 and raw(cap=-1) == -1 and raw(cap=npr.value) == 0
