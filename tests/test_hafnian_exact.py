"""Exact hafnians and loop hafnians of Gaussian-integer matrices
(sup_hafnian_complex_exact) on the host twin: every comparison of
the entry is == on Python ints.  Truth is the recursive definition for n <= 10
and, above, a Python-int restatement of Kan's sum that forms q' and r' from
nothing at every state (pinned against the recursion first)."""
import ctypes as C
import math
import subprocess

import numpy as np
import pytest

from test_complex import gauss_int_case
from test_gpu_hafnian import SHAPES
from test_hafnian import (err, hetero_lists, kan_states, mult_vectors, rank_one_bound,
                          rec_haf, sym_gauss_int, walk_shape)
from test_complex_fock import cmul
from test_hafnian_powertrace import measured as powertrace_measured


# ---- truth ------------------------------------------------------------------------------

def sym_gauss(M, seed, lim=3):
    """A symmetric M x M matrix and a vector mu with integer parts in [-lim, lim]."""
    rng = np.random.default_rng(seed)
    a = rng.integers(-lim, lim + 1, (M, M)) + 1j * rng.integers(-lim, lim + 1, (M, M))
    mu = rng.integers(-lim, lim + 1, M) + 1j * rng.integers(-lim, lim + 1, M)
    return np.triu(a) + np.triu(a, 1).T, mu


def pairs(A):
    return [[(int(z.real), int(z.imag)) for z in row] for row in np.atleast_2d(A)]


def omul(a, b):
    """(re, im) pairs of object arrays of Python ints."""
    return (a[0] * b[0] - a[1] * b[1], a[0] * b[1] + a[1] * b[0])


def kan_exact(A, idx, mu=None):
    """Kan's sum in Python ints: per state H = s - 2 v, q' = H^T Abar H and r' =
    mubar . H from nothing (int64 numpy: below 2^44 for parts below 2^31 and n
    <= 64), then the power q'^m, or sum_j c_j q'^j r'^(n-2j) by Horner's rule,
    and the weights in Python ints (object arrays over the states), and the
    division by m! 8^m or n! 2^(n+m) asserted exact."""
    idx = [int(i) for i in idx]
    n, m = len(idx), len(idx) // 2
    if mu is None and n % 2:
        return (0, 0)
    vals = list(dict.fromkeys(idx))
    mult = [idx.count(v) for v in vals]
    V, w = kan_states(mult)
    w = np.array(w, dtype=object)
    H = np.array(mult, dtype=np.int64)[None, :] - 2 * V
    Ab = np.asarray(A)[np.ix_(vals, vals)]
    re, im = np.rint(Ab.real).astype(np.int64), np.rint(Ab.imag).astype(np.int64)
    q = (np.einsum("tk,kl,tl->t", H, re, H).astype(object), np.einsum("tk,kl,tl->t", H, im, H).astype(object))
    one = (np.array([1] * len(w), dtype=object), np.array([0] * len(w), dtype=object))
    if mu is None:
        p = one
        for _ in range(m):
            p = omul(p, q)
    else:
        mb = np.asarray(mu)[vals]
        r = ((H @ np.rint(mb.real).astype(np.int64)).astype(object), (H @ np.rint(mb.imag).astype(np.int64)).astype(object))
        c = [math.factorial(n) // (math.factorial(j) * math.factorial(n - 2 * j)) * 2 ** (m - j) for j in range(m + 1)]
        R2, Rp = omul(r, r), one
        p = (c[m] * one[0], one[1])
        for j in range(m - 1, -1, -1):  # p = sum_{i >= j} c_i q^(i-j) (r^2)^(m-i)
            Rp = omul(Rp, R2)
            p = omul(p, q)
            p = (p[0] + c[j] * Rp[0], p[1] + c[j] * Rp[1])
        if n % 2:
            p = omul(p, r)
    tr, ti = int(np.sum(w * p[0])), int(np.sum(w * p[1]))
    d = math.factorial(m) * 8 ** m if mu is None else math.factorial(n) * 2 ** (n + m)
    assert (2 * tr) % d == 0 and (2 * ti) % d == 0
    return (2 * tr // d, 2 * ti // d)


def truth_of(A, idx, mu=None):
    if len(idx) <= 10:
        return tuple(rec_haf(pairs(A), idx, None if mu is None else pairs(mu[None, :])[0]))
    return kan_exact(A, idx, mu)


def dfact(k):
    return math.prod(range(k, 0, -2))


def test_restatement_is_the_recursive_definition():
    A, mu = sym_gauss(5, 1)
    rng = np.random.default_rng(2)
    for n in range(1, 11):
        for _ in range(3):
            idx = rng.integers(0, 5, n)
            assert kan_exact(A, idx) == tuple(rec_haf(pairs(A), idx))
            assert kan_exact(A, idx, mu) == tuple(rec_haf(pairs(A), idx, pairs(mu[None, :])[0]))


# ---- closed forms -----------------------------------------------------------------------

def test_small_orders_and_zero(sup):
    A = np.array([[2 - 3j, -1j, 4], [-1j, -5, 1 + 1j], [4, 1 + 1j, 7j]])
    mu = np.array([-2 + 0j, 3j, 1 - 1j])
    for k in range(3):
        assert sup.hafnian_exact_batch(A, [k], cpu=True) == (0, 0)                 # n = 1 plain
        z = mu[k]
        assert sup.hafnian_exact_batch(A, [k], mu=mu, loop=True, cpu=True) == (int(z.real), int(z.imag))
        z = A[k, k]
        assert sup.hafnian_exact_batch(A, [k, k], cpu=True) == (int(z.real), int(z.imag))
    assert sup.hafnian_exact_batch(A, [0, 1], cpu=True) == (0, -1)                 # purely imaginary
    assert sup.hafnian_exact_batch(A, [1, 1], cpu=True) == (-5, 0)                 # negative
    assert sup.hafnian_exact(A, cpu=True) == (0, 0)                                # n = 3 plain
    z = A[0, 1] + mu[0] * mu[1]
    assert sup.hafnian_exact_batch(A, [0, 1], mu=mu, loop=True, cpu=True) == (int(z.real), int(z.imag))
    z = mu[0] * mu[1] * mu[2] + A[0, 1] * mu[2] + A[0, 2] * mu[1] + A[1, 2] * mu[0]
    assert sup.loop_hafnian_exact(A, mu=mu, cpu=True) == (int(z.real), int(z.imag))  # n = 3 loop
    z = np.diag(A)[0] * np.diag(A)[1] + A[0, 1]
    assert sup.loop_hafnian_exact(A[:2, :2], cpu=True) == (int(z.real), int(z.imag))  # mu defaults to the diagonal
    Z = np.zeros((6, 6))
    assert sup.hafnian_exact(Z, cpu=True) == (0, 0) and sup.loop_hafnian_exact(Z, cpu=True) == (0, 0)
    assert sup.hafnian_exact_repeated(Z, [4, 4, 0, 0, 2, 2], cpu=True) == (0, 0)
    v, st = sup.hafnian_exact_batch(A, [[0, 1, 2], [2, 2, 1]], cpu=True, return_stats=True)
    assert v == [(0, 0), (0, 0)] and st["visited_steps"] == 0 and st["leaves"] == 2  # odd n: nothing walked


@pytest.mark.parametrize("n", [8, 16])
def test_all_ones_counts_the_perfect_matchings(sup, n):
    assert sup.hafnian_exact(np.ones((n, n)), cpu=True) == (dfact(n - 1), 0)


def test_one_mode_64_times(sup):
    one = np.ones((1, 1))
    v, st = sup.hafnian_exact_batch(one, [0] * 64, cpu=True, return_stats=True)
    assert v == (dfact(63), 0) and v[0].bit_length() == 147 and st["visited_steps"] == 64
    a = [1, 1]  # involutions: a_n = a_(n-1) + (n - 1) a_(n-2)
    for k in range(2, 65):
        a.append(a[-1] + (k - 1) * a[-2])
    assert sup.hafnian_exact_batch(one, [0] * 64, mu=[1], loop=True, cpu=True) == (a[64], 0)


@pytest.mark.parametrize("n,mult", [(17, (5, 4, 4, 4)), (24, (4,) * 6), (64, (16, 16, 16, 16))])
def test_rank_one_closed_form(sup, n, mult):
    """A = u u^T: haf = (n - 1)!! prod u_idx (0 for odd n)."""
    rng = np.random.default_rng(n)
    K = len(mult)
    u = rng.integers(-3, 4, K) + 1j * rng.integers(-3, 4, K)
    u[u == 0] = 1 - 2j
    idx = np.repeat(np.arange(K), mult)
    rng.shuffle(idx[1:])
    prod = (1, 0)
    for i in idx:
        prod = cmul(prod, (int(u[i].real), int(u[i].imag)))
    want = (dfact(n - 1) * prod[0], dfact(n - 1) * prod[1]) if n % 2 == 0 else (0, 0)
    v, st = sup.hafnian_exact_batch(np.outer(u, u), idx, cpu=True, return_stats=True)
    assert v == want
    assert st["visited_steps"] == (walk_shape(idx)[0] if n % 2 == 0 else 0)


def grid_adjacency(r, c):
    A = np.zeros((r * c, r * c))
    for i in range(r):
        for j in range(c):
            if j + 1 < c:
                A[i * c + j, i * c + j + 1] = A[i * c + j + 1, i * c + j] = 1
            if i + 1 < r:
                A[i * c + j, (i + 1) * c + j] = A[(i + 1) * c + j, i * c + j] = 1
    return A


def test_domino_tilings(sup):
    fib = [1, 1]
    for k in range(2, 12):
        fib.append(fib[-1] + fib[-2])
    for k in range(1, 11):
        assert sup.hafnian_exact(grid_adjacency(2, k), cpu=True) == (fib[k], 0)
    for (r, c), want in (((4, 4), 36), ((4, 5), 95), ((4, 6), 281)):
        assert sup.hafnian_exact(grid_adjacency(r, c), cpu=True) == (want, 0)


# ---- random cases -----------------------------------------------------------------------

@pytest.mark.parametrize("total", [6, 8])
def test_every_multiplicity_vector(sup, total):
    A, mu = sym_gauss(4, 70 + total)
    vecs = mult_vectors(total)
    idx = np.stack([np.repeat(np.arange(4), s) for s in vecs])
    got = sup.hafnian_exact_batch(A, idx, cpu=True)
    gotl = sup.hafnian_exact_batch(A, idx, mu=mu, loop=True, cpu=True)
    for k, s in enumerate(vecs):
        assert got[k] == truth_of(A, idx[k]), s
        assert gotl[k] == truth_of(A, idx[k], mu), s
        if k % 17 == 0:
            assert sup.hafnian_exact_repeated(A, list(s), mu=mu, loop=True, cpu=True) == gotl[k]


@pytest.mark.parametrize("n", range(4, 15))
def test_distinct_modes(sup, n):
    A, mu = sym_gauss(n, 100 + n)
    v, st = sup.hafnian_exact(A, cpu=True, return_stats=True)
    assert v == truth_of(A, range(n))
    assert st["visited_steps"] == (2 ** (n - 1) if n % 2 == 0 else 0)
    assert sup.loop_hafnian_exact(A, mu=mu, cpu=True) == truth_of(A, range(n), mu)


@pytest.mark.parametrize("name", ["n16_no_walk", "n17_loop_odd", "n18_walks"])
def test_walk_shapes_of_the_device_tests(sup, name):
    n, patterns, want, forms = SHAPES[name]
    rng = np.random.default_rng(7000 + n)
    A, mu = sym_gauss(24, 7100 + n)
    idx = np.stack([np.repeat(rng.choice(24, len(s), replace=False), s) for s in patterns])
    assert [walk_shape(idx[k])[:3] for k in range(len(want))] == want
    for loop in forms:
        idx_l = idx
        v, st = sup.hafnian_exact_batch(A, idx_l, mu=mu if loop else None, loop=loop, cpu=True, return_stats=True)
        assert st["visited_steps"] == sum(w[0] for w in want[:len(idx_l)]) and st["est_ops_per_step"] > 0
        assert st["seg_cached_bits"] >= 1 and st["seg_pair_bits"] == -(-st["seg_cached_bits"] // 8)
        for k in range(len(idx_l)):
            assert v[k] == kan_exact(A, idx_l[k], mu if loop else None), (name, loop, k)


# ---- weights above 2^53 -----------------------------------------------------------------

def test_weights_above_2_53(sup):
    """(32, 32): s' = (31, 32), both high digits, C(31,15) C(32,16) > 2^53.
    (57, 1 x 7): the walk digit holds 57 copies, the most the layout rule (H >=
    64 left of n <= 64) allows, and C(57, 28) > 2^53."""
    assert math.comb(31, 15) * math.comb(32, 16) > 2 ** 53 and math.comb(57, 28) > 2 ** 53
    A, mu = sym_gauss(8, 53)
    idx = np.repeat([0, 1], 32)
    assert walk_shape(idx)[:3] == (1056, 1, 1056)
    assert sup.hafnian_exact_batch(A, idx, cpu=True) == kan_exact(A, idx)
    assert sup.hafnian_exact_batch(A, idx, mu=mu, loop=True, cpu=True) == kan_exact(A, idx, mu)
    idx = np.array([0] * 57 + list(range(1, 8)))
    assert walk_shape(idx)[:3] == (58 * 64, 58, 64)
    assert sup.hafnian_exact_batch(A, idx, cpu=True) == kan_exact(A, idx)
    assert sup.hafnian_exact_batch(A, idx, mu=mu, loop=True, cpu=True) == kan_exact(A, idx, mu)


# ---- the project's own truth ------------------------------------------------------------

@pytest.mark.parametrize("n", [8, 11])
def test_bipartite_block_matrix_is_the_exact_permanent(sup, n):
    B = gauss_int_case(n, 900 + n)
    Z = np.zeros((n, n))
    assert sup.hafnian_exact(np.block([[Z, B], [B.T, Z]]), cpu=True) == sup.perman_complex_exact(B, cpu=True)


# ---- edges --------------------------------------------------------------------------------

BIG = 2 ** 31 - 1


@pytest.mark.parametrize("idx", [list(range(6)), [0] * 3 + [1] * 3 + [2] * 3 + [3] * 3])
def test_largest_entries(sup, idx):
    """+-(2^31 - 1)(1 + i): the largest prime below 2^25 taken, residues at the
    edge of 2.25 p^2 < 2^52; at n = 12 the plain form takes 10 primes (two
    launches of the device's 8, the second partly filled), the loop form 18."""
    rng = np.random.default_rng(len(idx))
    sg = rng.choice([-1, 1], (6, 6))
    sg = np.triu(sg) + np.triu(sg, 1).T
    A = sg * (BIG * (1 + 1j))
    mu = np.diag(A).copy()
    v, st = sup.hafnian_exact_batch(A, idx, cpu=True, return_stats=True)
    assert v == truth_of(A, idx)
    assert (st["seg_cached_bits"], st["seg_pair_bits"]) == ((5, 1) if len(idx) == 6 else (10, 2))
    v, st = sup.hafnian_exact_batch(A, idx, mu=mu, loop=True, cpu=True, return_stats=True)
    assert v == truth_of(A, idx, mu)
    assert (st["seg_cached_bits"], st["seg_pair_bits"]) == ((9, 2) if len(idx) == 6 else (18, 3))


def test_part_of_2_31_is_refused(sup):
    A = np.zeros((3, 3), dtype=complex)
    A[1, 2] = A[2, 1] = -2.0 ** 31 * 1j
    with pytest.raises(sup.SupError) as e:
        sup.hafnian_exact_batch(A, [0, 1], cpu=True)
    assert e.value.code == -1 and "row 1, column 2, Im part" in str(e.value) and "out of range" in str(e.value)
    with pytest.raises(sup.SupError) as e:
        sup.hafnian_exact_batch(np.zeros((2, 2)), [0, 1], mu=[0, 2 ** 31], loop=True, cpu=True)
    assert e.value.code == -1 and "mu entry (index 1, Re part)" in str(e.value)
    with pytest.raises(sup.SupError) as e:
        sup.hafnian_exact(np.array([[0, 2 ** 53], [2 ** 53, 0]], dtype=object), cpu=True)
    assert "not exactly representable" in str(e.value)


def test_self_check_failure_is_an_error_not_a_number(sup, monkeypatch):
    """haf of J_4 is 3: with the factor 2 of 2T / (m! 8^m) replaced by 1 (test
    hook, read per call) the numerator is not divisible."""
    J = np.ones((4, 4))
    assert sup.hafnian_exact(J, cpu=True) == (3, 0)
    monkeypatch.setenv("SUP_HAFNIAN_EXACT_TEST_MUL", "1")
    with pytest.raises(sup.SupError) as e:
        sup.hafnian_exact(J, cpu=True)
    assert e.value.code == -3 and "self-check failed (2T not divisible by m! 8^m)" in str(e.value)
    Z, mu = np.zeros((4, 4)), np.ones(4)  # A = 0, mu = 1: the one matching of four loops
    with pytest.raises(sup.SupError) as e:
        sup.loop_hafnian_exact(Z, mu=mu, cpu=True)
    assert e.value.code == -3 and "self-check failed (2L not divisible by n! 2^(n+m))" in str(e.value)
    monkeypatch.delenv("SUP_HAFNIAN_EXACT_TEST_MUL")
    assert sup.loop_hafnian_exact(Z, mu=mu, cpu=True) == (1, 0)
    assert sup.loop_hafnian_exact(J, cpu=True) == (10, 0)  # involutions of 4 points


# ---- host splits and batches ------------------------------------------------------------

@pytest.mark.parametrize("n", [9, 14])
def test_batch_is_the_single_call_on_any_thread_count(sup, n):
    A, mu = sym_gauss(12, 400 + n)
    idx = hetero_lists(n, 65, 400 + n)
    for loop in (False, True):
        one = [sup.hafnian_exact_batch(A, idx[k], mu=mu, loop=loop, cpu=True, threads=1) for k in range(65)]
        for threads in (1, 3, 16):
            assert sup.hafnian_exact_batch(A, idx, mu=mu, loop=loop, cpu=True, threads=threads) == one
    assert sup.hafnian_exact_batch(A, np.zeros((0, n), dtype=int), cpu=True) == []


# ---- errors and the CLI -----------------------------------------------------------------

def test_errors_name_the_place(sup):
    A, mu = sym_gauss(4, 9)
    lib = sup._lib.load()
    a = np.ascontiguousarray(A, dtype=np.complex128)
    m = np.ascontiguousarray(mu, dtype=np.complex128)
    idx = np.array([0, 1, 2, 3], dtype=np.int32)
    re, im = C.create_string_buffer(768), C.create_string_buffer(768)

    def call(a_=a, M=4, mu_=None, idx_=idx, n=4, count=1, re_=re, im_=im, ln=768, cpu=1):
        rc = lib.sup_hafnian_complex_exact(None if a_ is None else a_.ctypes.data, M,
                                           None if mu_ is None else mu_.ctypes.data,
                                           None if idx_ is None else idx_.ctypes.data, n, count, None, cpu, re_, im_, ln,
                                           None)
        return rc, lib.sup_last_error().decode()

    assert call()[0] == 0 and (int(re.value), int(im.value)) == truth_of(A, idx)
    for kw in ({"a_": None}, {"idx_": None}, {"re_": None}, {"im_": None}):
        rc, msg = call(**kw)
        assert rc == -1 and "null pointer" in msg, kw
    for n in (0, 65, -1):
        rc, msg = call(n=n)
        assert rc == -1 and "outside [1, 64]" in msg
    rc, msg = call(M=0)
    assert rc == -1 and "at least one row" in msg
    b = a.copy()
    b[1, 3] += 1
    rc, msg = call(a_=b)
    assert rc == -1 and "A[1][3] and A[3][1] differ" in msg
    rc, msg = call(idx_=np.array([0, 1, 4, 3], dtype=np.int32))
    assert rc == -1 and "position 2] = 4 outside [0, 4)" in msg
    b = a.copy()
    b[2, 0] = b[0, 2] = 0.5
    rc, msg = call(a_=b)
    assert rc == -1 and "A entry (row 0, column 2, Re part) is not an integer" in msg
    b[2, 0] = b[0, 2] = complex(1, np.inf)
    rc, msg = call(a_=b)
    assert rc == -1 and "A entry (row 0, column 2, Im part) is not an integer" in msg
    m2 = m.copy()
    m2[3] = 1.25j
    rc, msg = call(mu_=m2)
    assert rc == -1 and "mu entry (index 3, Im part) is not an integer" in msg
    big = np.ascontiguousarray(np.ones((4, 4)) * 1000, dtype=np.complex128)
    rc, msg = call(a_=big, ln=4)
    assert rc == -1 and "out_len = 4 but a result needs 8 bytes" in msg  # haf = 3 x 10^6
    assert call(a_=big, ln=8)[0] == 0 and re.value == b"3000000"
    assert call(count=0, re_=None, im_=None)[0] == 0
    with pytest.raises(ValueError):
        sup.hafnian_exact_batch(A, [0, 1], mu=[1, 2, 3], loop=True, cpu=True)
    with pytest.raises(ValueError):
        sup.hafnian_exact_batch(np.ones((2, 3)), [0, 1], cpu=True)


def test_too_many_chunks_is_refused_before_any_work(sup):
    with pytest.raises(sup.SupError) as e:
        sup.hafnian_exact(np.ones((42, 42)), cpu=True)
    assert e.value.code == -7 and "more than 2^40" in str(e.value)  # SUP_EUNSUPPORTED


def test_no_device_is_an_error_not_a_cpu_fallback(sup):
    A, mu = sym_gauss(6, 19)
    idx = np.random.default_rng(1).integers(0, 6, (4, 6))
    if sup.device_count() == 0:
        for loop in (False, True):
            with pytest.raises(sup.SupError) as e:
                sup.hafnian_exact_batch(A, idx, mu=mu, loop=loop)
            assert e.value.code == -2
    else:
        assert sup.hafnian_exact_batch(A, idx) == sup.hafnian_exact_batch(A, idx, cpu=True)


def run_cli(sup, *args):
    return subprocess.run([sup._lib.PERMAN_BIN, *args], capture_output=True, text=True, timeout=120)


def write_mtx(path, A, fmt):
    n = A.shape[0]
    with open(path, "w") as f:
        f.write(f"%%MatrixMarket matrix coordinate complex symmetric\n{n} {n} {n * (n + 1) // 2}\n")
        for i in range(n):
            for j in range(i + 1):
                f.write(f"{i + 1} {j + 1} {fmt(A[i, j].real)} {fmt(A[i, j].imag)}\n")


def test_cli_exact_hafnian_on_host_threads(sup, tmp_path):
    A, _ = sym_gauss(5, 21)
    path = tmp_path / "h5.mtx"
    write_mtx(path, A, lambda x: str(int(x)))
    for extra, want in ((("--rpt", "1,1,1,1"), sup.hafnian_exact(A[:4, :4], cpu=True)),
                        (("--rpt", "2,0,3,0,1"), sup.hafnian_exact_repeated(A, [2, 0, 3, 0, 1], cpu=True)),
                        (("--loop",), sup.loop_hafnian_exact(A, cpu=True)),
                        (("--loop", "--rpt", "0,2,1"), sup.hafnian_exact_repeated(A, [0, 2, 1, 0, 0], loop=True, cpu=True)),
                        ((), (0, 0))):
        r = run_cli(sup, "-f", str(path), "--hafnian", "--exact", "-c", *extra)
        assert r.returncode == 0, r.stderr
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("Hafnian (exact): ")]
        assert len(line) == 1 and ("cpu_loop_hafnian64_complex_exact" if "--loop" in extra
                                   else "cpu_hafnian64_complex_exact") in r.stdout
        assert tuple(int(x) for x in line[0].split()[2:]) == want, (extra, line, want)
    for bad, msg in ((("--hafnian", "--exact", "--powertrace"), "--hafnian --exact does not combine with --powertrace"),
                     (("--hafnian", "--exact", "--complex-exact"), "--hafnian does not combine with --complex-exact"),
                     (("--hafnian", "--exact", "-q"), "--hafnian does not combine with -q"),
                     (("--exact", "--loop"), "--loop and --rpt go with --hafnian")):
        r = run_cli(sup, "-f", str(path), "-c", *bad)
        assert r.returncode == 1 and msg in r.stderr, (bad, r.stderr)
    half = tmp_path / "half.mtx"
    write_mtx(half, A / 2, lambda x: repr(float(x)))
    r = run_cli(sup, "-f", str(half), "--hafnian", "--exact", "-c", "--rpt", "1,1,1,1")
    assert r.returncode == 1 and "is not an integer" in r.stderr


# ---- judging the floating entries -------------------------------------------------------

def kan_scale_distinct(A, mu, n, loop):
    """S = 2 sum_v |term| (/ m!) of the Kan walk on n distinct modes (weights
    +-1, v_0 = 0: the first mode's copy is held), vectorised."""
    m = n // 2
    t = np.arange(2 ** (n - 1), dtype=np.int64)
    V = np.concatenate([np.zeros((len(t), 1)), ((t[:, None] >> np.arange(n - 1)) & 1).astype(float)], axis=1)
    h = 0.5 - V
    q = np.abs(np.einsum("tk,tk->t", h @ (A / 2), h))
    if not loop:
        return 2 * float(np.sum(q ** m)) / math.factorial(m)
    r = np.abs(h @ mu)
    return 2 * float(sum(np.sum(q ** j * r ** (n - 2 * j)) / (math.factorial(j) * math.factorial(n - 2 * j))
                         for j in range(m + 1)))


@pytest.mark.parametrize("n", [20, 22])
def test_floating_entries_against_the_exact_integers(sup, n):
    """hafnian, loop_hafnian and hafnian_powertrace on entries in {-1,0,1} +
    {-1,0,1} i, measured from the exact integers, each within the bound its own
    tests assert: test_hafnian's 2^-52 (m or n) (Tw + K) (+ n + 2) of S
    (rank_one_bound) and test_hafnian_powertrace's 8 max(e_np, n 2^-52) of its S."""
    A = sym_gauss_int(n, 300 + n)
    mu = np.diag(sym_gauss_int(n, 600 + n)).copy()
    idx = np.arange(n)
    T, Tw, H, K = walk_shape(idx)
    for loop in (False, True):
        truth = sup.hafnian_exact_batch(A, idx, mu=mu, loop=loop, cpu=True)
        v = sup.hafnian_batch(A, idx, mu=mu, loop=loop, cpu=True)
        S = kan_scale_distinct(A, mu, n, loop)
        e, bound = err(v, truth) / S, rank_one_bound(n, Tw, K, loop)
        print(f"kan n={n} loop={loop} truth={truth} error/S={e:.3e} bound={bound:.3e} S/|truth|={S / max(abs(complex(*truth)), 1):.3e}")
        assert e <= bound
    for m_ in (None, mu):
        truth = sup.hafnian_exact_batch(A, idx, mu=m_, loop=m_ is not None, cpu=True)
        e, e_np = powertrace_measured(sup, A, idx, m_, truth, "exact")
        print(f"powertrace n={n} loop={m_ is not None} error/S={e:.3e} numpy restatement {e_np:.3e}")
