"""The complex fp64 walk on the GPU (walk_cplx.hip through sup_perman_complex
and sup_perman_complex_range): bit-identical to its host twin (cplx.cpp; the
same cx.hpp operations in the same order) for whole permanents and for chunk
ranges of the large orders, whose whole walks are out of reach."""
import os
import subprocess

import numpy as np
import pytest

from test_complex import as_complex, exact_perm, gauss_int_case, write_mtx

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def need_gpu(sup):
    if sup.device_count() < 1:
        pytest.fail("no HIP device visible: -m gpu tests must run on the MI355X box")


def dense_complex(n, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))


@pytest.mark.parametrize("n,seed", [(1, 1), (2, 2), (5, 3), (13, 4), (20, 5), (24, 6)])
def test_gpu_complex_bit_identical_to_host_twin(sup, n, seed):
    a = dense_complex(n, seed)
    v, st = sup.perman_complex(a, return_stats=True)
    assert st["devices_used"] == 1 and st["kernel_ms"] > 0 and st["grid"] >= 1
    assert v == sup.perman_complex(a, cpu=True, threads=16)
    vd, sd = sup.perman_complex(a, gpu_num=sup.device_count(), return_stats=True)
    assert vd == v
    assert sd["devices_used"] == min(sup.device_count(), 1 << sup.layout(n)[2]) and sd["kernel_ms"] > 0


# walk_log2 = 10: 64 wave-chunks are 2^22 Gray steps.  33: two SGPR pieces per
# plane; 41: past the double-double walk's two-wave request; 55 / 56: either
# side of this walk's switch from two waves per SIMD to one; 64: the last
# range sets the top bits of the 47-bit chunk index.
@pytest.mark.parametrize("n", [33, 41, 48, 55, 56, 63, 64])
@pytest.mark.parametrize("where", ["first", "scattered", "last"])
def test_gpu_complex_ranges_of_large_orders(sup, n, where):
    a = dense_complex(n, 100 + n)
    chunks = 1 << (n - 1 - 6 - 10)
    c = {"first": 0, "scattered": 0x5A5AA5A55A69 & (chunks - 1) & ~63, "last": chunks - 64}[where]
    assert 0 <= c <= chunks - 64
    v, st = sup.perman_complex_range(a, c, c + 64, walk_log2=10, return_stats=True)
    assert st["walk_bits"] == 10 and st["lane_bits"] == 6 and st["gray_steps"] == 1 << 22
    assert st["devices_used"] == 1 and st["kernel_ms"] > 0
    assert np.isfinite(v.real) and np.isfinite(v.imag) and v != 0
    assert v == sup.perman_complex_range(a, c, c + 64, cpu=True, threads=16, walk_log2=10)


def test_gpu_complex_exact_gaussian_integer_anchor(sup):
    """The n = 8 Gaussian-integer case of test_complex.py (every intermediate
    exactly representable): the device gives the exact permanent."""
    a = gauss_int_case(8, 3)
    assert sup.perman_complex(a) == as_complex(exact_perm(a))


def test_cli_complex_gpu(sup, tmp_path):
    n = 13
    a = dense_complex(n, 4)
    ent = [(i + 1, j + 1, float(a[i, j].real), float(a[i, j].imag)) for i in range(n) for j in range(n)]
    path = write_mtx(tmp_path / "m.mtx", "general", n, ent)
    exe = os.path.join(os.path.dirname(sup.__file__), "bin", "perman")
    out = subprocess.run([exe, "-f", path, "--complex", "-g"], capture_output=True, text=True, check=True).stdout
    line = [l for l in out.splitlines() if l.startswith("Permanent:")][0].split()
    assert complex(float(line[1]), float(line[2])) == sup.perman_complex(a, cpu=True)
    assert "gpu_perman64_complex" in out
