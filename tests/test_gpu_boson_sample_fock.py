"""The boson sampler on the collision-aware one-walk minors on the GPU
(sup_boson_sample_fock; walk_cplxfm.hip per stage): the device draws the host
twin's samples."""
import numpy as np
import pytest

from test_boson_sample import CHI2_34_1M, chi_square, haar_unitary, outcome_distribution

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def need_gpu(sup):
    if sup.device_count() < 1:
        pytest.fail("no HIP device visible: -m gpu tests must run on the MI355X box")


@pytest.mark.parametrize("M,inputs,nsamples", [(5, [0, 2, 3], 1000), (8, [1, 4, 5, 7, 0], 300), (16, list(range(12)), 40),
                                              (4, [2], 64)])
def test_gpu_samples_equal_the_host_twin(sup, M, inputs, nsamples):
    """Stage k walks T <= 2^(k-2) states: at most 2^10 at 12 photons (Tw <=
    16, H = 64 there; Tw = 1, H = T below T = 128); one photon walks nothing."""
    U = haar_unitary(M, 40 + M)
    want = sup.boson_sample(U, inputs, nsamples, seed=21, cpu=True, threads=16, collision_aware=True)
    got, st = sup.boson_sample(U, inputs, nsamples, seed=21, return_stats=True, collision_aware=True)
    assert np.array_equal(got, want)
    n = len(inputs)
    assert st["gray_steps"] == nsamples * sum(1 << (k - 2) for k in range(2, n + 1))
    assert st["visited_steps"] <= st["gray_steps"] and st["leaves"] == nsamples
    assert st["devices_used"] == (1 if n > 1 else 0) and (st["kernel_ms"] > 0) == (n > 1)


def test_gpu_outcome_distribution_chi_square(sup):
    """test_boson_sample's chi^2 test on the device path: M = 5, inputs
    [0, 2, 3], 20000 samples, the same quantile (T <= 2, Tw = 1, H = T)."""
    U, P = outcome_distribution()
    s = sup.boson_sample(U, [0, 2, 3], 20000, seed=4, collision_aware=True)
    chi2 = chi_square(s, P)
    print(f"chi2 = {chi2:.1f} over 35 cells (threshold {CHI2_34_1M})")
    assert chi2 < CHI2_34_1M
