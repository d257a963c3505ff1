"""The boson sampler on the GPU (sup_boson_sample with the minors on the
device): the samples equal the host twin's exactly, and follow the outcome
distribution."""
import numpy as np
import pytest

from test_boson_sample import CHI2_34_1M, chi_square, haar_unitary, outcome_distribution

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def need_gpu(sup):
    if sup.device_count() < 1:
        pytest.fail("no HIP device visible: -m gpu tests must run on the MI355X box")


@pytest.mark.parametrize("M,inputs,nsamples", [(6, [0, 1, 3, 5], 257), (8, [7, 0, 2, 3, 5, 6], 65)])
def test_gpu_samples_equal_the_host_twin(sup, M, inputs, nsamples):
    U = haar_unitary(M, 100 + M)
    got, st = sup.boson_sample(U, inputs, nsamples, seed=77, return_stats=True)
    assert st["devices_used"] == 1 and st["kernel_ms"] > 0 and st["leaves"] == nsamples
    assert np.array_equal(got, sup.boson_sample(U, inputs, nsamples, seed=77, cpu=True))


def test_gpu_outcome_distribution_chi_square(sup):
    U, P = outcome_distribution()
    s = sup.boson_sample(U, [0, 2, 3], 20000, seed=4)
    chi2 = chi_square(s, P)
    print(f"seed 4 (device): chi2 = {chi2:.1f} over 35 cells (threshold {CHI2_34_1M})")
    assert chi2 < CHI2_34_1M
