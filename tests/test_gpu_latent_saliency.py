"""GPU: intent saliency on the gfx950 build -- the same checks the CPU suite runs through the host emulator
(tests/latent_saliency_checks.py), where the MFMA layouts, the cross-lane reductions, the LDS budget of the weights in both
orientations beside the per-wave slabs and the grid geometry are the hardware's.  Worst errors are logged the way
tests/test_gpu_parity_fullsize.py logs its own."""
import pytest

from tests import latent_saliency_checks as SC
from tests.test_gpu_parity_fullsize import _log

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.mark.parametrize("E,N,d,Z,Lw,J,n_nets,K,windows,target", SC.KERNEL_CASES)
def test_enc_saliency_kernel_vs_fp64(E, N, d, Z, Lw, J, n_nets, K, windows, target):
    name = f"enc_saliency_kernel_E{E}_N{N}_d{d}_Z{Z}_L{Lw}_J{J}_n{n_nets}_K{K}_{target}"
    _log(name, SC.check_kernel(DEV, E, N, d, Z, Lw, J, n_nets, K, windows, target))


def test_enc_saliency_window_lengths():
    _log("enc_saliency_window_lengths", SC.check_window_lengths(DEV))


def test_enc_saliency_exact_zeros():
    SC.check_exact_zeros(DEV)


def test_enc_saliency_linear_in_the_cotangent():
    _log("enc_saliency_linearity", SC.check_linearity(DEV))


def test_enc_saliency_placement_and_repeatability():
    SC.check_placement(DEV)


@pytest.mark.parametrize("E,N,d,Z,Lw,J,n_nets,K,windows", [(1, 17, 5, 8, 2, 4, 2, 1, (1, 3)), (3, 11, 12, 1, 3, 3, 1, 2, (0, 2)), (1, 2, 16, 16, 1, 2, 5, 0, (0, 1))])
def test_enc_saliency_writes_only_what_it_owns(E, N, d, Z, Lw, J, n_nets, K, windows):
    SC.check_sentinel(DEV, E, N, d, Z, Lw, J, n_nets, K, windows)


def test_enc_saliency_latent_vs_latent_trace():
    _log("enc_saliency_latent_vs_latent_trace", SC.check_latent_vs_trace(DEV))


def test_latent_saliency_on_loaded_checkpoint(tmp_path):
    _log("latent_saliency_policy_methods", SC.check_policy_methods(DEV, tmp_path))


def test_latent_saliency_touches_nothing():
    SC.check_touches_nothing(DEV)


def test_enc_saliency_refusals():
    SC.check_kernel_refusals(DEV)


def test_latent_saliency_refusals():
    SC.check_method_refusals(DEV)
