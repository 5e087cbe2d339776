"""CPU (host-emulated kernels): intent saliency -- csrc/enc_saliency.hip through ops.enc_saliency, and
Behavior_policy.latent_saliency -- against fp64 autograd through the restated encoder chain (tests/latent_saliency_checks.py)."""
import pytest

from iplan_amd import _lib as L
from tests import latent_saliency_checks as SC
from tests.emu.emu_lib import get_emu_lib


@pytest.fixture(autouse=True)
def emu():
    L.use_library_for_tests(get_emu_lib())
    yield
    L.use_library_for_tests(None)


@pytest.mark.parametrize("E,N,d,Z,Lw,J,n_nets,K,windows,target", SC.KERNEL_CASES)
def test_enc_saliency_kernel_vs_fp64(E, N, d, Z, Lw, J, n_nets, K, windows, target):
    SC.check_kernel("cpu", E, N, d, Z, Lw, J, n_nets, K, windows, target)


def test_enc_saliency_window_lengths():
    SC.check_window_lengths("cpu")


def test_enc_saliency_exact_zeros():
    SC.check_exact_zeros("cpu")


def test_enc_saliency_linear_in_the_cotangent():
    SC.check_linearity("cpu")


def test_enc_saliency_placement_and_repeatability():
    SC.check_placement("cpu")


@pytest.mark.parametrize("E,N,d,Z,Lw,J,n_nets,K,windows", [(1, 17, 5, 8, 2, 4, 2, 1, (1, 3)), (3, 11, 12, 1, 3, 3, 1, 2, (0, 2)), (1, 2, 16, 16, 1, 2, 5, 0, (0, 1))])
def test_enc_saliency_writes_only_what_it_owns(E, N, d, Z, Lw, J, n_nets, K, windows):
    SC.check_sentinel("cpu", E, N, d, Z, Lw, J, n_nets, K, windows)


def test_enc_saliency_latent_vs_latent_trace():
    SC.check_latent_vs_trace("cpu")


def test_latent_saliency_on_loaded_checkpoint(tmp_path):
    SC.check_policy_methods("cpu", tmp_path)


def test_latent_saliency_touches_nothing():
    SC.check_touches_nothing("cpu")


def test_enc_saliency_refusals():
    SC.check_kernel_refusals("cpu")


def test_latent_saliency_refusals():
    SC.check_method_refusals("cpu")
