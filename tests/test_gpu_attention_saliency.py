"""GPU: attention saliency on the gfx950 build -- the checks the CPU suite runs through the host emulator
(tests/attention_saliency_checks.py), where the MFMA layouts, the cross-lane reductions and the hand-off of the pair-step gradients
between the waves of a scene are the hardware's; the entity counts at the upper edges of the ego tile and of the four-tile
workgroup, and four scenes of 55 entities at the shipped tau, run here only.  Worst errors are logged the way
tests/test_gpu_parity_fullsize.py logs its own."""
import pytest

from tests import attention_saliency_checks as SC
from tests.test_gpu_parity_fullsize import _log

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.mark.parametrize("case", SC.kernel_cases(SC.EDGE_N_EMU) + SC.kernel_cases(SC.EDGE_N_GPU), ids=SC.case_id)
def test_saliency_kernel_vs_fp64(case):
    _log("gat_saliency_" + SC.case_id(case), SC.check_kernel(DEV, *case))


@pytest.mark.parametrize("n,B,N,noise", [(1, 1, 17, True), (1, 1, 17, False), (1, 4, 55, True), (1, 4, 55, False)])
def test_saliency_at_the_shipped_tau(n, B, N, noise):
    _log(f"gat_saliency_tau0.01_B{B}_N{N}_{'noise' if noise else 'nonoise'}", SC.check_shipped_tau(DEV, n, B, N, noise))


def test_saliency_exact_statements():
    SC.check_exact(DEV)


def test_saliency_is_linear_in_the_cotangent():
    _log("gat_saliency_linearity", SC.check_linearity(DEV))


def test_saliency_writes_only_what_it_owns():
    SC.check_ownership(DEV)


def test_attention_saliency_method():
    _log("attention_saliency_method", SC.check_methods(DEV))


def test_attention_saliency_continues_the_policy_saliency():
    _log("attention_saliency_chain", SC.check_chain(DEV))


def test_attention_saliency_touches_nothing():
    SC.check_touches_nothing(DEV)


def test_saliency_entry_point_refusals():
    SC.check_entry_point_refusals(DEV)


def test_attention_saliency_method_refusals():
    SC.check_method_refusals(DEV)
