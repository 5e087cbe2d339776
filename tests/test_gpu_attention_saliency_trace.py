"""GPU: attention saliency through time on the gfx950 build -- the checks the CPU suite runs through the host emulator
(tests/attention_saliency_trace_checks.py), where the MFMA layouts, the cross-lane reductions, the cotangent table in LDS and the
hand-off of the pair-step gradients between the waves of a workgroup are the hardware's; the entity counts at the upper edges of the
ego tile and of the four-tile workgroup, and one scene of 55 entities at the shipped tau, run here only.  Worst errors are logged the
way tests/test_gpu_parity_fullsize.py logs its own."""
import pytest

from tests import attention_saliency_trace_checks as TC
from tests.test_gpu_parity_fullsize import _log

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.mark.parametrize("case", TC.KERNEL_CASES_EMU + TC.KERNEL_CASES_GPU, ids=TC.kernel_case_id)
def test_trace_slots_are_the_one_step_kernels_bits(case):
    TC.check_kernel_bits(DEV, *case)


@pytest.mark.parametrize("target,noise,gate,targets,K", [("tensor", False, "through", None, 2), ("self", True, "through", [1, 3], 3),
                                                         (7, True, "held", [0, 2, 3], 1), ("self", False, "through", None, 0)])
def test_method_is_the_by_hand_route_of_the_one_step_methods(target, noise, gate, targets, K):
    TC.check_public_route(DEV, K=K, targets=targets, target=target, noise=noise, gate=gate)


@pytest.mark.parametrize("N,K,tau", TC.FP64_CASES + [(55, 2, 0.01)])
def test_trace_vs_fp64_per_lag(N, K, tau):
    _log(f"gat_saliency_trace_N{N}_K{K}_tau{tau}", TC.check_fp64(DEV, N, K, tau))


def test_trace_vs_fp64_held_gate_with_noise():
    _log("gat_saliency_trace_held_noise", TC.check_fp64(DEV, 5, 2, 0.25, gate="held", noise=True))


def test_trace_exact_statements():
    _log("attention_saliency_trace_exact", TC.check_exact(DEV))


def test_trace_is_linear_in_the_cotangent_at_every_lag():
    _log("gat_saliency_trace_linearity", TC.check_linearity(DEV))


def test_trace_slots_are_independent():
    TC.check_independence(DEV)


def test_trace_writes_only_what_it_owns():
    TC.check_ownership(DEV)


def test_trace_continues_the_policy_saliency_through_time():
    _log("attention_saliency_trace_chain", TC.check_chain(DEV))


def test_trace_touches_nothing():
    TC.check_touches_nothing(DEV)


def test_trace_entry_point_refusals():
    TC.check_entry_point_refusals(DEV)


def test_trace_method_refusals():
    TC.check_method_refusals(DEV)
