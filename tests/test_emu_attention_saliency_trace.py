"""CPU (host-emulated kernels): attention saliency through time -- csrc/gat_saliency_trace.hip through ops.gat_saliency_trace, and
Prediction_policy.attention_saliency_trace -- against the one-step kernel and methods bit for bit, and against fp64 autograd through
the chained oracle (tests/attention_saliency_trace_checks.py)."""
import pytest

from iplan_amd import _lib as L
from tests import attention_saliency_trace_checks as TC
from tests.emu.emu_lib import get_emu_lib


@pytest.fixture(autouse=True)
def emu():
    L.use_library_for_tests(get_emu_lib())
    yield
    L.use_library_for_tests(None)


@pytest.mark.parametrize("case", TC.KERNEL_CASES_EMU, ids=TC.kernel_case_id)
def test_trace_slots_are_the_one_step_kernels_bits(case):
    TC.check_kernel_bits("cpu", *case)


@pytest.mark.parametrize("target,noise,gate,targets,K", [("tensor", False, "through", None, 2), ("self", True, "through", [1, 3], 3),
                                                         (7, True, "held", [0, 2, 3], 1), ("self", False, "through", None, 0)])
def test_method_is_the_by_hand_route_of_the_one_step_methods(target, noise, gate, targets, K):
    TC.check_public_route("cpu", K=K, targets=targets, target=target, noise=noise, gate=gate)


@pytest.mark.parametrize("N,K,tau", TC.FP64_CASES)
def test_trace_vs_fp64_per_lag(N, K, tau):
    TC.check_fp64("cpu", N, K, tau)


def test_trace_vs_fp64_held_gate_with_noise():
    TC.check_fp64("cpu", 5, 2, 0.25, gate="held", noise=True)


def test_trace_exact_statements():
    TC.check_exact("cpu")


def test_trace_is_linear_in_the_cotangent_at_every_lag():
    TC.check_linearity("cpu")


def test_trace_slots_are_independent():
    TC.check_independence("cpu")


def test_trace_writes_only_what_it_owns():
    TC.check_ownership("cpu")


def test_trace_continues_the_policy_saliency_through_time():
    TC.check_chain("cpu")


def test_trace_touches_nothing():
    TC.check_touches_nothing("cpu")


def test_trace_entry_point_refusals():
    TC.check_entry_point_refusals("cpu")


def test_trace_method_refusals():
    TC.check_method_refusals("cpu")
