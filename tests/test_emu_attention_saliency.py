"""CPU (host-emulated kernels): attention saliency -- csrc/gat_saliency.hip through ops.gat_saliency, and
Prediction_policy.attention_saliency -- against fp64 autograd through the oracle (tests/attention_saliency_checks.py)."""
import pytest

from iplan_amd import _lib as L
from tests import attention_saliency_checks as SC
from tests.emu.emu_lib import get_emu_lib


@pytest.fixture(autouse=True)
def emu():
    L.use_library_for_tests(get_emu_lib())
    yield
    L.use_library_for_tests(None)


@pytest.mark.parametrize("case", SC.kernel_cases(SC.EDGE_N_EMU), ids=SC.case_id)
def test_saliency_kernel_vs_fp64(case):
    SC.check_kernel("cpu", *case)


@pytest.mark.parametrize("noise", [True, False])
def test_saliency_at_the_shipped_tau(noise):
    SC.check_shipped_tau("cpu", 1, 1, 17, noise)


def test_saliency_exact_statements():
    SC.check_exact("cpu")


def test_saliency_is_linear_in_the_cotangent():
    SC.check_linearity("cpu")


def test_saliency_writes_only_what_it_owns():
    SC.check_ownership("cpu")


def test_attention_saliency_method():
    SC.check_methods("cpu")


def test_attention_saliency_continues_the_policy_saliency():
    SC.check_chain("cpu")


def test_attention_saliency_touches_nothing():
    SC.check_touches_nothing("cpu")


def test_saliency_entry_point_refusals():
    SC.check_entry_point_refusals("cpu")


def test_attention_saliency_method_refusals():
    SC.check_method_refusals("cpu")
