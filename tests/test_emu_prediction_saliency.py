"""CPU (host-emulated kernels): prediction saliency -- csrc/pdec_saliency.hip through ops.pdec_saliency, and
Prediction_policy.prediction_saliency -- against fp64 autograd through the oracle (tests/prediction_saliency_checks.py)."""
import pytest

from iplan_amd import _lib as L
from tests import prediction_saliency_checks as SC
from tests.emu.emu_lib import get_emu_lib


@pytest.fixture(autouse=True)
def emu():
    L.use_library_for_tests(get_emu_lib())
    yield
    L.use_library_for_tests(None)


@pytest.mark.parametrize("case", SC.KERNEL_CASES, ids=SC.case_id)
def test_saliency_kernel_vs_fp64(case):
    SC.check_kernel("cpu", *case)


def test_saliency_every_combination_of_outputs():
    SC.check_output_combinations("cpu")


def test_saliency_exact_statements():
    SC.check_exact("cpu")


def test_saliency_is_linear_in_the_cotangent():
    SC.check_linearity("cpu")


def test_saliency_reads_in_place_and_writes_only_what_it_owns():
    SC.check_ownership("cpu")


def test_prediction_saliency_method():
    SC.check_methods("cpu")


def test_prediction_saliency_continues_through_the_gat():
    SC.check_chain("cpu")


def test_prediction_saliency_touches_nothing():
    SC.check_touches_nothing("cpu")


def test_saliency_entry_point_refusals():
    SC.check_entry_point_refusals("cpu")


def test_prediction_saliency_method_refusals():
    SC.check_method_refusals("cpu")
