"""CPU (host-emulated kernels): trajectory-prediction inference -- csrc/predict.hip through ops.predict, and
Prediction_policy.predict / evaluate -- against the fp64 oracle (tests/predict_checks.py)."""
import pytest

from iplan_amd import _lib as L
from tests import predict_checks as PC
from tests.emu.emu_lib import get_emu_lib


@pytest.fixture(autouse=True)
def emu():
    L.use_library_for_tests(get_emu_lib())
    yield
    L.use_library_for_tests(None)


@pytest.mark.parametrize("S,N,P,d,n_nets", PC.KERNEL_CASES)
def test_predict_kernel_vs_fp64(S, N, P, d, n_nets):
    PC.check_kernel("cpu", S, N, P, d, n_nets)


def test_predict_optional_operands():
    PC.check_optional_operands("cpu")


@pytest.mark.parametrize("S,N,P,d,n_nets", [(1, 17, 5, 5, 2), (5, 13, 3, 4, 1), (1, 2, 1, 16, 5)])
def test_predict_writes_only_what_it_owns(S, N, P, d, n_nets):
    PC.check_sentinel("cpu", S, N, P, d, n_nets)


def test_predict_weighting():
    PC.check_weighting("cpu")


def test_predict_repeatable():
    PC.check_repeatable("cpu")


def test_predict_agrees_with_training_forward():
    PC.check_agrees_with_training("cpu")


def test_policy_predict_on_loaded_checkpoint(tmp_path):
    PC.check_predict_method("cpu", tmp_path)


@pytest.mark.parametrize("stride", [1, 3])
def test_policy_evaluate_on_loaded_checkpoint(tmp_path, stride):
    PC.check_evaluate_method("cpu", tmp_path, stride)


def test_learn_unaffected_by_evaluate():
    PC.check_learn_unaffected_by_evaluate("cpu")
