"""GPU: trajectory-prediction inference on the gfx950 build -- the same checks the CPU suite runs through the host emulator
(tests/predict_checks.py), where the MFMA layouts, the cross-lane reductions, the unaligned row loads and the grid geometry are
the hardware's.  Worst errors are logged the way tests/test_gpu_parity_fullsize.py logs its own."""
import pytest

from tests import predict_checks as PC
from tests.test_gpu_parity_fullsize import _log

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.mark.parametrize("S,N,P,d,n_nets", PC.KERNEL_CASES)
def test_predict_kernel_vs_fp64(S, N, P, d, n_nets):
    _log(f"predict_kernel_S{S}_N{N}_P{P}_d{d}_n{n_nets}", PC.check_kernel(DEV, S, N, P, d, n_nets))


def test_predict_optional_operands():
    _log("predict_optional_operands", PC.check_optional_operands(DEV))


@pytest.mark.parametrize("S,N,P,d,n_nets", [(1, 17, 5, 5, 2), (5, 13, 3, 4, 1), (1, 2, 1, 16, 5)])
def test_predict_writes_only_what_it_owns(S, N, P, d, n_nets):
    PC.check_sentinel(DEV, S, N, P, d, n_nets)


def test_predict_weighting():
    _log("predict_weighting", PC.check_weighting(DEV))


def test_predict_repeatable():
    PC.check_repeatable(DEV)


def test_predict_agrees_with_training_forward():
    _log("predict_vs_training_forward", PC.check_agrees_with_training(DEV))


def test_policy_predict_on_loaded_checkpoint(tmp_path):
    _log("predict_method", PC.check_predict_method(DEV, tmp_path))


@pytest.mark.parametrize("stride", [1, 3])
def test_policy_evaluate_on_loaded_checkpoint(tmp_path, stride):
    _log(f"evaluate_method_stride{stride}", PC.check_evaluate_method(DEV, tmp_path, stride))


def test_learn_unaffected_by_evaluate():
    PC.check_learn_unaffected_by_evaluate(DEV)
