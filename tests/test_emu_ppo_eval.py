"""CPU (host-emulated kernels): PPO inspection -- csrc/ppo_eval.hip through ops.ppo_eval, and IPPOLearner.evaluate -- against the fp64
oracle (tests/ppo_eval_checks.py)."""
import pytest

from iplan_amd import _lib as L
from tests import ppo_eval_checks as PC
from tests.emu.emu_lib import get_emu_lib


@pytest.fixture(autouse=True)
def emu():
    L.use_library_for_tests(get_emu_lib())
    yield
    L.use_library_for_tests(None)


@pytest.mark.parametrize("shape,masked,flags", PC.KERNEL_CASES, ids=PC.CASE_IDS)
def test_eval_kernel_vs_fp64(shape, masked, flags):
    PC.check_kernel("cpu", shape, masked, flags)


def test_eval_any_number_of_workgroups_same_bits():
    PC.check_parts("cpu")


def test_eval_repeatable():
    PC.check_repeatable("cpu", 2)


def test_eval_writes_only_what_it_owns():
    PC.check_sentinel("cpu")


def test_eval_reads_only_what_it_owns():
    PC.check_poison("cpu")


def test_eval_same_policy_is_exact():
    PC.check_identity("cpu")


def test_eval_agrees_with_prepare():
    PC.check_agrees_with_prepare("cpu")


def test_eval_agrees_with_loss_kernel():
    PC.check_agrees_with_loss("cpu")


def test_eval_bad_arguments():
    PC.check_bad_arguments("cpu")


def test_evaluate_vs_oracle():
    PC.check_method("cpu")


def test_evaluate_vs_train_and_snapshot():
    PC.check_method_vs_train("cpu")


def test_train_unaffected_by_evaluate():
    PC.check_train_unaffected("cpu")
