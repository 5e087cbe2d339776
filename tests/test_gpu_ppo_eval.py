"""GPU: PPO inspection on the gfx950 build -- the same checks the CPU suite runs through the host emulator (tests/ppo_eval_checks.py),
where the wave butterflies, the workgroup barriers, expf and the launch boundaries between the phases are the hardware's.  Worst
errors are logged the way tests/test_gpu_parity_fullsize.py logs its own."""
import pytest

from tests import ppo_eval_checks as PC
from tests.test_gpu_parity_fullsize import _log

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.mark.parametrize("shape,masked,flags", PC.KERNEL_CASES, ids=PC.CASE_IDS)
def test_eval_kernel_vs_fp64(shape, masked, flags):
    _log("ppo_eval_kernel_" + "_".join(map(str, shape)) + ("_terminated" if masked else "_all_live") + f"_flags{flags}", PC.check_kernel(DEV, shape, masked, flags))


def test_eval_any_number_of_workgroups_same_bits():
    PC.check_parts(DEV)


def test_eval_repeatable():
    PC.check_repeatable(DEV, 20)


def test_eval_writes_only_what_it_owns():
    PC.check_sentinel(DEV)


def test_eval_reads_only_what_it_owns():
    PC.check_poison(DEV)


def test_eval_same_policy_is_exact():
    PC.check_identity(DEV)


def test_eval_agrees_with_prepare():
    _log("ppo_eval_vs_prepare", PC.check_agrees_with_prepare(DEV))


def test_eval_agrees_with_loss_kernel():
    _log("ppo_eval_vs_loss_kernel", PC.check_agrees_with_loss(DEV))


def test_eval_bad_arguments():
    PC.check_bad_arguments(DEV)


def test_evaluate_vs_oracle():
    _log("ppo_evaluate_method", PC.check_method(DEV))


def test_evaluate_vs_train_and_snapshot():
    _log("ppo_evaluate_vs_train_and_snapshot", PC.check_method_vs_train(DEV))


def test_train_unaffected_by_evaluate():
    PC.check_train_unaffected(DEV)
