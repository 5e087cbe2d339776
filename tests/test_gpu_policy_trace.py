"""GPU: policy inspection on the gfx950 build -- the same checks the CPU suite runs through the host emulator
(tests/policy_trace_checks.py), where the MFMA layouts, the cross-lane reductions, the per-step barrier and the LDS hand-off of the
GRU state are the hardware's.  Worst errors are logged the way tests/test_gpu_parity_fullsize.py logs its own."""
import pytest

from tests import policy_trace_checks as PC
from tests.test_gpu_parity_fullsize import _log

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.mark.parametrize("dims,opt", PC.KERNEL_CASES, ids=PC.CASE_IDS)
def test_trace_kernel_vs_fp64(dims, opt):
    _log("policy_trace_kernel_" + "_".join(map(str, dims)) + "".join(f"_{k}{v}" for k, v in sorted(opt.items())), PC.check_kernel(DEV, dims, opt))


def test_trace_step_splitting_is_exact():
    PC.check_step_splitting(DEV)


def test_trace_tiling_is_exact():
    PC.check_tiling(DEV)


def test_trace_writes_only_what_it_owns():
    PC.check_sentinel(DEV)


def test_trace_reads_only_what_it_owns():
    PC.check_poison(DEV)


def test_trace_optional_operands():
    _log("policy_trace_optional_operands", PC.check_optional_operands(DEV))


def test_trace_agrees_with_one_step_kernel():
    _log("policy_trace_vs_ac_forward", PC.check_agrees_with_ac_forward(DEV))


@pytest.mark.parametrize("n_act", [5, 3])
def test_inspection_ops_share_one_categorical(n_act):
    PC.check_one_categorical(DEV, n_act)


def test_trace_repeatable():
    PC.check_repeatable(DEV, 20)


def test_trace_bad_arguments():
    PC.check_bad_arguments(DEV)


def test_policy_methods_on_loaded_checkpoint(tmp_path):
    _log("policy_trace_methods", PC.check_methods(DEV, tmp_path))


def test_trace_replays_rollout():
    _log("policy_trace_replays_rollout", PC.check_replays_rollout(DEV))


def test_train_unaffected_by_trace():
    PC.check_train_unaffected(DEV)
