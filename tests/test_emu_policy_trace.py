"""CPU (host-emulated kernels): policy inspection -- csrc/policy_trace.hip through ops.policy_trace, and DcntrlMAC.policy_trace /
action_distribution -- against the fp64 oracle (tests/policy_trace_checks.py)."""
import pytest

from iplan_amd import _lib as L
from tests import policy_trace_checks as PC
from tests.emu.emu_lib import get_emu_lib


@pytest.fixture(autouse=True)
def emu():
    L.use_library_for_tests(get_emu_lib())
    yield
    L.use_library_for_tests(None)


@pytest.mark.parametrize("dims,opt", PC.KERNEL_CASES, ids=PC.CASE_IDS)
def test_trace_kernel_vs_fp64(dims, opt):
    PC.check_kernel("cpu", dims, opt)


def test_trace_step_splitting_is_exact():
    PC.check_step_splitting("cpu")


def test_trace_tiling_is_exact():
    PC.check_tiling("cpu")


def test_trace_writes_only_what_it_owns():
    PC.check_sentinel("cpu")


def test_trace_reads_only_what_it_owns():
    PC.check_poison("cpu")


def test_trace_optional_operands():
    PC.check_optional_operands("cpu")


def test_trace_agrees_with_one_step_kernel():
    PC.check_agrees_with_ac_forward("cpu")


@pytest.mark.parametrize("n_act", [5, 3])
def test_inspection_ops_share_one_categorical(n_act):
    PC.check_one_categorical("cpu", n_act)


def test_trace_repeatable():
    PC.check_repeatable("cpu", 2)


def test_trace_bad_arguments():
    PC.check_bad_arguments("cpu")


def test_policy_methods_on_loaded_checkpoint(tmp_path):
    PC.check_methods("cpu", tmp_path)


def test_trace_replays_rollout():
    PC.check_replays_rollout("cpu")


def test_train_unaffected_by_trace():
    PC.check_train_unaffected("cpu")
