"""CPU (host-emulated kernels): behaviour-model inference -- csrc/behavior_eval.hip through ops.beh_eval, and
Behavior_policy.evaluate / latent_trace -- against the fp64 oracle (tests/behavior_eval_checks.py)."""
import pytest

from iplan_amd import _lib as L
from tests import behavior_eval_checks as BC
from tests.emu.emu_lib import get_emu_lib


@pytest.fixture(autouse=True)
def emu():
    L.use_library_for_tests(get_emu_lib())
    yield
    L.use_library_for_tests(None)


@pytest.mark.parametrize("E,N,Lw,J,d,Z,n_nets", BC.KERNEL_CASES)
def test_beh_eval_kernel_vs_fp64(E, N, Lw, J, d, Z, n_nets):
    BC.check_kernel("cpu", E, N, Lw, J, d, Z, n_nets)


def test_beh_eval_output_combinations():
    BC.check_output_combinations("cpu")


@pytest.mark.parametrize("E,N,Lw,J,d,Z,n_nets", [(1, 17, 2, 3, 5, 8, 2), (5, 13, 3, 2, 4, 1, 1), (1, 2, 1, 1, 12, 4, 5)])
def test_beh_eval_writes_only_what_it_owns(E, N, Lw, J, d, Z, n_nets):
    BC.check_sentinel("cpu", E, N, Lw, J, d, Z, n_nets)


def test_beh_eval_masks():
    BC.check_masks("cpu")


def test_beh_eval_repeatable():
    BC.check_repeatable("cpu")


def test_beh_eval_invalid_dims():
    BC.check_invalid_dims("cpu")


def test_beh_eval_agrees_with_training_forward():
    BC.check_agrees_with_training("cpu")


def test_policy_methods_on_loaded_checkpoint(tmp_path):
    BC.check_policy_methods("cpu", tmp_path)


def test_policy_evaluate_masks():
    BC.check_policy_masks("cpu")


def test_policy_dropout_and_rng():
    BC.check_dropout_and_rng("cpu")


def test_latent_trace_vs_latent_update(tmp_path):
    BC.check_latent_trace_vs_latent_update("cpu", tmp_path)


def test_learn_unaffected_by_evaluate():
    BC.check_learn_unaffected_by_evaluate("cpu")


def test_evaluate_after_deferred_learn():
    BC.check_evaluate_after_deferred_learn("cpu")


def test_subclasses_refuse():
    BC.check_subclasses_refuse("cpu")
