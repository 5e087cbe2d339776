"""GPU: behaviour-model inference on the gfx950 build -- the same checks the CPU suite runs through the host emulator
(tests/behavior_eval_checks.py), where the MFMA layouts, the cross-lane moves and reductions, the unaligned row loads, the LDS
budget and the grid geometry are the hardware's -- plus the device-memory condition.  Worst errors are logged the way
tests/test_gpu_parity_fullsize.py logs its own."""
import pytest

from tests import behavior_eval_checks as BC
from tests.test_gpu_parity_fullsize import _log

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.mark.parametrize("E,N,Lw,J,d,Z,n_nets", BC.KERNEL_CASES)
def test_beh_eval_kernel_vs_fp64(E, N, Lw, J, d, Z, n_nets):
    _log(f"beh_eval_kernel_E{E}_N{N}_L{Lw}_J{J}_d{d}_Z{Z}_n{n_nets}", BC.check_kernel(DEV, E, N, Lw, J, d, Z, n_nets))


def test_beh_eval_output_combinations():
    _log("beh_eval_output_combinations", BC.check_output_combinations(DEV))


@pytest.mark.parametrize("E,N,Lw,J,d,Z,n_nets", [(1, 17, 2, 3, 5, 8, 2), (5, 13, 3, 2, 4, 1, 1), (1, 2, 1, 1, 12, 4, 5)])
def test_beh_eval_writes_only_what_it_owns(E, N, Lw, J, d, Z, n_nets):
    BC.check_sentinel(DEV, E, N, Lw, J, d, Z, n_nets)


def test_beh_eval_masks():
    _log("beh_eval_masks", BC.check_masks(DEV))


def test_beh_eval_repeatable():
    BC.check_repeatable(DEV)


def test_beh_eval_invalid_dims():
    BC.check_invalid_dims(DEV)


def test_beh_eval_agrees_with_training_forward():
    _log("beh_eval_vs_training_forward", BC.check_agrees_with_training(DEV))


def test_policy_methods_on_loaded_checkpoint(tmp_path):
    _log("beh_eval_policy_methods", BC.check_policy_methods(DEV, tmp_path))


def test_policy_evaluate_masks():
    BC.check_policy_masks(DEV)


def test_policy_dropout_and_rng():
    BC.check_dropout_and_rng(DEV)


def test_latent_trace_vs_latent_update(tmp_path):
    _log("beh_eval_trace_vs_latent_update", BC.check_latent_trace_vs_latent_update(DEV, tmp_path))


def test_learn_unaffected_by_evaluate():
    BC.check_learn_unaffected_by_evaluate(DEV)


def test_evaluate_after_deferred_learn():
    BC.check_evaluate_after_deferred_learn(DEV)


def test_subclasses_refuse():
    BC.check_subclasses_refuse(DEV)


def test_evaluate_device_memory():
    _log("beh_eval_device_memory", BC.check_device_memory(DEV))
