"""GPU: policy knock-out attribution on the gfx950 build -- the same checks the CPU suite runs through the host emulator
(tests/policy_knockout_checks.py), where the MFMA layouts, the cross-lane reads of the tile's base column and the rounding of the KL
epilogue are the hardware's.  Worst errors are logged the way tests/test_gpu_parity_fullsize.py logs its own."""
import pytest

from tests import policy_knockout_checks as PK
from tests.test_gpu_parity_fullsize import _log

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.mark.parametrize("dims,J,opt", PK.KERNEL_CASES, ids=PK.CASE_IDS)
def test_policy_knockout_same_bits_as_rerun(dims, J, opt):
    _log("policy_knockout_same_bits_" + PK.CASE_IDS[PK.KERNEL_CASES.index((dims, J, opt))], PK.check_same_bits(DEV, dims, J, opt))


@pytest.mark.parametrize("sources,baseline", PK.SOURCE_CASES)
def test_policy_knockout_sources_and_baseline(sources, baseline):
    PK.check_sources_and_baseline(DEV, sources, baseline)


def test_policy_knockout_no_flag_is_the_base():
    PK.check_no_flag(DEV)


def test_policy_knockout_override():
    PK.check_override(DEV)


@pytest.mark.parametrize("dims,J,opt", PK.FP64_CASES, ids=PK.FP64_IDS)
def test_policy_knockout_vs_fp64(dims, J, opt):
    _log("policy_knockout_fp64_" + PK.FP64_IDS[PK.FP64_CASES.index((dims, J, opt))], PK.check_vs_fp64(DEV, dims, J, opt))


@pytest.mark.parametrize("dims,opt,mode", [((2, 3, 2, 3, 5, 5), {}, "zeros"), ((2, 3, 2, 3, 5, 5), {}, "baseline"),
                                           ((1, 2, 2, 2, 5, 5), dict(tanh=True, gat=False), "zeros")])
def test_policy_knockout_exact_zeros(dims, opt, mode):
    PK.check_exact_zeros(DEV, dims, opt, mode)


def test_policy_knockout_independence():
    PK.check_independence(DEV)


def test_policy_knockout_repeatable():
    PK.check_repeatable(DEV, 20)


@pytest.mark.parametrize("dims,J", [((2, 3, 2, 3, 5, 5), 4), ((1, 5, 1, 3, 5, 5), 16), ((1, 1, 1, 2, 5, 5), 1)])
def test_policy_knockout_writes_only_what_it_owns(dims, J):
    PK.check_ownership(DEV, dims, J)


@pytest.mark.parametrize("steps", [1, slice(1, 3)], ids=["one_step", "sliced"])
def test_policy_knockout_method_on_loaded_checkpoint(tmp_path, steps):
    _log(f"policy_knockout_methods_{steps}", PK.check_methods(DEV, tmp_path, steps))


def test_policy_knockout_chain_from_attention_knockout(tmp_path):
    PK.check_chain(DEV, tmp_path)


def test_policy_knockout_touches_nothing_and_train_unaffected():
    PK.check_touches_nothing(DEV)


def test_policy_knockout_bad_arguments():
    PK.check_bad_arguments(DEV)


def test_policy_knockout_method_refusals():
    PK.check_method_refusals(DEV)


def test_policy_knockout_abi():
    PK.check_abi()
