"""CPU (host-emulated kernels): policy knock-out attribution -- csrc/policy_knockout.hip through ops.policy_knockout, and
DcntrlMAC.knockout -- against the same method on explicit batch copies, bit for bit, against one-step traces and against the fp64
oracle (tests/policy_knockout_checks.py)."""
import pytest

from iplan_amd import _lib as L
from tests import policy_knockout_checks as PK
from tests.emu.emu_lib import get_emu_lib


@pytest.fixture(autouse=True)
def emu():
    L.use_library_for_tests(get_emu_lib())
    yield
    L.use_library_for_tests(None)


@pytest.mark.parametrize("dims,J,opt", PK.KERNEL_CASES, ids=PK.CASE_IDS)
def test_policy_knockout_same_bits_as_rerun(dims, J, opt):
    PK.check_same_bits("cpu", dims, J, opt)


@pytest.mark.parametrize("sources,baseline", PK.SOURCE_CASES)
def test_policy_knockout_sources_and_baseline(sources, baseline):
    PK.check_sources_and_baseline("cpu", sources, baseline)


def test_policy_knockout_no_flag_is_the_base():
    PK.check_no_flag("cpu")


def test_policy_knockout_override():
    PK.check_override("cpu")


@pytest.mark.parametrize("dims,J,opt", PK.FP64_CASES, ids=PK.FP64_IDS)
def test_policy_knockout_vs_fp64(dims, J, opt):
    PK.check_vs_fp64("cpu", dims, J, opt)


@pytest.mark.parametrize("dims,opt,mode", [((2, 3, 2, 3, 5, 5), {}, "zeros"), ((2, 3, 2, 3, 5, 5), {}, "baseline"),
                                           ((1, 2, 2, 2, 5, 5), dict(tanh=True, gat=False), "zeros")])
def test_policy_knockout_exact_zeros(dims, opt, mode):
    PK.check_exact_zeros("cpu", dims, opt, mode)


def test_policy_knockout_independence():
    PK.check_independence("cpu")


def test_policy_knockout_repeatable():
    PK.check_repeatable("cpu", 2)


@pytest.mark.parametrize("dims,J", [((2, 3, 2, 3, 5, 5), 4), ((1, 5, 1, 3, 5, 5), 16), ((1, 1, 1, 2, 5, 5), 1)])
def test_policy_knockout_writes_only_what_it_owns(dims, J):
    PK.check_ownership("cpu", dims, J)


@pytest.mark.parametrize("steps", [1, slice(1, 3)], ids=["one_step", "sliced"])
def test_policy_knockout_method_on_loaded_checkpoint(tmp_path, steps):
    PK.check_methods("cpu", tmp_path, steps)


def test_policy_knockout_chain_from_attention_knockout(tmp_path):
    PK.check_chain("cpu", tmp_path)


def test_policy_knockout_touches_nothing_and_train_unaffected():
    PK.check_touches_nothing("cpu")


def test_policy_knockout_bad_arguments():
    PK.check_bad_arguments("cpu")


def test_policy_knockout_method_refusals():
    PK.check_method_refusals("cpu")


def test_policy_knockout_abi():
    PK.check_abi()
