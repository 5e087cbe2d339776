"""CPU (host-emulated kernels): the social knock-out chain through time -- csrc/policy_knockout_chain.hip through
ops.policy_knockout_trace(override=, override_base=), and DcntrlMAC.knockout_trace(override=, override_base=, social=) -- against the
nets' own trace of explicit batch copies, bit for bit, against knockout_trace and knockout where they overlap, against the two public
calls made by hand and against the fp64 oracle chain (tests/knockout_chain_checks.py)."""
import pytest

from iplan_amd import _lib as L
from tests import knockout_chain_checks as KC
from tests.emu.emu_lib import get_emu_lib


@pytest.fixture(autouse=True)
def emu():
    L.use_library_for_tests(get_emu_lib())
    yield
    L.use_library_for_tests(None)


@pytest.mark.parametrize("dims,J,win,opt,ch", KC.BIT_CASES, ids=KC.BIT_IDS)
def test_knockout_chain_same_bits_as_rerun(dims, J, win, opt, ch):
    KC.check_same_bits("cpu", dims, J, win, opt, ch)


def test_knockout_chain_reduces_to_knockout_trace():
    KC.check_reduces_to_knockout_trace("cpu")


def test_knockout_chain_agrees_with_knockout_at_one_step():
    KC.check_agrees_with_knockout("cpu")


@pytest.mark.parametrize("dims,win,opt", [(KC.DIMS, KC.WIN, {}), (KC.DIMS, (0, 2, 4), {}), ((1, 2, 4, 2, 5, 5), (1, 1, 3), dict(tanh=True, gat=False))])
def test_knockout_chain_exact_zeros(dims, win, opt):
    KC.check_exact_zeros("cpu", dims, win, opt)


def test_knockout_chain_social_equals_the_two_calls_by_hand(tmp_path):
    KC.check_social("cpu", tmp_path)


@pytest.mark.parametrize("dims,J,win,opt,ch", KC.FP64_CASES, ids=KC.FP64_IDS)
def test_knockout_chain_vs_fp64(dims, J, win, opt, ch):
    KC.check_vs_fp64("cpu", dims, J, win, opt, ch)


def test_knockout_chain_independence_and_repeatability():
    KC.check_independence("cpu")


@pytest.mark.parametrize("dims,J,win", [(KC.DIMS, 4, KC.WIN), ((1, 2, 3, 17, 5, 5), 16, (0, 2, 3)), ((1, 1, 1, 2, 5, 5), 1, (0, 1, 1))])
def test_knockout_chain_writes_only_what_it_owns(dims, J, win):
    KC.check_ownership("cpu", dims, J, win)


def test_knockout_chain_touches_nothing_and_train_unaffected():
    KC.check_touches_nothing("cpu")


def test_knockout_chain_method_on_loaded_checkpoint(tmp_path):
    KC.check_methods("cpu", tmp_path)


def test_knockout_chain_method_refusals():
    KC.check_method_refusals("cpu")


def test_knockout_chain_bad_arguments():
    KC.check_bad_arguments("cpu")


def test_knockout_chain_abi():
    KC.check_abi()
