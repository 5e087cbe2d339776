"""GPU: the social knock-out chain through time on the gfx950 build -- the same checks the CPU suite runs through the host emulator
(tests/knockout_chain_checks.py), where the MFMA layouts, the per-column override gather, the LDS hand-off of the per-job states and
the rounding of the KL and state-shift epilogues are the hardware's.  Worst errors are logged the way tests/test_gpu_parity_fullsize.py
logs its own."""
import pytest

from tests import knockout_chain_checks as KC
from tests.test_gpu_parity_fullsize import _log

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.mark.parametrize("dims,J,win,opt,ch", KC.BIT_CASES, ids=KC.BIT_IDS)
def test_knockout_chain_same_bits_as_rerun(dims, J, win, opt, ch):
    KC.check_same_bits(DEV, dims, J, win, opt, ch)


def test_knockout_chain_reduces_to_knockout_trace():
    KC.check_reduces_to_knockout_trace(DEV)


def test_knockout_chain_agrees_with_knockout_at_one_step():
    _log("knockout_chain_vs_knockout", KC.check_agrees_with_knockout(DEV))


@pytest.mark.parametrize("dims,win,opt", [(KC.DIMS, KC.WIN, {}), (KC.DIMS, (0, 2, 4), {}), ((1, 2, 4, 2, 5, 5), (1, 1, 3), dict(tanh=True, gat=False))])
def test_knockout_chain_exact_zeros(dims, win, opt):
    KC.check_exact_zeros(DEV, dims, win, opt)


def test_knockout_chain_social_equals_the_two_calls_by_hand(tmp_path):
    KC.check_social(DEV, tmp_path)


@pytest.mark.parametrize("dims,J,win,opt,ch", KC.FP64_CASES, ids=KC.FP64_IDS)
def test_knockout_chain_vs_fp64(dims, J, win, opt, ch):
    _log("knockout_chain_fp64_" + KC.FP64_IDS[KC.FP64_CASES.index((dims, J, win, opt, ch))], KC.check_vs_fp64(DEV, dims, J, win, opt, ch))


def test_knockout_chain_independence_and_repeatability():
    KC.check_independence(DEV)


@pytest.mark.parametrize("dims,J,win", [(KC.DIMS, 4, KC.WIN), ((1, 2, 3, 17, 5, 5), 16, (0, 2, 3)), ((1, 1, 1, 2, 5, 5), 1, (0, 1, 1))])
def test_knockout_chain_writes_only_what_it_owns(dims, J, win):
    KC.check_ownership(DEV, dims, J, win)


def test_knockout_chain_touches_nothing_and_train_unaffected():
    KC.check_touches_nothing(DEV)


def test_knockout_chain_method_on_loaded_checkpoint(tmp_path):
    _log("knockout_chain_methods", KC.check_methods(DEV, tmp_path))


def test_knockout_chain_method_refusals():
    KC.check_method_refusals(DEV)


def test_knockout_chain_bad_arguments():
    KC.check_bad_arguments(DEV)


def test_knockout_chain_abi():
    KC.check_abi()
