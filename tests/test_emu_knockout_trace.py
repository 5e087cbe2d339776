"""CPU (host-emulated kernels): policy knock-out through time -- csrc/policy_knockout_trace.hip through ops.policy_knockout_trace, and
DcntrlMAC.knockout_trace -- against the nets' own trace of explicit batch copies, bit for bit, against knockout() at the first step and
against the fp64 oracle chain (tests/knockout_trace_checks.py)."""
import pytest

from iplan_amd import _lib as L
from tests import knockout_trace_checks as KT
from tests.emu.emu_lib import get_emu_lib


@pytest.fixture(autouse=True)
def emu():
    L.use_library_for_tests(get_emu_lib())
    yield
    L.use_library_for_tests(None)


@pytest.mark.parametrize("dims,J,win,opt", KT.BIT_CASES, ids=KT.BIT_IDS)
def test_knockout_trace_same_bits_as_rerun(dims, J, win, opt):
    KT.check_same_bits("cpu", dims, J, win, opt)


def test_knockout_trace_agrees_with_knockout_at_first_step():
    KT.check_agrees_with_knockout("cpu")


@pytest.mark.parametrize("dims,J,win,opt", KT.FP64_CASES, ids=KT.FP64_IDS)
def test_knockout_trace_vs_fp64(dims, J, win, opt):
    KT.check_vs_fp64("cpu", dims, J, win, opt)


@pytest.mark.parametrize("dims,win,opt,mode", [(KT.DIMS, KT.WIN, {}, "zeros"), (KT.DIMS, (0, 2, 4), {}, "baseline"),
                                               ((1, 2, 4, 2, 5, 5), (1, 1, 3), dict(tanh=True, gat=False), "zeros")])
def test_knockout_trace_exact_zeros(dims, win, opt, mode):
    KT.check_exact_zeros("cpu", dims, win, opt, mode)


def test_knockout_trace_echo_sees_the_recorded_inputs():
    KT.check_echo("cpu")


def test_knockout_trace_independence_and_repeatability():
    KT.check_independence("cpu")


@pytest.mark.parametrize("dims,J,win", [(KT.DIMS, 4, KT.WIN), ((1, 2, 3, 17, 5, 5), 16, (0, 2, 3)), ((1, 1, 1, 2, 5, 5), 1, (0, 1, 1))])
def test_knockout_trace_writes_only_what_it_owns(dims, J, win):
    KT.check_ownership("cpu", dims, J, win)


def test_knockout_trace_touches_nothing_and_train_unaffected():
    KT.check_touches_nothing("cpu")


def test_knockout_trace_method_on_loaded_checkpoint(tmp_path):
    KT.check_methods("cpu", tmp_path)


def test_knockout_trace_method_refusals():
    KT.check_method_refusals("cpu")


def test_knockout_trace_bad_arguments():
    KT.check_bad_arguments("cpu")


def test_knockout_trace_abi():
    KT.check_abi()
