"""GPU: policy knock-out through time on the gfx950 build -- the same checks the CPU suite runs through the host emulator
(tests/knockout_trace_checks.py), where the MFMA layouts, the LDS hand-off of the per-job states, the cross-lane reads of the tile's
base column and the rounding of the KL and state-shift epilogues are the hardware's.  Worst errors are logged the way
tests/test_gpu_parity_fullsize.py logs its own."""
import pytest

from tests import knockout_trace_checks as KT
from tests.test_gpu_parity_fullsize import _log

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.mark.parametrize("dims,J,win,opt", KT.BIT_CASES, ids=KT.BIT_IDS)
def test_knockout_trace_same_bits_as_rerun(dims, J, win, opt):
    KT.check_same_bits(DEV, dims, J, win, opt)


def test_knockout_trace_agrees_with_knockout_at_first_step():
    _log("knockout_trace_vs_knockout", KT.check_agrees_with_knockout(DEV))


@pytest.mark.parametrize("dims,J,win,opt", KT.FP64_CASES, ids=KT.FP64_IDS)
def test_knockout_trace_vs_fp64(dims, J, win, opt):
    _log("knockout_trace_fp64_" + KT.FP64_IDS[KT.FP64_CASES.index((dims, J, win, opt))], KT.check_vs_fp64(DEV, dims, J, win, opt))


@pytest.mark.parametrize("dims,win,opt,mode", [(KT.DIMS, KT.WIN, {}, "zeros"), (KT.DIMS, (0, 2, 4), {}, "baseline"),
                                               ((1, 2, 4, 2, 5, 5), (1, 1, 3), dict(tanh=True, gat=False), "zeros")])
def test_knockout_trace_exact_zeros(dims, win, opt, mode):
    KT.check_exact_zeros(DEV, dims, win, opt, mode)


def test_knockout_trace_echo_sees_the_recorded_inputs():
    KT.check_echo(DEV)


def test_knockout_trace_independence_and_repeatability():
    KT.check_independence(DEV)


@pytest.mark.parametrize("dims,J,win", [(KT.DIMS, 4, KT.WIN), ((1, 2, 3, 17, 5, 5), 16, (0, 2, 3)), ((1, 1, 1, 2, 5, 5), 1, (0, 1, 1))])
def test_knockout_trace_writes_only_what_it_owns(dims, J, win):
    KT.check_ownership(DEV, dims, J, win)


def test_knockout_trace_touches_nothing_and_train_unaffected():
    KT.check_touches_nothing(DEV)


def test_knockout_trace_method_on_loaded_checkpoint(tmp_path):
    _log("knockout_trace_methods", KT.check_methods(DEV, tmp_path))


def test_knockout_trace_method_refusals():
    KT.check_method_refusals(DEV)


def test_knockout_trace_bad_arguments():
    KT.check_bad_arguments(DEV)


def test_knockout_trace_abi():
    KT.check_abi()
