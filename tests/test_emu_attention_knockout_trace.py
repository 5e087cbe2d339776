"""CPU (host-emulated kernels): neighbour knock-out through time -- csrc/gat_knockout_trace.hip through ops.gat_knockout_trace, and
Prediction_policy.attention_knockout_trace -- against the existing walk on explicit copies of the episode fields, bit for bit, and
against the fp64 oracle (tests/attention_knockout_trace_checks.py)."""
import pytest

from iplan_amd import _lib as L
from tests import attention_knockout_trace_checks as TC
from tests.emu.emu_lib import get_emu_lib


@pytest.fixture(autouse=True)
def emu():
    L.use_library_for_tests(get_emu_lib())
    yield
    L.use_library_for_tests(None)


@pytest.mark.parametrize("n,B,N,d0,d1,window", TC.SAME_BITS_CASES)
def test_knockout_trace_same_bits_as_existing_path(n, B, N, d0, d1, window):
    TC.check_same_bits("cpu", n, B, N, d0, d1, window)


@pytest.mark.parametrize("noise,knock,baseline", [(False, None, False), (True, (False, True), False), (True, (True, False), True),
                                                  (False, None, True)])
def test_knockout_trace_same_bits_sources_and_baseline(noise, knock, baseline):
    TC.check_same_bits("cpu", 2, 2, 5, 5, 3, (1, 2, 4), noise=noise, knock=knock, baseline=baseline)


@pytest.mark.parametrize("n,B,N,d0,d1,window", [(1, 1, 17, 5, 3, (1, 2, 4)), (1, 2, 33, 5, 0, (0, 1, 3))])
def test_knockout_trace_same_bits_without_noise(n, B, N, d0, d1, window):
    # (tau = 0.25: without noise the shipped 0.01 closes every gate of these random nets, and no knocked latent would move)
    TC.check_same_bits("cpu", n, B, N, d0, d1, window, noise=False, tau=0.25)


@pytest.mark.parametrize("n,B,N,d0,d1,baseline", [(1, 1, 2, 5, 0, False), (5, 2, 5, 5, 3, True), (1, 1, 17, 7, 9, False)])
def test_knockout_trace_exact_zeros(n, B, N, d0, d1, baseline):
    TC.check_exact_zeros("cpu", n, B, N, d0, d1, baseline)


@pytest.mark.parametrize("n,B,N,d0,d1,tau", TC.FP64_CASES)
def test_knockout_trace_vs_fp64(n, B, N, d0, d1, tau):
    TC.check_vs_fp64("cpu", n, B, N, d0, d1, tau)


def test_knockout_trace_independence_and_prefix():
    TC.check_independence("cpu")


def test_knockout_trace_repeatable():
    TC.check_repeatable("cpu", 2)


@pytest.mark.parametrize("n,B,N", [(1, 2, 2), (1, 1, 17), (5, 1, 5)])
def test_knockout_trace_writes_only_what_it_owns(n, B, N):
    TC.check_ownership("cpu", n, B, N)


def test_knockout_trace_bad_arguments():
    TC.check_bad_arguments("cpu")


@pytest.mark.parametrize("E,S", [(2, 3), (1, 4)])
def test_knockout_trace_method_on_loaded_checkpoint(tmp_path, E, S):
    TC.check_methods("cpu", tmp_path, E, S)


def test_knockout_trace_touches_nothing(tmp_path):
    TC.check_nothing_touched("cpu", tmp_path, 2)


def test_learn_unaffected_by_knockout_trace():
    TC.check_learn_unaffected("cpu")


def test_knockout_trace_method_refusals():
    TC.check_method_refusals("cpu")
