"""GPU: neighbour knock-out through time on the gfx950 build -- the same checks the CPU suite runs through the host emulator
(tests/attention_knockout_trace_checks.py), where the MFMA layouts, the packed fp32 operations of the recurrence, the LDS hand-off of
the knocked chain's latent from step to step and to the distance epilogue, and the barriers between them are the hardware's.  Worst
errors are logged the way tests/test_gpu_knockout.py logs its own."""
import pytest

from tests import attention_knockout_trace_checks as TC
from tests.test_gpu_parity_fullsize import _log

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.mark.parametrize("n,B,N,d0,d1,window", TC.SAME_BITS_CASES)
def test_knockout_trace_same_bits_as_existing_path(n, B, N, d0, d1, window):
    _log(f"attention_knockout_trace_same_bits_n{n}_B{B}_N{N}_d{d0}_{d1}_w{'_'.join(map(str, window))}", TC.check_same_bits(DEV, n, B, N, d0, d1, window))


@pytest.mark.parametrize("noise,knock,baseline", [(False, None, False), (True, (False, True), False), (True, (True, False), True),
                                                  (False, None, True)])
def test_knockout_trace_same_bits_sources_and_baseline(noise, knock, baseline):
    TC.check_same_bits(DEV, 2, 2, 5, 5, 3, (1, 2, 4), noise=noise, knock=knock, baseline=baseline)


@pytest.mark.parametrize("n,B,N,d0,d1,window", [(1, 1, 17, 5, 3, (1, 2, 4)), (1, 2, 33, 5, 0, (0, 1, 3))])
def test_knockout_trace_same_bits_without_noise(n, B, N, d0, d1, window):
    # (tau = 0.25: without noise the shipped 0.01 closes every gate of these random nets, and no knocked latent would move)
    TC.check_same_bits(DEV, n, B, N, d0, d1, window, noise=False, tau=0.25)


@pytest.mark.parametrize("n,B,N,d0,d1,baseline", [(1, 1, 2, 5, 0, False), (5, 2, 5, 5, 3, True), (1, 1, 17, 7, 9, False)])
def test_knockout_trace_exact_zeros(n, B, N, d0, d1, baseline):
    TC.check_exact_zeros(DEV, n, B, N, d0, d1, baseline)


@pytest.mark.parametrize("n,B,N,d0,d1,tau", TC.FP64_CASES)
def test_knockout_trace_vs_fp64(n, B, N, d0, d1, tau):
    _log(f"attention_knockout_trace_fp64_n{n}_B{B}_N{N}_d{d0}_{d1}_tau{tau}", TC.check_vs_fp64(DEV, n, B, N, d0, d1, tau))


def test_knockout_trace_independence_and_prefix():
    TC.check_independence(DEV)


def test_knockout_trace_repeatable():
    TC.check_repeatable(DEV, 20)


@pytest.mark.parametrize("n,B,N", [(1, 2, 2), (1, 1, 17), (5, 1, 5)])
def test_knockout_trace_writes_only_what_it_owns(n, B, N):
    TC.check_ownership(DEV, n, B, N)


def test_knockout_trace_bad_arguments():
    TC.check_bad_arguments(DEV)


@pytest.mark.parametrize("E,S", [(2, 3), (1, 4)])
def test_knockout_trace_method_on_loaded_checkpoint(tmp_path, E, S):
    _log(f"attention_knockout_trace_methods_E{E}_S{S}", TC.check_methods(DEV, tmp_path, E, S))


def test_knockout_trace_touches_nothing(tmp_path):
    TC.check_nothing_touched(DEV, tmp_path, 20)


def test_learn_unaffected_by_knockout_trace():
    TC.check_learn_unaffected(DEV)


def test_knockout_trace_method_refusals():
    TC.check_method_refusals(DEV)
