"""GPU: neighbour knock-out attribution on the gfx950 build -- the same checks the CPU suite runs through the host emulator
(tests/knockout_checks.py), where the MFMA layouts, the packed fp32 operations of the recurrence, the LDS hand-off of the knocked
latent to the distance epilogue and the rounding of that epilogue are the hardware's.  Worst errors are logged the way
tests/test_gpu_parity_fullsize.py logs its own."""
import pytest

from tests import knockout_checks as KC
from tests.test_gpu_parity_fullsize import _log

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.mark.parametrize("n,B,N,d0,d1", KC.KERNEL_CASES)
def test_knockout_same_bits_as_existing_path(n, B, N, d0, d1):
    _log(f"knockout_same_bits_n{n}_B{B}_N{N}_d{d0}_{d1}", KC.check_same_bits(DEV, n, B, N, d0, d1))


@pytest.mark.parametrize("noise,knock,baseline", [(False, None, False), (True, (False, True), False), (True, (True, False), True),
                                                  (False, None, True)])
def test_knockout_same_bits_sources_and_baseline(noise, knock, baseline):
    KC.check_same_bits(DEV, 2, 2, 5, 5, 3, noise=noise, knock=knock, baseline=baseline)


@pytest.mark.parametrize("n,B,N,d0,d1", [(1, 1, 17, 5, 3), (1, 2, 33, 5, 0)])
def test_knockout_same_bits_without_noise(n, B, N, d0, d1):
    # (tau = 0.25: without noise the shipped 0.01 closes every gate of these random nets, and no knocked latent would move)
    KC.check_same_bits(DEV, n, B, N, d0, d1, noise=False, tau=0.25)


@pytest.mark.parametrize("n,B,N,d0,d1,baseline", [(1, 1, 2, 5, 0, False), (5, 2, 5, 5, 3, True), (1, 1, 17, 7, 9, False)])
def test_knockout_exact_zeros(n, B, N, d0, d1, baseline):
    KC.check_exact_zeros(DEV, n, B, N, d0, d1, baseline)


@pytest.mark.parametrize("n,B,N,d0,d1,tau", KC.FP64_CASES)
def test_knockout_vs_fp64(n, B, N, d0, d1, tau):
    _log(f"knockout_fp64_n{n}_B{B}_N{N}_d{d0}_{d1}_tau{tau}", KC.check_vs_fp64(DEV, n, B, N, d0, d1, tau))


def test_knockout_independence():
    KC.check_independence(DEV)


def test_knockout_repeatable():
    KC.check_repeatable(DEV, 20)


@pytest.mark.parametrize("n,B,N", [(1, 2, 2), (1, 1, 17), (5, 1, 5)])
def test_knockout_writes_only_what_it_owns(n, B, N):
    KC.check_ownership(DEV, n, B, N)


def test_knockout_bad_arguments():
    KC.check_bad_arguments(DEV)


@pytest.mark.parametrize("E,S", [(2, 1), (1, 2)])
def test_knockout_method_on_loaded_checkpoint(tmp_path, E, S):
    _log(f"knockout_methods_E{E}_S{S}", KC.check_methods(DEV, tmp_path, E, S))


def test_knockout_touches_nothing(tmp_path):
    KC.check_nothing_touched(DEV, tmp_path, 20)


def test_learn_unaffected_by_knockout():
    KC.check_learn_unaffected(DEV)


def test_knockout_method_refusals():
    KC.check_method_refusals(DEV)
