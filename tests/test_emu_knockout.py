"""CPU (host-emulated kernels): neighbour knock-out attribution -- csrc/gat_knockout.hip through ops.gat_knockout, and
Prediction_policy.attention_knockout -- against the existing paths on explicit input copies, bit for bit, and against the fp64
oracle (tests/knockout_checks.py)."""
import pytest

from iplan_amd import _lib as L
from tests import knockout_checks as KC
from tests.emu.emu_lib import get_emu_lib


@pytest.fixture(autouse=True)
def emu():
    L.use_library_for_tests(get_emu_lib())
    yield
    L.use_library_for_tests(None)


@pytest.mark.parametrize("n,B,N,d0,d1", KC.KERNEL_CASES)
def test_knockout_same_bits_as_existing_path(n, B, N, d0, d1):
    KC.check_same_bits("cpu", n, B, N, d0, d1)


@pytest.mark.parametrize("noise,knock,baseline", [(False, None, False), (True, (False, True), False), (True, (True, False), True),
                                                  (False, None, True)])
def test_knockout_same_bits_sources_and_baseline(noise, knock, baseline):
    KC.check_same_bits("cpu", 2, 2, 5, 5, 3, noise=noise, knock=knock, baseline=baseline)


@pytest.mark.parametrize("n,B,N,d0,d1", [(1, 1, 17, 5, 3), (1, 2, 33, 5, 0)])
def test_knockout_same_bits_without_noise(n, B, N, d0, d1):
    # (tau = 0.25: without noise the shipped 0.01 closes every gate of these random nets, and no knocked latent would move)
    KC.check_same_bits("cpu", n, B, N, d0, d1, noise=False, tau=0.25)


@pytest.mark.parametrize("n,B,N,d0,d1,baseline", [(1, 1, 2, 5, 0, False), (5, 2, 5, 5, 3, True), (1, 1, 17, 7, 9, False)])
def test_knockout_exact_zeros(n, B, N, d0, d1, baseline):
    KC.check_exact_zeros("cpu", n, B, N, d0, d1, baseline)


@pytest.mark.parametrize("n,B,N,d0,d1,tau", KC.FP64_CASES)
def test_knockout_vs_fp64(n, B, N, d0, d1, tau):
    KC.check_vs_fp64("cpu", n, B, N, d0, d1, tau)


def test_knockout_independence():
    KC.check_independence("cpu")


def test_knockout_repeatable():
    KC.check_repeatable("cpu", 2)


@pytest.mark.parametrize("n,B,N", [(1, 2, 2), (1, 1, 17), (5, 1, 5)])
def test_knockout_writes_only_what_it_owns(n, B, N):
    KC.check_ownership("cpu", n, B, N)


def test_knockout_bad_arguments():
    KC.check_bad_arguments("cpu")


@pytest.mark.parametrize("E,S", [(2, 1), (1, 2)])
def test_knockout_method_on_loaded_checkpoint(tmp_path, E, S):
    KC.check_methods("cpu", tmp_path, E, S)


def test_knockout_touches_nothing(tmp_path):
    KC.check_nothing_touched("cpu", tmp_path, 2)


def test_learn_unaffected_by_knockout():
    KC.check_learn_unaffected("cpu")


def test_knockout_method_refusals():
    KC.check_method_refusals("cpu")
