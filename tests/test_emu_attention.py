"""CPU (host-emulated kernels): attention inspection -- csrc/gat_trace.hip through ops.gat_trace, and
Prediction_policy.attention_map / attention_trace -- against the fp64 oracle (tests/attention_checks.py)."""
import pytest

from iplan_amd import _lib as L
from tests import attention_checks as AC
from tests.emu.emu_lib import get_emu_lib


@pytest.fixture(autouse=True)
def emu():
    L.use_library_for_tests(get_emu_lib())
    yield
    L.use_library_for_tests(None)


@pytest.mark.parametrize("n,B,S,N,d0,d1", AC.KERNEL_CASES)
def test_trace_kernel_vs_fp64(n, B, S, N, d0, d1):
    AC.check_kernel("cpu", n, B, S, N, d0, d1)


@pytest.mark.parametrize("N", [5, 17, 33])
def test_trace_same_bits_as_rollout_path(N):
    AC.check_same_bits_as_rollout("cpu", N)


@pytest.mark.parametrize("n,B,S,N", [(1, 2, 2, 2), (1, 1, 2, 17), (5, 1, 2, 5)])
def test_trace_writes_only_what_it_owns(n, B, S, N):
    AC.check_sentinel("cpu", n, B, S, N)


def test_trace_optional_operands():
    AC.check_optional_operands("cpu")


def test_trace_repeatable():
    AC.check_repeatable("cpu", 2)


def test_trace_bad_arguments():
    AC.check_bad_arguments("cpu")


def test_attention_methods_on_loaded_checkpoint(tmp_path):
    AC.check_methods("cpu", tmp_path)


def test_learn_unaffected_by_trace():
    AC.check_learn_unaffected_by_trace("cpu")


def test_trace_replays_rollout():
    AC.check_replays_rollout("cpu")
