"""GPU: attention inspection on the gfx950 build -- the same checks the CPU suite runs through the host emulator
(tests/attention_checks.py), where the MFMA layouts, the cross-lane reductions, the barriers of the step loop and the LDS hand-off of
the hidden state are the hardware's.  Worst errors are logged the way tests/test_gpu_parity_fullsize.py logs its own."""
import pytest

from tests import attention_checks as AC
from tests.test_gpu_parity_fullsize import _log

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.mark.parametrize("n,B,S,N,d0,d1", AC.KERNEL_CASES)
def test_trace_kernel_vs_fp64(n, B, S, N, d0, d1):
    _log(f"trace_kernel_n{n}_B{B}_S{S}_N{N}_d{d0}_{d1}", AC.check_kernel(DEV, n, B, S, N, d0, d1))


@pytest.mark.parametrize("N", [5, 17, 33])
def test_trace_same_bits_as_rollout_path(N):
    _log(f"trace_same_bits_N{N}", AC.check_same_bits_as_rollout(DEV, N))


@pytest.mark.parametrize("n,B,S,N", [(1, 2, 2, 2), (1, 1, 2, 17), (5, 1, 2, 5)])
def test_trace_writes_only_what_it_owns(n, B, S, N):
    AC.check_sentinel(DEV, n, B, S, N)


def test_trace_optional_operands():
    _log("trace_optional_operands", AC.check_optional_operands(DEV))


def test_trace_repeatable():
    AC.check_repeatable(DEV, 20)


def test_trace_bad_arguments():
    AC.check_bad_arguments(DEV)


def test_attention_methods_on_loaded_checkpoint(tmp_path):
    _log("attention_methods", AC.check_methods(DEV, tmp_path))


def test_learn_unaffected_by_trace():
    AC.check_learn_unaffected_by_trace(DEV)


def test_trace_replays_rollout():
    AC.check_replays_rollout(DEV)
