"""CPU (host-emulated kernels): policy saliency through time -- csrc/policy_saliency_lag.hip through ops.saliency_lag and
DcntrlMAC.saliency_trace -- against fp64 autograd through the unrolled oracle chain (tests/saliency_trace_checks.py)."""
import pytest

from iplan_amd import _lib as L
from tests import saliency_trace_checks as TC
from tests.emu.emu_lib import get_emu_lib


@pytest.fixture(autouse=True)
def emu():
    L.use_library_for_tests(get_emu_lib())
    yield
    L.use_library_for_tests(None)


@pytest.mark.parametrize("dims,opt", TC.KERNEL_CASES, ids=TC.CASE_IDS)
def test_saliency_trace_kernel_vs_fp64(dims, opt):
    TC.check_kernel("cpu", dims, opt)


def test_saliency_trace_lag0_is_saliency_and_states_are_policy_trace():
    TC.check_lag0("cpu")


def test_saliency_trace_prefix():
    TC.check_prefix("cpu")


def test_saliency_trace_placement_and_repeatability():
    TC.check_placement("cpu")


def test_saliency_trace_writes_only_what_it_owns():
    TC.check_sentinel("cpu")


def test_saliency_trace_touches_nothing():
    TC.check_touches_nothing("cpu")


def test_saliency_trace_filled_weighting():
    TC.check_filled_weighting("cpu")


def test_saliency_trace_bad_arguments():
    TC.check_bad_arguments("cpu")
