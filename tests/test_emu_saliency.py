"""CPU (host-emulated kernels): policy saliency -- csrc/policy_saliency.hip through ops.saliency and DcntrlMAC.saliency -- against fp64
autograd of the oracle (tests/saliency_checks.py)."""
import pytest

from iplan_amd import _lib as L
from tests import saliency_checks as SC
from tests.emu.emu_lib import get_emu_lib


@pytest.fixture(autouse=True)
def emu():
    L.use_library_for_tests(get_emu_lib())
    yield
    L.use_library_for_tests(None)


@pytest.mark.parametrize("dims,opt", SC.KERNEL_CASES, ids=SC.CASE_IDS)
def test_saliency_kernel_vs_fp64(dims, opt):
    SC.check_kernel("cpu", dims, opt)


def test_saliency_greedy_matches_policy_trace():
    SC.check_greedy_matches_trace("cpu")


def test_saliency_placement_and_repeatability():
    SC.check_placement("cpu")


def test_saliency_writes_only_what_it_owns():
    SC.check_sentinel("cpu")


def test_saliency_touches_nothing():
    SC.check_touches_nothing("cpu")


def test_saliency_host_api():
    SC.check_host_api("cpu")


def test_saliency_bad_arguments():
    SC.check_bad_arguments("cpu")
