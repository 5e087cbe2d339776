"""GPU: policy saliency through time on the gfx950 build -- the same checks the CPU suite runs through the host emulator
(tests/saliency_trace_checks.py), where the MFMA layouts, the cross-lane reductions and the seed / carry hand-off between the launches
are the hardware's.  Worst errors are logged the way tests/test_gpu_parity_fullsize.py logs its own."""
import pytest

from tests import saliency_trace_checks as TC
from tests.test_gpu_parity_fullsize import _log

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.mark.parametrize("dims,opt", TC.KERNEL_CASES, ids=TC.CASE_IDS)
def test_saliency_trace_kernel_vs_fp64(dims, opt):
    _log("saliency_trace_kernel_" + "_".join(map(str, dims)) + "".join(f"_{k}{v}" for k, v in sorted(opt.items())), TC.check_kernel(DEV, dims, opt))


def test_saliency_trace_lag0_is_saliency_and_states_are_policy_trace():
    _log("saliency_trace_lag0", TC.check_lag0(DEV))


def test_saliency_trace_prefix():
    TC.check_prefix(DEV)


def test_saliency_trace_placement_and_repeatability():
    TC.check_placement(DEV, reps=5)


def test_saliency_trace_writes_only_what_it_owns():
    TC.check_sentinel(DEV)


def test_saliency_trace_touches_nothing():
    TC.check_touches_nothing(DEV)


def test_saliency_trace_filled_weighting():
    _log("saliency_trace_filled", TC.check_filled_weighting(DEV))


def test_saliency_trace_bad_arguments():
    TC.check_bad_arguments(DEV)
