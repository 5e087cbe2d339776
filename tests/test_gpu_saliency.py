"""GPU: policy saliency on the gfx950 build -- the same checks the CPU suite runs through the host emulator (tests/saliency_checks.py),
where the MFMA layouts of fc1 and fc1^T, the cross-lane reductions and the in-wave LDS hand-off of the entity sums are the hardware's.
Worst errors are logged the way tests/test_gpu_parity_fullsize.py logs its own."""
import pytest

from tests import saliency_checks as SC
from tests.test_gpu_parity_fullsize import _log

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.mark.parametrize("dims,opt", SC.KERNEL_CASES, ids=SC.CASE_IDS)
def test_saliency_kernel_vs_fp64(dims, opt):
    _log("saliency_kernel_" + "_".join(map(str, dims)) + "".join(f"_{k}{v}" for k, v in sorted(opt.items())), SC.check_kernel(DEV, dims, opt))


def test_saliency_greedy_matches_policy_trace():
    _log("saliency_vs_policy_trace", SC.check_greedy_matches_trace(DEV))


def test_saliency_placement_and_repeatability():
    SC.check_placement(DEV, reps=5)


def test_saliency_writes_only_what_it_owns():
    SC.check_sentinel(DEV)


def test_saliency_touches_nothing():
    SC.check_touches_nothing(DEV)


def test_saliency_host_api():
    _log("saliency_host_api", SC.check_host_api(DEV))


def test_saliency_bad_arguments():
    SC.check_bad_arguments(DEV)
