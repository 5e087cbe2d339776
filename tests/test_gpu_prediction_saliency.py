"""GPU: prediction saliency on the gfx950 build -- the checks the CPU suite runs through the host emulator
(tests/prediction_saliency_checks.py), where the MFMA layouts, the cross-lane hand-over of the column sums and the lane-private LDS
slabs are the hardware's.  Worst errors are logged the way tests/test_gpu_parity_fullsize.py logs its own."""
import pytest

from tests import prediction_saliency_checks as SC
from tests.test_gpu_parity_fullsize import _log

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.mark.parametrize("case", SC.KERNEL_CASES, ids=SC.case_id)
def test_saliency_kernel_vs_fp64(case):
    _log("pdec_saliency_" + SC.case_id(case), SC.check_kernel(DEV, *case))


def test_saliency_every_combination_of_outputs():
    _log("pdec_saliency_outputs", SC.check_output_combinations(DEV))


def test_saliency_exact_statements():
    SC.check_exact(DEV)


def test_saliency_is_linear_in_the_cotangent():
    _log("pdec_saliency_linearity", SC.check_linearity(DEV))


def test_saliency_reads_in_place_and_writes_only_what_it_owns():
    SC.check_ownership(DEV)


def test_prediction_saliency_method():
    _log("prediction_saliency_method", SC.check_methods(DEV))


def test_prediction_saliency_continues_through_the_gat():
    _log("prediction_saliency_chain", SC.check_chain(DEV))


def test_prediction_saliency_touches_nothing():
    SC.check_touches_nothing(DEV)


def test_saliency_entry_point_refusals():
    SC.check_entry_point_refusals(DEV)


def test_prediction_saliency_method_refusals():
    SC.check_method_refusals(DEV)
