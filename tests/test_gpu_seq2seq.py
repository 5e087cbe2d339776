"""GPU: the Seq2Seq kernels alone on the gfx950 build -- the same checks the CPU suite runs through the host emulator
(tests/seq2seq_checks.py), where several workgroups are in flight, waves 2 and 3 hold rows, the backward's LDS carry is the hardware's
(64 KiB a workgroup at 4 layers x 64) and the gate functions are the hardware's exp2 / rcp.  Worst errors are logged the way
tests/test_gpu_parity_fullsize.py logs its own."""
import pytest

from tests import seq2seq_checks as S
from tests.test_gpu_parity_fullsize import _log

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.mark.parametrize("c", S.ROW_CASES, ids=S.case_id)
def test_rows_vs_fp64(c):
    _log("seq2seq_rows_" + S.case_id(c), S.check_case(DEV, c))


@pytest.mark.parametrize("c", S.IN_CASES, ids=S.case_id)
def test_input_widths_vs_fp64(c):
    _log("seq2seq_in_" + S.case_id(c), S.check_case(DEV, c))


@pytest.mark.parametrize("c", S.O_CASES, ids=S.case_id)
def test_output_widths_vs_fp64(c):
    _log("seq2seq_o_" + S.case_id(c), S.check_case(DEV, c))


@pytest.mark.parametrize("c", S.STACK_CASES, ids=S.case_id)
def test_layers_and_hidden_widths_vs_fp64(c):
    _log("seq2seq_stack_" + S.case_id(c), S.check_case(DEV, c))


@pytest.mark.parametrize("c", S.STEP_CASES, ids=S.case_id)
def test_one_step_and_long_walk_vs_fp64(c):
    _log("seq2seq_steps_" + S.case_id(c), S.check_case(DEV, c))


@pytest.mark.parametrize("c", S.FEEDBACK_CASES, ids=S.case_id)
def test_feedback_forms_vs_fp64(c):
    _log("seq2seq_feedback_" + S.case_id(c), S.check_case(DEV, c))


def test_feedback_forms_bit_identities():
    _log("seq2seq_feedback_identities", S.check_feedback_forms(DEV))


@pytest.mark.parametrize("c", S.DROPOUT_CASES, ids=S.case_id)
def test_dropout_forms_vs_fp64(c):
    _log("seq2seq_dropout_" + S.case_id(c), S.check_case(DEV, c))


def test_rows_are_independent():
    _log("seq2seq_rows_independent", S.check_rows_independent(DEV, alone=range(S.LARGEST.rows)))


def test_reads_stay_inside_the_contract():
    _log("seq2seq_reads", S.check_reads(DEV))


def test_misaligned_bases():
    _log("seq2seq_misaligned", S.check_misaligned(DEV))


def test_repeatable():
    _log("seq2seq_repeatable", S.check_repeatable(DEV))


def test_seq2seq_refusals():
    _log("seq2seq_refusals", S.check_refusals(DEV))
