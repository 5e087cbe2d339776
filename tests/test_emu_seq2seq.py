"""CPU (host-emulated kernels): the Seq2Seq kernels alone -- csrc/seq2seq.hip's iplan_seq2seq_fwd (saving and non-saving) and
iplan_seq2seq_bwd, with more than one workgroup, at the width edges, in every feedback and dropout form -- against the fp64 oracle
and the step-by-step reference of tests/seq2seq_checks.py."""
import pytest

from iplan_amd import _lib as L
from tests import seq2seq_checks as S
from tests.emu.emu_lib import get_emu_lib


@pytest.fixture(autouse=True)
def emu():
    L.use_library_for_tests(get_emu_lib())
    yield
    L.use_library_for_tests(None)


@pytest.mark.parametrize("c", S.ROW_CASES, ids=S.case_id)
def test_rows_vs_fp64(c):
    S.check_case("cpu", c)


@pytest.mark.parametrize("c", S.IN_CASES, ids=S.case_id)
def test_input_widths_vs_fp64(c):
    S.check_case("cpu", c)


@pytest.mark.parametrize("c", S.O_CASES, ids=S.case_id)
def test_output_widths_vs_fp64(c):
    S.check_case("cpu", c)


@pytest.mark.parametrize("c", S.STACK_CASES, ids=S.case_id)
def test_layers_and_hidden_widths_vs_fp64(c):
    S.check_case("cpu", c)


@pytest.mark.parametrize("c", S.STEP_CASES, ids=S.case_id)
def test_one_step_and_long_walk_vs_fp64(c):
    S.check_case("cpu", c)


@pytest.mark.parametrize("c", S.FEEDBACK_CASES, ids=S.case_id)
def test_feedback_forms_vs_fp64(c):
    S.check_case("cpu", c)


def test_feedback_forms_bit_identities():
    S.check_feedback_forms("cpu")


@pytest.mark.parametrize("c", S.DROPOUT_CASES, ids=S.case_id)
def test_dropout_forms_vs_fp64(c):
    S.check_case("cpu", c)


def test_rows_are_independent():
    S.check_rows_independent("cpu")


def test_reads_stay_inside_the_contract():
    S.check_reads("cpu")


def test_misaligned_bases():
    S.check_misaligned("cpu")


def test_repeatable():
    S.check_repeatable("cpu", n=3)


def test_seq2seq_refusals():
    S.check_refusals("cpu")
