"""GPU: the behaviour learning kernels alone on the gfx950 build -- csrc/behavior_learn.hip through ops.beh_forward +
ops.beh_backward and ops.bdec_forward against fp64 autograd of the oracle (tests/behavior_learn_checks.py), where the MFMA layouts,
the role-split waves and their LDS-counter hand-offs, the window-range pipeline on its side streams and the grid geometry are the
hardware's.  Every case of the check lists runs here, with what the host emulator's file leaves out: the 97-row shape in every
form, the 513-window case, every form at 49 rows, the seeded draw in all four decoder form pairs.  Worst errors (kernel and fp32
reference beside each other) are logged the way tests/test_gpu_parity_fullsize.py logs its own."""
import pytest

from tests import behavior_learn_checks as BL
from tests.test_gpu_parity_fullsize import _log

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _ids(cases):
    return [BL.case_id(*c) for c in cases]


@pytest.mark.parametrize("case", BL.ROW_CASES, ids=_ids(BL.ROW_CASES))
def test_row_edges_vs_fp64(case):
    _log("beh_learn_rows_" + BL.case_id(*case), BL.check_shape(DEV, *case))


@pytest.mark.parametrize("case", BL.WIDTH_CASES, ids=_ids(BL.WIDTH_CASES))
def test_width_edges_vs_fp64(case):
    """d <= 8 selects the decoder forward's second form, d > 8 -- (9, 7), (12, 4), (15, 1) -- the first form under the second-form
    BPTT with its in-kernel thin gradients"""
    _log("beh_learn_width_" + BL.case_id(*case), BL.check_shape(DEV, *case))


@pytest.mark.parametrize("case", BL.WINDOW_CASES[:-1], ids=_ids(BL.WINDOW_CASES[:-1]))
def test_window_edges_vs_fp64(case):
    _log("beh_learn_windows_" + BL.case_id(*case), BL.check_shape(DEV, *case))


def test_short_first_window_range_vs_fp64(monkeypatch):
    """J = 26: 4 forward and 6 BPTT pieces (the defaults here, set explicitly) take _piece_bounds' short-first-range form"""
    case = BL.SHORT_RANGE_CASE
    _log("beh_learn_windows_" + BL.case_id(*case),
         BL.check_shape(DEV, *case, env={"IPLAN_BEH_PIECES_FWD": "4", "IPLAN_BEH_PIECES_BWD": "6"}, monkeypatch=monkeypatch))


def test_short_first_window_range_default_pieces_vs_fp64():
    """... and with no knob set at all"""
    case = BL.SHORT_RANGE_CASE
    _log("beh_learn_windows_default_" + BL.case_id(*case), BL.check_shape(DEV, *case))


def test_more_windows_than_a_second_form_launch_takes(monkeypatch):
    """513 windows: the decoder forward runs its first form, beh_backward splits the one BPTT piece it was asked for"""
    _log("beh_learn_windows_" + BL.case_id(*BL.LONG_CASE), BL.check_long_episode(DEV, monkeypatch))


@pytest.mark.parametrize("kind", BL.MASK_KINDS)
def test_mask_kinds_vs_fp64(kind):
    _log("beh_learn_mask_" + kind, BL.check_mask_kind(DEV, kind))


@pytest.mark.parametrize("rows,form", [(r, f) for r in BL.FORM_SHAPES for f in BL.FORMS])
def test_forms_vs_fp64(monkeypatch, rows, form):
    _log(f"beh_learn_form_{form}_rows{rows}", BL.check_form(DEV, monkeypatch, rows, form))


@pytest.mark.parametrize("rows", list(BL.FORM_SHAPES))
def test_forms_agree(monkeypatch, rows):
    _log(f"beh_learn_forms_agree_rows{rows}", BL.check_forms_agree(DEV, monkeypatch, rows))


@pytest.mark.parametrize("rows,fwd_v1,bwd_v1", [(r, f, b) for r in (17, 49) for f in (False, True) for b in (False, True)])
def test_seeded_draw_equals_explicit_keep(monkeypatch, rows, fwd_v1, bwd_v1):
    _log(f"beh_learn_seeded_rows{rows}_fwd{2 - fwd_v1}_bwd{2 - bwd_v1}", BL.check_seeded_equals_explicit(DEV, monkeypatch, rows, fwd_v1, bwd_v1))


@pytest.mark.parametrize("rows,bwd_v1", [(17, False), (17, True), (49, False), (49, True)])
def test_arena_ownership_and_repeatability(monkeypatch, rows, bwd_v1):
    BL.check_ownership_and_repeatability(DEV, monkeypatch, bwd_v1, rows=rows)


def test_row_independence():
    BL.check_row_independence(DEV)


def test_refusals(monkeypatch):
    BL.check_refusals(DEV, monkeypatch)


@pytest.mark.parametrize("rows,d,Z,with_keep", [(r, d, Z, k) for r in (1, 16, 17, 49) for d, Z in ((5, 8), (9, 7)) for k in (False, True)])
def test_single_window_decoder_vs_fp64(rows, d, Z, with_keep):
    _log(f"beh_learn_bdec_rows{rows}_d{d}_Z{Z}_keep{int(with_keep)}", BL.check_bdec_forward(DEV, rows, d, Z, with_keep))
