"""CPU (host-emulated kernels): the behaviour learning kernels alone -- csrc/behavior_learn.hip through ops.beh_forward +
ops.beh_backward and ops.bdec_forward -- against fp64 autograd of the oracle (tests/behavior_learn_checks.py);
tests/test_gpu_behavior_learn.py runs the same checks on the gfx950 build.

The emulator runs a workgroup's waves one after the other (an emulated launch pair costs 0.7 s at 17 rows x 2 nets, 1.2 s at 49
rows), so this file runs a stated subset and no launch twice.  Left to the GPU:
  * rows: 97 rows (row edge and every form), five nets at 65 rows (two here); the 17- and 49-row row edges are test_forms_agree's
    default form here;
  * the width (12, 4), the 513-window case, the single-window decoder at 16 rows;
  * masks: "random" and "ones" with explicit keep flags (the row edge at 15 rows is the random mask with flags);
  * forms: IPLAN_FWD_SAVE_ACT and IPLAN_BEH_SERIAL (no side stream here: the knob changes nothing), IPLAN_BEH_PIECES=1 (the
    emulator's default) and equal pieces (J = 3 gives equal pieces anyway) at 17 rows; at 49 rows everything but the four decoder
    forms of test_forms_agree, three pieces and the env shards;
  * the seeded draw in the two mixed form pairs and at 49 rows, and drop_p = 0.5 / the hard update in the first forms;
  * ownership under IPLAN_DEC_BWD_V1: the repeated call and the contiguous copy (sentinel and NaN prefill run here)."""
import pytest

from iplan_amd import _lib as L
from tests import behavior_learn_checks as BL
from tests.emu.emu_lib import get_emu_lib


@pytest.fixture(autouse=True)
def emu():
    L.use_library_for_tests(get_emu_lib())
    yield
    L.use_library_for_tests(None)


def _ids(cases):
    return [BL.case_id(*c) for c in cases]


def test_restatement_is_the_oracle_loop():
    BL.check_restatement()


def test_seeded_draw_statistics():
    BL.check_seeded_draw_statistics()


ROW_CASES = [c if c[:2] != (5, 13) else c[:6] + (2,) for c in BL.ROW_CASES if c[0] * c[1] not in (17, 49, 97)]


@pytest.mark.parametrize("case", ROW_CASES, ids=_ids(ROW_CASES))
def test_row_edges_vs_fp64(case):
    BL.check_shape("cpu", *case)


WIDTH_CASES = [c for c in BL.WIDTH_CASES if c[4:6] != (12, 4)]


@pytest.mark.parametrize("case", WIDTH_CASES, ids=_ids(WIDTH_CASES))
def test_width_edges_vs_fp64(case):
    """d <= 8 selects the decoder forward's second form, d > 8 the first form under the second-form BPTT"""
    BL.check_shape("cpu", *case)


@pytest.mark.parametrize("case", BL.WINDOW_CASES[:-1], ids=_ids(BL.WINDOW_CASES[:-1]))
def test_window_edges_vs_fp64(case):
    BL.check_shape("cpu", *case)


def test_short_first_window_range_vs_fp64(monkeypatch):
    """J = 26 at the GPU's default 4 forward / 6 BPTT pieces (set here: the emulator's default is one piece)"""
    BL.check_shape("cpu", *BL.SHORT_RANGE_CASE, env={"IPLAN_BEH_PIECES_FWD": "4", "IPLAN_BEH_PIECES_BWD": "6"}, monkeypatch=monkeypatch)


@pytest.mark.parametrize("kind", BL.MASK_KINDS)
def test_mask_kinds_vs_fp64(kind):
    BL.check_mask_kind("cpu", kind, drops=(False,) if kind in ("random", "ones") else (False, True))


def _emulated_form(rows, form):
    """see the module docstring (test_forms_agree runs the four decoder forms against fp64 at both shapes)"""
    if form in ("default", "dec_fwd_v1", "dec_bwd_v1", "dec_thin_rows", "fwd_save_act", "serial", "pieces_1", "pieces_3_equal"):
        return False
    return rows == 17 or form in ("pieces_3", "accumulate")


@pytest.mark.parametrize("rows,form", [(r, f) for r in (17, 49) for f in BL.FORMS if _emulated_form(r, f)])
def test_forms_vs_fp64(monkeypatch, rows, form):
    BL.check_form("cpu", monkeypatch, rows, form)


@pytest.mark.parametrize("rows", [17, 49])
def test_forms_agree(monkeypatch, rows):
    BL.check_forms_agree("cpu", monkeypatch, rows)


@pytest.mark.parametrize("rows,fwd_v1,bwd_v1,configs", [(17, False, False, (0, 1, 2)), (17, True, True, (0,))])
def test_seeded_draw_equals_explicit_keep(monkeypatch, rows, fwd_v1, bwd_v1, configs):
    BL.check_seeded_equals_explicit("cpu", monkeypatch, rows, fwd_v1, bwd_v1, configs=configs, drop0=len(configs) > 1)


@pytest.mark.parametrize("bwd_v1", [False, True])
def test_arena_ownership_and_repeatability(monkeypatch, bwd_v1):
    BL.check_ownership_and_repeatability("cpu", monkeypatch, bwd_v1, runs=2 if bwd_v1 else 4)


def test_row_independence():
    BL.check_row_independence("cpu")


def test_refusals(monkeypatch):
    BL.check_refusals("cpu", monkeypatch)


@pytest.mark.parametrize("rows,d,Z,with_keep", [(r, d, Z, k) for r in (1, 17, 49) for d, Z in ((5, 8), (9, 7)) for k in (False, True)])
def test_single_window_decoder_vs_fp64(rows, d, Z, with_keep):
    BL.check_bdec_forward("cpu", rows, d, Z, with_keep)
