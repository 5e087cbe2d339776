"""GPU: the actor / critic backward alone on the gfx950 build -- the same checks the CPU suite runs through the host emulator
(tests/ac_backward_checks.py), where the MFMA layouts, the LDS-staged transposed weights of the 128-row tail workgroup, the split-bf16
contraction and the side stream of the critic's wgrad jobs are the hardware's.  Worst errors are logged the way
tests/test_gpu_parity_fullsize.py logs its own."""
import pytest

from tests import ac_backward_checks as AB
from tests.test_gpu_parity_fullsize import _log

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.mark.parametrize("rows", tuple(AB.ROWS))
@pytest.mark.parametrize("form", ("stream", "pre"))
def test_every_gradient_vs_fp64(monkeypatch, form, rows):
    _log(f"ac_backward_{form}_rows{rows}", AB.check_vs_fp64(DEV, monkeypatch, form, f"rows{rows}"))


@pytest.mark.parametrize("form", ("stats", "module"))
def test_every_gradient_vs_fp64_other_forwards(monkeypatch, form):
    _log(f"ac_backward_{form}_rows33", AB.check_vs_fp64(DEV, monkeypatch, form, "rows33"))


@pytest.mark.parametrize("case", AB.K_CASES, ids=[c[0] for c in AB.K_CASES])
@pytest.mark.parametrize("form", ("stream", "pre"))
def test_k_axis_vs_fp64(monkeypatch, form, case):
    _log(f"ac_backward_{form}_k_{case[0]}", AB.check_vs_fp64(DEV, monkeypatch, form, "k_" + case[0]))


@pytest.mark.parametrize("which", (0, 1, 2))
@pytest.mark.parametrize("form", AB.FP32_FORMS)
def test_which_and_ownership(monkeypatch, form, which):
    _log(f"ac_backward_{form}_which{which}", AB.check_which(DEV, monkeypatch, form, which))


def test_ownership_split_form(monkeypatch):
    _log("ac_backward_pre_which2", AB.check_which(DEV, monkeypatch, "pre", 2))


@pytest.mark.parametrize("ent_rows", (False, True), ids=("g_entropy_const", "g_entropy_rows"))
@pytest.mark.parametrize("rows", (33, 129))
@pytest.mark.parametrize("form", ("stream", "pre"))
def test_row_gradients_and_head_edges(monkeypatch, form, rows, ent_rows):
    _log(f"ac_backward_{form}_rowgrads{rows}_{'ent_rows' if ent_rows else 'ent_const'}", AB.check_rows(DEV, monkeypatch, form, rows, ent_rows))


@pytest.mark.parametrize("form", AB.FORMS)
def test_same_bits_where_promised(monkeypatch, form):
    _log(f"ac_backward_{form}_reversed", AB.check_same_bits(DEV, monkeypatch, form))


@pytest.mark.parametrize("rows", (33, 129))
@pytest.mark.parametrize("form", ("stream", "pre"))
def test_rechunked_fc1_replays(monkeypatch, form, rows):
    _log(f"ac_backward_{form}_rechunk{rows}", AB.check_rechunk(DEV, monkeypatch, form, rows))


def test_backward_refusals(monkeypatch):
    _log("ac_backward_refusals", AB.check_refusals(DEV, monkeypatch))
