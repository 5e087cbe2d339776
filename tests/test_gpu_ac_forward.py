"""GPU: the actor / critic forward kernel alone on the gfx950 build -- the same checks the CPU suite runs through the host emulator
(tests/ac_forward_checks.py), where the MFMA layouts, the cross-wave and cross-workgroup reductions, the atomic tickets and the
staged four-wave tail are the hardware's.  Worst errors are logged the way tests/test_gpu_parity_fullsize.py logs its own."""
import pytest

from tests import ac_forward_checks as AC
from tests.test_gpu_parity_fullsize import _log

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.mark.parametrize("rows", AC.ROWS_ALL)
@pytest.mark.parametrize("form", AC.FORMS)
def test_form_vs_fp64(monkeypatch, form, rows):
    _log(f"ac_forward_{form}_rows{rows}", AC.check_vs_fp64(DEV, monkeypatch, form, AC.dims_of(rows)))


@pytest.mark.parametrize("rows", AC.ROWS_STREAM)
@pytest.mark.parametrize("form", ("stream", "stream_packed"))
def test_streaming_row_tile_edges_vs_fp64(monkeypatch, form, rows):
    _log(f"ac_forward_{form}_rows{rows}", AC.check_vs_fp64(DEV, monkeypatch, form, AC.dims_of(rows)))


@pytest.mark.parametrize("case", AC.K_CASES, ids=[c[0] for c in AC.K_CASES])
@pytest.mark.parametrize("form", AC.K_FORMS)
def test_k_axis_vs_fp64(monkeypatch, form, case):
    _log(f"ac_forward_{form}_{case[0]}", AC.check_vs_fp64(DEV, monkeypatch, form, case[1], case[2]))


@pytest.mark.parametrize("which", (0, 1, 2))
@pytest.mark.parametrize("form", AC.THREE)
def test_which_vs_fp64(monkeypatch, form, which):
    _log(f"ac_forward_{form}_which{which}", AC.check_vs_fp64(DEV, monkeypatch, form, AC.dims_of(33), which=which))


@pytest.mark.parametrize("form", ("stream", "stats", "pre", "module"))
def test_saving_launch_vs_fp64(monkeypatch, form):
    _log(f"ac_forward_{form}_save", AC.check_vs_fp64(DEV, monkeypatch, form, AC.dims_of(33), save=True))


@pytest.mark.parametrize("form", AC.THREE)
def test_greedy_head(monkeypatch, form):
    _log(f"ac_forward_{form}_greedy", AC.check_greedy(DEV, monkeypatch, form)[0])


@pytest.mark.parametrize("form", AC.THREE)
def test_sampled_head(monkeypatch, form):
    _log(f"ac_forward_{form}_sampled", AC.check_sampled(DEV, monkeypatch, form)[0])


@pytest.mark.parametrize("form", AC.THREE)
def test_exact_ties_go_to_the_lower_index(monkeypatch, form):
    AC.check_ties(DEV, monkeypatch, form)


@pytest.mark.parametrize("mode", (0, 1))
@pytest.mark.parametrize("rows", (17, 33))
@pytest.mark.parametrize("form", AC.THREE)
def test_write_back_destinations(monkeypatch, form, rows, mode):
    AC.check_write_back(DEV, monkeypatch, form, rows, mode)


@pytest.mark.parametrize("form", AC.THREE)
def test_reads_only_what_it_owns(monkeypatch, form):
    AC.check_poison(DEV, monkeypatch, form)


@pytest.mark.parametrize("form", AC.FORMS)
def test_row_independence(monkeypatch, form):
    AC.check_row_independence(DEV, monkeypatch, form)


@pytest.mark.parametrize("form", ("rollout_kw2", "rollout_kw4", "rollout_kw8"))
def test_ksplit_wg_repeatable_and_tickets_zero(monkeypatch, form):
    AC.check_repeatable(DEV, monkeypatch, form)


def test_ksplit_wg_actions_agree(monkeypatch):
    AC.check_kw_actions_agree(DEV, monkeypatch)


def test_refusals(monkeypatch):
    _log("ac_forward_refusals", AC.check_refusals(DEV, monkeypatch))


@pytest.mark.parametrize("shift", AC.SWEEP_SHIFTS)
def test_layernorm_conditioning_sweep(monkeypatch, shift):
    _log(f"ac_forward_conditioning_shift{shift:g}", AC.check_conditioning(DEV, monkeypatch, shift))
