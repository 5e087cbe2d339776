"""CPU (host-emulated kernels): the actor / critic forward kernel alone -- csrc/actor_critic.hip, csrc/ac_fwd_body.h through
ops.ac_forward -- in each of its launch forms against the fp64 oracle (tests/ac_forward_checks.py)."""
import pytest

from iplan_amd import _lib as L
from tests import ac_forward_checks as AC
from tests.emu.emu_lib import get_emu_lib

DEV = "cpu"


@pytest.fixture(autouse=True)
def emu():
    L.use_library_for_tests(get_emu_lib())
    yield
    L.use_library_for_tests(None)


@pytest.mark.parametrize("rows", AC.ROWS_ALL)
@pytest.mark.parametrize("form", AC.FORMS)
def test_form_vs_fp64(monkeypatch, form, rows):
    AC.check_vs_fp64(DEV, monkeypatch, form, AC.dims_of(rows))


@pytest.mark.parametrize("rows", AC.ROWS_STREAM)
@pytest.mark.parametrize("form", ("stream", "stream_packed"))
def test_streaming_row_tile_edges_vs_fp64(monkeypatch, form, rows):
    AC.check_vs_fp64(DEV, monkeypatch, form, AC.dims_of(rows))


@pytest.mark.parametrize("case", AC.K_CASES, ids=[c[0] for c in AC.K_CASES])
@pytest.mark.parametrize("form", AC.K_FORMS)
def test_k_axis_vs_fp64(monkeypatch, form, case):
    AC.check_vs_fp64(DEV, monkeypatch, form, case[1], case[2])


@pytest.mark.parametrize("which", (0, 1, 2))
@pytest.mark.parametrize("form", AC.THREE)
def test_which_vs_fp64(monkeypatch, form, which):
    AC.check_vs_fp64(DEV, monkeypatch, form, AC.dims_of(33), which=which)


@pytest.mark.parametrize("form", ("stream", "stats", "pre", "module"))
def test_saving_launch_vs_fp64(monkeypatch, form):
    AC.check_vs_fp64(DEV, monkeypatch, form, AC.dims_of(33), save=True)


@pytest.mark.parametrize("form", AC.THREE)
def test_greedy_head(monkeypatch, form):
    AC.check_greedy(DEV, monkeypatch, form)


@pytest.mark.parametrize("form", AC.THREE)
def test_sampled_head(monkeypatch, form):
    AC.check_sampled(DEV, monkeypatch, form)


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
    AC.check_refusals(DEV, monkeypatch)


def test_q_seeds_leave_no_row_inside_the_margin():
    for rows, seed in AC.Q_SEEDS.items():
        assert AC.pick_q_seed(rows) == seed


@pytest.mark.parametrize("shift", AC.SWEEP_SHIFTS)
def test_layernorm_conditioning_sweep(monkeypatch, shift):
    AC.check_conditioning(DEV, monkeypatch, shift)
