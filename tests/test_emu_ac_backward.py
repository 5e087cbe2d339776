"""CPU (host-emulated kernel build): fused actor / critic backward vs autograd of the oracle; below the first three tests, the
kernel-level checks of tests/ac_backward_checks.py, the same parametrisations tests/test_gpu_ac_backward.py runs on the gfx950 build."""
import pytest

from iplan_amd import _lib as L
from tests import ac_backward_checks as AB
from tests import kernel_checks as KC
from tests.emu.emu_lib import get_emu_lib


@pytest.fixture(autouse=True)
def emu():
    L.use_library_for_tests(get_emu_lib())
    yield
    L.use_library_for_tests(None)


def test_actor_critic_backward_matches_autograd():
    KC.check_ac_backward("cpu")


def test_actor_critic_backward_ragged_shape():
    """3 agents, 7 entities, 3 x 7 = 21 rows per agent: not a multiple of the 16-row tile"""
    KC.check_ac_backward("cpu", n_agents=3, max_vehicle_num=7, E=3, T=7)


def test_module_level_autograd():
    """R_Actor.evaluate_actions / R_Critic.forward / GAT_Net.forward called as plain nn.Modules under
    autograd (the way the reference's learner calls them) give the oracle's gradients."""
    KC.check_module_level_autograd("cpu")


# ---- the backward alone, per form, at tile, workgroup and chunk edges (tests/ac_backward_checks.py) ---------------------------
DEV = "cpu"


@pytest.mark.parametrize("rows", tuple(AB.ROWS))
@pytest.mark.parametrize("form", ("stream", "pre"))
def test_every_gradient_vs_fp64(monkeypatch, form, rows):
    AB.check_vs_fp64(DEV, monkeypatch, form, f"rows{rows}")


@pytest.mark.parametrize("form", ("stats", "module"))
def test_every_gradient_vs_fp64_other_forwards(monkeypatch, form):
    AB.check_vs_fp64(DEV, monkeypatch, form, "rows33")


@pytest.mark.parametrize("case", AB.K_CASES, ids=[c[0] for c in AB.K_CASES])
@pytest.mark.parametrize("form", ("stream", "pre"))
def test_k_axis_vs_fp64(monkeypatch, form, case):
    AB.check_vs_fp64(DEV, monkeypatch, form, "k_" + case[0])


@pytest.mark.parametrize("which", (0, 1, 2))
@pytest.mark.parametrize("form", AB.FP32_FORMS)
def test_which_and_ownership(monkeypatch, form, which):
    AB.check_which(DEV, monkeypatch, form, which)


def test_ownership_split_form(monkeypatch):
    AB.check_which(DEV, monkeypatch, "pre", 2)


@pytest.mark.parametrize("ent_rows", (False, True), ids=("g_entropy_const", "g_entropy_rows"))
@pytest.mark.parametrize("rows", (33, 129))
@pytest.mark.parametrize("form", ("stream", "pre"))
def test_row_gradients_and_head_edges(monkeypatch, form, rows, ent_rows):
    AB.check_rows(DEV, monkeypatch, form, rows, ent_rows)


@pytest.mark.parametrize("form", AB.FORMS)
def test_same_bits_where_promised(monkeypatch, form):
    AB.check_same_bits(DEV, monkeypatch, form)


@pytest.mark.parametrize("rows", (33, 129))
@pytest.mark.parametrize("form", ("stream", "pre"))
def test_rechunked_fc1_replays(monkeypatch, form, rows):
    AB.check_rechunk(DEV, monkeypatch, form, rows)


def test_backward_refusals(monkeypatch):
    AB.check_refusals(DEV, monkeypatch)


def test_seeds_keep_the_fp32_oracle_within_the_relu_hint_cap():
    for name, seed in AB.SEEDS.items():
        assert AB.pick_seed(name) == seed, name
