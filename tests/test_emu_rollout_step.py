"""CPU (host-emulated kernels): the three kernels of a rollout vector step alone -- enc_fwd_kernel through ops.enc_forward,
gat_enc_fwd_kernel and gat_enc_ac_fwd_kernel through ops.gat_forward(fuse_enc=, fuse_ac=) -- at the edges of their tiles and grids
(tests/rollout_step_checks.py).  The emulator runs workgroups in index order on plain memory: it checks the index math, the
ownership and the argument checks here; the hand-off between workgroups is the GPU twin's (tests/test_gpu_rollout_step.py)."""
import pytest

from iplan_amd import _lib as L
from tests import rollout_step_checks as RS
from tests.emu.emu_lib import get_emu_lib

DEV = "cpu"


@pytest.fixture(autouse=True)
def emu():
    L.use_library_for_tests(get_emu_lib())
    yield
    L.use_library_for_tests(None)


@pytest.mark.parametrize("case", RS.ENC_CASES, ids=[c[0] for c in RS.ENC_CASES])
def test_encoder_alone_vs_fp64(case):
    RS.check_encoder(DEV, case)


@pytest.mark.parametrize("case", RS.TWO_WAY_CASES, ids=[c[0] for c in RS.TWO_WAY_CASES])
def test_scenes_and_encoder_in_one_launch(case):
    RS.check_two_way(DEV, case, exact=True)


@pytest.mark.parametrize("case", RS.BODY_CASES, ids=[RS.body_case_id(c) for c in RS.BODY_CASES])
def test_rollout_body_at_edge_shapes(case, monkeypatch):
    monkeypatch.delenv("IPLAN_AC_KSPLIT_WG", raising=False)
    worst = RS.check_body(DEV, case)
    assert max(worst.values()) < 1e-5


@pytest.mark.parametrize("case", RS.BODY_CASES, ids=[RS.body_case_id(c) for c in RS.BODY_CASES])
def test_body_seeds_leave_no_row_inside_the_key_margin(case):
    assert RS.body_key_margin(case) >= RS.KEY_MARGIN


@pytest.mark.parametrize("case", RS.STALE_CASES, ids=[RS.body_case_id(c) for c in RS.STALE_CASES])
def test_stale_seeds_leave_no_row_inside_the_key_margin(case):
    assert RS.body_key_margin(case, episodes=(0, 1)) >= RS.KEY_MARGIN


def test_launch_picks_ksplit_wg_2_at_42_units(monkeypatch):
    RS.check_launch_picks_kw2(DEV, monkeypatch)


@pytest.mark.parametrize("case", RS.STALE_CASES, ids=[RS.body_case_id(c) for c in RS.STALE_CASES])
def test_second_episode_into_a_used_container(case, monkeypatch):
    monkeypatch.delenv("IPLAN_AC_KSPLIT_WG", raising=False)
    RS.check_stale_latents(DEV, case)


@pytest.mark.parametrize("rows", RS.STEP_ROWS)
def test_one_fused_step_from_ops_pieces(monkeypatch, rows):
    RS.check_step(DEV, monkeypatch, rows, exact=True)


def test_step_q_seeds_leave_no_row_inside_the_margin():
    for rows, seed in RS.STEP_Q_SEEDS.items():
        assert RS.pick_step_q_seed(rows) == seed


def test_grid_sizes_of_the_three_launches(monkeypatch):
    import ctypes
    fn = get_emu_lib().c.iplan_emu_blocks_launched
    fn.restype = ctypes.c_ulonglong
    RS.check_grids(DEV, monkeypatch, fn)


def test_refusals(monkeypatch):
    RS.check_refusals(DEV, monkeypatch)
