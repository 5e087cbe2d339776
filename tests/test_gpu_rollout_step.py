"""GPU: the three kernels of a rollout vector step alone on the gfx950 build -- the same case lists the CPU suite runs through the
host emulator (tests/rollout_step_checks.py), where the device-coherent stores of the scenes and encoder tiles, their drain and
count into sync[0], the action selection's poll and its untracked coherent loads are the hardware's.  Worst errors are logged the
way tests/test_gpu_parity_fullsize.py logs its own."""
import pytest

from tests import rollout_step_checks as RS
from tests.test_gpu_parity_fullsize import _log

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.mark.parametrize("case", RS.ENC_CASES, ids=[c[0] for c in RS.ENC_CASES])
def test_encoder_alone_vs_fp64(case):
    _log(f"rollout_step_encoder_{case[0]}", RS.check_encoder(DEV, case))


@pytest.mark.parametrize("case", RS.TWO_WAY_CASES, ids=[c[0] for c in RS.TWO_WAY_CASES])
def test_scenes_and_encoder_in_one_launch(case):
    _log(f"rollout_step_two_way_{case[0]}", RS.check_two_way(DEV, case, exact=False))


@pytest.mark.parametrize("case", RS.BODY_CASES, ids=[RS.body_case_id(c) for c in RS.BODY_CASES])
def test_rollout_body_at_edge_shapes(case, monkeypatch):
    monkeypatch.delenv("IPLAN_AC_KSPLIT_WG", raising=False)
    _log(f"rollout_step_body_{RS.body_case_id(case)}", RS.check_body(DEV, case))


def test_launch_picks_ksplit_wg_2_at_42_units(monkeypatch):
    RS.check_launch_picks_kw2(DEV, monkeypatch)


@pytest.mark.parametrize("case", RS.STALE_CASES, ids=[RS.body_case_id(c) for c in RS.STALE_CASES])
def test_second_episode_into_a_used_container(case, monkeypatch):
    monkeypatch.delenv("IPLAN_AC_KSPLIT_WG", raising=False)
    _log(f"rollout_step_stale_{RS.body_case_id(case)}", RS.check_stale_latents(DEV, case))


@pytest.mark.parametrize("rows", RS.STEP_ROWS)
def test_one_fused_step_from_ops_pieces(monkeypatch, rows):
    _log(f"rollout_step_direct_rows{rows}", RS.check_step(DEV, monkeypatch, rows, exact=False))


def test_refusals(monkeypatch):
    _log("rollout_step_refusals", RS.check_refusals(DEV, monkeypatch))
