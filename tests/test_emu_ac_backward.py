"""CPU (host-emulated kernel build): fused actor / critic backward vs autograd of the oracle."""
import pytest

from iplan_amd import _lib as L
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
