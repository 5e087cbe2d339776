"""CPU (host-emulated kernels): intent knock-out through time -- csrc/enc_knockout.hip through ops.enc_knockout, and
Behavior_policy.latent_knockout -- against beh_eval / latent_trace on explicit copies (bit for bit), fp32 host loops and the fp64
oracle stepped on the modified history (tests/latent_knockout_checks.py)."""
import pytest

from iplan_amd import _lib as L
from tests import latent_knockout_checks as KC
from tests.emu.emu_lib import get_emu_lib


@pytest.fixture(autouse=True)
def emu():
    L.use_library_for_tests(get_emu_lib())
    yield
    L.use_library_for_tests(None)


@pytest.mark.parametrize("E,N,d,Z,Lw,J,n_nets,starts,D,H,cols,baseline", KC.KERNEL_CASES)
def test_enc_knockout_vs_beh_eval_on_a_copy(E, N, d, Z, Lw, J, n_nets, starts, D, H, cols, baseline):
    KC.check_vs_trace("cpu", E, N, d, Z, Lw, J, n_nets, starts, D, H, cols, baseline)


def test_enc_knockout_host_loops():
    KC.check_host_loops("cpu")


def test_enc_knockout_exact_zeros():
    KC.check_exact_zeros("cpu")


def test_enc_knockout_independence():
    KC.check_independence("cpu")


@pytest.mark.parametrize("E,N,d,Z,Lw,J,n_nets,starts,D,H,cols,baseline", KC.ORACLE_CASES)
def test_enc_knockout_vs_fp64(E, N, d, Z, Lw, J, n_nets, starts, D, H, cols, baseline):
    KC.check_vs_fp64("cpu", E, N, d, Z, Lw, J, n_nets, starts, D, H, cols, baseline)


@pytest.mark.parametrize("E,N,d,Z,Lw,J,n_nets,starts,D,H", KC.SENTINEL_CASES)
def test_enc_knockout_writes_only_what_it_owns(E, N, d, Z, Lw, J, n_nets, starts, D, H):
    KC.check_sentinel("cpu", E, N, d, Z, Lw, J, n_nets, starts, D, H)


def test_latent_knockout_on_loaded_checkpoint(tmp_path):
    KC.check_policy_methods("cpu", tmp_path)


def test_latent_knockout_config3_widths(tmp_path):
    KC.check_config3_widths("cpu", tmp_path)


def test_latent_knockout_touches_nothing():
    KC.check_touches_nothing("cpu")


def test_enc_knockout_refusals():
    KC.check_kernel_refusals("cpu")


def test_latent_knockout_refusals():
    KC.check_method_refusals("cpu")


def test_latent_knockout_into_the_policy():
    KC.check_policy_continuation("cpu")
