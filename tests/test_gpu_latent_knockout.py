"""GPU: intent knock-out through time on the gfx950 build -- the same checks the CPU suite runs through the host emulator
(tests/latent_knockout_checks.py), where the MFMA layouts, the cross-lane gathers of the sums of squares, the contraction of the
soft-update expression and the grid geometry are the hardware's and the compiler's.  Worst errors are logged the way
tests/test_gpu_parity_fullsize.py logs its own."""
import pytest

from tests import latent_knockout_checks as KC
from tests.test_gpu_parity_fullsize import _log

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.mark.parametrize("E,N,d,Z,Lw,J,n_nets,starts,D,H,cols,baseline", KC.KERNEL_CASES)
def test_enc_knockout_vs_beh_eval_on_a_copy(E, N, d, Z, Lw, J, n_nets, starts, D, H, cols, baseline):
    KC.check_vs_trace(DEV, E, N, d, Z, Lw, J, n_nets, starts, D, H, cols, baseline)


def test_enc_knockout_host_loops():
    _log("enc_knockout_host_loops", KC.check_host_loops(DEV))


def test_enc_knockout_exact_zeros():
    KC.check_exact_zeros(DEV)


def test_enc_knockout_independence():
    KC.check_independence(DEV)


@pytest.mark.parametrize("E,N,d,Z,Lw,J,n_nets,starts,D,H,cols,baseline", KC.ORACLE_CASES)
def test_enc_knockout_vs_fp64(E, N, d, Z, Lw, J, n_nets, starts, D, H, cols, baseline):
    name = f"enc_knockout_E{E}_N{N}_d{d}_Z{Z}_L{Lw}_J{J}_n{n_nets}_Q{len(starts)}_D{D}_H{H}_{baseline}"
    _log(name, KC.check_vs_fp64(DEV, E, N, d, Z, Lw, J, n_nets, starts, D, H, cols, baseline))


@pytest.mark.parametrize("E,N,d,Z,Lw,J,n_nets,starts,D,H", KC.SENTINEL_CASES)
def test_enc_knockout_writes_only_what_it_owns(E, N, d, Z, Lw, J, n_nets, starts, D, H):
    KC.check_sentinel(DEV, E, N, d, Z, Lw, J, n_nets, starts, D, H)


def test_latent_knockout_on_loaded_checkpoint(tmp_path):
    _log("latent_knockout_policy_methods", KC.check_policy_methods(DEV, tmp_path))


def test_latent_knockout_config3_widths(tmp_path):
    _log("latent_knockout_config3_widths", KC.check_config3_widths(DEV, tmp_path))


def test_latent_knockout_touches_nothing():
    KC.check_touches_nothing(DEV)


def test_enc_knockout_refusals():
    KC.check_kernel_refusals(DEV)


def test_latent_knockout_refusals():
    KC.check_method_refusals(DEV)


def test_latent_knockout_into_the_policy():
    _log("latent_knockout_into_the_policy", KC.check_policy_continuation(DEV))
