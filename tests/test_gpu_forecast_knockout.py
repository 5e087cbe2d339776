"""GPU: forecasts under occlusion through time on the gfx950 build -- the same checks the CPU suite runs through the host emulator
(tests/forecast_knockout_checks.py), where the MFMA layouts, the cross-lane fetch of the ``pos`` columns and the unfused fp32
differences are the hardware's.  Worst errors are logged the way tests/test_gpu_knockout.py logs its own."""
import pytest

from tests import forecast_knockout_checks as FC
from tests.test_gpu_parity_fullsize import _log

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _name(spec):
    n, B, J, H, N, P, d, pos, S, start = spec
    return f"n{n}_B{B}_J{J}_H{H}_N{N}_P{P}_d{d}_pos{'_'.join(map(str, pos))}_S{S}_s{start}"


@pytest.mark.parametrize("spec", FC.KERNEL_CASES)
def test_predict_knockout_same_bits_and_ownership(spec):
    _log(f"forecast_knockout_same_bits_{_name(spec)}", FC.check_kernel(DEV, *spec))


@pytest.mark.parametrize("spec", FC.KERNEL_CASES)
def test_predict_knockout_vs_fp64(spec):
    _log(f"forecast_knockout_fp64_{_name(spec)}", FC.check_vs_fp64(DEV, *spec))


def test_predict_knockout_independence_and_prefix():
    FC.check_independence(DEV, 20)


def test_predict_knockout_bad_arguments():
    FC.check_bad_arguments(DEV)


def test_forecast_knockout_method_on_loaded_checkpoint(tmp_path):
    _log("forecast_knockout_methods", FC.check_methods(DEV, tmp_path))


def test_forecast_knockout_one_step_is_attention_knockout(tmp_path):
    _log("forecast_knockout_one_step", FC.check_one_step(DEV, tmp_path))


def test_forecast_knockout_touches_nothing(tmp_path):
    FC.check_nothing_touched(DEV, tmp_path, 20)


def test_learn_unaffected_by_forecast_knockout():
    FC.check_learn_unaffected(DEV)


def test_forecast_knockout_method_refusals():
    FC.check_method_refusals(DEV)
