"""CPU (host-emulated kernels): forecasts under occlusion through time -- csrc/predict_knockout.hip through ops.predict_knockout, and
Prediction_policy.attention_knockout_trace(forecast=True) -- against ops.predict and the fp32 host loops, bit for bit, and against the
fp64 oracle (tests/forecast_knockout_checks.py)."""
import pytest

from iplan_amd import _lib as L
from tests import forecast_knockout_checks as FC
from tests.emu.emu_lib import get_emu_lib


@pytest.fixture(autouse=True)
def emu():
    L.use_library_for_tests(get_emu_lib())
    yield
    L.use_library_for_tests(None)


@pytest.mark.parametrize("spec", FC.KERNEL_CASES)
def test_predict_knockout_same_bits_and_ownership(spec):
    FC.check_kernel("cpu", *spec)


@pytest.mark.parametrize("spec", FC.KERNEL_CASES)
def test_predict_knockout_vs_fp64(spec):
    FC.check_vs_fp64("cpu", *spec)


def test_predict_knockout_independence_and_prefix():
    FC.check_independence("cpu", 2)


def test_predict_knockout_bad_arguments():
    FC.check_bad_arguments("cpu")


def test_forecast_knockout_method_on_loaded_checkpoint(tmp_path):
    FC.check_methods("cpu", tmp_path)


def test_forecast_knockout_one_step_is_attention_knockout(tmp_path):
    FC.check_one_step("cpu", tmp_path)


def test_forecast_knockout_touches_nothing(tmp_path):
    FC.check_nothing_touched("cpu", tmp_path, 2)


def test_learn_unaffected_by_forecast_knockout():
    FC.check_learn_unaffected("cpu")


def test_forecast_knockout_method_refusals():
    FC.check_method_refusals("cpu")
