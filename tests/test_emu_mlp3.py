"""CPU (host-emulated kernels): the stacked three-layer perceptron of the FC ablation (csrc/mlp3.hip) against torch
autograd in fp64 (tests/kernel_checks.py: check_mlp3) -- odd input / output widths, ragged row counts, both output modes and
both gradient sources."""
import pytest

from iplan_amd import _lib as L
from tests import kernel_checks as KC
from tests.emu.emu_lib import get_emu_lib


@pytest.fixture(autouse=True)
def emu():
    L.use_library_for_tests(get_emu_lib())
    yield
    L.use_library_for_tests(None)


MLP3_SHAPES, MLP3_ROW_EDGES = KC.MLP3_SHAPES, KC.MLP3_ROW_EDGES


@pytest.mark.parametrize("K0,H,O,rows,softmax", MLP3_SHAPES)
def test_mlp3_forward_backward_vs_autograd(K0, H, O, rows, softmax):
    KC.check_mlp3("cpu", K0, H, O, rows, softmax)


@pytest.mark.parametrize("K0,H,O,rows,softmax", MLP3_ROW_EDGES)
def test_mlp3_row_edges_vs_autograd(K0, H, O, rows, softmax):
    KC.check_mlp3("cpu", K0, H, O, rows, softmax)
