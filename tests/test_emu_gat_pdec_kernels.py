"""CPU (host-emulated kernels): the GAT forward / backward and the prediction-decoder forward / loss / backward kernels alone --
ops.gat_forward(save=True) + ops.gat_backward and ops.pdec_forward + ops.pdec_backward called directly -- against the fp64 oracle
(tests/kernel_checks.py); tests/test_gpu_kernels.py runs the same checks on the gfx950 build."""
import pytest

from iplan_amd import _lib as L
from tests import kernel_checks as KC
from tests.emu.emu_lib import get_emu_lib


@pytest.fixture(autouse=True)
def emu():
    L.use_library_for_tests(get_emu_lib())
    yield
    L.use_library_for_tests(None)


def _emulated(B, N, d0, d1, tau, kw):
    """The emulator runs the waves of a scene one after the other -- 0.3 to 1.2 s per scene.  It takes every code path of the case
    list once (a single pair, one tile below / at / one past its 16 egos, a ragged third tile, the narrowest and the widest input
    with and without src1, five nets, strided operands, tau = 0.25); the entity counts that repeat a path at a larger size (32, 48,
    49, 63, 64), the widths between, the 15-scene launches and the 4 x 55 tau = 0.01 case run on the GPU only."""
    if tau < 0.25 or (N, d0, d1) not in [(n, 5, 8) for n in (2, 3, 15, 16, 17, 33)] + [(17, 1, 0), (17, 5, 1), (17, 64, 64)]:
        return False
    return (kw.get("n_nets", 2) == 2 or B == 1) and not (kw.get("strided") and N != 17)


@pytest.mark.parametrize("case", [c for c in KC.GAT_CASES if _emulated(*c)], ids=lambda c: KC.gat_case_id(*c))
def test_gat_kernels_vs_fp64(case):
    B, N, d0, d1, tau, kw = case
    KC.check_gat_kernels("cpu", B, N, d0, d1, tau, **kw)


def test_gat_kernels_write_what_they_own_and_repeat():
    KC.check_gat_ownership_and_repeatability("cpu")


def _emulated_pdec(S, N, P, d, n_nets, keep, teacher, mask_kind, mask_sum):
    """every case but three of the option cross at 65 rows x 5 nets (0.9 s each on the emulator): there the teacher patterns run
    with the keep flags, and the mixed pattern also without them"""
    return not ((S, N, n_nets) == (5, 13, 5) and mask_kind == "random" and not keep and teacher != "mixed" and not mask_sum)


@pytest.mark.parametrize("case", [c for c in KC.PDEC_CASES if _emulated_pdec(*c)], ids=lambda c: KC.pdec_case_id(*c))
def test_pdec_kernels_vs_fp64(case):
    KC.check_pdec_kernels("cpu", *case)


def test_pdec_teacher_flags_that_change_nothing():
    KC.check_pdec_teacher_identities("cpu")


def test_pdec_kernels_write_what_they_own():
    KC.check_pdec_ownership("cpu")


def test_gat_pdec_bad_arguments_are_refused():
    KC.check_gat_pdec_bad_arguments("cpu")
