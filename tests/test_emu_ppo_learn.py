"""CPU (host-emulated kernels): the PPO learning kernels alone -- csrc/ppo.hip's iplan_ppo_prepare, iplan_ppo_adv_norm and iplan_ppo_loss
in every launch form -- against the fp64 oracle (tests/ppo_learn_checks.py).  The committed seeds are held to the conditions on the
inputs here, from the oracle alone."""
import pytest

from iplan_amd import _lib as L
from tests import ppo_learn_checks as PL
from tests.emu.emu_lib import get_emu_lib


@pytest.fixture(autouse=True)
def emu():
    L.use_library_for_tests(get_emu_lib())
    yield
    L.use_library_for_tests(None)


def test_committed_seeds_are_the_first_admissible():
    assert set(PL.SEEDS) == {(nA, r, "drawn") for nA in (1, 3) for r in PL.LOSS_ROWS + (5,)} | {(nA, r, "all") for nA in (1, 3) for r in (65, 1025)}
    for key, seed in PL.SEEDS.items():
        PL.build_rows(*key, seed)                             # (asserts the margins, the edge rows and the branches)
        assert PL.pick_seed(*key) == seed, key


@pytest.mark.parametrize("nA", (1, 3))
@pytest.mark.parametrize("bs,T", PL.PREP_SHAPES)
def test_prepare_vs_fp64(bs, T, nA):
    PL.check_prepare("cpu", nA, bs, T)


@pytest.mark.parametrize("nA", (1, 3))
@pytest.mark.parametrize("n0,n1", PL.NORM_PAIRS)
def test_adv_norm_two_ranks_vs_fp64(n0, n1, nA):
    PL.check_adv_norm_two_ranks("cpu", nA, n0, n1)


@pytest.mark.parametrize("bs,T", PL.NORM_ONE_RANK)
def test_adv_norm_one_rank_is_prepares_own(bs, T):
    PL.check_adv_norm_one_rank("cpu", bs, T)


@pytest.mark.parametrize("nA,rows,live,flags", PL.LOSS_CASES, ids=PL.LOSS_IDS)
def test_loss_one_workgroup_vs_fp64(nA, rows, live, flags):
    PL.check_loss("cpu", nA, rows, live, flags)


@pytest.mark.parametrize("nA", (1, 3))
@pytest.mark.parametrize("rows,P", PL.PART_CASES)
def test_loss_in_parts_vs_fp64(rows, P, nA):
    PL.check_loss_parts("cpu", nA, rows, P)


def test_loss_two_ranks_vs_fp64():
    PL.check_loss_two_ranks("cpu")


@pytest.mark.parametrize("n_parts,rows", ((0, 65), (3, 1025)))
def test_loss_owns_only_its_outputs(n_parts, rows):
    PL.check_loss_ownership("cpu", n_parts, rows=rows)


def test_prepare_owns_only_its_outputs():
    PL.check_prepare_ownership("cpu")


def test_ppo_refusals():
    PL.check_refusals("cpu")
