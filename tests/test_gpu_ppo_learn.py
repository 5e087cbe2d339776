"""GPU: the PPO learning kernels alone on the gfx950 build -- the same checks the CPU suite runs through the host emulator
(tests/ppo_learn_checks.py), where the 16-wave tree of the 1024-thread workgroup, its barriers, expf, the division and the grid of
n_parts workgroups per agent are the hardware's.  Worst errors are logged the way tests/test_gpu_parity_fullsize.py logs its own."""
import pytest

from tests import ppo_learn_checks as PL
from tests.test_gpu_parity_fullsize import _log

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.mark.parametrize("nA", (1, 3))
@pytest.mark.parametrize("bs,T", PL.PREP_SHAPES)
def test_prepare_vs_fp64(bs, T, nA):
    _log(f"ppo_learn_prepare_nA{nA}_bs{bs}_T{T}", PL.check_prepare(DEV, nA, bs, T))


@pytest.mark.parametrize("nA", (1, 3))
@pytest.mark.parametrize("n0,n1", PL.NORM_PAIRS)
def test_adv_norm_two_ranks_vs_fp64(n0, n1, nA):
    _log(f"ppo_learn_adv_norm_nA{nA}_{n0}_{n1}", PL.check_adv_norm_two_ranks(DEV, nA, n0, n1))


@pytest.mark.parametrize("bs,T", PL.NORM_ONE_RANK)
def test_adv_norm_one_rank_is_prepares_own(bs, T):
    _log(f"ppo_learn_adv_norm_one_rank_bs{bs}_T{T}", PL.check_adv_norm_one_rank(DEV, bs, T))


@pytest.mark.parametrize("nA,rows,live,flags", PL.LOSS_CASES, ids=PL.LOSS_IDS)
def test_loss_one_workgroup_vs_fp64(nA, rows, live, flags):
    _log(f"ppo_learn_loss_nA{nA}_rows{rows}_{live}_flags{flags}", PL.check_loss(DEV, nA, rows, live, flags))


@pytest.mark.parametrize("nA", (1, 3))
@pytest.mark.parametrize("rows,P", PL.PART_CASES)
def test_loss_in_parts_vs_fp64(rows, P, nA):
    _log(f"ppo_learn_loss_parts_nA{nA}_rows{rows}_P{P}", PL.check_loss_parts(DEV, nA, rows, P))


def test_loss_two_ranks_vs_fp64():
    _log("ppo_learn_loss_two_ranks", PL.check_loss_two_ranks(DEV))


@pytest.mark.parametrize("n_parts,rows", ((0, 65), (3, 1025)))
def test_loss_owns_only_its_outputs(n_parts, rows):
    _log(f"ppo_learn_loss_ownership_parts{n_parts}", PL.check_loss_ownership(DEV, n_parts, rows=rows))


def test_prepare_owns_only_its_outputs():
    _log("ppo_learn_prepare_ownership", PL.check_prepare_ownership(DEV))


def test_ppo_refusals():
    _log("ppo_learn_refusals", PL.check_refusals(DEV))
