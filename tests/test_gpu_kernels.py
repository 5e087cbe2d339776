"""GPU: the standalone kernels one at a time against fp64 references (tests/kernel_checks.py) -- the same checks the CPU suite
runs through the host emulator, on the gfx950 build, where the MFMA operand layouts, the bf16 conversions of the split form,
the cross-lane reductions and the grid geometry are the hardware's: every wgrad job shape at the edges of its chunk geometry
(incl. the row counts at which the virtual chunks reach their target, and the mixed launch whose wide chunks are trimmed as in
production), wgrad one product at a time, its fixed reduction order, mlp3, the actor / critic backward, the optimiser kernels,
the rollout body in config 1's feature layout (GAT and behaviour off), and the prediction learner's four kernels alone: GAT
forward + backward at every tile edge of the entity count with a well-conditioned gate (tau = 1, 0.25), the prediction decoder
with its teacher / mask_sum / keep arguments.
Worst errors are logged the way tests/test_gpu_parity_fullsize.py logs its own (copied to profiles/ as the tolerance evidence)."""
import os

import pytest
import torch

from tests import kernel_checks as KC
from tests.test_gpu_parity_fullsize import _log

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.mark.parametrize("O,K,rows,n_inner,shift", KC.WGRAD_JOB_SHAPES)
def test_wgrad_job_shapes(O, K, rows, n_inner, shift):
    _log(f"kernel_wgrad_shape_O{O}_K{K}_r{rows}x{n_inner}_s{shift}", KC.check_wgrad_shapes(DEV, O, K, rows, n_inner, shift))


@pytest.mark.parametrize("n_nets", [1, 5])
@pytest.mark.parametrize("O,K,rows,n_inner,shift", KC.WGRAD_JOB_SHAPES)
def test_wgrad_job_shapes_options_and_nets(O, K, rows, n_inner, shift, n_nets):
    _log(f"kernel_wgrad_options_O{O}_K{K}_r{rows}x{n_inner}_s{shift}_n{n_nets}",
                  KC.check_wgrad_shapes(DEV, O, K, rows, n_inner, shift, n_nets=n_nets, options=K > 0))


@pytest.mark.parametrize("total", KC.WGRAD_EDGE_ROWS)
@pytest.mark.parametrize("kind", sorted(KC.WGRAD_KINDS))
def test_wgrad_row_counts_at_block_edges(kind, total):
    O, K = KC.WGRAD_KINDS[kind]
    x0 = kind == "wide_x0"
    worst = KC.check_wgrad_shapes(DEV, O, K, total, 1, 0)
    if total % 3 == 0 or x0:
        n_inner = 3 if total % 3 == 0 else 1
        for w in (KC.check_wgrad_shapes(DEV, O, K, total // n_inner, n_inner, -1, x0=x0), KC.check_wgrad_shapes(DEV, O, K, total // n_inner, n_inner, 1)):
            worst = {k: max(worst[k], w[k]) for k in worst}
    _log(f"kernel_wgrad_rows_{kind}_{total}", worst)


@pytest.mark.parametrize("n_nets", [1, 5])
@pytest.mark.parametrize("kind", sorted(KC.WGRAD_KINDS))
def test_wgrad_row_counts_at_chunk_target(kind, n_nets):
    """the row count at which a problem's virtual chunks reach their target (128, 1024 for the thin kinds) with chunks longer
    than the minimum and a ragged last one"""
    O, K = KC.WGRAD_KINDS[kind]
    rows = KC.wgrad_rows_at_chunk_target(O, K, KC.wgrad_chunks_wide(KC.wgrad_wide_jobs(O, K), n_nets))
    x0 = kind == "wide_x0"
    _log(f"kernel_wgrad_chunk_target_{kind}_n{n_nets}", KC.check_wgrad_shapes(DEV, O, K, rows, 1, -1 if x0 else 0, n_nets=n_nets, x0=x0))


def test_wgrad_x0_initial_state_form():
    worst = {}
    for w in (KC.check_wgrad_shapes(DEV, 192, 64, 45, 7, -1, x0=True), KC.check_wgrad_shapes(DEV, 130, 40, 23, 9, -1, x0=True, options=True),
              KC.check_wgrad_shapes(DEV, 100, 70, 31, 5, -1, x0=True)):
        worst = {k: max(worst.get(k, 0.0), w[k]) for k in w}
    _log("kernel_wgrad_x0", worst)


@pytest.mark.parametrize("size", ["small", "chunk_target"])
def test_wgrad_mixed_launch_and_fixed_order(size):
    """every job kind and a GRU pair in one launch of 5 nets, the wide chunks trimmed to 68; three runs and the unpaired form
    bitwise equal.  `chunk_target`: 68 chunks of 80 rows, the last one ragged"""
    kw = KC.MIXED_LARGE if size == "chunk_target" else {}
    _log(f"kernel_wgrad_mixed_{size}", KC.check_wgrad_mixed_launch(DEV, **kw))


@pytest.mark.parametrize("form", KC.SINGLE_FORMS)
def test_wgrad_single_products(form):
    _log(f"kernel_wgrad_single_products_{form}", KC.check_wgrad_single_products(DEV, form))


@pytest.mark.parametrize("O,K,s0", [(192, 64, 0), (192, 64, 3), (40, 13, 0), (5, 64, 2)])
def test_wgrad_column_grouped_operands(O, K, s0):
    _log(f"kernel_wgrad_column_grouped_O{O}_K{K}_s{s0}", KC.check_wgrad_column_grouped(DEV, O, K, s0))


@pytest.mark.parametrize("s0,steps,tiles", [(0, 7, 3), (3, 9, 2), (0, 70, 1)])
def test_wgrad_gru_pair(s0, steps, tiles):
    _log(f"kernel_wgrad_gru_pair_s{s0}_{steps}x{tiles}", KC.check_wgrad_gru_pair(DEV, s0, steps, tiles))


@pytest.mark.parametrize("K0,H,O,rows,softmax", KC.MLP3_SHAPES + KC.MLP3_ROW_EDGES)
def test_mlp3_vs_autograd(K0, H, O, rows, softmax):
    _log(f"kernel_mlp3_K{K0}_H{H}_O{O}_r{rows}_{'softmax' if softmax else 'identity'}", KC.check_mlp3(DEV, K0, H, O, rows, softmax))


@pytest.mark.parametrize("shape", ["small", "ragged"])
def test_actor_critic_backward_vs_autograd(shape):
    kw = dict(n_agents=3, max_vehicle_num=7, E=3, T=7) if shape == "ragged" else {}
    _log(f"kernel_ac_backward_{shape}", KC.check_ac_backward(DEV, **kw))


def test_module_level_autograd():
    _log("kernel_module_level_autograd", KC.check_module_level_autograd(DEV))


def test_clip_adam():
    _log("kernel_clip_adam", KC.check_clip_adam(DEV))


def test_adam_weight_decay():
    _log("kernel_adam_weight_decay", KC.check_adam_weight_decay(DEV))


@pytest.mark.parametrize("n", KC.ADAM_SIZES)
def test_clip_adam_sizes(n):
    _log(f"kernel_clip_adam_n{n}", KC.check_clip_adam_sizes(DEV, n))


@pytest.mark.parametrize("case", KC.GAT_CASES, ids=lambda c: KC.gat_case_id(*c))
def test_gat_kernels_vs_fp64(case):
    B, N, d0, d1, tau, kw = case
    _log("kernel_gat_" + KC.gat_case_id(*case), KC.check_gat_kernels(DEV, B, N, d0, d1, tau, **kw))


def test_gat_kernels_write_what_they_own_and_repeat():
    _log("kernel_gat_ownership_repeatability", KC.check_gat_ownership_and_repeatability(DEV))


@pytest.mark.parametrize("case", KC.PDEC_CASES, ids=lambda c: KC.pdec_case_id(*c))
def test_pdec_kernels_vs_fp64(case):
    _log("kernel_pdec_" + KC.pdec_case_id(*case), KC.check_pdec_kernels(DEV, *case))


def test_pdec_teacher_flags_that_change_nothing():
    _log("kernel_pdec_teacher_identities", KC.check_pdec_teacher_identities(DEV))


def test_pdec_kernels_write_what_they_own():
    _log("kernel_pdec_ownership", KC.check_pdec_ownership(DEV))


def test_gat_pdec_bad_arguments_are_refused():
    _log("kernel_gat_pdec_bad_arguments", KC.check_gat_pdec_bad_arguments(DEV))


def test_rollout_body_config1_vs_oracle():
    """config 1's feature layout (GAT off, behaviour off): 4 envs x 5 agents x 55 entities, 4 steps"""
    from iplan_amd.config import default_args
    from tests.rollout_oracle import check_rollout_body
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    args = default_args("highway", use_cuda=True, GAT_enable=False, Behavior_enable=False, GAT_use_behavior=False, episode_limit=4,
                        batch_size_run=4)
    _log("kernel_rollout_body_cfg1_E4_T4", check_rollout_body(args, 4, DEV, seed=24))
