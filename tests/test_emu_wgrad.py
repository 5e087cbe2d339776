"""CPU (host-emulated kernel build): the weight-gradient contraction against plain torch."""
import pytest
import torch

from iplan_amd import _lib as L
from iplan_amd import ops
from tests import kernel_checks as KC
from tests.emu.emu_lib import get_emu_lib


@pytest.fixture(autouse=True)
def emu():
    L.use_library_for_tests(get_emu_lib())
    yield
    L.use_library_for_tests(None)


def test_wgrad_dense_and_recurrent():
    torch.manual_seed(0)
    n_nets, n_outer, n_inner, H = 2, 7, 5, 32
    dy = torch.randn(n_nets, n_outer, n_inner, 4 * H)          # [dr, dz, dn_i, dn_h]
    hs = torch.randn(n_nets, n_outer, n_inner, H)
    h0 = torch.randn(n_nets, n_outer, H)
    xin = torch.randn(n_nets, n_outer, n_inner, 13)
    grad = torch.zeros(n_nets, 20000)
    grad[:, 5000:5000 + 96 * 13] = 1.0                           # beta = 1 target
    w = ops.Wgrad(grad, n_nets)
    st = (dy.stride(0), dy.stride(1), dy.stride(2))
    # W_hh: dgh = [dr, dz, dn_h] against h_{t-1} (shift -1, h0 for the first step); bias too
    w.add(dy, st, 3 * H, n_outer, n_inner, x=hs, x_strides=(hs.stride(0), hs.stride(1), hs.stride(2)), K=H,
          dw_off=0, db_off=4000, seg=(2 * H, 0, 3 * H), x_shift=-1, x0=h0, x0_strides=(h0.stride(0), h0.stride(1)))
    # W_ih: dgi = [dr, dz, dn_i] against the step input (odd K), accumulated, scaled
    w.add(dy, st, 3 * H, n_outer, n_inner, x=xin, x_strides=(xin.stride(0), xin.stride(1), xin.stride(2)), K=13,
          dw_off=5000, db_off=-1, beta=1.0, scale=0.5)
    # reverse-direction recurrent weight: previous state is step + 1, zeros beyond the end; strided dW
    w.add(dy, st, 3 * H, n_outer, n_inner, x=hs, x_strides=(hs.stride(0), hs.stride(1), hs.stride(2)), K=H,
          dw_off=8000, dw_ld=2 * H, dw_col0=H, x_shift=1)
    # bias only
    w.add(dy, st, 4 * H, n_outer, n_inner, db_off=16000)
    w.run()
    for n in range(n_nets):
        d = dy[n].reshape(-1, 4 * H)
        dgh = torch.cat([d[:, :2 * H], d[:, 3 * H:]], 1)
        hprev = torch.cat([h0[n][:, None], hs[n][:, :-1]], 1).reshape(-1, H)
        ref = dgh.t() @ hprev
        assert torch.allclose(grad[n, :96 * H].view(96, H), ref, rtol=1e-5, atol=1e-5)
        assert torch.allclose(grad[n, 4000:4096], dgh.sum(0), rtol=1e-5, atol=1e-5)
        ref = 1.0 + 0.5 * (d[:, :3 * H].t() @ xin[n].reshape(-1, 13))
        assert torch.allclose(grad[n, 5000:5000 + 96 * 13].view(96, 13), ref, rtol=1e-5, atol=1e-5)
        hnext = torch.cat([hs[n][:, 1:], torch.zeros(n_outer, 1, H)], 1).reshape(-1, H)
        ref = d[:, :3 * H].t() @ hnext
        got = grad[n, 8000:8000 + 96 * 2 * H].view(96, 2 * H)
        assert torch.allclose(got[:, H:], ref, rtol=1e-5, atol=1e-5)
        assert got[:, :H].abs().max() == 0
        assert torch.allclose(grad[n, 16000:16000 + 4 * H], d.sum(0), rtol=1e-5, atol=1e-5)


def test_wgrad_many_rows_chunked():
    torch.manual_seed(1)
    R = 1000
    dy = torch.randn(1, R, 1, 20)
    x = torch.randn(1, R, 1, 70)
    grad = torch.zeros(1, 4000)
    ops.Wgrad(grad, 1).add(dy, (0, 20, 20), 20, R, 1, x=x, x_strides=(0, 70, 70), K=70, dw_off=0, db_off=3000).run()
    ref = dy[0, :, 0].t() @ x[0, :, 0]
    assert torch.allclose(grad[0, :1400].view(20, 70), ref, rtol=1e-5, atol=1e-4)
    assert torch.allclose(grad[0, 3000:3020], dy[0, :, 0].sum(0), rtol=1e-5, atol=1e-4)


JOB_SHAPES, KINDS, EDGE_ROWS = KC.WGRAD_JOB_SHAPES, KC.WGRAD_KINDS, KC.WGRAD_EDGE_ROWS


@pytest.mark.parametrize("O,K,rows,n_inner,shift", JOB_SHAPES)
def test_wgrad_job_shapes_vs_torch(O, K, rows, n_inner, shift):
    """every job shape of wgrad.hip (wide / square / thin), ragged edges, row tails and the shifted recurrent operand: fp64
    reference, 1e-5 of the tensor's maximum, nothing written outside the destinations (tests/kernel_checks.py)"""
    KC.check_wgrad_shapes("cpu", O, K, rows, n_inner, shift)


@pytest.mark.parametrize("n_nets", [1, 5])
@pytest.mark.parametrize("O,K,rows,n_inner,shift", JOB_SHAPES)
def test_wgrad_job_shapes_options_and_nets(O, K, rows, n_inner, shift, n_nets):
    """the same shapes with 1 and 5 nets and -- where there is a dW -- beta = 1 with scale != 1 on a pre-filled destination,
    dw_ld > K with dw_col0 > 0 and the two-segment column map"""
    KC.check_wgrad_shapes("cpu", O, K, rows, n_inner, shift, n_nets=n_nets, options=K > 0)


@pytest.mark.parametrize("total", EDGE_ROWS)
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_wgrad_row_counts_at_block_edges(kind, total):
    O, K = KINDS[kind]
    x0 = kind == "wide_x0"
    KC.check_wgrad_shapes("cpu", O, K, total, 1, 0, x0=False)
    if total % 3 == 0 or x0:                                    # the same total as (outer, inner) rows with the recurrent shifts
        n_inner = 3 if total % 3 == 0 else 1
        KC.check_wgrad_shapes("cpu", O, K, total // n_inner, n_inner, -1, x0=x0)
        KC.check_wgrad_shapes("cpu", O, K, total // n_inner, n_inner, 1)


@pytest.mark.parametrize("n_nets", [1, 5])
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_wgrad_row_counts_at_chunk_target(kind, n_nets):
    """the row count at which a problem's virtual chunks reach their target (128 chunks, 1024 for the thin kinds) with chunks of
    80 rows -- longer than the 64-row minimum -- and a ragged last one: 10 235 / 81 915 rows"""
    O, K = KINDS[kind]
    rows = KC.wgrad_rows_at_chunk_target(O, K, KC.wgrad_chunks_wide(KC.wgrad_wide_jobs(O, K), n_nets))
    x0 = kind == "wide_x0"
    KC.check_wgrad_shapes("cpu", O, K, rows, 1, -1 if x0 else 0, n_nets=n_nets, x0=x0)


def test_wgrad_x0_initial_state_form():
    """the wide job with an initial-state operand (fp32 kernel), ragged on both axes, and a narrow one"""
    KC.check_wgrad_shapes("cpu", 192, 64, 45, 7, -1, x0=True)
    KC.check_wgrad_shapes("cpu", 130, 40, 23, 9, -1, x0=True, options=True)
    KC.check_wgrad_shapes("cpu", 100, 70, 31, 5, -1, x0=True)


def test_wgrad_mixed_launch_and_fixed_order():
    """all four job kinds, a bias-only problem and a GRU pair in one launch of 5 nets (wide chunks trimmed to 68); bitwise equal
    over three runs and against IPLAN_WG_NO_PAIR=1.  The size at which the trimmed chunk count is reached (kernel_checks.MIXED_LARGE:
    5 nets x 5 376 rows through three wide jobs, four launches) takes a minute and a half under the emulator and runs on the GPU
    only (tests/test_gpu_kernels.py)."""
    KC.check_wgrad_mixed_launch("cpu")


@pytest.mark.parametrize("form", KC.SINGLE_FORMS)
def test_wgrad_single_products(form):
    """one product per dW element, every kernel form: db bit-exact, dW within one rounding (fp32 forms) / 2^-22 (split-bf16)"""
    w = KC.check_wgrad_single_products("cpu", form)
    print(form, w)


@pytest.mark.parametrize("O,K,s0", [(192, 64, 0), (192, 64, 3), (40, 13, 0), (5, 64, 2)])
def test_wgrad_column_grouped_operands(O, K, s0):
    """column-grouped operands (the behaviour decoder's records: [tile][16-column group][step][chain][16]; rows = (tile,
    step * 16 + chain)), dY columns through the segment map, X through x_col0, and the recurrent operand read 16 rows back --
    in place where the rows in front of a window range exist (x_pre_valid), zeros in front of step 0"""
    KC.check_wgrad_column_grouped("cpu", O, K, s0)


@pytest.mark.parametrize("s0,steps,tiles", [(0, 7, 3), (3, 9, 2), (0, 70, 1)])
def test_wgrad_gru_pair_shares_the_gate_gradients(s0, steps, tiles):
    """the two wide problems of a 64-wide GRU on column-grouped records (the behaviour decoder's deferred update: dW_ih from
    [dr dz dn_i] x u, dW_hh from [dr dz dn_h] x h_{t-1}) run as ONE paired launch that fetches [dr dz] once
    (wgrad_pair_bf16_kernel): against fp64, and BIT-identical to the two unpaired jobs (IPLAN_WG_NO_PAIR=1); ragged row tail
    (rows not a multiple of 32), a window range that starts past step 0, several row chunks"""
    KC.check_wgrad_gru_pair("cpu", s0, steps, tiles)
