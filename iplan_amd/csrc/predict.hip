// Trajectory-prediction INFERENCE: the chain of pdec_fwd_kernel (preddec.hip) in eval mode,
//    y_p, h = Linear(tanh(GRU(ReLU(Linear(y_{p-1})), h))),  y_{-1} = state at the start step,  h_0 = GAT output,  p < P
// (Prediction_Decoder.forward(last_state, None, hidden) under .eval(), nova/prediction_net.py:40-63: no teacher forcing, no
// dropout), forward only.  Same work layout as the training kernel -- one wave = 16 (sample, entity) rows of one agent-net,
// weights in LDS, the chain in registers in the D layout (wave_tile.h), the same fp32 MFMA chains in the same order -- but
//   * no activation record (the training forward streams IPLAN_PDEC_SAVE = 256 floats per (row, step) for its backward),
//   * no dropout and no teacher operand,
//   * the start state and the targets are read IN PLACE from the episode buffer through one element offset per (net, sample)
//     and the buffer's entity / time-step strides: no gathered copy of either exists,
//   * optional outputs: the predictions, and / or three weighted error sums per (net, horizon step) -- displacement over the
//     position columns, L1 over all columns, weight -- from which ADE / FDE follow.  Without the sums no target is read.
// The sums are reduced in a fixed order (per-tile partials, then one wave per (net, step, sum) over the tiles): no
// floating-point atomics, two launches on the same inputs give the same bits.
#include "api_util.h"
#include "gru_tile.h"

namespace iplan {

constexpr int QH = 32;            // attention_dim == decoder hidden
constexpr int QLD = QH + 4;

// Columns 4g .. 4g+3 of a d-wide row that need not be 16-byte aligned (d = 5 rows of an episode buffer): four unconditional
// dword loads from clamped addresses, zeroed by a lane mask -- no branch around a load, so the loads of the next step can stay
// in flight under this step's arithmetic (wave_tile.h: keep_if).  `row` must be a readable row even where `ok` is false.
__device__ __forceinline__ f32x4 row_load(const float* __restrict__ row, bool ok, int d) {
    const int c0 = 4 * (lane_id() >> 4);
    const IPLAN_GLOBAL_AS float* p = as_global(row);
    f32x4 v;
    for (int q = 0; q < 4; ++q) {
        const bool in = c0 + q < d;
        v[q] = keep_if(ok && in, p[in ? c0 + q : 0]);
    }
    return v;
}

__device__ __forceinline__ float chain_sum_q(float v) {
    v += __shfl_xor(v, 1);
    v += __shfl_xor(v, 2);
    v += __shfl_xor(v, 4);
    v += __shfl_xor(v, 8);
    return v;
}

// [value of column `col` of the chain's row != 0], on every lane of the chain
__device__ __forceinline__ float present(f32x4 v, int col) {
    const int c0 = 4 * (lane_id() >> 4);
    float f = 0.f;
    for (int q = 0; q < 4; ++q)
        if (c0 + q == col && v[q] != 0.f) f = 1.f;
    return group_sum(f);
}

template <bool METRICS>
__global__ __launch_bounds__(256) void predict_kernel(IplanPredictArgs a) {
    __shared__ __attribute__((aligned(16))) float s_lin[QH * 20];
    __shared__ __attribute__((aligned(16))) float s_wih[3 * QH * QLD];
    __shared__ __attribute__((aligned(16))) float s_whh[3 * QH * QLD];
    __shared__ __attribute__((aligned(16))) float s_out[16 * QLD];
    __shared__ __attribute__((aligned(16))) float s_blin[QH], s_bih[3 * QH], s_bhh[3 * QH], s_bout[16];

    const int net = (int)blockIdx.y;
    const float* __restrict__ W = a.params + (int64_t)net * a.params_s_net;
    stage_matrix(s_lin, 20, QH, W + a.off[IPLAN_DEC_LIN_W], QH, a.d);
    stage_matrix(s_wih, QLD, 3 * QH, W + a.off[IPLAN_DEC_WIH], 3 * QH, QH);
    stage_matrix(s_whh, QLD, 3 * QH, W + a.off[IPLAN_DEC_WHH], 3 * QH, QH);
    stage_matrix(s_out, QLD, 16, W + a.off[IPLAN_DEC_OUT_W], a.d, QH);
    stage_vector(s_blin, QH, W + a.off[IPLAN_DEC_LIN_B], QH);
    stage_vector(s_bih, 3 * QH, W + a.off[IPLAN_DEC_BIH], 3 * QH);
    stage_vector(s_bhh, 3 * QH, W + a.off[IPLAN_DEC_BHH], 3 * QH);
    stage_vector(s_bout, 16, W + a.off[IPLAN_DEC_OUT_B], a.d);
    __syncthreads();

    const int l = lane_id(), n = l & 15, g = l >> 4;
    const int rows = a.S * a.N;
    const int tile = (int)blockIdx.x * 4 + wave_id();
    const int tiles = (rows + 15) / 16;
    if (tile >= tiles) return;
    const int row = tile * 16 + n;
    const bool valid = row < rows;
    const int rc = valid ? row : 0;                       // padding lanes of a ragged last tile read row 0 and write nothing
    const int s = rc / a.N, e = rc - s * a.N;
    const int64_t gr = (int64_t)net * rows + rc;
    const int64_t at = a.offset[(int64_t)net * a.S + s] + (int64_t)e * a.ent_stride;

    f32x4 x[1], h[2];
    x[0] = row_load(a.x0 + at, valid, a.d);
    h[0] = vload(a.h0 + gr * QH, valid, QH, 0);
    h[1] = vload(a.h0 + gr * QH, valid, QH, 1);
    float w0 = 0.f;
    f32x4 tg = splat4(0.f);
    if (METRICS) {
        w0 = valid ? (a.weight ? a.weight[(int64_t)net * a.S + s] : 1.0f) : 0.f;
        if (a.presence_col >= 0) w0 *= present(x[0], a.presence_col);
        tg = row_load(a.target + at + a.step_stride, valid, a.d);
    }
    for (int p = 0; p < a.P; ++p) {
        // the target rows are the only HBM stream inside the loop: step p + 1's row is requested before step p's arithmetic
        // (the last step re-reads its own row: an address that is always inside the window)
        f32x4 tg_next = tg;
        if (METRICS) tg_next = row_load(a.target + at + (int64_t)(p + 2 < a.P + 1 ? p + 2 : a.P) * a.step_stride, valid, a.d);
        f32x4 u[2];
        u[0] = relu4(dense_tile<1>(s_lin, 20, 0, x, bfrag_lds(s_blin, 0)));
        u[1] = relu4(dense_tile<1>(s_lin, 20, 16, x, bfrag_lds(s_blin, 1)));
        gru_step_lds<2, 2>(s_wih, QLD, s_whh, QLD, s_bih, s_bhh, u, h, nullptr);
        f32x4 act[2];
        for (int T = 0; T < 2; ++T)
            for (int q = 0; q < 4; ++q) act[T][q] = tanh_f(h[T][q]);
        const f32x4 y = dense_tile<2>(s_out, QLD, 0, act, bfrag_lds(s_bout, 0));
        if (a.pred) {
            float* prow = a.pred + (gr * a.P + p) * a.d;
            for (int q = 0; q < 4; ++q)
                if (valid && 4 * g + q < a.d) prow[4 * g + q] = y[q];
        }
        if (METRICS) {
            float sq = 0.f, l1 = 0.f;
            for (int q = 0; q < 4; ++q) {
                const int c = 4 * g + q;
                const float dlt = c < a.d ? tg[q] - y[q] : 0.f;
                l1 += fabsf(dlt);
                if (c >= a.pos_first && c < a.pos_first + a.pos_count) sq = fmaf(dlt, dlt, sq);
            }
            float w = w0;
            if (a.presence_col >= 0) w *= present(tg, a.presence_col);
            const float dist = sqrtf(group_sum(sq));
            l1 = group_sum(l1);
            // every lane of a chain holds the chain's values; lane group 0 alone enters the sum over the 16 chains.  A zero
            // weight drops the row whatever its error is (also a non-finite one)
            const bool on = w != 0.f;
            const float s0 = chain_sum_q(on ? w * dist : 0.f);
            const float s1 = chain_sum_q(on ? w * l1 : 0.f);
            const float s2 = chain_sum_q(w);
            if (l < 3) a.part[(((int64_t)net * a.P + p) * 3 + l) * tiles + tile] = l == 0 ? s0 : (l == 1 ? s1 : s2);
            tg = tg_next;
        }
        x[0] = y;
    }
}

// metrics[net][p][k] = sum over the tiles of part[net][p][k][tile]: lane i adds tiles i, i + 64, ... in order, then the butterfly
__global__ __launch_bounds__(64) void predict_reduce_kernel(IplanPredictArgs a) {
    const int64_t j = (int64_t)blockIdx.x;                // (net, p, k)
    const int tiles = (a.S * a.N + 15) / 16;
    float v = 0.f;
    for (int i = lane_id(); i < tiles; i += 64) v += a.part[j * tiles + i];
    v = wave_sum(v);
    if (lane_id() == 0) a.metrics[j] = v;
}

}  // namespace iplan

extern "C" int iplan_predict(const IplanPredictArgs* a, iplan_stream_t stream) {
    using namespace iplan;
    if (!a) return fail(IPLAN_EINVAL, "iplan_predict: null args");
    if (a->n_nets < 1 || a->n_nets > IPLAN_MAX_NETS || a->S < 1 || a->N < 1 || a->P < 1 || a->d < 1 || a->d > 16 ||
        (int64_t)a->S * a->N > 0x7fffffff - 16)
        return fail(IPLAN_EINVAL, "iplan_predict: unsupported dims n_nets=%d S=%d N=%d P=%d d=%d", a->n_nets, a->S, a->N, a->P, a->d);
    if (!a->x0 || !a->h0 || !a->offset || !a->params) return fail(IPLAN_EINVAL, "iplan_predict: null tensor pointer");
    if (!a->pred && !a->metrics) return fail(IPLAN_EINVAL, "iplan_predict: neither pred nor metrics asked for");
    if (a->metrics) {
        if (!a->target || !a->part) return fail(IPLAN_EINVAL, "iplan_predict: metrics need target and part");
        if (a->presence_col >= a->d || a->pos_first < 0 || a->pos_count < 1 || a->pos_first + a->pos_count > a->d)
            return fail(IPLAN_EINVAL, "iplan_predict: presence_col=%d pos_first=%d pos_count=%d outside d=%d", a->presence_col,
                        a->pos_first, a->pos_count, a->d);
    }
    const int tiles = (a->S * a->N + 15) / 16;
    const dim3 grid((unsigned)((tiles + 3) / 4), (unsigned)a->n_nets);
    if (a->metrics) {
        hipLaunchKernelGGL(predict_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, *a);
        hipLaunchKernelGGL(predict_reduce_kernel, dim3((unsigned)(a->n_nets * a->P * 3)), dim3(64), 0, (hipStream_t)stream, *a);
    } else {
        hipLaunchKernelGGL(predict_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, *a);
    }
    return check_launch("iplan_predict");
}
