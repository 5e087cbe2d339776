// Forecasts of the knocked chains through time: predict_kernel's decoder chain (predict.hip)
//    y_p, h = Linear(tanh(GRU(ReLU(Linear(y_{p-1})), h))),  y_{-1} = state at the row's step,  h_0 = the knocked chain's latent,  p < P
// run over the latents gat_knockout_trace.hip wrote, and reduced where it runs to P numbers per row -- "vehicle j was out of sight for
// D steps; how far does every ego's forecast of the scene move, and how much worse does it get against what then happened?".
//
// One wave = 16 rows of one agent-net, weights in LDS, the chain in registers in the D layout (wave_tile.h), the same fp32 MFMA chains in
// the same order as predict_kernel: pred_ko carries iplan_predict's bits.  The decoder step is RESTATED here, not shared through a
// header with predict.hip: that file's code object stays the parent's byte for byte, and the step is nine lines of gru_tile.h calls.
// A row is (net, b, job slot q, window step h, entity i), in the order a contiguous latent_ko [n_nets, B, J, H, N, 32] lies in memory;
// every operand and output is addressed through (net, b, job, step) strides, so that a chunk of a larger result is written in place.
//   * h_0 = latent_ko row; y_{-1} = history row (net, b, start + h, i), read in place at any alignment (d = 5 rows) and NEVER knocked,
//     whatever the job was: the result isolates the social path.
//   * fshift_sq[row][p] = sum over k of (y_p[pos[k]] - base_p[pos[k]])^2, k ascending, base = pred_base row (net, b, h, i) written by an
//     earlier iplan_predict launch on the walk with nothing knocked.  Every lane squares the differences of its own four columns; the
//     columns of `pos` may lie in different lane groups, so every lane of a row fetches them by __shfl in `pos` order and lane group 0
//     stores.  Difference, product and sum are rounded one by one (no fma): the plain fp32 host loop gives the same bits.
//   * ferr_sq[row][p]: the same sum against the recorded future, history row (net, b, start + h + 1 + p, i); +0.0 where that step is
//     not recorded (the address is clamped to the last recorded step and the loaded value masked: no branch around a load).
//   * The base and target rows are the only HBM streams inside the loop: step p + 1's rows are requested before step p's arithmetic.
// No atomics, no sums across rows: a slot's bits depend on its row and the arguments only.  The padding lanes of a ragged last tile
// walk row 0 and write nothing.
#include "api_util.h"
#include "gru_tile.h"

namespace iplan {
namespace {

constexpr int KH = 32;            // attention_dim == decoder hidden
constexpr int KLD = KH + 4;

#ifdef IPLAN_HOST_EMULATION
inline float __fsub_rn(float a, float b) { return a - b; }
inline float __fmul_rn(float a, float b) { return a * b; }
inline float __fadd_rn(float a, float b) { return a + b; }
#endif

// predict.hip's row_load: columns 4g .. 4g+3 of a d-wide row of any alignment, four unconditional dword loads from clamped addresses,
// zeroed by a lane mask.  `row` must be a readable row even where `ok` is false.
__device__ __forceinline__ f32x4 ko_row_load(const float* __restrict__ row, bool ok, int d) {
    const int c0 = 4 * (lane_id() >> 4);
    const IPLAN_GLOBAL_AS float* p = as_global(row);
    f32x4 v;
    for (int q = 0; q < 4; ++q) {
        const bool in = c0 + q < d;
        v[q] = keep_if(ok && in, p[in ? c0 + q : 0]);
    }
    return v;
}

// (y[c] - ref[c])^2 of the lane's four columns.  Contraction is off for the whole function (knock_shift.h: the __f*_rn of the HIP
// headers are plain operators and would fuse again once inlined under the default -ffp-contract=fast).
__device__ __forceinline__ f32x4 ko_sq_diff(f32x4 y, f32x4 ref) {
#pragma clang fp contract(off)
    f32x4 r;
    for (int q = 0; q < 4; ++q) {
        const float dl = __fsub_rn(y[q], ref[q]);
        r[q] = __fmul_rn(dl, dl);
    }
    return r;
}

// sum over k of the row's sq[pos[k]], k ascending, on every lane of the row: column c lives in component c & 3 of lane group c >> 2
__device__ __forceinline__ float ko_pos_sum(f32x4 sq, const IplanPredictKnockoutArgs& a) {
#pragma clang fp contract(off)
    const int n = lane_id() & 15;
    float s = 0.f;
    for (int k = 0; k < a.n_pos; ++k) {
        const int c = a.pos[k], q = c & 3;
        const float mine = q == 0 ? sq[0] : (q == 1 ? sq[1] : (q == 2 ? sq[2] : sq[3]));
        s = __fadd_rn(s, __shfl(mine, n + 16 * (c >> 2)));
    }
    return s;
}

template <bool SHIFT, bool ERR>
__global__ __launch_bounds__(256) void predict_knockout_kernel(IplanPredictKnockoutArgs a) {
    __shared__ __attribute__((aligned(16))) float s_lin[KH * 20];
    __shared__ __attribute__((aligned(16))) float s_wih[3 * KH * KLD];
    __shared__ __attribute__((aligned(16))) float s_whh[3 * KH * KLD];
    __shared__ __attribute__((aligned(16))) float s_out[16 * KLD];
    __shared__ __attribute__((aligned(16))) float s_blin[KH], s_bih[3 * KH], s_bhh[3 * KH], s_bout[16];

    const int net = (int)blockIdx.y;
    const float* __restrict__ W = a.params + (int64_t)net * a.params_s_net;
    stage_matrix(s_lin, 20, KH, W + a.off[IPLAN_DEC_LIN_W], KH, a.d);
    stage_matrix(s_wih, KLD, 3 * KH, W + a.off[IPLAN_DEC_WIH], 3 * KH, KH);
    stage_matrix(s_whh, KLD, 3 * KH, W + a.off[IPLAN_DEC_WHH], 3 * KH, KH);
    stage_matrix(s_out, KLD, 16, W + a.off[IPLAN_DEC_OUT_W], a.d, KH);
    stage_vector(s_blin, KH, W + a.off[IPLAN_DEC_LIN_B], KH);
    stage_vector(s_bih, 3 * KH, W + a.off[IPLAN_DEC_BIH], 3 * KH);
    stage_vector(s_bhh, 3 * KH, W + a.off[IPLAN_DEC_BHH], 3 * KH);
    stage_vector(s_bout, 16, W + a.off[IPLAN_DEC_OUT_B], a.d);
    __syncthreads();

    const int l = lane_id(), n = l & 15, g = l >> 4;
    const int rows = a.B * a.J * a.H * a.N;
    const int tile = (int)blockIdx.x * 4 + wave_id();
    const int tiles = (rows + 15) / 16;
    if (tile >= tiles) return;
    const int row = tile * 16 + n;
    const bool valid = row < rows;
    const int rc = valid ? row : 0;                       // padding lanes of a ragged last tile read row 0 and write nothing
    int t = rc / a.N;
    const int i = rc - t * a.N;
    const int h = t % a.H;
    t /= a.H;
    const int q = t % a.J, b = t / a.J;
    const int P = a.P, d = a.d;

    const float* hrow = a.history + (int64_t)net * a.hist_s_net + (int64_t)b * a.hist_s_b + (int64_t)i * a.hist_s_ent;
    const float* lrow = a.latent_ko + (int64_t)net * a.lat_s_net + (int64_t)b * a.lat_s_b + (int64_t)q * a.lat_s_job +
                        (int64_t)h * a.lat_s_step + (int64_t)i * KH;
    const float* brow = nullptr;
    if (SHIFT) brow = a.pred_base + (int64_t)net * a.pb_s_net + (int64_t)b * a.pb_s_b + (int64_t)h * a.pb_s_step + (int64_t)i * P * d;
    // the row's outputs, [P] and [P, d] at entity i of (net, b, q, h)
    const int64_t fs_at = (int64_t)net * a.fs_s_net + (int64_t)b * a.fs_s_b + (int64_t)q * a.fs_s_job + (int64_t)h * a.fs_s_step + (int64_t)i * P;
    const int64_t fe_at = (int64_t)net * a.fe_s_net + (int64_t)b * a.fe_s_b + (int64_t)q * a.fe_s_job + (int64_t)h * a.fe_s_step + (int64_t)i * P;
    const int64_t pk_at = (int64_t)net * a.pk_s_net + (int64_t)b * a.pk_s_b + (int64_t)q * a.pk_s_job + (int64_t)h * a.pk_s_step + (int64_t)i * P * d;
    const int s0 = a.start + h;                           // the row's own step; its targets are steps s0 + 1 + p
    const int last = a.S - 1;                             // ERR: the last recorded step, >= s0 (the entry point)

    f32x4 x[1], hh[2];
    x[0] = ko_row_load(hrow + (int64_t)s0 * a.hist_s_step, valid, d);
    hh[0] = vload(lrow, valid, KH, 0);
    hh[1] = vload(lrow, valid, KH, 1);
    f32x4 yb = splat4(0.f), tg = splat4(0.f);
    if (SHIFT) yb = ko_row_load(brow, valid, d);
    if (ERR) tg = ko_row_load(hrow + (int64_t)imin(s0 + 1, last) * a.hist_s_step, valid && s0 + 1 <= last, d);
    for (int p = 0; p < P; ++p) {
        // step p + 1's base and target rows are requested before step p's arithmetic (the last step re-reads its own base row; a
        // target step that is not recorded is clamped to the last recorded one and masked)
        f32x4 yb_next = yb, tg_next = tg;
        if (SHIFT) yb_next = ko_row_load(brow + (int64_t)imin(p + 1, P - 1) * d, valid, d);
        if (ERR) tg_next = ko_row_load(hrow + (int64_t)imin(s0 + 2 + p, last) * a.hist_s_step, valid && s0 + 2 + p <= last, d);
        f32x4 u[2];
        u[0] = relu4(dense_tile<1>(s_lin, 20, 0, x, bfrag_lds(s_blin, 0)));
        u[1] = relu4(dense_tile<1>(s_lin, 20, 16, x, bfrag_lds(s_blin, 1)));
        gru_step_lds<2, 2>(s_wih, KLD, s_whh, KLD, s_bih, s_bhh, u, hh, nullptr);
        f32x4 act[2];
        for (int T = 0; T < 2; ++T)
            for (int c = 0; c < 4; ++c) act[T][c] = tanh_f(hh[T][c]);
        const f32x4 y = dense_tile<2>(s_out, KLD, 0, act, bfrag_lds(s_bout, 0));
        if (a.pred_ko) {
            float* prow = a.pred_ko + pk_at + (int64_t)p * d;
            for (int c = 0; c < 4; ++c)
                if (valid && 4 * g + c < d) prow[4 * g + c] = y[c];
        }
        if (SHIFT) {
            const float s = ko_pos_sum(ko_sq_diff(y, yb), a);
            if (valid && g == 0) a.fshift_sq[fs_at + p] = s;
            yb = yb_next;
        }
        if (ERR) {
            const float s = ko_pos_sum(ko_sq_diff(y, tg), a);
            if (valid && g == 0) a.ferr_sq[fe_at + p] = s0 + 1 + p <= last ? s : 0.f;
            tg = tg_next;
        }
        x[0] = y;
    }
}

}  // namespace
}  // namespace iplan

extern "C" int iplan_predict_knockout(const IplanPredictKnockoutArgs* a, iplan_stream_t stream) {
    using namespace iplan;
    const char* who = "iplan_predict_knockout";
    if (!a) return fail(IPLAN_EINVAL, "%s: null args", who);
    if (a->n_nets < 1 || a->n_nets > IPLAN_MAX_NETS || a->B < 1 || a->J < 1 || a->H < 1 || a->N < 1 || a->P < 1 || a->d < 1 || a->d > 16 ||
        a->start < 0)
        return fail(IPLAN_EINVAL, "%s: unsupported dims n_nets=%d B=%d J=%d H=%d N=%d P=%d d=%d start=%d", who, a->n_nets, a->B, a->J, a->H,
                    a->N, a->P, a->d, a->start);
    if ((int64_t)a->B * a->J * a->H * a->N > 0x7fffffff - 16)
        return fail(IPLAN_EINVAL, "%s: B * J * H * N = %lld rows per net exceed 2^31 - 17", who, (long long)a->B * a->J * a->H * a->N);
    if (!a->history || !a->latent_ko || !a->params) return fail(IPLAN_EINVAL, "%s: null tensor pointer", who);
    if (!a->fshift_sq && !a->ferr_sq && !a->pred_ko) return fail(IPLAN_EINVAL, "%s: no output asked for", who);
    if (a->fshift_sq && !a->pred_base)
        return fail(IPLAN_EINVAL, "%s: fshift_sq needs pred_base, the forecasts of the window with nothing knocked", who);
    if (a->ferr_sq && (int64_t)a->start + a->H > a->S)
        return fail(IPLAN_EINVAL, "%s: ferr_sq needs a readable window, start + H = %lld > S = %d recorded steps", who,
                    (long long)a->start + a->H, a->S);
    if (a->fshift_sq || a->ferr_sq) {
        if (a->n_pos < 1 || a->n_pos > 16) return fail(IPLAN_EINVAL, "%s: n_pos=%d outside [1,16]", who, a->n_pos);
        unsigned seen = 0;
        for (int k = 0; k < a->n_pos; ++k) {
            const int c = a->pos[k];
            if (c < 0 || c >= a->d) return fail(IPLAN_EINVAL, "%s: pos[%d]=%d outside [0,%d)", who, k, c, a->d);
            if (seen >> c & 1u) return fail(IPLAN_EINVAL, "%s: pos[%d]=%d is repeated", who, k, c);
            seen |= 1u << c;
        }
    }
    if (!aligned16(a->latent_ko) || (a->lat_s_net & 3) || (a->lat_s_b & 3) || (a->lat_s_job & 3) || (a->lat_s_step & 3))
        return fail(IPLAN_EALIGN, "%s: latent_ko must be 16-byte aligned with strides %% 4 == 0", who);
    const int tiles = (a->B * a->J * a->H * a->N + 15) / 16;
    const dim3 grid((unsigned)((tiles + 3) / 4), (unsigned)a->n_nets);
    const hipStream_t st = (hipStream_t)stream;
    if (a->fshift_sq && a->ferr_sq)
        hipLaunchKernelGGL((predict_knockout_kernel<true, true>), grid, dim3(256), 0, st, *a);
    else if (a->fshift_sq)
        hipLaunchKernelGGL((predict_knockout_kernel<true, false>), grid, dim3(256), 0, st, *a);
    else if (a->ferr_sq)
        hipLaunchKernelGGL((predict_knockout_kernel<false, true>), grid, dim3(256), 0, st, *a);
    else
        hipLaunchKernelGGL((predict_knockout_kernel<false, false>), grid, dim3(256), 0, st, *a);
    return check_launch(who);
}
