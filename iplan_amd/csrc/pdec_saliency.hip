// Prediction saliency: d <v, y_p> / d x0 and d <v, y_p> / d h0, the input Jacobian of the trajectory predictor's chain (the one predict.hip walks;
// Prediction_Decoder.forward(last_state, None, hidden) under .eval(): Linear -> ReLU -> GRU32 -> tanh -> Linear, fed back autoregressively):
//    x_0 = start state, h_{-1} = h0;  t < P:  u_t = ReLU(W_lin x_t + b),  h_t = GRU32(u_t, h_{t-1}),  y_t = W_out tanh(h_t) + b_out,  x_{t+1} = y_t
// Against pdec_bwd_kernel (preddec.hip), which forms PARAMETER gradients of the loss from 256 recorded floats per (row, step) and sums over the
// rows: this one differentiates a chosen output with respect to the INPUTS, per row, and records nothing in global memory.
// Work layout: one wave per (16-row tile, job), a job = (horizon step p, cotangent v).  The wave walks the chain from (x0, h0) to step p - 1,
// keeping the state and the input every step ENTERS with in its own LDS slab (3 KB per step: 16 rows x (32 + 16) floats), then walks back from
// d y_p = v with each step's gates recomputed from (h_{t-1}, x_t):
//    dh += tanh'(h_t) . W_out^T dy,   [dr dz dn] from gru_gates_bwd,   dh = z dh + W_hh^T [dr | dz | r dn],   dy = dx_t = W_lin^T (relu' . W_ih^T [dr | dz | dn])
// One more wave per tile (asked for with pred / active) walks all P steps forward with predict_kernel's arithmetic in its order and writes the
// predictions and the ReLU branch masks.  Why a wave per job and not a wave per tile walking its jobs: the chain is short (P = 5) and a tile's jobs
// are independent, so the grid is K times larger where rows are few (110 tiles per net at the shipped sizes against 1024 SIMDs) for p extra forward
// steps per job; the slab is sized by the deepest horizon asked for and the number of waves per workgroup follows from it.
// All weights sit in LDS in BOTH orientations, staged once per workgroup (70 KB); the slab is lane-private (every lane reads back only what it wrote:
// D layout in, D layout out), so a wave never waits for another.  No atomics, no sums across rows: the MFMA keeps rows in separate columns, so a
// slot's bits do not depend on its lane, tile, workgroup, on P, on the other jobs or on which outputs were asked for.
#include "api_util.h"
#include "gru_tile.h"

namespace iplan {

constexpr int PH = 32, PHT = 2, PHLD = PH + 8;     // attention_dim == decoder hidden; leading dims: ld % 16 == 8 -> conflict-free fragment reads
constexpr int PLLD = 24;                           // leading dim of [.. x 16] matrices (d <= 16 real columns)
constexpr int PGLD = 3 * PH + 8;                   // leading dim of the transposed GRU weights [32 x 96]
constexpr int P_LIN = 0;                           // W_lin   [32 x d]
constexpr int P_LINT = P_LIN + PH * PLLD;          // W_lin^T [16 x 32]
constexpr int P_WIH = P_LINT + 16 * PHLD;          // W_ih    [96 x 32]
constexpr int P_WHH = P_WIH + 3 * PH * PHLD;       // W_hh    [96 x 32]
constexpr int P_WIHT = P_WHH + 3 * PH * PHLD;      // W_ih^T  [32 x 96]
constexpr int P_WHHT = P_WIHT + PH * PGLD;         // W_hh^T  [32 x 96]
constexpr int P_OUT = P_WHHT + PH * PGLD;          // W_out   [d x 32]
constexpr int P_OUTT = P_OUT + 16 * PHLD;          // W_out^T [32 x d]
constexpr int P_B = P_OUTT + PH * PLLD;            // biases: linear 0 (32) | b_ih 32 (96) | b_hh 128 (96) | out 224 (16)
constexpr int P_W_FLOATS = P_B + PH + 6 * PH + 16;
constexpr int P_LDS_FLOATS = 160 * 1024 / 4;
constexpr int P_STEP_FLOATS = 16 * PH + 16 * 16;   // per wave and chain step: the entering state and the input of 16 rows
static_assert(P_W_FLOATS % 4 == 0 && P_B % 4 == 0 && P_LINT % 4 == 0 && P_OUTT % 4 == 0, "16-byte aligned fragments");
static_assert(P_W_FLOATS + IPLAN_PDEC_SAL_MAX_P * P_STEP_FLOATS <= P_LDS_FLOATS, "one wave's slab must fit beside the weights");
static_assert(P_W_FLOATS + (IPLAN_PDEC_SAL_MAX_P + 1) * P_STEP_FLOATS > P_LDS_FLOATS, "IPLAN_PDEC_SAL_MAX_P is what the LDS budget admits");
static_assert(IPLAN_PDEC_SAL_MAX_P >= 8, "horizons up to 8 at least");

inline int pdec_sal_waves(int Pn) { return imin(4, (P_LDS_FLOATS - P_W_FLOATS) / (Pn * P_STEP_FLOATS)); }

__device__ __forceinline__ void pdec_sal_stage(float* lds, const IplanPdecSaliencyArgs& a, int net) {
    const float* __restrict__ W = a.params + (int64_t)net * a.params_s_net;
    stage_matrix(lds + P_LIN, PLLD, PH, W + a.off[IPLAN_DEC_LIN_W], PH, a.d);
    stage_matrix_t(lds + P_LINT, PHLD, 16, W + a.off[IPLAN_DEC_LIN_W], PH, a.d);
    stage_matrix(lds + P_WIH, PHLD, 3 * PH, W + a.off[IPLAN_DEC_WIH], 3 * PH, PH);
    stage_matrix(lds + P_WHH, PHLD, 3 * PH, W + a.off[IPLAN_DEC_WHH], 3 * PH, PH);
    stage_matrix_t(lds + P_WIHT, PGLD, PH, W + a.off[IPLAN_DEC_WIH], 3 * PH, PH);
    stage_matrix_t(lds + P_WHHT, PGLD, PH, W + a.off[IPLAN_DEC_WHH], 3 * PH, PH);
    stage_matrix(lds + P_OUT, PHLD, 16, W + a.off[IPLAN_DEC_OUT_W], a.d, PH);
    stage_matrix_t(lds + P_OUTT, PLLD, PH, W + a.off[IPLAN_DEC_OUT_W], a.d, PH);
    stage_vector(lds + P_B, PH, W + a.off[IPLAN_DEC_LIN_B], PH);
    stage_vector(lds + P_B + 32, 3 * PH, W + a.off[IPLAN_DEC_BIH], 3 * PH);
    stage_vector(lds + P_B + 128, 3 * PH, W + a.off[IPLAN_DEC_BHH], 3 * PH);
    stage_vector(lds + P_B + 224, 16, W + a.off[IPLAN_DEC_OUT_B], a.d);
}

// columns 4g .. 4g+3 of a d-wide row that need not be 16-byte aligned, zero past column d (the loads are clamped to the row and masked
// bitwise: a NaN in a float that is not the row's own never enters the arithmetic)
__device__ __forceinline__ f32x4 pdec_sal_row(const float* __restrict__ row, int d, int g) {
    const IPLAN_GLOBAL_AS float* p = as_global(row);
    f32x4 v;
    for (int q = 0; q < 4; ++q) {
        const int i = 4 * g + q;
        v[q] = keep_if(i < d, p[i < d ? i : 0]);
    }
    return v;
}

// one chain step, predict_kernel's arithmetic in its order: u = ReLU(W_lin x + b_lin), h = GRU32(u, h); `keep`: the gates for the way back
__device__ __forceinline__ void pdec_sal_step(const float* lds, f32x4 xv, f32x4 (&u)[PHT], f32x4 (&h)[PHT], GruGates* keep) {
    const f32x4 x[1] = {xv};
    u[0] = relu4(dense_tile<1>(lds + P_LIN, PLLD, 0, x, bfrag_lds(lds + P_B, 0)));
    u[1] = relu4(dense_tile<1>(lds + P_LIN, PLLD, 16, x, bfrag_lds(lds + P_B, 1)));
    gru_step_lds<PHT, PHT>(lds + P_WIH, PHLD, lds + P_WHH, PHLD, lds + P_B + 32, lds + P_B + 128, u, h, keep);
}

// y = W_out tanh(h) + b_out; `act` returns tanh(h)
__device__ __forceinline__ f32x4 pdec_sal_out(const float* lds, const f32x4 (&h)[PHT], f32x4 (&act)[PHT]) {
    for (int T = 0; T < PHT; ++T)
        for (int q = 0; q < 4; ++q) act[T][q] = tanh_f(h[T][q]);
    return dense_tile<PHT>(lds + P_OUT, PHLD, 0, act, bfrag_lds(lds + P_B + 224, 0));
}

// sum_c |G_c| and sum_c G_c X_c over the `dim` real columns of a row, in COLUMN order on one lane: the row's four lanes hand their
// columns over one at a time.  Every product and every sum is rounded on its own (no contraction into an fma), so the results are the
// plain fp32 loops over the stored gradient.
template <int NT>
__device__ __forceinline__ void pdec_sal_sums(const f32x4 (&G)[NT], const f32x4 (&X)[NT], int dim, float& l1, float& gx) {
#pragma clang fp contract(off)
    const int n = lane_id() & 15;
    float s1 = 0.f, s2 = 0.f;
    for (int T = 0; T < NT; ++T)
        for (int gg = 0; gg < 4; ++gg)
            for (int q = 0; q < 4; ++q) {
                const float gv = __shfl(G[T][q], n + 16 * gg);
                const float xv = __shfl(X[T][q], n + 16 * gg);
                if (16 * T + 4 * gg + q < dim) {
                    const float pr = gv * xv;
                    s1 = s1 + fabsf(gv);
                    s2 = s2 + pr;
                }
            }
    l1 = s1;
    gx = s2;
}

// KT = tasks per tile: the jobs 0 .. Kj-1 and, with pred / active asked for, the forward walk as task Kj
__global__ __launch_bounds__(256) void pdec_sal_kernel(IplanPdecSaliencyArgs a, int Pn, int wpb, int Kj, int KT) {
    IPLAN_DYN_LDS(lds);
    const int net = (int)blockIdx.y;
    pdec_sal_stage(lds, a, net);
    __syncthreads();
    const int l = lane_id(), n = l & 15, g = l >> 4;
    const int rows = a.S * a.N;
    const int tiles = (rows + 15) / 16;
    const int P = a.P, d = a.d, K = a.K;
    const int64_t task = (int64_t)blockIdx.x * wpb + uniform_i(wave_id());
    if (task >= (int64_t)tiles * KT) return;
    const int tile = (int)(task / KT), k = uniform_i((int)(task - (int64_t)tile * KT));
    const int row = tile * 16 + n;
    const bool valid = row < rows;
    const int rc = valid ? row : 0;                       // padding lanes of a ragged last tile walk row 0 and write nothing
    const int s = rc / a.N, e = rc - s * a.N;
    const int64_t gr = (int64_t)net * rows + rc;
    const int64_t at = a.offset[(int64_t)net * a.S + s] + (int64_t)e * a.ent_stride;

    f32x4 x = pdec_sal_row(a.x0 + at, d, g), h[PHT];
    for (int T = 0; T < PHT; ++T) h[T] = vload(a.h0 + gr * PH, true, PH, T);

    if (k >= Kj) {
        // ---- the forward walk: the predictions (bit for bit iplan_predict's) and the ReLU branches of every step
        for (int t = 0; t < P; ++t) {
            f32x4 u[PHT], act[PHT];
            pdec_sal_step(lds, x, u, h, nullptr);
            const f32x4 y = pdec_sal_out(lds, h, act);
            if (a.pred) {
                float* prow = a.pred + (gr * P + t) * d;
                for (int q = 0; q < 4; ++q)
                    if (valid && 4 * g + q < d) prow[4 * g + q] = y[q];
            }
            if (a.active) {
                uint32_t bits = 0;
                for (int T = 0; T < PHT; ++T)
                    for (int q = 0; q < 4; ++q) bits |= u[T][q] > 0.0f ? 1u << (16 * T + 4 * g + q) : 0u;
                int b = (int)bits;
                b |= __shfl_xor(b, 16);
                b |= __shfl_xor(b, 32);
                if (valid && g == 0) a.active[gr * P + t] = b;
            }
            x = y;
        }
        return;
    }

    // ---- one job: walk to step p, then back
    const int p = a.jobs[2 * k], c = a.jobs[2 * k + 1];
    // lane-private LDS: the entering states hs[t][T] and inputs xs[t], one f32x4 per lane each
    float* slab = lds + P_W_FLOATS + wave_id() * Pn * P_STEP_FLOATS;
    f32x4* hs = reinterpret_cast<f32x4*>(slab) + l;                     // hs[(t * PHT + T) * 64]
    f32x4* xs = reinterpret_cast<f32x4*>(slab + Pn * 16 * PH) + l;      // xs[t * 64]
    const f32x4 x0 = x;
    f32x4 h0[PHT];
    for (int T = 0; T < PHT; ++T) h0[T] = h[T];
    for (int t = 0; t < p; ++t) {
        for (int T = 0; T < PHT; ++T) hs[(t * PHT + T) * 64] = h[T];
        xs[t * 64] = x;
        f32x4 u[PHT], act[PHT];
        pdec_sal_step(lds, x, u, h, nullptr);
        x = pdec_sal_out(lds, h, act);
    }
    for (int T = 0; T < PHT; ++T) hs[(p * PHT + T) * 64] = h[T];
    xs[p * 64] = x;

    f32x4 dy;                                                           // the cotangent on y_p, columns 4g .. 4g+3
    if (c < 0) {
        const float* vrow = a.v + (gr * P + p) * d;
        for (int q = 0; q < 4; ++q) dy[q] = 4 * g + q < d ? vrow[4 * g + q] : 0.f;
    } else {
        for (int q = 0; q < 4; ++q) dy[q] = 4 * g + q == c ? 1.f : 0.f;
    }
    f32x4 dh[PHT];
    for (int T = 0; T < PHT; ++T) dh[T] = splat4(0.f);
    for (int t = p; t >= 0; --t) {
        f32x4 hp[PHT], ht[PHT], u[PHT], act[PHT];
        for (int T = 0; T < PHT; ++T) ht[T] = hp[T] = hs[(t * PHT + T) * 64];
        GruGates keep[PHT];
        pdec_sal_step(lds, xs[t * 64], u, ht, keep);
        for (int T = 0; T < PHT; ++T)
            for (int q = 0; q < 4; ++q) act[T][q] = tanh_f(ht[T][q]);
        // y_t = W_out tanh(h_t) + b: the output layer and tanh', onto what the later steps handed back for h_t
        const f32x4 dyv[1] = {dy};
        f32x4 di[3 * PHT], dg[3 * PHT], direct[PHT];
        for (int T = 0; T < PHT; ++T) {
            const f32x4 da = dense_tile<1>(lds + P_OUTT, PLLD, 16 * T, dyv, splat4(0.f));
            for (int q = 0; q < 4; ++q) dh[T][q] += da[q] * (1.0f - act[T][q] * act[T][q]);
            const GruGrads o = gru_gates_bwd(dh[T], keep[T].r, keep[T].z, keep[T].n, keep[T].hn, hp[T]);
            di[T] = dg[T] = o.dr;
            di[PHT + T] = dg[PHT + T] = o.dz;
            di[2 * PHT + T] = o.dni;
            dg[2 * PHT + T] = o.dnh;
            direct[T] = o.dh_direct;
        }
        f32x4 du[PHT];
        for (int T = 0; T < PHT; ++T) {
            du[T] = dense_tile<3 * PHT>(lds + P_WIHT, PGLD, 16 * T, di, splat4(0.f));
            dh[T] = dense_tile<3 * PHT>(lds + P_WHHT, PGLD, 16 * T, dg, direct[T]);
            for (int q = 0; q < 4; ++q) du[T][q] = u[T][q] > 0.0f ? du[T][q] : 0.0f;
        }
        dy = dense_tile<PHT>(lds + P_LINT, PHLD, 0, du, splat4(0.f));   // dx_t, and x_t = y_{t-1}
    }

    const int64_t slot = gr * K + k;
    if (a.state_grad) {
        float* grow = a.state_grad + slot * d;
        for (int q = 0; q < 4; ++q)
            if (valid && 4 * g + q < d) grow[4 * g + q] = dy[q];
    }
    if (a.latent_grad)
        for (int T = 0; T < PHT; ++T) vstore(a.latent_grad + slot * PH, valid, PH, T, dh[T]);
    if (a.state_l1 || a.state_gxi) {
        const f32x4 G[1] = {dy}, X[1] = {x0};
        float l1, gx;
        pdec_sal_sums<1>(G, X, d, l1, gx);
        if (valid && g == 0) {
            if (a.state_l1) a.state_l1[slot] = l1;
            if (a.state_gxi) a.state_gxi[slot] = gx;
        }
    }
    if (a.latent_l1 || a.latent_gxi) {
        float l1, gx;
        pdec_sal_sums<PHT>(dh, h0, PH, l1, gx);
        if (valid && g == 0) {
            if (a.latent_l1) a.latent_l1[slot] = l1;
            if (a.latent_gxi) a.latent_gxi[slot] = gx;
        }
    }
}

}  // namespace iplan

extern "C" int iplan_pdec_saliency(const IplanPdecSaliencyArgs* a, iplan_stream_t stream) {
    using namespace iplan;
    if (!a) return fail(IPLAN_EINVAL, "iplan_pdec_saliency: null args");
    if (a->n_nets < 1 || a->n_nets > IPLAN_MAX_NETS || a->S < 1 || a->N < 1 || a->P < 1 || a->P > IPLAN_PDEC_SAL_MAX_P || a->d < 1 || a->d > 16 ||
        a->K < 0 || (int64_t)a->S * a->N > 0x7fffffff - 16)
        return fail(IPLAN_EINVAL, "iplan_pdec_saliency: unsupported dims n_nets=%d S=%d N=%d P=%d d=%d K=%d (P <= %d, d <= 16)", a->n_nets, a->S, a->N,
                    a->P, a->d, a->K, IPLAN_PDEC_SAL_MAX_P);
    if (!a->x0 || !a->h0 || !a->offset || !a->params) return fail(IPLAN_EINVAL, "iplan_pdec_saliency: null tensor pointer (x0, h0, offset or params)");
    const bool per_job = a->state_grad || a->latent_grad || a->state_l1 || a->state_gxi || a->latent_l1 || a->latent_gxi;
    const bool walk = a->pred || a->active;
    if (!per_job && !walk) return fail(IPLAN_EINVAL, "iplan_pdec_saliency: no output asked for");
    int Pn = 1;
    if (per_job) {
        if (a->K < 1 || !a->jobs || !a->jobs_host) return fail(IPLAN_EINVAL, "iplan_pdec_saliency: a per-job output needs K >= 1, jobs and jobs_host");
        for (int k = 0; k < a->K; ++k) {
            const int32_t p = a->jobs_host[2 * k], c = a->jobs_host[2 * k + 1];
            if (p < 0 || p >= a->P) return fail(IPLAN_EINVAL, "iplan_pdec_saliency: jobs[%d]: horizon step %d outside [0, P=%d)", k, p, a->P);
            if (c < -1 || c >= a->d) return fail(IPLAN_EINVAL, "iplan_pdec_saliency: jobs[%d]: column %d outside [0, d=%d) (-1: the row of v)", k, c, a->d);
            if (c < 0 && !a->v) return fail(IPLAN_EINVAL, "iplan_pdec_saliency: jobs[%d] takes its cotangent from v, which is null", k);
            Pn = imax(Pn, p + 1);
        }
    }
    const int rows = a->S * a->N, tiles = (rows + 15) / 16;
    const int Kj = per_job ? a->K : 0, KT = Kj + (walk ? 1 : 0);
    const int wpb = pdec_sal_waves(Pn);
    const int64_t tasks = (int64_t)tiles * KT;
    if (tasks > 0x7fffffff - 4)
        return fail(IPLAN_EINVAL, "iplan_pdec_saliency: %d tiles x %d jobs are too many for one launch", tiles, KT);
    const size_t lds = sizeof(float) * (P_W_FLOATS + (size_t)(Kj ? wpb * Pn * P_STEP_FLOATS : 0));
#ifndef IPLAN_HOST_EMULATION
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(pdec_sal_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
#endif
    hipLaunchKernelGGL(pdec_sal_kernel, dim3((unsigned)((tasks + wpb - 1) / wpb), (unsigned)a->n_nets), dim3(64 * (unsigned)wpb), lds, (hipStream_t)stream, *a,
                       Pn, wpb, Kj, KT);
    return check_launch("iplan_pdec_saliency");
}
