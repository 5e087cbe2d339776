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
// The chain's steps in both directions, the weights in LDS and the lane-private slab (here: the entering states and inputs) are chain_sal.h's,
// shared with enc_saliency.hip.  No atomics, no sums across rows: the MFMA keeps rows in separate columns, so a slot's bits do not depend on
// its lane, tile, workgroup, on P, on the other jobs or on which outputs were asked for.
#include "chain_sal.h"

namespace iplan {

static_assert(chain_fits(IPLAN_PDEC_SAL_MAX_P), "one wave's slab must fit beside the weights");
static_assert(!chain_fits(IPLAN_PDEC_SAL_MAX_P + 1), "IPLAN_PDEC_SAL_MAX_P is what the LDS budget admits");
static_assert(IPLAN_PDEC_SAL_MAX_P >= 8, "horizons up to 8 at least");

// y = W_out tanh(h) + b_out; `act` returns tanh(h)
__device__ __forceinline__ f32x4 pdec_sal_out(const float* lds, const f32x4 (&h)[CHT], f32x4 (&act)[CHT]) {
    for (int T = 0; T < CHT; ++T)
        for (int q = 0; q < 4; ++q) act[T][q] = tanh_f(h[T][q]);
    return dense_tile<CHT>(lds + C_OUT, CHLD, 0, act, bfrag_lds(lds + C_BOUT, 0));
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
    chain_stage(lds, a.params + (int64_t)net * a.params_s_net, a.off, a.d, a.d);
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

    f32x4 x = chain_row_load(a.x0 + at, true, d, g), h[CHT];
    for (int T = 0; T < CHT; ++T) h[T] = vload(a.h0 + gr * CH, true, CH, T);

    if (k >= Kj) {
        // ---- the forward walk: the predictions (bit for bit iplan_predict's) and the ReLU branches of every step
        for (int t = 0; t < P; ++t) {
            f32x4 u[CHT], act[CHT];
            chain_step(lds, x, u, h, nullptr);
            const f32x4 y = pdec_sal_out(lds, h, act);
            if (a.pred) chain_row_store(a.pred + (gr * P + t) * d, valid, d, g, y);
            if (a.active) {
                const uint32_t b = chain_row_or(chain_relu_bits(u, g));
                if (valid && g == 0) a.active[gr * P + t] = b;
            }
            x = y;
        }
        return;
    }

    // ---- one job: walk to step p, then back
    const int p = a.jobs[2 * k], c = a.jobs[2 * k + 1];
    // lane-private LDS: the entering states hs[t][T] and inputs xs[t], one f32x4 per lane each
    float* slab = lds + C_W_FLOATS + wave_id() * Pn * C_STEP_FLOATS;
    f32x4* hs = reinterpret_cast<f32x4*>(slab) + l;                     // hs[(t * CHT + T) * 64]
    f32x4* xs = reinterpret_cast<f32x4*>(slab + Pn * 16 * CH) + l;      // xs[t * 64]
    const f32x4 x0 = x;
    f32x4 h0[CHT];
    for (int T = 0; T < CHT; ++T) h0[T] = h[T];
    for (int t = 0; t < p; ++t) {
        for (int T = 0; T < CHT; ++T) hs[(t * CHT + T) * 64] = h[T];
        xs[t * 64] = x;
        f32x4 u[CHT], act[CHT];
        chain_step(lds, x, u, h, nullptr);
        x = pdec_sal_out(lds, h, act);
    }
    for (int T = 0; T < CHT; ++T) hs[(p * CHT + T) * 64] = h[T];
    xs[p * 64] = x;

    f32x4 dy;                                                           // the cotangent on y_p, columns 4g .. 4g+3
    if (c < 0) {
        const float* vrow = a.v + (gr * P + p) * d;
        for (int q = 0; q < 4; ++q) dy[q] = 4 * g + q < d ? vrow[4 * g + q] : 0.f;
    } else {
        for (int q = 0; q < 4; ++q) dy[q] = 4 * g + q == c ? 1.f : 0.f;
    }
    f32x4 dh[CHT];
    for (int T = 0; T < CHT; ++T) dh[T] = splat4(0.f);
    for (int t = p; t >= 0; --t) {
        f32x4 hp[CHT], ht[CHT], u[CHT], act[CHT];
        for (int T = 0; T < CHT; ++T) ht[T] = hp[T] = hs[(t * CHT + T) * 64];
        GruGates keep[CHT];
        chain_step(lds, xs[t * 64], u, ht, keep);
        for (int T = 0; T < CHT; ++T)
            for (int q = 0; q < 4; ++q) act[T][q] = tanh_f(ht[T][q]);
        // y_t = W_out tanh(h_t) + b: the output layer and tanh', onto what the later steps handed back for h_t
        const f32x4 dyv[1] = {dy};
        for (int T = 0; T < CHT; ++T) {
            const f32x4 da = dense_tile<1>(lds + C_OUTT, CLLD, 16 * T, dyv, splat4(0.f));
            for (int q = 0; q < 4; ++q) dh[T][q] += da[q] * (1.0f - act[T][q] * act[T][q]);
        }
        dy = chain_step_bwd(lds, keep, hp, u, dh, g, nullptr);                          // dx_t, and x_t = y_{t-1}
    }

    const int64_t slot = gr * K + k;
    if (a.state_grad) chain_row_store(a.state_grad + slot * d, valid, d, g, dy);
    if (a.latent_grad)
        for (int T = 0; T < CHT; ++T) vstore(a.latent_grad + slot * CH, valid, CH, T, dh[T]);
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
        pdec_sal_sums<CHT>(dh, h0, CH, l1, gx);
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
    const int wpb = chain_waves(Pn);
    const int64_t tasks = (int64_t)tiles * KT;
    if (tasks > 0x7fffffff - 4)
        return fail(IPLAN_EINVAL, "iplan_pdec_saliency: %d tiles x %d jobs are too many for one launch", tiles, KT);
    const size_t lds = sizeof(float) * (C_W_FLOATS + (size_t)(Kj ? wpb * Pn * C_STEP_FLOATS : 0));
#ifndef IPLAN_HOST_EMULATION
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(pdec_sal_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
#endif
    hipLaunchKernelGGL(pdec_sal_kernel, dim3((unsigned)((tasks + wpb - 1) / wpb), (unsigned)a->n_nets), dim3(64 * (unsigned)wpb), lds, (hipStream_t)stream, *a,
                       Pn, wpb, Kj, KT);
    return check_launch("iplan_pdec_saliency");
}
