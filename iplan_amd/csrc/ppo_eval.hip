// PPO inspection (include/iplan_hip.h: IplanPpoEvalArgs): the statistics of a recorded batch under the nets -- iplan_ppo_loss's
// five numbers, the two KL estimates, clip fractions, ratio extrema, explained variance, advantage and return statistics, and a
// per-step breakdown -- with no gradient.  The raw advantage is normalised here, as iplan_ppo_prepare normalises it.
//
// Reduction order.  The row axis is cut into chunks of CH = IPLAN_PPO_EVAL_CHUNK rows.  A chunk is reduced by ONE workgroup of CH
// threads, a row per thread: per quantity an fp32 xor-butterfly over each wave, then the four wave sums added in wave order in
// fp64 and stored as the chunk's partial (fp64, `workspace`).  A total is the chunk partials added in chunk order in fp64, by
// whoever needs it (every workgroup of the next phase for the few values it needs up front, the last kernel for the statistics).
// Nothing depends on which workgroup reduced a chunk or on how many there are, and there is no atomic: any n_parts and any repeat
// give the same bits.  A phase reads the partials of the phase before it across a launch boundary, never inside a launch.
//
//   ppo_eval_sums_kernel     A: sum adv (all row_stride entries), sum m, sum m ret, sum m (ret - vpred)         (m, ret: rows)
//   ppo_eval_moments_kernel  B: sum (adv - mean)^2, sum m (ret - mean)^2, sum m (res - mean)^2
//   ppo_eval_rows_kernel     C: loss terms, KLs, fractions, extrema per chunk; ratio and adv_norm per row
//   ppo_eval_final_kernel    block 0 of an agent: totals -> stats; blocks 1..: a thread per step t walks the episodes in order
#include "api_util.h"
#include "wave_tile.h"

namespace iplan {

constexpr int CH = IPLAN_PPO_EVAL_CHUNK;       // rows per chunk == threads per workgroup
constexpr int CW = CH / 64;                    // waves per workgroup
constexpr int WS = IPLAN_PPO_EVAL_WS;          // fp64 slots per (agent, chunk)
constexpr int WS_A = 0, NA = 4;                // phase 1 partials
constexpr int WS_B = 4, NB = 3;                // phase 2
constexpr int WS_C = 7, NC = 9;                // phase 3 sums ...
constexpr int WS_MAX = WS_C + NC, WS_MIN = WS_MAX + 1;     // ... and the ratio extrema
constexpr int STEP_THREADS = 64;
static_assert(CH % 64 == 0 && WS_MIN < WS && NC <= 16, "workspace layout");

__device__ __forceinline__ float wave_min(float v) {
    for (int m = 1; m < 64; m <<= 1) v = fminf(v, __shfl_xor(v, m));
    return v;
}

__device__ __forceinline__ float eval_huber(float e, float d) {      // util.py:33-36 (one-sided), as iplan_ppo_loss
    const float ae = fabsf(e);
    return (ae <= d ? e * e * 0.5f : 0.f) + (e > d ? d * (ae - d * 0.5f) : 0.f);
}

__host__ __device__ __forceinline__ int eval_chunks(const IplanPpoEvalArgs& a) { return (int)((a.row_stride + CH - 1) / CH); }

// The chunk's partial of N quantities: wave butterflies, then the waves in order.  Ends behind a barrier (s_wave is free again).
template <int N>
__device__ __forceinline__ void chunk_store(const float (&v)[N], float* s_wave, double* dst) {
    for (int q = 0; q < N; ++q) {
        const float r = wave_sum(v[q]);
        if (lane_id() == 0) s_wave[wave_id() * 16 + q] = r;
    }
    __syncthreads();
    if ((int)threadIdx.x < N) {
        double t = 0.0;
        for (int w = 0; w < CW; ++w) t += (double)s_wave[w * 16 + (int)threadIdx.x];
        dst[threadIdx.x] = t;
    }
    __syncthreads();
}

// Totals of partial slots first .. first + n - 1 of an agent, chunk order, one thread per slot -> s_tot[0 .. n - 1].
__device__ __forceinline__ void chunk_totals(const double* __restrict__ ws_net, int n_chunks, int first, int n, double* s_tot) {
    if ((int)threadIdx.x < n) {
        double t = 0.0;
        for (int c = 0; c < n_chunks; ++c) t += ws_net[(int64_t)c * WS + first + (int)threadIdx.x];
        s_tot[threadIdx.x] = t;
    }
    __syncthreads();
}

__global__ __launch_bounds__(CH) void ppo_eval_sums_kernel(IplanPpoEvalArgs a) {
    __shared__ float s_wave[CW * 16];
    const int net = (int)blockIdx.y, n_chunks = eval_chunks(a);
    const int64_t o = (int64_t)net * a.row_stride;
    double* ws = (double*)a.workspace + (int64_t)net * n_chunks * WS;
    for (int c = (int)blockIdx.x; c < n_chunks; c += (int)gridDim.x) {
        const int64_t i = (int64_t)c * CH + (int)threadIdx.x;
        float v[NA] = {0.f, 0.f, 0.f, 0.f};
        if (i < a.row_stride) v[0] = a.adv[o + i];
        if (i < a.rows) {
            const float m = a.mask[o + i], rt = a.returns[o + i];
            v[1] = m;
            v[2] = m * rt;
            v[3] = m * (rt - a.value_preds[o + i]);
        }
        chunk_store<NA>(v, s_wave, ws + (int64_t)c * WS + WS_A);
    }
}

__global__ __launch_bounds__(CH) void ppo_eval_moments_kernel(IplanPpoEvalArgs a) {
    __shared__ float s_wave[CW * 16];
    __shared__ double s_tot[NA];
    const int net = (int)blockIdx.y, n_chunks = eval_chunks(a);
    const int64_t o = (int64_t)net * a.row_stride;
    double* ws = (double*)a.workspace + (int64_t)net * n_chunks * WS;
    chunk_totals(ws, n_chunks, WS_A, NA, s_tot);
    const float mean_adv = (float)(s_tot[0] / (double)a.row_stride);
    const float mean_ret = (float)(s_tot[2] / s_tot[1]), mean_res = (float)(s_tot[3] / s_tot[1]);
    for (int c = (int)blockIdx.x; c < n_chunks; c += (int)gridDim.x) {
        const int64_t i = (int64_t)c * CH + (int)threadIdx.x;
        float v[NB] = {0.f, 0.f, 0.f};
        if (i < a.row_stride) { const float d = a.adv[o + i] - mean_adv; v[0] = d * d; }
        if (i < a.rows) {
            const float m = a.mask[o + i], rt = a.returns[o + i];
            // (a dead row adds an exact zero: its deviation is not formed, so an empty agent's NaN means stay out of the sums)
            if (m != 0.f) {
                const float d1 = rt - mean_ret, d2 = (rt - a.value_preds[o + i]) - mean_res;
                v[1] = m * d1 * d1;
                v[2] = m * d2 * d2;
            }
        }
        chunk_store<NB>(v, s_wave, ws + (int64_t)c * WS + WS_B);
    }
}

__global__ __launch_bounds__(CH) void ppo_eval_rows_kernel(IplanPpoEvalArgs a) {
    __shared__ float s_wave[CW * 16];
    __shared__ float s_ext[2 * CW];
    __shared__ double s_tot[NA + NB];
    const int net = (int)blockIdx.y, n_chunks = eval_chunks(a);
    const int64_t o = (int64_t)net * a.row_stride, on = (int64_t)net * a.rows;
    double* ws = (double*)a.workspace + (int64_t)net * n_chunks * WS;
    chunk_totals(ws, n_chunks, WS_A, NA + NB, s_tot);         // (slots A and B are adjacent)
    const float mean = (float)(s_tot[0] / (double)a.row_stride);
    const float var = (float)(s_tot[WS_B] / (double)(a.row_stride - 1));            // th.std_mean: unbiased
    const float inv = 1.0f / (sqrtf(var) + 1e-5f);
    const bool mse = a.flags & IPLAN_PPO_MSE, no_vclip = a.flags & IPLAN_PPO_NO_VCLIP;
    const bool v_mean = a.flags & IPLAN_PPO_VALUE_MEAN, p_mean = a.flags & IPLAN_PPO_POLICY_MEAN;
    const float lo = 1.0f - a.clip, hi = 1.0f + a.clip;
    for (int c = (int)blockIdx.x; c < n_chunks; c += (int)gridDim.x) {
        const int64_t i = (int64_t)c * CH + (int)threadIdx.x;
        float v[NC] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        float rmax = -INFINITY, rmin = INFINITY;
        float ad = 0.f;
        if (i < a.row_stride) {
            ad = (a.adv[o + i] - mean) * inv;
            if (a.adv_norm) a.adv_norm[o + i] = ad;
        }
        if (i < a.rows) {
            const float m = a.mask[o + i];
            const float d = a.logp[on + i] - a.old_logp[o + i];
            const float ratio = expf(d);
            if (a.ratio) a.ratio[on + i] = ratio;
            const float rc = fminf(fmaxf(ratio, lo), hi);
            v[0] = -fminf(ratio * ad, rc * ad) * (p_mean ? 1.0f : m);
            const float val = a.values[on + i], vp = a.value_preds[o + i], rt = a.returns[o + i];
            const float dv = val - vp;
            const float vc = vp + fminf(fmaxf(dv, -a.clip), a.clip);
            const float e1 = rt - val, e2 = rt - vc;
            const float h1 = mse ? 0.5f * e1 * e1 : eval_huber(e1, a.huber_delta), h2 = mse ? 0.5f * e2 * e2 : eval_huber(e2, a.huber_delta);
            v[1] = (no_vclip ? h1 : fmaxf(h1, h2)) * (v_mean ? 1.0f : m);
            v[2] = ratio;
            v[3] = a.entropy[on + i];
            v[4] = -m * d;
            v[5] = m * ((ratio - 1.0f) - d);
            v[6] = fabsf(ratio - 1.0f) > a.clip ? m : 0.f;
            v[7] = fabsf(dv) > a.clip ? m : 0.f;
            v[8] = m * fabsf(e1);
            if (m != 0.f) { rmax = ratio; rmin = ratio; }
        }
        rmax = wave_max(rmax);
        rmin = wave_min(rmin);
        if (lane_id() == 0) { s_ext[wave_id()] = rmax; s_ext[CW + wave_id()] = rmin; }
        double* dst = ws + (int64_t)c * WS;
        chunk_store<NC>(v, s_wave, dst + WS_C);               // (its first barrier publishes s_ext, its last one frees it)
        if (threadIdx.x == 0) {
            float mx = s_ext[0], mn = s_ext[CW];
            for (int w = 1; w < CW; ++w) { mx = fmaxf(mx, s_ext[w]); mn = fminf(mn, s_ext[CW + w]); }
            dst[WS_MAX] = (double)mx;
            dst[WS_MIN] = (double)mn;
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(STEP_THREADS) void ppo_eval_final_kernel(IplanPpoEvalArgs a) {
    __shared__ double s_tot[WS];
    const int net = (int)blockIdx.y, n_chunks = eval_chunks(a);
    const int64_t o = (int64_t)net * a.row_stride, on = (int64_t)net * a.rows;
    if (blockIdx.x == 0) {
        const double* ws = (const double*)a.workspace + (int64_t)net * n_chunks * WS;
        const int k = (int)threadIdx.x;
        if (k <= WS_MIN) {
            double t = k == WS_MAX ? -(double)INFINITY : (k == WS_MIN ? (double)INFINITY : 0.0);
            for (int c = 0; c < n_chunks; ++c) {
                const double p = ws[(int64_t)c * WS + k];
                t = k == WS_MAX ? fmax(t, p) : (k == WS_MIN ? fmin(t, p) : t + p);
            }
            s_tot[k] = t;
        }
        __syncthreads();
        if (k != 0) return;
        const double n = (double)a.rows, S = s_tot[WS_A + 1];
        const bool v_mean = a.flags & IPLAN_PPO_VALUE_MEAN, p_mean = a.flags & IPLAN_PPO_POLICY_MEAN;
        const double* C = s_tot + WS_C;
        float* st = a.stats + (int64_t)net * IPLAN_PPO_EVAL_STATS;
        st[0] = (float)(C[0] / (p_mean ? n : S));             // policy_loss
        st[1] = (float)(C[1] / (v_mean ? n : S));             // value_loss
        st[2] = (float)(C[2] / n);                            // imp_weights.mean()
        st[3] = (float)(C[3] / n);                            // dist_entropy (unmasked mean, act.py:164)
        st[4] = (float)S;
        st[5] = (float)(C[4] / S);                            // approx_kl (k1)
        st[6] = (float)(C[5] / S);                            // approx_kl_k3
        st[7] = (float)(C[6] / S);                            // clip_fraction
        st[8] = (float)s_tot[WS_MAX];
        st[9] = (float)s_tot[WS_MIN];
        st[10] = (float)(1.0 - s_tot[WS_B + 2] / s_tot[WS_B + 1]);                 // explained_variance (the two 1 / S cancel)
        st[11] = (float)(C[7] / S);                           // value_clip_fraction
        st[12] = (float)(s_tot[WS_A] / (double)a.row_stride);                      // raw advantage: mean ...
        st[13] = sqrtf((float)(s_tot[WS_B] / (double)(a.row_stride - 1)));         // ... and unbiased std, as the normaliser forms it
        st[14] = (float)(s_tot[WS_A + 2] / S);                // masked mean return
        st[15] = (float)(C[8] / S);                           // masked mean |returns - values|
        return;
    }
    // per-step statistics: thread = step t, episodes in order
    const int t = ((int)blockIdx.x - 1) * STEP_THREADS + (int)threadIdx.x;
    if (t >= a.T) return;
    const int nb = a.rows / a.T;
    double cnt = 0.0, s_adv = 0.0, s_err = 0.0, s_rat = 0.0, s_ent = 0.0, s_clip = 0.0;
    for (int b = 0; b < nb; ++b) {
        const int64_t i = (int64_t)b * a.T + t;
        const float m = a.mask[o + i];
        if (m == 0.f) continue;
        const float ratio = expf(a.logp[on + i] - a.old_logp[o + i]);
        cnt += (double)m;
        s_adv += (double)(m * a.adv[o + i]);
        s_err += (double)(m * fabsf(a.returns[o + i] - a.values[on + i]));
        s_rat += (double)(m * ratio);
        s_ent += (double)(m * a.entropy[on + i]);
        s_clip += fabsf(ratio - 1.0f) > a.clip ? (double)m : 0.0;
    }
    float* ss = a.step_stats + ((int64_t)net * a.T + t) * IPLAN_PPO_EVAL_STEP_STATS;
    const bool live = cnt > 0.0;
    ss[0] = (float)cnt;
    ss[1] = live ? (float)(s_adv / cnt) : 0.f;
    ss[2] = live ? (float)(s_err / cnt) : 0.f;
    ss[3] = live ? (float)(s_rat / cnt) : 0.f;
    ss[4] = live ? (float)(s_ent / cnt) : 0.f;
    ss[5] = live ? (float)(s_clip / cnt) : 0.f;
}

// the four launches of iplan_ppo_eval; the arguments were checked by the caller (api.cpp)
int ppo_eval_launch(const IplanPpoEvalArgs& a, hipStream_t stream) {
    const int n_chunks = eval_chunks(a);
    int parts = a.n_parts > 1 ? a.n_parts : 1;
    if (parts > n_chunks) parts = n_chunks;
    if (parts > 1024) parts = 1024;
    const dim3 grid((unsigned)parts, (unsigned)a.n_agents);
    hipLaunchKernelGGL(ppo_eval_sums_kernel, grid, dim3(CH), 0, stream, a);
    hipLaunchKernelGGL(ppo_eval_moments_kernel, grid, dim3(CH), 0, stream, a);
    hipLaunchKernelGGL(ppo_eval_rows_kernel, grid, dim3(CH), 0, stream, a);
    hipLaunchKernelGGL(ppo_eval_final_kernel, dim3((unsigned)(1 + (a.T + STEP_THREADS - 1) / STEP_THREADS), (unsigned)a.n_agents), dim3(STEP_THREADS), 0,
                       stream, a);
    return check_launch("iplan_ppo_eval");
}

}  // namespace iplan
