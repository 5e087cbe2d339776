// Behaviour-model INFERENCE: the chain of the behaviour learn forward (behavior_learn.hip; Behavior_policy.learn, soft update,
// nova/stable_behavior_policy.py:161-246 with nova/behavior_net.py:17-22, 39-69) without dropout, forward only.  Per (env, entity)
// chain of an agent-net, from latent = 0 and zero hidden states, for the windows j < J = T - 1 - L:
//    curr_t = step j-L+1+t (zero where that is < 0),   next_t = step j+1+t,   t < L
//    y_t   = Linear(tanh(GRU64(ReLU(Linear([curr_t, latent_{j-1}])))))         decoder, hidden carried across the windows
//    lat_j = (1 - coef) lat_{j-1} + coef softmax(out(GRU32(ReLU(Linear(curr_t)))))   encoder, hidden carried across the windows
// One wave = 16 chains of one agent-net, encoder AND decoder in the same wave (two independent MFMA chains per step: one's
// gate math fills the other's issue gaps), the chain state in registers in the D layout (wave_tile.h), all fp32 weights of both
// nets staged ONCE per workgroup in LDS (157 KB of the CU's 160: one workgroup per CU, one wave per SIMD).  Against the
// training forward:
//   * no activation record (the training kernels stream IPLAN_BEH_SAVE_DEC + IPLAN_BEH_SAVE_ENC = 688 floats per chain-step),
//     no carry buffers, no dropout, no seed,
//   * any d + Z <= 16 (the training forward's second form needs d <= 8),
//   * optional outputs: the latent after every window, the reconstruction, and / or two sums per (net, window, step) -- the
//     masked L1 error against next_t and the clamped distance to curr_t -- from which the losses follow on the host side.
//     Without the sums neither next_t nor the mask is read.
// The sums are reduced in a fixed order (per-tile partials, then one wave per (net, window, step, sum) over the tiles): no
// floating-point atomics, two launches on the same inputs give the same bits.
// The encoder's half -- its LDS block, staging, row fetch, step, head with the soft update, the tile -> chain mapping and the look-ahead
// index -- is enc_chain.h's, which enc_knockout.hip walks too.
#include "enc_chain.h"

namespace iplan {

constexpr int VD = 64, VDT = 4, VDLD = VD + 8;     // decoder_rnn_dim; LDS leading dims: ld % 16 == 8 -> conflict-free fragment reads
constexpr int VLLD = 24;                           // leading dim of the decoder's input Linear (<= 16 real columns)
constexpr int V_DWIH = 0;
constexpr int V_DWHH = V_DWIH + 3 * VD * VDLD;
constexpr int V_DOUT = V_DWHH + 3 * VD * VDLD;
constexpr int V_DLIN = V_DOUT + 16 * VDLD;
constexpr int V_EWIH = V_DLIN + VD * VLLD;         // the encoder's weights part (enc_chain.h: W_ih first)
constexpr int V_DB = V_EWIH + EC_W_FLOATS;         // decoder biases: linear 0 (64) | b_ih 64 (192) | b_hh 256 (192) | out 448 (16)
constexpr int V_EB = V_DB + VD + 6 * VD + 16;      // the encoder's bias part
constexpr int V_LDS_FLOATS = V_EB + EC_B_FLOATS;
static_assert(V_LDS_FLOATS * sizeof(float) <= 160 * 1024, "the weights of both nets must fit one CU's LDS");
static_assert(V_DB % 4 == 0 && V_EB % 4 == 0 && V_DLIN % 4 == 0 && V_EWIH % 4 == 0, "16-byte aligned fragments");

// The latent (columns 0 .. Z-1 of a D-layout tile) moved to columns d .. d+Z-1, zero elsewhere: the decoder's input tile is
// [x (d) | latent (Z)].  Column c of the result is column c - d of the source: register (c - d) & 3 -- the same on every lane for a
// given destination register -- of lane group (c - d) >> 2 of the same chain.
__device__ __forceinline__ f32x4 beh_eval_shift(f32x4 lat, int d, int Z) {
    const int l = lane_id(), n = l & 15, g = l >> 4;
    f32x4 o;
    for (int q = 0; q < 4; ++q) {
        const int s = 4 * g + q - d;
        const int r = (q - d) & 3;
        const float v = r == 0 ? lat[0] : (r == 1 ? lat[1] : (r == 2 ? lat[2] : lat[3]));
        const float w = __shfl(v, n + 16 * (s >= 0 ? s >> 2 : 0));
        o[q] = (s >= 0 && s < Z) ? w : 0.f;
    }
    return o;
}

__device__ __forceinline__ float beh_eval_chain_sum(float v) {     // over the 16 chains of a lane group
    v += __shfl_xor(v, 1);
    v += __shfl_xor(v, 2);
    v += __shfl_xor(v, 4);
    v += __shfl_xor(v, 8);
    return v;
}

template <bool SUMS>
__global__ __launch_bounds__(256) void beh_eval_kernel(IplanBehEvalArgs a) {
    IPLAN_DYN_LDS(lds);
    const int net = (int)blockIdx.y;
    {
        const float* __restrict__ PD = a.dec_params + (int64_t)net * a.dec_s_net;
        const float* __restrict__ PE = a.enc_params + (int64_t)net * a.enc_s_net;
        stage_matrix(lds + V_DWIH, VDLD, 3 * VD, PD + a.dec_off[IPLAN_DEC_WIH], 3 * VD, VD);
        stage_matrix(lds + V_DWHH, VDLD, 3 * VD, PD + a.dec_off[IPLAN_DEC_WHH], 3 * VD, VD);
        stage_matrix(lds + V_DOUT, VDLD, 16, PD + a.dec_off[IPLAN_DEC_OUT_W], a.d, VD);
        stage_matrix(lds + V_DLIN, VLLD, VD, PD + a.dec_off[IPLAN_DEC_LIN_W], VD, a.d + a.Z);
        enc_chain_stage_w(lds + V_EWIH, PE, a.enc_off, a.d, a.Z);
        stage_vector(lds + V_DB, VD, PD + a.dec_off[IPLAN_DEC_LIN_B], VD);
        stage_vector(lds + V_DB + 64, 3 * VD, PD + a.dec_off[IPLAN_DEC_BIH], 3 * VD);
        stage_vector(lds + V_DB + 256, 3 * VD, PD + a.dec_off[IPLAN_DEC_BHH], 3 * VD);
        stage_vector(lds + V_DB + 448, 16, PD + a.dec_off[IPLAN_DEC_OUT_B], a.d);
        enc_chain_stage_b(lds + V_EB, PE, a.enc_off, a.Z);
    }
    __syncthreads();
    const float* s_dwih = lds + V_DWIH;
    const float* s_dwhh = lds + V_DWHH;
    const float* s_dout = lds + V_DOUT;
    const float* s_dlin = lds + V_DLIN;
    const float* s_ew = lds + V_EWIH;
    const float* s_db = lds + V_DB;
    const float* s_eb = lds + V_EB;

    const int l = lane_id(), n = l & 15, g = l >> 4;
    const int tiles = (a.E * a.N + 15) / 16;
    const int tile = (int)blockIdx.x * 4 + wave_id();
    if (tile >= tiles) return;
    const EncChain c = enc_chain_of(a, net, tile, n);
    const bool valid = c.valid;
    const int L = a.L, d = a.d, Z = a.Z, J = a.T - 1 - L;
    const float* __restrict__ hrow = c.hrow;
    const float* __restrict__ mrow = SUMS ? a.mask + ((int64_t)net * a.E + c.e) * a.T : nullptr;
    const int64_t gr = c.gr;

    f32x4 hd[VDT], he[ECT], lat = splat4(0.f);
    for (int t = 0; t < VDT; ++t) hd[t] = splat4(0.f);
    for (int t = 0; t < ECT; ++t) he[t] = splat4(0.f);

    // curr_t, next_t and the mask entry of the step AFTER the current one are requested before the current step's arithmetic;
    // a step index below 0 (the zero padding of the first windows) fetches step 0 and is masked where it is consumed
    auto fetch = [&](int st) { return enc_chain_row(hrow + (int64_t)(st < 0 ? 0 : st) * a.h_s_t, d, g); };
    f32x4 x_raw = fetch(1 - L), y_raw = splat4(0.f);
    float m_raw = 0.f;
    if (SUMS) {
        y_raw = fetch(1);
        m_raw = mrow[1];
    }
    for (int j = 0; j < J; ++j) {
        const f32x4 lsh = beh_eval_shift(lat, d, Z);          // latent_{j-1} at the decoder's input columns d .. d+Z-1
        for (int t = 0; t < L; ++t) {
            const bool has = j - (L - 1) + t >= 0;
            f32x4 x[1], xin[1];
            for (int q = 0; q < 4; ++q) {
                x[0][q] = keep_if(has && 4 * g + q < d, x_raw[q]);
                xin[0][q] = 4 * g + q < d ? x[0][q] : lsh[q];
            }
            const f32x4 tg = y_raw;
            const float m = m_raw;
            const EncNext nx = enc_chain_next(j, t, L, j, J);
            x_raw = fetch(nx.j - (L - 1) + nx.t);
            if (SUMS) {
                y_raw = fetch(nx.j + 1 + nx.t);
                m_raw = mrow[nx.j + 1 + nx.t];
            }
            enc_chain_step(s_ew, s_eb, x, he);
            // decoder step
            f32x4 ud[VDT];
            for (int T = 0; T < VDT; ++T) ud[T] = relu4(dense_tile<1>(s_dlin, VLLD, 16 * T, xin, bfrag_lds(s_db, T)));
            gru_step_lds<VDT, VDT>(s_dwih, VDLD, s_dwhh, VDLD, s_db + 64, s_db + 256, ud, hd, nullptr);
            f32x4 act[VDT];
            for (int T = 0; T < VDT; ++T)
                for (int q = 0; q < 4; ++q) act[T][q] = tanh_f(hd[T][q]);
            const f32x4 y = dense_tile<VDT>(s_dout, VDLD, 0, act, bfrag_lds(s_db + 448, 0));
            if (a.recon) {
                float* prow = a.recon + ((gr * J + j) * L + t) * d;
                for (int q = 0; q < 4; ++q)
                    if (valid && 4 * g + q < d) prow[4 * g + q] = y[q];
            }
            if (SUMS) {
                float l1 = 0.f, sq = 0.f;
                for (int q = 0; q < 4; ++q) {
                    const bool in = 4 * g + q < d;
                    const float dn = in ? tg[q] - y[q] : 0.f, dc = in ? x[0][q] - y[q] : 0.f;
                    l1 += fabsf(dn);
                    sq = fmaf(dc, dc, sq);
                }
                l1 = group_sum(l1);
                const float over = fmaxf(sqrtf(group_sum(sq)) - a.thres, 0.f);
                // every lane of a chain holds the chain's values; a zero mask drops the row whatever its error is
                const float s0 = beh_eval_chain_sum(valid && m != 0.f ? m * l1 : 0.f);
                const float s1 = beh_eval_chain_sum(valid ? over : 0.f);
                if (l < 2) a.part[((((int64_t)net * J + j) * L + t) * 2 + l) * tiles + tile] = l == 0 ? s0 : s1;
            }
        }
        // latent head + soft update (stable_behavior_policy.py:223-230)
        enc_chain_latent(s_ew, s_eb, he, lat, Z, g, a.coef);
        if (a.latent) {
            float* lrow = a.latent + (gr * J + j) * Z;
            for (int q = 0; q < 4; ++q)
                if (valid && 4 * g + q < Z) lrow[4 * g + q] = lat[q];
        }
    }
}

// sums[net][j][t][k] = sum over the tiles of part[net][j][t][k][tile]: lane i adds tiles i, i + 64, ... in order, then the butterfly
__global__ __launch_bounds__(64) void beh_eval_reduce_kernel(IplanBehEvalArgs a) {
    const int64_t i = (int64_t)blockIdx.x;                // (net, j, t, k)
    const int tiles = (a.E * a.N + 15) / 16;
    float v = 0.f;
    for (int k = lane_id(); k < tiles; k += 64) v += a.part[i * tiles + k];
    v = wave_sum(v);
    if (lane_id() == 0) a.sums[i] = v;
}

}  // namespace iplan

extern "C" int iplan_beh_eval(const IplanBehEvalArgs* a, iplan_stream_t stream) {
    using namespace iplan;
    if (!a) return fail(IPLAN_EINVAL, "iplan_beh_eval: null args");
    const int64_t J = (int64_t)a->T - 1 - a->L;
    if (a->n_nets < 1 || a->n_nets > IPLAN_MAX_NETS || a->E < 1 || a->N < 1 || a->L < 1 || J < 1 || a->d < 1 || a->Z < 1 ||
        a->d + a->Z > 16 || (int64_t)a->E * a->N > 0x7fffffff - 16 || (int64_t)a->n_nets * J * a->L * 2 > 0x7fffffff)
        return fail(IPLAN_EINVAL, "iplan_beh_eval: unsupported dims n_nets=%d E=%d N=%d T=%d L=%d d=%d Z=%d", a->n_nets, a->E, a->N,
                    a->T, a->L, a->d, a->Z);
    if (!a->hist || !a->enc_params || !a->dec_params) return fail(IPLAN_EINVAL, "iplan_beh_eval: null tensor pointer");
    if (!a->latent && !a->recon && !a->sums) return fail(IPLAN_EINVAL, "iplan_beh_eval: no output asked for");
    if (a->sums && (!a->mask || !a->part)) return fail(IPLAN_EINVAL, "iplan_beh_eval: sums need mask and part");
    const int tiles = (a->E * a->N + 15) / 16;
    const dim3 grid((unsigned)((tiles + 3) / 4), (unsigned)a->n_nets);
    const size_t lds = sizeof(float) * V_LDS_FLOATS;
    if (a->sums) {
#ifndef IPLAN_HOST_EMULATION
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(beh_eval_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
#endif
        hipLaunchKernelGGL(beh_eval_kernel<true>, grid, dim3(256), lds, (hipStream_t)stream, *a);
        hipLaunchKernelGGL(beh_eval_reduce_kernel, dim3((unsigned)(a->n_nets * J * a->L * 2)), dim3(64), 0, (hipStream_t)stream, *a);
    } else {
#ifndef IPLAN_HOST_EMULATION
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(beh_eval_kernel<false>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
#endif
        hipLaunchKernelGGL(beh_eval_kernel<false>, grid, dim3(256), lds, (hipStream_t)stream, *a);
    }
    return check_launch("iplan_beh_eval");
}
