// Intent saliency: d <v, lat_j> / d x_{j-r}, the derivative of the intent latent with respect to the RAW history, by BPTT through the
// behaviour encoder's chain (enc_chain.h states it: Linear -> ReLU -> GRU32 -> Linear -> softmax p_j -> soft update, no decoder).
// Against beh_enc_bwd_kernel (behavior_learn.hip), which forms PARAMETER gradients from 688 recorded floats per chain-step: this one
// differentiates with respect to the INPUT and records nothing but he_j (32 floats per chain-window).  Two passes:
//   1. enc_sal_fwd_kernel: one wave per 16-chain tile walks windows 0 .. max(windows), keeps he_j in scratch and, at the target
//      windows, writes lat_j and the argmax the one-hot cotangent selects.
//   2. enc_sal_bwd_kernel: one wave per (tile, target window j) walks windows w = j, j-1, .., j-Kj.  Each is restarted from he_{w-1}
//      with its L entering states kept in the wave's LDS slab, then walked backwards with the gates recomputed from (h_{t-1}, x_t):
//          dh += W_out^T (c (1-c)^(j-w) softmax'(v))  at the window's end,   [dr dz dn] from gru_gates_bwd,
//          dh  = z dh + W_hh^T [dr | dz | r dn],      dx_s = W_lin^T (relu' . W_ih^T [dr | dz | dn])
//      A step is read by up to L windows; windows are walked downwards, so step s is complete once window w = s has been walked:
//      at most L rows are pending at a time (a ring in LDS), and a finished row is reduced to its outputs and written once.
// The chain's steps in both directions, the weights in LDS and the lane-private slab (here: the entering states and the ring) are
// chain_sal.h's, shared with pdec_saliency.hip; the number of waves per workgroup follows from L.  The head p_j, the argmax and the
// tile -> chain mapping are enc_chain.h's, shared with behavior_eval.hip and enc_knockout.hip.  No atomics, no cross-chain
// sums: the MFMA keeps chains in separate columns, so a slot's bits do not depend on its lane, tile, workgroup or on the other windows.
#include "chain_sal.h"
#include "enc_chain.h"

namespace iplan {

static_assert(chain_fits(IPLAN_ENC_SAL_MAX_L), "one wave's slab and ring must fit beside the weights");
static_assert(!chain_fits(IPLAN_ENC_SAL_MAX_L + 1), "IPLAN_ENC_SAL_MAX_L is what the LDS budget admits");
static_assert(CH == EC && CHT == ECT, "chain_sal.h's state tiles are enc_chain.h's");

// columns 4g .. 4g+3 of step `st` of a chain's history, zero past column d and for the zero padding st < 0
__device__ __forceinline__ f32x4 enc_sal_x(const float* __restrict__ hrow, int64_t s_t, int st, int d, int g) {
    return chain_row_load(hrow + (int64_t)(st < 0 ? 0 : st) * s_t, st >= 0, d, g);
}

// p = softmax(W_out h + b_out) on chain_sal.h's layout
__device__ __forceinline__ f32x4 enc_sal_softmax(const float* lds, const f32x4 (&h)[CHT], int Z, int g) {
    return enc_chain_softmax(lds + C_OUT, CHLD, lds + C_BOUT, h, Z, g);
}

// d <gv, p> / d logits = p (gv - <p, gv>).  Every product and the difference are rounded on their own (no contraction into an fma):
// with Z = 1, p = 1 and <p, gv> = gv exactly, so the result is exactly 0 -- a fused p gv - p <p, gv> is not.
__device__ __forceinline__ f32x4 enc_sal_softmax_bwd(f32x4 p, f32x4 gv) {
#pragma clang fp contract(off)
    float dot = 0.f;
    for (int q = 0; q < 4; ++q) {
        const float pg = p[q] * gv[q];
        dot = dot + pg;
    }
    dot = group_sum(dot);
    f32x4 dl;
    for (int q = 0; q < 4; ++q) {
        const float df = gv[q] - dot;
        dl[q] = p[q] * df;
    }
    return dl;
}

// ---- pass 1: he_j for j <= max(windows); latent and argmax at the target windows --------------------------------------------------
__global__ __launch_bounds__(256) void enc_sal_fwd_kernel(IplanEncSaliencyArgs a, int Jn) {
    IPLAN_DYN_LDS(lds);
    const int net = (int)blockIdx.y;
    chain_stage(lds, a.enc_params + (int64_t)net * a.enc_s_net, a.enc_off, a.d, a.Z);
    __syncthreads();
    const int l = lane_id(), n = l & 15, g = l >> 4;
    const int rows = a.E * a.N;
    const int tiles = (rows + 15) / 16;
    const int tile = uniform_i((int)blockIdx.x * 4 + wave_id());
    if (tile >= tiles) return;
    const EncChain c = enc_chain_of(a, net, tile, n);
    const bool valid = c.valid;
    const int L = a.L, d = a.d, Z = a.Z, nW = a.nW;
    const float* __restrict__ hrow = c.hrow;
    const int64_t gr = c.gr;
    float* __restrict__ he_all = a.scratch;
    int32_t* __restrict__ tix = reinterpret_cast<int32_t*>(a.scratch + (int64_t)a.n_nets * rows * Jn * CH);

    f32x4 h[CHT], lat = splat4(0.f);
    for (int T = 0; T < CHT; ++T) h[T] = splat4(0.f);
    int wi = 0;
    for (int j = 0; j < Jn; ++j) {
        for (int t = 0; t < L; ++t) {
            f32x4 u[CHT];
            chain_step(lds, enc_sal_x(hrow, a.h_s_t, j - (L - 1) + t, d, g), u, h, nullptr);
        }
        for (int T = 0; T < CHT; ++T) vstore_a(he_all + (gr * Jn + j) * CH, valid, T, h[T]);
        // (the soft update in place, on a finished p: handed to a helper, the compiler contracts the other product into the fma and
        // lat_j changes in its last bit -- profiles/r29 notes)
        const f32x4 p = enc_sal_softmax(lds, h, Z, g);
        for (int q = 0; q < 4; ++q) lat[q] = (1.0f - a.coef) * lat[q] + p[q] * a.coef;
        if (wi < nW && a.windows[wi] == j) {
            if (a.latent) {                  // (not chain_row_store: with it the loops above land elsewhere and the call takes 0.3 % longer)
                float* lrow = a.latent + (gr * nW + wi) * Z;
                for (int q = 0; q < 4; ++q)
                    if (valid && 4 * g + q < Z) lrow[4 * g + q] = lat[q];
            }
            if (!a.seed) {
                const int bi = enc_chain_argmax(lat, Z, g);
                const int pick = a.seed_index >= 0 ? a.seed_index : bi;
                if (valid && g == 0) {
                    tix[gr * nW + wi] = pick;
                    if (a.target_index) a.target_index[gr * nW + wi] = pick;
                }
            }
            ++wi;
        }
    }
}

// ---- pass 2: BPTT of one (tile, target window) per wave -----------------------------------------------------------------------
__global__ __launch_bounds__(256) void enc_sal_bwd_kernel(IplanEncSaliencyArgs a, int Jn, int wpb) {
    IPLAN_DYN_LDS(lds);
    const int net = (int)blockIdx.y;
    chain_stage(lds, a.enc_params + (int64_t)net * a.enc_s_net, a.enc_off, a.d, a.Z);
    __syncthreads();
    const int l = lane_id(), n = l & 15, g = l >> 4;
    const int rows = a.E * a.N;
    const int tiles = (rows + 15) / 16;
    const int L = a.L, d = a.d, Z = a.Z, nW = a.nW, K = a.K, R = a.K + a.L;
    const int task = uniform_i((int)blockIdx.x * wpb + wave_id());
    if (task >= tiles * nW) return;
    const int tile = task / nW, wi = task - tile * nW;
    const EncChain c = enc_chain_of(a, net, tile, n);
    const bool valid = c.valid;
    const float* __restrict__ hrow = c.hrow;
    const int64_t gr = c.gr;
    const int64_t slot = gr * nW + wi;
    const float* __restrict__ he_all = a.scratch;
    const int32_t* __restrict__ tix = reinterpret_cast<const int32_t*>(a.scratch + (int64_t)a.n_nets * rows * Jn * CH);
    // lane-private LDS: entering states hs[t][T] and the ring of pending rows, one f32x4 per lane each
    float* slab = lds + C_W_FLOATS + wave_id() * L * C_STEP_FLOATS;
    f32x4* hs = reinterpret_cast<f32x4*>(slab) + l;                     // hs[(t * CHT + T) * 64]
    f32x4* ring = reinterpret_cast<f32x4*>(slab + L * 16 * CH) + l;     // ring[(s % L) * 64]

    const int j = a.windows[wi];
    const int Kj = imin(K, j), w0 = j - Kj;
    f32x4 v;                                                            // the cotangent, columns 4g .. 4g+3
    if (a.seed) {
        const float* srow = a.seed + slot * Z;
        for (int q = 0; q < 4; ++q) v[q] = 4 * g + q < Z ? srow[4 * g + q] : 0.f;
    } else {
        const int pick = tix[slot];
        for (int q = 0; q < 4; ++q) v[q] = 4 * g + q == pick ? 1.f : 0.f;
    }
    for (int t = 0; t < L; ++t) ring[t * 64] = splat4(0.f);
    f32x4 dh[CHT], feat = splat4(0.f);
    for (int T = 0; T < CHT; ++T) dh[T] = splat4(0.f);
    float sc = a.coef;                                                  // c (1 - c)^(j - w)

    // a finished row: G[r] of step s = j - r >= 0, reduced to the outputs
    auto emit = [&](int r, f32x4 G) {
        const f32x4 x = enc_sal_x(hrow, a.h_s_t, j - r, d, g);
        float l1 = 0.f, gx = 0.f;
        for (int q = 0; q < 4; ++q) {
            l1 += fabsf(G[q]);
            gx = fmaf(G[q], x[q], gx);
            feat[q] += fabsf(G[q]);
        }
        l1 = group_sum(l1);
        gx = group_sum(gx);
        if (a.grad) chain_row_store(a.grad + (slot * R + r) * d, valid, d, g, G);
        if (valid && g == 0) {
            if (a.step_l1) a.step_l1[slot * R + r] = l1;
            if (a.step_gxi) a.step_gxi[slot * R + r] = gx;
        }
    };

    for (int w = j; w >= w0; --w) {
        // restart window w from he_{w-1}
        f32x4 h[CHT];
        for (int T = 0; T < CHT; ++T) h[T] = w > 0 ? vload_a(he_all + (gr * Jn + (w - 1)) * CH, true, T) : splat4(0.f);
        for (int t = 0; t < L; ++t) {
            for (int T = 0; T < CHT; ++T) hs[(t * CHT + T) * 64] = h[T];
            f32x4 u[CHT];
            chain_step(lds, enc_sal_x(hrow, a.h_s_t, w - (L - 1) + t, d, g), u, h, nullptr);
        }
        // the window's share of lat_j: c (1 - c)^(j - w) p_w
        {
            const f32x4 p = enc_sal_softmax(lds, h, Z, g);
            const f32x4 dl[1] = {enc_sal_softmax_bwd(p, v * sc)};
            for (int T = 0; T < CHT; ++T) dh[T] = dense_tile<1>(lds + C_OUTT, CLLD, 16 * T, dl, dh[T]);
        }
        for (int t = L - 1; t >= 0; --t) {
            const int s = w - (L - 1) + t;
            f32x4 hp[CHT], ht[CHT], u[CHT];
            for (int T = 0; T < CHT; ++T) ht[T] = hp[T] = hs[(t * CHT + T) * 64];
            GruGates keep[CHT];
            chain_step(lds, enc_sal_x(hrow, a.h_s_t, s, d, g), u, ht, keep);
            uint32_t bits;
            const f32x4 dx = chain_step_bwd(lds, keep, hp, u, dh, g, &bits);
            if (s >= 0) ring[(s % L) * 64] += dx;
            if (a.active) {
                const uint32_t b = chain_row_or(bits);
                if (valid && g == 0) a.active[(slot * (K + 1) + (j - w)) * L + t] = b;
            }
        }
        emit(j - w, ring[(w % L) * 64]);                                 // no later window reads step w
        ring[(w % L) * 64] = splat4(0.f);
        sc *= 1.0f - a.coef;
    }
    const int s_lo = imax(w0 - (L - 1), 0);
    for (int s = w0 - 1; s >= s_lo; --s) emit(j - s, ring[(s % L) * 64]);
    // rows beyond the truncation and rows of the zero padding: exactly 0
    for (int r = j - s_lo + 1; r < R; ++r) {
        if (a.grad) chain_row_store(a.grad + (slot * R + r) * d, valid, d, g, splat4(0.f));
        if (valid && g == 0) {
            if (a.step_l1) a.step_l1[slot * R + r] = 0.f;
            if (a.step_gxi) a.step_gxi[slot * R + r] = 0.f;
        }
    }
    if (a.active && valid && g == 0)
        for (int k = Kj + 1; k <= K; ++k)
            for (int t = 0; t < L; ++t) a.active[(slot * (K + 1) + k) * L + t] = 0u;
    if (a.feature_l1) chain_row_store(a.feature_l1 + slot * d, valid, d, g, feat);
    if (a.carry_l2) {
        float sq = 0.f;
        for (int T = 0; T < CHT; ++T)
            for (int q = 0; q < 4; ++q) sq = fmaf(dh[T][q], dh[T][q], sq);
        sq = group_sum(sq);
        if (valid && g == 0) a.carry_l2[slot] = w0 > 0 ? sqrtf(sq) : 0.f;      // he_{-1} = 0 is a constant, not a state
    }
}

}  // namespace iplan

extern "C" int iplan_enc_saliency(const IplanEncSaliencyArgs* a, iplan_stream_t stream) {
    using namespace iplan;
    if (!a) return fail(IPLAN_EINVAL, "iplan_enc_saliency: null args");
    const int64_t J = (int64_t)a->T - 1 - a->L;
    if (a->n_nets < 1 || a->n_nets > IPLAN_MAX_NETS || a->E < 1 || a->N < 1 || a->L < 1 || a->L > IPLAN_ENC_SAL_MAX_L || J < 1 || a->d < 1 ||
        a->d > 16 || a->Z < 1 || a->Z > 16 || a->K < 0 || a->nW < 1 || (int64_t)a->E * a->N > 0x7fffffff - 16 ||
        (int64_t)a->K + a->L > 0x7fffffff)
        return fail(IPLAN_EINVAL, "iplan_enc_saliency: unsupported dims n_nets=%d E=%d N=%d T=%d L=%d d=%d Z=%d K=%d nW=%d (L <= %d, d <= 16, Z <= 16)",
                    a->n_nets, a->E, a->N, a->T, a->L, a->d, a->Z, a->K, a->nW, IPLAN_ENC_SAL_MAX_L);
    if (!a->hist || !a->enc_params || !a->windows || !a->windows_host || !a->scratch)
        return fail(IPLAN_EINVAL, "iplan_enc_saliency: null tensor pointer (hist, enc_params, windows, windows_host or scratch)");
    if (const int rc = enc_chain_check_list("iplan_enc_saliency", "windows", a->windows_host, a->nW, J)) return rc;
    if (!a->seed && (a->seed_index < -1 || a->seed_index >= a->Z))
        return fail(IPLAN_EINVAL, "iplan_enc_saliency: seed_index=%d outside [-1, Z=%d)", a->seed_index, a->Z);
    if (a->seed && a->target_index) return fail(IPLAN_EINVAL, "iplan_enc_saliency: target_index is only defined without a seed tensor");
    const bool bwd = a->grad || a->step_l1 || a->step_gxi || a->feature_l1 || a->carry_l2 || a->active;
    if (!bwd && !a->latent && !a->target_index) return fail(IPLAN_EINVAL, "iplan_enc_saliency: no output asked for");
    const int rows = a->E * a->N, tiles = (rows + 15) / 16;
    const int Jn = a->windows_host[a->nW - 1] + 1;
    const int64_t need = (int64_t)a->n_nets * rows * Jn * CH + (int64_t)a->n_nets * rows * a->nW;
    if (a->scratch_floats < need)
        return fail(IPLAN_EINVAL, "iplan_enc_saliency: scratch_floats=%lld, %lld are needed", (long long)a->scratch_floats, (long long)need);
    if ((int64_t)tiles * a->nW > 0x7fffffff - 4 || (int64_t)a->n_nets * rows * a->nW > 0x7fffffff / 16)
        return fail(IPLAN_EINVAL, "iplan_enc_saliency: %d tiles x %d windows are too many for one launch", tiles, a->nW);
    if (!aligned16(a->scratch)) return fail(IPLAN_EALIGN, "iplan_enc_saliency: scratch must be 16-byte aligned");
    {
        const size_t lds = sizeof(float) * C_W_FLOATS;
#ifndef IPLAN_HOST_EMULATION
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(enc_sal_fwd_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
#endif
        hipLaunchKernelGGL(enc_sal_fwd_kernel, dim3((unsigned)((tiles + 3) / 4), (unsigned)a->n_nets), dim3(256), lds, (hipStream_t)stream, *a, Jn);
    }
    if (bwd) {
        const int wpb = chain_waves(a->L);
        const size_t lds = sizeof(float) * (C_W_FLOATS + (size_t)wpb * a->L * C_STEP_FLOATS);
        const int tasks = tiles * a->nW;
#ifndef IPLAN_HOST_EMULATION
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(enc_sal_bwd_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
#endif
        hipLaunchKernelGGL(enc_sal_bwd_kernel, dim3((unsigned)((tasks + wpb - 1) / wpb), (unsigned)a->n_nets), dim3(64 * (unsigned)wpb), lds,
                           (hipStream_t)stream, *a, Jn, wpb);
    }
    return check_launch("iplan_enc_saliency");
}
