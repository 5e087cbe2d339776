// Intent knock-out through time: how far the intent latent moves, and for how many windows it remembers, when the encoder does not see
// some steps of the RAW history.  The base chain is enc_chain.h's: he_j and lat_j of windows j = 0, 1, .. from he_{-1} = 0, lat_{-1} = 0.
// Job q (start s = starts[q]) replaces the selected columns of steps s .. s+D-1 of every chain by a baseline -- a fixed row, or "hold":
// the chain's own row of step s-1 (zeros when s = 0) -- restarts the chain from the base chain's he_{s-1}, lat_{s-1} and walks the H
// windows s .. s+H-1.  Windows s .. s+D+L-2 read a replaced row; later ones differ only through the carried he and the averaged latent.
// Two kernels:
//   1. enc_ko_base_kernel: one wave per 16-chain tile walks windows 0 .. Jn-1 (Jn = min(J, max(starts) + H)), writes lat_j and its
//      argmax, and records every he_j in the caller's workspace (32 floats per chain-window) -- the jobs' start states and what
//      state_shift is formed against.
//   2. enc_ko_walk_kernel: one wave per (tile, job).  The history is read in place; a row of a knocked step is patched as it is consumed.
//      After each window: lat_ko, its argmax, and the two sums of squares against the base record.
// The LDS layout, the staging, the row fetch, the step, the head with its soft update and the argmax come from that header, which
// behavior_eval.hip walks too: a job's latent carries the bits behavior_eval.hip gives on an explicitly modified copy of the history.
// Here the encoder's weights are staged alone (37 KB: four workgroups per CU where that file's two nets allow one).  No atomics,
// no sums across chains: a slot's bits depend on its chain, its job and the arguments only.  Slots of windows past J are not written
// (the caller zero-fills them).
#include "enc_chain.h"

namespace iplan {

constexpr int KO_B = EC_W_FLOATS, KO_LDS_FLOATS = KO_B + EC_B_FLOATS;     // the weights part at 0, then the bias part
static_assert(4 * KO_LDS_FLOATS * sizeof(float) <= 160 * 1024, "four workgroups' weights must fit one CU's LDS");

__device__ __forceinline__ void enc_ko_stage(float* lds, const IplanEncKnockoutArgs& a, int net) {
    const float* __restrict__ PE = a.enc_params + (int64_t)net * a.enc_s_net;
    enc_chain_stage_w(lds, PE, a.enc_off, a.d, a.Z);
    enc_chain_stage_b(lds + KO_B, PE, a.enc_off, a.Z);
}

// sum_c (x[c] - base[c])^2 over the 16 * TT columns of a chain, c ascending, formed by every lane of the chain on its own from the four
// lane groups' registers.  Every difference, product and sum is rounded on its own (knock_shift.h is the pattern: contraction is off
// for the whole function), so the plain fp32 host loop gives the same bits; columns past the real width are 0 on both sides and add +0.
template <int TT>
__device__ __forceinline__ float enc_ko_shift_sq(const f32x4 (&x)[TT], const f32x4 (&base)[TT], int n) {
#pragma clang fp contract(off)
    float s = 0.f;
    for (int T = 0; T < TT; ++T)
        for (int gg = 0; gg < 4; ++gg)
            for (int q = 0; q < 4; ++q) {
                const float xv = __shfl(x[T][q], n + 16 * gg), bv = __shfl(base[T][q], n + 16 * gg);
                const float df = xv - bv;
                const float p = df * df;
                s = s + p;
            }
    return s;
}

// ---- 1: the base chain over windows 0 .. Jn-1 ------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void enc_ko_base_kernel(IplanEncKnockoutArgs a, int Jn) {
    IPLAN_DYN_LDS(lds);
    const int net = (int)blockIdx.y;
    enc_ko_stage(lds, a, net);
    __syncthreads();
    const int l = lane_id(), n = l & 15, g = l >> 4;
    const int tiles = (a.E * a.N + 15) / 16;
    const int tile = uniform_i((int)blockIdx.x * 4 + wave_id());
    if (tile >= tiles) return;
    const EncChain c = enc_chain_of(a, net, tile, n);
    const int L = a.L, d = a.d, Z = a.Z;
    float* __restrict__ he_all = a.workspace;

    f32x4 he[ECT], lat = splat4(0.f);
    for (int T = 0; T < ECT; ++T) he[T] = splat4(0.f);
    // the row of the step AFTER the current one is requested before the current step's arithmetic; a step index below 0 (the zero
    // padding of the first windows) fetches step 0 and is masked where it is consumed
    auto fetch = [&](int st) { return enc_chain_row(c.hrow + (int64_t)(st < 0 ? 0 : st) * a.h_s_t, d, g); };
    f32x4 x_raw = fetch(1 - L);
    for (int j = 0; j < Jn; ++j) {
        for (int t = 0; t < L; ++t) {
            const bool has = j - (L - 1) + t >= 0;
            f32x4 x[1];
            for (int q = 0; q < 4; ++q) x[0][q] = keep_if(has && 4 * g + q < d, x_raw[q]);
            {   // enc_chain_next(j, t, L, j, Jn), in place: through the helper this loop selects j + 1 by a v_cndmask / v_readfirstlane
                // pair where it has one s_cselect, and the call took 0.4 % longer (profiles/r29 notes)
                const bool last_t = t + 1 == L, more = j + 1 < Jn;
                const int jn = last_t && more ? j + 1 : j, tn = last_t ? (more ? 0 : t) : t + 1;
                x_raw = fetch(jn - (L - 1) + tn);
            }
            enc_chain_step(lds, lds + KO_B, x, he);
        }
        for (int T = 0; T < ECT; ++T) vstore_a(he_all + (c.gr * Jn + j) * EC, c.valid, T, he[T]);
        enc_chain_latent(lds, lds + KO_B, he, lat, Z, g, a.coef);
        float* lrow = a.latent + (c.gr * Jn + j) * Z;
        for (int q = 0; q < 4; ++q)
            if (c.valid && 4 * g + q < Z) lrow[4 * g + q] = lat[q];
        if (a.intent_base) {
            const int bi = enc_chain_argmax(lat, Z, g);
            if (c.valid && g == 0) a.intent_base[c.gr * Jn + j] = bi;
        }
    }
}

// ---- 2: one (tile, job) per wave: H windows from j = s on the patched history ------------------------------------------------------
__global__ __launch_bounds__(256, 2) void enc_ko_walk_kernel(IplanEncKnockoutArgs a, int Jn) {
    IPLAN_DYN_LDS(lds);
    const int net = (int)blockIdx.y;
    enc_ko_stage(lds, a, net);
    __syncthreads();
    const int l = lane_id(), n = l & 15, g = l >> 4;
    const int tiles = (a.E * a.N + 15) / 16;
    const int Q = a.Q, H = a.H;
    const int task = uniform_i((int)blockIdx.x * 4 + wave_id());
    if (task >= tiles * Q) return;
    const int tile = task / Q, qi = task - tile * Q;
    const EncChain c = enc_chain_of(a, net, tile, n);
    const int L = a.L, d = a.d, Z = a.Z, J = a.T - 1 - L;
    const int s = uniform_i(a.starts[qi]);
    const int s_end = s + imin(a.D, J - s);               // steps [s, s_end) are replaced; later ones no window reads
    const int nWin = imin(H, J - s);                      // windows s .. s+nWin-1 exist (s + nWin <= Jn)
    const float* __restrict__ he_all = a.workspace;

    // what replaces the selected columns: the chain's own row of step s-1 ("hold"; zeros when s = 0), or the net's fixed row (zeros
    // when there is none).  Unselected columns keep the row's own values.
    f32x4 fill = splat4(0.f);
    bool sel[4];
    for (int q = 0; q < 4; ++q) sel[q] = 4 * g + q < d && ((a.col_mask >> (4 * g + q)) & 1u) != 0u;
    if (a.hold) {
        if (s > 0) fill = enc_chain_row(c.hrow + (int64_t)(s - 1) * a.h_s_t, d, g);
    } else if (a.baseline) {
        fill = enc_chain_row(a.baseline + (int64_t)net * d, d, g);
    }

    f32x4 he[ECT], lat = splat4(0.f);
    for (int T = 0; T < ECT; ++T) he[T] = s > 0 ? vload_a(he_all + (c.gr * Jn + (s - 1)) * EC, true, T) : splat4(0.f);
    if (s > 0) {
        const IPLAN_GLOBAL_AS float* lrow = as_global(a.latent + (c.gr * Jn + (s - 1)) * Z);
        for (int q = 0; q < 4; ++q) lat[q] = keep_if(4 * g + q < Z, lrow[4 * g + q < Z ? 4 * g + q : Z - 1]);
    }

    auto fetch = [&](int st) { return enc_chain_row(c.hrow + (int64_t)(st < 0 ? 0 : st) * a.h_s_t, d, g); };
    int st = s - (L - 1);
    f32x4 x_raw = fetch(st);
    for (int h = 0; h < nWin; ++h) {
        const int j = s + h;
        for (int t = 0; t < L; ++t) {
            const bool has = st >= 0, knocked = st >= s && st < s_end;
            f32x4 x[1];
            for (int q = 0; q < 4; ++q) {
                const float own = keep_if(has && 4 * g + q < d, x_raw[q]);
                x[0][q] = knocked && sel[q] ? fill[q] : own;
            }
            const EncNext nx = enc_chain_next(j, t, L, h, nWin);
            st = nx.j - (L - 1) + nx.t;
            x_raw = fetch(st);
            enc_chain_step(lds, lds + KO_B, x, he);
        }
        enc_chain_latent(lds, lds + KO_B, he, lat, Z, g, a.coef);

        const int64_t slot = (c.gr * Q + qi) * H + h;
        if (a.latent_ko) {
            float* lrow = a.latent_ko + slot * Z;
            for (int q = 0; q < 4; ++q)
                if (c.valid && 4 * g + q < Z) lrow[4 * g + q] = lat[q];
        }
        if (a.hidden_ko)
            for (int T = 0; T < ECT; ++T) vstore_a(a.hidden_ko + slot * EC, c.valid, T, he[T]);
        if (a.intent) {
            const int bi = enc_chain_argmax(lat, Z, g);
            if (c.valid && g == 0) a.intent[slot] = bi;
        }
        if (a.latent_shift_sq) {
            const IPLAN_GLOBAL_AS float* brow = as_global(a.latent + (c.gr * Jn + j) * Z);
            f32x4 lb[1], lk[1] = {lat};
            for (int q = 0; q < 4; ++q) lb[0][q] = keep_if(4 * g + q < Z, brow[4 * g + q < Z ? 4 * g + q : Z - 1]);
            const float sq = enc_ko_shift_sq<1>(lk, lb, n);
            if (c.valid && g == 0) a.latent_shift_sq[slot] = sq;
        }
        if (a.state_shift_sq) {
            f32x4 hb[ECT];
            for (int T = 0; T < ECT; ++T) hb[T] = vload_a(he_all + (c.gr * Jn + j) * EC, true, T);
            const float sq = enc_ko_shift_sq<ECT>(he, hb, n);
            if (c.valid && g == 0) a.state_shift_sq[slot] = sq;
        }
    }
}

}  // namespace iplan

extern "C" int iplan_enc_knockout(const IplanEncKnockoutArgs* a, iplan_stream_t stream) {
    using namespace iplan;
    if (!a) return fail(IPLAN_EINVAL, "iplan_enc_knockout: null args");
    const int64_t J = (int64_t)a->T - 1 - a->L;
    if (a->n_nets < 1 || a->n_nets > IPLAN_MAX_NETS || a->E < 1 || a->N < 1 || a->L < 1 || a->L > IPLAN_ENC_SAL_MAX_L || J < 1 || a->d < 1 ||
        a->d > 16 || a->Z < 1 || a->Z > 16 || a->Q < 1 || a->D < 1 || a->H < 1 || (int64_t)a->E * a->N > 0x7fffffff - 16)
        return fail(IPLAN_EINVAL, "iplan_enc_knockout: unsupported dims n_nets=%d E=%d N=%d T=%d L=%d d=%d Z=%d Q=%d D=%d H=%d (L <= %d, d <= 16, Z <= 16)",
                    a->n_nets, a->E, a->N, a->T, a->L, a->d, a->Z, a->Q, a->D, a->H, IPLAN_ENC_SAL_MAX_L);
    if (!a->hist || !a->enc_params || !a->starts || !a->starts_host || !a->workspace || !a->latent)
        return fail(IPLAN_EINVAL, "iplan_enc_knockout: null tensor pointer (hist, enc_params, starts, starts_host, workspace or latent)");
    if (const int rc = enc_chain_check_list("iplan_enc_knockout", "starts", a->starts_host, a->Q, J)) return rc;
    if (a->col_mask == 0u || (a->d < 32 && (a->col_mask >> a->d) != 0u))
        return fail(IPLAN_EINVAL, "iplan_enc_knockout: col_mask=0x%x must select at least one of the d=%d columns and none beyond", a->col_mask, a->d);
    if (a->hold != 0 && a->hold != 1) return fail(IPLAN_EINVAL, "iplan_enc_knockout: hold=%d is neither 0 nor 1", a->hold);
    if (a->hold && a->baseline) return fail(IPLAN_EINVAL, "iplan_enc_knockout: a baseline row and hold exclude each other");
    const int rows = a->E * a->N, tiles = (rows + 15) / 16;
    const int64_t Jn64 = (int64_t)a->starts_host[a->Q - 1] + a->H < J ? (int64_t)a->starts_host[a->Q - 1] + a->H : J;
    const int Jn = (int)Jn64;
    const int64_t need = (int64_t)a->n_nets * rows * Jn * EC;
    if (a->workspace_floats < need)
        return fail(IPLAN_EINVAL, "iplan_enc_knockout: workspace_floats=%lld, %lld are needed", (long long)a->workspace_floats, (long long)need);
    if ((int64_t)tiles * a->Q > 0x7fffffff - 4 || (int64_t)a->Q * a->H > 0x7fffffff)
        return fail(IPLAN_EINVAL, "iplan_enc_knockout: %d tiles x %d jobs x %d windows are too many for one launch", tiles, a->Q, a->H);
    if (!aligned16(a->workspace) || (a->hidden_ko && !aligned16(a->hidden_ko)))
        return fail(IPLAN_EALIGN, "iplan_enc_knockout: workspace and hidden_ko must be 16-byte aligned");
    const size_t lds = sizeof(float) * KO_LDS_FLOATS;
    hipLaunchKernelGGL(enc_ko_base_kernel, dim3((unsigned)((tiles + 3) / 4), (unsigned)a->n_nets), dim3(256), lds, (hipStream_t)stream, *a, Jn);
    if (a->latent_ko || a->hidden_ko || a->intent || a->latent_shift_sq || a->state_shift_sq) {
        const int tasks = tiles * a->Q;
        hipLaunchKernelGGL(enc_ko_walk_kernel, dim3((unsigned)((tasks + 3) / 4), (unsigned)a->n_nets), dim3(256), lds, (hipStream_t)stream, *a, Jn);
    }
    return check_launch("iplan_enc_knockout");
}
