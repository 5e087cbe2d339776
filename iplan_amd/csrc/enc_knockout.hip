// Intent knock-out through time: how far the intent latent moves, and for how many windows it remembers, when the encoder does not see
// some steps of the RAW history.  The base chain is the one behavior_eval.hip walks (encoder half only; the header of enc_saliency.hip
// states it):
//    he_{-1} = 0, lat_{-1} = 0;  window j:  h = he_{j-1};  t < L:  s = j-L+1+t, x~ = x_s (0 where s < 0), u = ReLU(W_lin x~ + b), h = GRU32(u, h)
//    he_j = h,  lat_j = (1 - c) lat_{j-1} + c softmax(W_out he_j + b_out)
// Job q (start s = starts[q]) replaces the selected columns of steps s .. s+D-1 of every chain by a baseline -- a fixed row, or "hold":
// the chain's own row of step s-1 (zeros when s = 0) -- restarts the chain from the base chain's he_{s-1}, lat_{s-1} and walks the H
// windows s .. s+H-1.  Windows s .. s+D+L-2 read a replaced row; later ones differ only through the carried he and the averaged latent.
// Two kernels:
//   1. enc_ko_base_kernel: one wave per 16-chain tile walks windows 0 .. Jn-1 (Jn = min(J, max(starts) + H)), writes lat_j and its
//      argmax, and records every he_j in the caller's workspace (32 floats per chain-window) -- the jobs' start states and what
//      state_shift is formed against.
//   2. enc_ko_walk_kernel: one wave per (tile, job).  The history is read in place; a row of a knocked step is patched as it is consumed.
//      After each window: lat_ko, its argmax, and the two sums of squares against the base record.
// The encoder's weights are staged alone (37 KB in behavior_eval.hip's layout: four workgroups per CU where that file's two nets allow
// one), and the per-step arithmetic is beh_eval_kernel's encoder half restated -- dense_tile<1> on the input Linear, gru_step_lds<KET, KET>,
// the head, the softmax and the soft-update expression in that text -- so that a job's latent carries the bits behavior_eval.hip gives
// on an explicitly modified copy of the history.  No atomics, no sums across chains: a slot's bits depend on its chain, its job and the
// arguments only.  Slots of windows past J are not written (the caller zero-fills them).
#include "api_util.h"
#include "gru_tile.h"

namespace iplan {

constexpr int KE = 32, KET = 2, KELD = KE + 8;     // encoder_rnn_dim; LDS leading dims: ld % 16 == 8 -> conflict-free fragment reads
constexpr int KLLD = 24;                           // leading dim of the input Linear (<= 16 real columns)
constexpr int K_EWIH = 0;
constexpr int K_EWHH = K_EWIH + 3 * KE * KELD;
constexpr int K_EOUT = K_EWHH + 3 * KE * KELD;
constexpr int K_ELIN = K_EOUT + 16 * KELD;
constexpr int K_EB = K_ELIN + KE * KLLD;           // encoder biases: linear 0 (32) | b_ih 32 (96) | b_hh 128 (96) | out 224 (16)
constexpr int K_LDS_FLOATS = K_EB + KE + 6 * KE + 16;
static_assert(4 * K_LDS_FLOATS * sizeof(float) <= 160 * 1024, "four workgroups' weights must fit one CU's LDS");
static_assert(K_EB % 4 == 0 && K_ELIN % 4 == 0 && K_EOUT % 4 == 0, "16-byte aligned fragments");

__device__ __forceinline__ void enc_ko_stage(float* lds, const float* __restrict__ PE, const int64_t* off, int d, int Z) {
    stage_matrix(lds + K_EWIH, KELD, 3 * KE, PE + off[IPLAN_ENC_WIH], 3 * KE, KE);
    stage_matrix(lds + K_EWHH, KELD, 3 * KE, PE + off[IPLAN_ENC_WHH], 3 * KE, KE);
    stage_matrix(lds + K_EOUT, KELD, 16, PE + off[IPLAN_ENC_OUT_W], Z, KE);
    stage_matrix(lds + K_ELIN, KLLD, KE, PE + off[IPLAN_ENC_LIN_W], KE, d);
    stage_vector(lds + K_EB, KE, PE + off[IPLAN_ENC_LIN_B], KE);
    stage_vector(lds + K_EB + 32, 3 * KE, PE + off[IPLAN_ENC_BIH], 3 * KE);
    stage_vector(lds + K_EB + 128, 3 * KE, PE + off[IPLAN_ENC_BHH], 3 * KE);
    stage_vector(lds + K_EB + 224, 16, PE + off[IPLAN_ENC_OUT_B], Z);
}

// entries 4g .. 4g+3 of a d-wide row of any alignment: four dword loads from addresses clamped to the row, NOT masked (the consumer
// masks them: the loads of the next step stay in flight under this step's arithmetic) -- beh_eval_row of behavior_eval.hip
__device__ __forceinline__ f32x4 enc_ko_row(const float* __restrict__ row, int d, int g) {
    const IPLAN_GLOBAL_AS float* p = as_global(row);
    f32x4 v;
    for (int q = 0; q < 4; ++q) {
        const int i = 4 * g + q;
        v[q] = p[i < d ? i : d - 1];
    }
    return v;
}

// one step of the chain on the masked row x: the encoder step of beh_eval_kernel
__device__ __forceinline__ void enc_ko_step(const float* lds, const f32x4 (&x)[1], f32x4 (&he)[KET]) {
    const float* s_eb = lds + K_EB;
    f32x4 ue[KET];
    for (int T = 0; T < KET; ++T) ue[T] = relu4(dense_tile<1>(lds + K_ELIN, KLLD, 16 * T, x, bfrag_lds(s_eb, T)));
    gru_step_lds<KET, KET>(lds + K_EWIH, KELD, lds + K_EWHH, KELD, s_eb + 32, s_eb + 128, ue, he, nullptr);
}

// latent head + soft update, as beh_eval_kernel does it
__device__ __forceinline__ void enc_ko_update(const float* lds, const f32x4 (&he)[KET], f32x4& lat, int Z, int g, float coef) {
    const f32x4 lg = dense_tile<KET>(lds + K_EOUT, KELD, 0, he, bfrag_lds(lds + K_EB + 224, 0));
    float mx = -INFINITY;
    for (int q = 0; q < 4; ++q)
        if (4 * g + q < Z) mx = fmaxf(mx, lg[q]);
    mx = fmaxf(mx, __shfl_xor(mx, 16));
    mx = fmaxf(mx, __shfl_xor(mx, 32));
    f32x4 ex;
    float ss = 0.f;
    for (int q = 0; q < 4; ++q) {
        ex[q] = (4 * g + q < Z) ? expf(lg[q] - mx) : 0.f;
        ss += ex[q];
    }
    ss = group_sum(ss);
    for (int q = 0; q < 4; ++q) lat[q] = (1.0f - coef) * lat[q] + (ex[q] / ss) * coef;
}

// argmax over the Z components, lowest index on ties: within the lane, then across the chain's four lane groups (enc_sal_fwd_kernel's)
__device__ __forceinline__ int enc_ko_argmax(f32x4 lat, int Z, int g) {
    float bv = -INFINITY;
    int bi = 16;
    for (int q = 0; q < 4; ++q)
        if (4 * g + q < Z && lat[q] > bv) { bv = lat[q]; bi = 4 * g + q; }
    for (int m = 16; m <= 32; m <<= 1) {
        const float ov = __shfl_xor(bv, m);
        const int oi = __shfl_xor(bi, m);
        if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
    }
    return bi;
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

// the chains of a wave: tile -> (row, validity, history row pointer, global row index)
struct EncKoChain {
    bool valid;
    const float* hrow;
    int64_t gr;
};
__device__ __forceinline__ EncKoChain enc_ko_chain(const IplanEncKnockoutArgs& a, int net, int tile, int n) {
    const int rows = a.E * a.N;
    const int row = tile * 16 + n;
    EncKoChain c;
    c.valid = row < rows;
    const int rc = c.valid ? row : 0;                     // padding lanes of a ragged last tile walk row 0 and write nothing
    const int e = rc / a.N, ent = rc - e * a.N;
    c.hrow = a.hist + (int64_t)net * a.h_s_net + (int64_t)e * a.h_s_e + (int64_t)ent * a.d;
    c.gr = (int64_t)net * rows + rc;
    return c;
}

// ---- 1: the base chain over windows 0 .. Jn-1 ------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void enc_ko_base_kernel(IplanEncKnockoutArgs a, int Jn) {
    IPLAN_DYN_LDS(lds);
    const int net = (int)blockIdx.y;
    enc_ko_stage(lds, a.enc_params + (int64_t)net * a.enc_s_net, a.enc_off, a.d, a.Z);
    __syncthreads();
    const int l = lane_id(), n = l & 15, g = l >> 4;
    const int tiles = (a.E * a.N + 15) / 16;
    const int tile = uniform_i((int)blockIdx.x * 4 + wave_id());
    if (tile >= tiles) return;
    const EncKoChain c = enc_ko_chain(a, net, tile, n);
    const int L = a.L, d = a.d, Z = a.Z;
    float* __restrict__ he_all = a.workspace;

    f32x4 he[KET], lat = splat4(0.f);
    for (int T = 0; T < KET; ++T) he[T] = splat4(0.f);
    // the row of the step AFTER the current one is requested before the current step's arithmetic; a step index below 0 (the zero
    // padding of the first windows) fetches step 0 and is masked where it is consumed
    auto fetch = [&](int st) { return enc_ko_row(c.hrow + (int64_t)(st < 0 ? 0 : st) * a.h_s_t, d, g); };
    f32x4 x_raw = fetch(1 - L);
    for (int j = 0; j < Jn; ++j) {
        for (int t = 0; t < L; ++t) {
            const bool has = j - (L - 1) + t >= 0;
            f32x4 x[1];
            for (int q = 0; q < 4; ++q) x[0][q] = keep_if(has && 4 * g + q < d, x_raw[q]);
            {
                const bool last_t = t + 1 == L, more = j + 1 < Jn;
                const int jn = last_t && more ? j + 1 : j, tn = last_t ? (more ? 0 : t) : t + 1;
                x_raw = fetch(jn - (L - 1) + tn);
            }
            enc_ko_step(lds, x, he);
        }
        for (int T = 0; T < KET; ++T) vstore_a(he_all + (c.gr * Jn + j) * KE, c.valid, T, he[T]);
        enc_ko_update(lds, he, lat, Z, g, a.coef);
        float* lrow = a.latent + (c.gr * Jn + j) * Z;
        for (int q = 0; q < 4; ++q)
            if (c.valid && 4 * g + q < Z) lrow[4 * g + q] = lat[q];
        if (a.intent_base) {
            const int bi = enc_ko_argmax(lat, Z, g);
            if (c.valid && g == 0) a.intent_base[c.gr * Jn + j] = bi;
        }
    }
}

// ---- 2: one (tile, job) per wave: H windows from j = s on the patched history ------------------------------------------------------
__global__ __launch_bounds__(256, 2) void enc_ko_walk_kernel(IplanEncKnockoutArgs a, int Jn) {
    IPLAN_DYN_LDS(lds);
    const int net = (int)blockIdx.y;
    enc_ko_stage(lds, a.enc_params + (int64_t)net * a.enc_s_net, a.enc_off, a.d, a.Z);
    __syncthreads();
    const int l = lane_id(), n = l & 15, g = l >> 4;
    const int tiles = (a.E * a.N + 15) / 16;
    const int Q = a.Q, H = a.H;
    const int task = uniform_i((int)blockIdx.x * 4 + wave_id());
    if (task >= tiles * Q) return;
    const int tile = task / Q, qi = task - tile * Q;
    const EncKoChain c = enc_ko_chain(a, net, tile, n);
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
        if (s > 0) fill = enc_ko_row(c.hrow + (int64_t)(s - 1) * a.h_s_t, d, g);
    } else if (a.baseline) {
        fill = enc_ko_row(a.baseline + (int64_t)net * d, d, g);
    }

    f32x4 he[KET], lat = splat4(0.f);
    for (int T = 0; T < KET; ++T) he[T] = s > 0 ? vload_a(he_all + (c.gr * Jn + (s - 1)) * KE, true, T) : splat4(0.f);
    if (s > 0) {
        const IPLAN_GLOBAL_AS float* lrow = as_global(a.latent + (c.gr * Jn + (s - 1)) * Z);
        for (int q = 0; q < 4; ++q) lat[q] = keep_if(4 * g + q < Z, lrow[4 * g + q < Z ? 4 * g + q : Z - 1]);
    }

    auto fetch = [&](int st) { return enc_ko_row(c.hrow + (int64_t)(st < 0 ? 0 : st) * a.h_s_t, d, g); };
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
            {
                const bool last_t = t + 1 == L, more = h + 1 < nWin;
                const int jn = last_t && more ? j + 1 : j, tn = last_t ? (more ? 0 : t) : t + 1;
                st = jn - (L - 1) + tn;
                x_raw = fetch(st);
            }
            enc_ko_step(lds, x, he);
        }
        enc_ko_update(lds, he, lat, Z, g, a.coef);

        const int64_t slot = (c.gr * Q + qi) * H + h;
        if (a.latent_ko) {
            float* lrow = a.latent_ko + slot * Z;
            for (int q = 0; q < 4; ++q)
                if (c.valid && 4 * g + q < Z) lrow[4 * g + q] = lat[q];
        }
        if (a.hidden_ko)
            for (int T = 0; T < KET; ++T) vstore_a(a.hidden_ko + slot * KE, c.valid, T, he[T]);
        if (a.intent) {
            const int bi = enc_ko_argmax(lat, Z, g);
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
            f32x4 hb[KET];
            for (int T = 0; T < KET; ++T) hb[T] = vload_a(he_all + (c.gr * Jn + j) * KE, true, T);
            const float sq = enc_ko_shift_sq<KET>(he, hb, n);
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
    for (int q = 0; q < a->Q; ++q) {
        const int32_t s = a->starts_host[q];
        if (s < 0 || s >= J) return fail(IPLAN_EINVAL, "iplan_enc_knockout: starts[%d]=%d outside [0, J=%lld)", q, s, (long long)J);
        if (q > 0 && s <= a->starts_host[q - 1]) return fail(IPLAN_EINVAL, "iplan_enc_knockout: starts must be sorted and distinct (entry %d)", q);
    }
    if (a->col_mask == 0u || (a->d < 32 && (a->col_mask >> a->d) != 0u))
        return fail(IPLAN_EINVAL, "iplan_enc_knockout: col_mask=0x%x must select at least one of the d=%d columns and none beyond", a->col_mask, a->d);
    if (a->hold != 0 && a->hold != 1) return fail(IPLAN_EINVAL, "iplan_enc_knockout: hold=%d is neither 0 nor 1", a->hold);
    if (a->hold && a->baseline) return fail(IPLAN_EINVAL, "iplan_enc_knockout: a baseline row and hold exclude each other");
    const int rows = a->E * a->N, tiles = (rows + 15) / 16;
    const int64_t Jn64 = (int64_t)a->starts_host[a->Q - 1] + a->H < J ? (int64_t)a->starts_host[a->Q - 1] + a->H : J;
    const int Jn = (int)Jn64;
    const int64_t need = (int64_t)a->n_nets * rows * Jn * KE;
    if (a->workspace_floats < need)
        return fail(IPLAN_EINVAL, "iplan_enc_knockout: workspace_floats=%lld, %lld are needed", (long long)a->workspace_floats, (long long)need);
    if ((int64_t)tiles * a->Q > 0x7fffffff - 4 || (int64_t)a->Q * a->H > 0x7fffffff)
        return fail(IPLAN_EINVAL, "iplan_enc_knockout: %d tiles x %d jobs x %d windows are too many for one launch", tiles, a->Q, a->H);
    if (!aligned16(a->workspace) || (a->hidden_ko && !aligned16(a->hidden_ko)))
        return fail(IPLAN_EALIGN, "iplan_enc_knockout: workspace and hidden_ko must be 16-byte aligned");
    const size_t lds = sizeof(float) * K_LDS_FLOATS;
    hipLaunchKernelGGL(enc_ko_base_kernel, dim3((unsigned)((tiles + 3) / 4), (unsigned)a->n_nets), dim3(256), lds, (hipStream_t)stream, *a, Jn);
    if (a->latent_ko || a->hidden_ko || a->intent || a->latent_shift_sq || a->state_shift_sq) {
        const int tasks = tiles * a->Q;
        hipLaunchKernelGGL(enc_ko_walk_kernel, dim3((unsigned)((tasks + 3) / 4), (unsigned)a->n_nets), dim3(256), lds, (hipStream_t)stream, *a, Jn);
    }
    return check_launch("iplan_enc_knockout");
}
