// The behaviour encoder's chain, forward, as the inspection kernels walk it: one wave = 16 (env, entity) chains of one agent-net, the state
// in registers in the D layout (wave_tile.h), the fp32 weights in LDS.  Per chain, from he_{-1} = 0 and lat_{-1} = 0:
//    window j:  h = he_{j-1};  t < L:  s = j-L+1+t, x~ = x_s (0 where s < 0), u = ReLU(W_lin x~ + b), h = GRU32(u, h)
//    he_j = h,  p_j = softmax(W_out he_j + b_out),  lat_j = (1 - c) lat_{j-1} + c p_j
// behavior_eval.hip (beside its decoder), enc_knockout.hip (base chain and knocked chains) and enc_saliency.hip (the forward walk in
// front of its BPTT) promise the same bits for lat_j; they get them from the one text below.  The LDS block is the caller's: a weights
// part and a bias part, each relative to a base pointer of its own, so that a kernel with more in LDS places them where it likes.
// enc_saliency.hip keeps chain_sal.h's both-orientation layout and takes from here what does not depend on a layout: the head (handed
// its matrix, leading dimension and bias), the argmax, the tile -> chain mapping and the host check of an index list.
#pragma once
#include "api_util.h"
#include "gru_tile.h"

namespace iplan {

constexpr int EC = 32, ECT = 2, ECLD = EC + 8;     // encoder_rnn_dim; LDS leading dims: ld % 16 == 8 -> conflict-free fragment reads
constexpr int ECLLD = 24;                          // leading dim of the input Linear (<= 16 real columns)
constexpr int EC_WIH = 0;                          // the weights part: W_ih | W_hh | W_out | W_lin
constexpr int EC_WHH = EC_WIH + 3 * EC * ECLD;
constexpr int EC_OUT = EC_WHH + 3 * EC * ECLD;
constexpr int EC_LIN = EC_OUT + 16 * ECLD;
constexpr int EC_W_FLOATS = EC_LIN + EC * ECLLD;
constexpr int EC_BLIN = 0, EC_BIH = 32, EC_BHH = 128, EC_BOUT = 224;     // the bias part: linear (32) | b_ih (96) | b_hh (96) | out (16)
constexpr int EC_B_FLOATS = EC_BOUT + 16;
static_assert(EC_OUT % 4 == 0 && EC_LIN % 4 == 0 && EC_W_FLOATS % 4 == 0 && EC_B_FLOATS % 4 == 0, "16-byte aligned fragments");

// the matrices of one net (`PE`: its parameters, `off`: the IPLAN_ENC_* offset table) into the weights part; all threads call it
__device__ __forceinline__ void enc_chain_stage_w(float* w, const float* __restrict__ PE, const int64_t* off, int d, int Z) {
    stage_matrix(w + EC_WIH, ECLD, 3 * EC, PE + off[IPLAN_ENC_WIH], 3 * EC, EC);
    stage_matrix(w + EC_WHH, ECLD, 3 * EC, PE + off[IPLAN_ENC_WHH], 3 * EC, EC);
    stage_matrix(w + EC_OUT, ECLD, 16, PE + off[IPLAN_ENC_OUT_W], Z, EC);
    stage_matrix(w + EC_LIN, ECLLD, EC, PE + off[IPLAN_ENC_LIN_W], EC, d);
}

// ... and its vectors into the bias part
__device__ __forceinline__ void enc_chain_stage_b(float* b, const float* __restrict__ PE, const int64_t* off, int Z) {
    stage_vector(b + EC_BLIN, EC, PE + off[IPLAN_ENC_LIN_B], EC);
    stage_vector(b + EC_BIH, 3 * EC, PE + off[IPLAN_ENC_BIH], 3 * EC);
    stage_vector(b + EC_BHH, 3 * EC, PE + off[IPLAN_ENC_BHH], 3 * EC);
    stage_vector(b + EC_BOUT, 16, PE + off[IPLAN_ENC_OUT_B], Z);
}

// entries 4g .. 4g+3 of a d-wide row of any alignment: four dword loads from addresses clamped to the row, NOT masked (the consumer
// masks them: the loads of the next step stay in flight under this step's arithmetic)
__device__ __forceinline__ f32x4 enc_chain_row(const float* __restrict__ row, int d, int g) {
    const IPLAN_GLOBAL_AS float* p = as_global(row);
    f32x4 v;
    for (int q = 0; q < 4; ++q) {
        const int i = 4 * g + q;
        v[q] = p[i < d ? i : d - 1];
    }
    return v;
}

// one step of the chain on the masked row x: u = ReLU(W_lin x + b_lin), he = GRU32(u, he)
__device__ __forceinline__ void enc_chain_step(const float* w, const float* b, const f32x4 (&x)[1], f32x4 (&he)[ECT]) {
    f32x4 ue[ECT];
    for (int T = 0; T < ECT; ++T) ue[T] = relu4(dense_tile<1>(w + EC_LIN, ECLLD, 16 * T, x, bfrag_lds(b + EC_BLIN, T)));
    gru_step_lds<ECT, ECT>(w + EC_WIH, ECLD, w + EC_WHH, ECLD, b + EC_BIH, b + EC_BHH, ue, he, nullptr);
}

// the latent head before its normalisation: ex = exp(W_out he + b_out - max) over the Z real columns, 0 elsewhere -> their sum
__device__ __forceinline__ float enc_chain_exp(const float* w_out, int ld, const float* b_out, const f32x4 (&he)[ECT], int Z, int g, f32x4& ex) {
    const f32x4 lg = dense_tile<ECT>(w_out, ld, 0, he, bfrag_lds(b_out, 0));
    float mx = -INFINITY;
    for (int q = 0; q < 4; ++q)
        if (4 * g + q < Z) mx = fmaxf(mx, lg[q]);
    mx = fmaxf(mx, __shfl_xor(mx, 16));
    mx = fmaxf(mx, __shfl_xor(mx, 32));
    float ss = 0.f;
    for (int q = 0; q < 4; ++q) {
        ex[q] = (4 * g + q < Z) ? expf(lg[q] - mx) : 0.f;
        ss += ex[q];
    }
    return group_sum(ss);
}

// p = softmax(W_out he + b_out)
__device__ __forceinline__ f32x4 enc_chain_softmax(const float* w_out, int ld, const float* b_out, const f32x4 (&he)[ECT], int Z, int g) {
    f32x4 ex;
    const float ss = enc_chain_exp(w_out, ld, b_out, he, Z, g, ex);
    for (int q = 0; q < 4; ++q) ex[q] = ex[q] / ss;
    return ex;
}

// head and soft update on this header's layout: lat_{j-1} -> lat_j = (1 - c) lat_{j-1} + p c from he_j, every component of p formed
// where it is used
__device__ __forceinline__ void enc_chain_latent(const float* w, const float* b, const f32x4 (&he)[ECT], f32x4& lat, int Z, int g, float coef) {
    f32x4 ex;
    const float ss = enc_chain_exp(w + EC_OUT, ECLD, b + EC_BOUT, he, Z, g, ex);
    for (int q = 0; q < 4; ++q) lat[q] = (1.0f - coef) * lat[q] + (ex[q] / ss) * coef;
}

// argmax over the Z components, lowest index on ties: within the lane, then across the chain's four lane groups
__device__ __forceinline__ int enc_chain_argmax(f32x4 lat, int Z, int g) {
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

// the chain of lane column n of a tile: validity, env, history row pointer, global row index (`Args`: any descriptor with E, N, d, hist
// and the h_s_* strides)
struct EncChain {
    bool valid;
    int e;
    const float* hrow;
    int64_t gr;
};
template <class Args>
__device__ __forceinline__ EncChain enc_chain_of(const Args& a, int net, int tile, int n) {
    const int rows = a.E * a.N;
    const int row = tile * 16 + n;
    EncChain c;
    c.valid = row < rows;
    const int rc = c.valid ? row : 0;                     // padding lanes of a ragged last tile walk row 0 and write nothing
    c.e = rc / a.N;
    const int ent = rc - c.e * a.N;
    c.hrow = a.hist + (int64_t)net * a.h_s_net + (int64_t)c.e * a.h_s_e + (int64_t)ent * a.d;
    c.gr = (int64_t)net * rows + rc;
    return c;
}

// (window, position) of the step after position t of window j, for the look-ahead fetch; the window is the k-th of the `kend` the
// caller walks, and the last step of the last one names itself
struct EncNext {
    int j, t;
};
__device__ __forceinline__ EncNext enc_chain_next(int j, int t, int L, int k, int kend) {
    const bool last_t = t + 1 == L, more = k + 1 < kend;
    return {last_t && more ? j + 1 : j, last_t ? (more ? 0 : t) : t + 1};
}

// host side: `v[0 .. n)` is sorted, distinct and inside [0, J); `fn`: the entry point, `what`: the list's name
inline int enc_chain_check_list(const char* fn, const char* what, const int32_t* v, int n, int64_t J) {
    for (int i = 0; i < n; ++i) {
        if (v[i] < 0 || v[i] >= J) return fail(IPLAN_EINVAL, "%s: %s[%d]=%d outside [0, J=%lld)", fn, what, i, v[i], (long long)J);
        if (i > 0 && v[i] <= v[i - 1]) return fail(IPLAN_EINVAL, "%s: %s must be sorted and distinct (entry %d)", fn, what, i);
    }
    return IPLAN_OK;
}

}  // namespace iplan
