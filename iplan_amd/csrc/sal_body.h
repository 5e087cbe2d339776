// The saliency kernels (policy_saliency.hip: ac_saliency_kernel; policy_saliency_lag.hip: ac_saliency_lag_kernel): the helpers here, the
// statements of the kernel body in sal_body_impl.h, one source for both so that lag 0 of the BPTT kernel is the plain kernel's arithmetic.
// The body is included as TEXT into each kernel, not called: a body that is a function of its own is optimised once before it is inlined
// and once after, and that changes ac_saliency_kernel's register allocation (106 SGPRs with 129 spilled against 97 with none).  The layout, the five
// passes over F and the determinism rules are described in policy_saliency.hip; what the lag modes add is described beside
// IplanAcSaliencyLagArgs (include/iplan_hip.h) and in policy_saliency_lag.hip.
//   MODE 0  iplan_ac_saliency: head seed, nothing else                                       (`x` is not read)
//   MODE 1  lag 0: the same, the entity sums / input_grad at lag 0 of the [.., n_lags, ..] results, and carry = d y / d h_prev
//   MODE 2  lag k >= 1: slot (e, s) works on the inputs and the entering state of step s - k, its backward seeded at the GRU output
//           with the slot's seed (no LN3, head or softmax); slots with s < k write nothing
#pragma once
#include "api_util.h"
#include "wave_tile.h"
#include "gru_tile.h"
#include "ac_kmap.h"
#include "ac_categorical.h"

namespace iplan {

constexpr int SM = IPLAN_AC_HIDDEN;        // 64
constexpr int ST = SM / 16;                // 4 tiles
constexpr int SAL_WAVES = 4;               // row tiles per workgroup
constexpr int SAL_GROUP = 8;               // k-tiles per partial sum of fc1 (the trunk kernel's)
constexpr int SAL_LD = 20;                 // LDS row stride of a k-tile's 16 products (16-byte aligned rows)

struct SalShared {
    __attribute__((aligned(16))) float v[SAL_WAVES][2][16][SAL_LD];
};

// MLPBase activation (utils/mappo_utils/mlp.py:10) and its derivative from the activation's own value; `tanh` is uniform
__device__ __forceinline__ f32x4 sal_act4(f32x4 v, bool tanh) {
    f32x4 r;
    for (int q = 0; q < 4; ++q) r[q] = tanh ? tanh_f(v[q]) : (v[q] > 0.0f ? v[q] : 0.0f);
    return r;
}
__device__ __forceinline__ f32x4 sal_dact4(f32x4 d, f32x4 a, bool tanh) {
    f32x4 r;
    for (int q = 0; q < 4; ++q) r[q] = tanh ? d[q] * (1.0f - a[q] * a[q]) : (a[q] > 0.0f ? d[q] : 0.0f);
    return r;
}

// LayerNorm(64) backward in place: g = d / d(output) -> d / d(v); v the values that were normalised with (mu, rstd)
__device__ __forceinline__ void sal_ln_bwd(f32x4 (&g)[ST], const f32x4 (&v)[ST], float mu, float rstd, const float* __restrict__ gamma) {
    constexpr float inv = 1.0f / SM;
    f32x4 xh[ST];
    float s1 = 0.f, s2 = 0.f;
    for (int t = 0; t < ST; ++t) {
        const f32x4 gm = bfrag_a(gamma, t);
        for (int k = 0; k < 4; ++k) {
            xh[t][k] = (v[t][k] - mu) * rstd;
            g[t][k] *= gm[k];
            s1 += g[t][k];
            s2 = fmaf(g[t][k], xh[t][k], s2);
        }
    }
    const float m1 = group_sum(s1) * inv, m2 = group_sum(s2) * inv;
    for (int t = 0; t < ST; ++t)
        for (int k = 0; k < 4; ++k) g[t][k] = (g[t][k] - m1 - xh[t][k] * m2) * rstd;
}

// y = W^T x over KT input tiles, W row-major [16 KT x 64]: output tile t
template <int KT>
__device__ __forceinline__ f32x4 sal_dense_t(const float* __restrict__ W, int t, const f32x4 (&x)[KT]) {
    f32x4 acc = splat4(0.f);
    for (int T = 0; T < KT; ++T) acc = mma_block(wfrag_ta(W, SM, 16 * t, 16 * T), x[T], acc);
    return acc;
}

// The K map of ac_kmap.h (make_kmap, ktile_at: same values) held as scalars: this kernel is large enough that the compiler leaves a
// K map whose arrays are indexed by the run-time block in private memory (80 bytes of scratch per lane; selects over the array's
// elements are folded back into the indexed load), and the kernel is to have none.
struct SalMap {
    int kt00, kt01, kt02, kt03, KT;        // first k-tile of block 0..3, and the total
    int len0, len1, len2, len3;            // valid entries of each block
    int w0, w1, w2, off1, off2;            // (off0 = 0)
    int W, NW;
};
__device__ __forceinline__ SalMap sal_make_map(const IplanAcFeatures& ft) {
    SalMap k;
    k.w0 = ft.w[0]; k.w1 = ft.w[1]; k.w2 = ft.w[2];
    k.off1 = k.w0; k.off2 = k.w0 + k.w1;
    k.W = k.w0 + k.w1 + k.w2;
    k.NW = ft.N * k.W;
    k.len0 = ft.N * k.w0; k.len1 = ft.N * k.w1; k.len2 = ft.N * k.w2; k.len3 = ft.n_actions + ft.n_id;
    k.kt00 = 0;
    k.kt01 = (k.len0 + 15) / 16;
    k.kt02 = k.kt01 + (k.len1 + 15) / 16;
    k.kt03 = k.kt02 + (k.len2 + 15) / 16;
    k.KT = k.kt03 + (k.len3 + 15) / 16;
    return k;
}
__device__ __forceinline__ KTile sal_ktile_at(const SalMap& k, int T, int c4) {
    // (every field is read unconditionally first: a load under a condition is what gets folded into an indexed one)
    const int kt00 = k.kt00, kt01 = k.kt01, kt02 = k.kt02, kt03 = k.kt03, len0 = k.len0, len1 = k.len1, len2 = k.len2, len3 = k.len3;
    const int w0 = k.w0, w1 = k.w1, w2 = k.w2, off1 = k.off1, off2 = k.off2;
    KTile o;
    o.s = T >= kt03 ? 3 : (T >= kt02 ? 2 : (T >= kt01 ? 1 : 0));
    const int kt0 = o.s == 0 ? kt00 : (o.s == 1 ? kt01 : (o.s == 2 ? kt02 : kt03));
    const int len = o.s == 0 ? len0 : (o.s == 1 ? len1 : (o.s == 2 ? len2 : len3));
    o.f0 = 16 * (T - kt0) + c4;
    const int rem = len - o.f0;
    o.nv = rem >= 4 ? 4 : (rem > 0 ? rem : 0);
    if (o.s == 3) {
        for (int q = 0; q < 4; ++q) o.c[q] = k.NW + o.f0 + q;
        o.contig = true;
        return o;
    }
    const int w = o.s == 0 ? w0 : (o.s == 1 ? w1 : w2);
    const int off = o.s == 0 ? 0 : (o.s == 1 ? off1 : off2);
    o.contig = (w & 3) == 0;
    if (o.contig) {
        const int e = o.f0 / w;
        const int c0 = e * k.W + off + (o.f0 - e * w);
        for (int q = 0; q < 4; ++q) o.c[q] = c0 + q;
    } else {
        for (int q = 0; q < 4; ++q) {
            const int f = o.f0 + q, e = f / w;
            o.c[q] = e * k.W + off + (f - e * w);
        }
    }
    return o;
}
__device__ __forceinline__ KTile sal_ktile(const SalMap& k, int T) { return sal_ktile_at(k, T, 4 * (lane_id() >> 4)); }

struct SalTile {                           // one k-tile of the backward passes, this lane's 4 entries
    KTile kt;
    f32x4 x, xh, gh;                       // raw features, normalised features, gamma * (W1^T delta)
};

}  // namespace iplan
