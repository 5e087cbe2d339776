// Policy saliency: d log pi(a* | x) / d x of the actors and d V / d x of the critics for E*S independent rows, the GRU state given and
// held constant (include/iplan_hip.h: IplanAcSaliencyArgs).  One row-parallel kernel, forward + input-backward:
//
//   LN(F) -> fc1 -> act -> LN -> fc2 -> act -> LN -> GRU cell (h given) -> LN -> head -> y      y = log_softmax(masked logits)[a*] | V
//   dx <- LN(F)' <- fc1^T <- act' <- LN' <- fc2^T <- act' <- LN' <- W_ih^T <- gates' <- LN' <- head^T <- dy = 1
//
// Shape: the trunk kernel of policy_trace.hip -- one wave per 16-row tile, four tiles per workgroup, grid = ceil(tiles / 4) x n_agents x
// nets, rows gathered in place through the K map (ac_kmap.h), the 64-wide layers from L2-resident weights.  The forward half is that
// kernel's arithmetic (same k-tile order, same partial sums of every 8 k-tiles) followed by the walk kernel's step with the recurrent
// product taken by this wave alone.  Everything 64 wide stays in registers in the D layout (wave_tile.h); a transposed layer is the
// same MFMA chain with the A fragment read down a column of the weight matrix (wfrag_ta).
//
// The F axis is passed over five times and nothing F wide is kept:
//   1, 2  mean, centred second moment of x                      (LayerNorm(F) statistics, as the trunk kernel takes them)
//   3     z1 = W1 LN(x) + b1                                     (fc1 on v_mfma_f32_16x16x4_f32)
//   4     u = W1^T delta, g^ = gamma u:  mean g^, mean g^ x^     (fc1^T on the same instruction: 16 MFMAs per k-tile)
//   5     u again, dx = (g^ - mean g^ - x^ mean(g^ x^)) / sigma  -> input_grad, and the per-entity sums
// fc1^T per k-tile: the tile's 16 K-order entries are the OUTPUT rows, the 64 hidden units the contraction.  A = W1^T: lane (m, g) reads
// W1[16 t + 4 g + q][column of entry m]; B = delta in the D layout; D: lane (n, g) gets u of entries 4 g .. 4 g + 3 of row n -- the very
// entries ktile() / kfeat() hand this lane, so x, gamma and u meet lane-locally.  From the fragment-major pack the same element is
// packed[((T * 4 + t) * 64 + (4 g + q) + 16 (m >> 2)) * 4 + (m & 3)]: same values (zeros past a block's end in both), same instructions.
//
// Per-entity sums (sum g x, sum |g| over one source's columns of one entity): an entity's columns straddle lanes and k-tiles (w = 5), so
// the tile's 16 products go through 2 x 16 x 16 floats of LDS per wave and ONE lane per row (g = 0) adds them in K order -- which inside
// a source block is the reference's column order -- carrying the running sum across k-tiles and storing it when the entity's last column
// has been added.  Hand-off inside the wave only (IPLAN_WAVE_SYNC), no barrier in the kernel.
//
// Determinism: a row's arithmetic is lane-local apart from the MFMAs (column n of the product depends on column n of B only), the fixed
// xor butterflies over the row's four lanes and the row's own LDS line; no atomics, no cross-row sums.  Writes: the requested outputs
// only; parameter, gradient and batch memory is read.
#include "api_util.h"
#include "wave_tile.h"
#include "gru_tile.h"
#include "ac_kmap.h"

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

__global__ __launch_bounds__(64 * SAL_WAVES) void ac_saliency_kernel(IplanAcSaliencyArgs a) {
    __shared__ __attribute__((aligned(16))) SalShared sh;
    const int net = (int)blockIdx.y, which = a.which == 2 ? (int)blockIdx.z : a.which;
    const IplanAcNet& nw = which ? a.critic : a.actor;
    const float* __restrict__ P = nw.params + (int64_t)net * nw.params_s_net;
    const IplanAcFeatures& ft = a.feat;
    const int l = lane_id(), w = uniform_i(wave_id()), n = l & 15, g = l >> 4;
    const int64_t rows = (int64_t)a.E * a.S;
    const int64_t tile = (int64_t)blockIdx.x * SAL_WAVES + w;
    if (tile * 16 >= rows) return;                                           // (whole wave; the kernel has no barrier)
    const int64_t r = tile * 16 + n;
    const bool valid = r < rows;
    const int64_t ec = valid ? r / a.S : 0, sc = valid ? r % a.S : 0;
    const int64_t pr = ec * ft.T_phys + sc;
    const int64_t orow = (int64_t)net * rows + (valid ? r : 0);
    const float* src[3];
    for (int s = 0; s < 3; ++s) src[s] = ft.w[s] > 0 ? ft.src[s] + (int64_t)net * ft.s_net[s] + pr * ft.s_row[s] : nullptr;
    int last = -1;
    if (valid && ft.n_actions > 0) {
        if (ft.last_action) last = ft.last_action[(int64_t)net * ft.la_s_net + pr * ft.la_s_row];
        else if (ft.last_action64) last = (int)ft.last_action64[(int64_t)net * ft.la64_s_net + pr * ft.la64_s_row];
    }
    const KMap km = make_kmap(ft);                                           // (kfeat reads the one-hot widths from it)
    const SalMap sm = sal_make_map(ft);
    const int F = sm.NW + ft.n_actions + ft.n_id, KT = sm.KT;
    const bool tanh = a.act_tanh != 0;

    // ---- passes 1, 2: LayerNorm(F) statistics
    float sum = 0.f;
    for (int T = 0; T < KT; ++T) {
        const f32x4 x = kfeat(km, sal_ktile(sm, T), src, valid, last, net);
        sum += (x[0] + x[1]) + (x[2] + x[3]);
    }
    const float mu = group_sum(sum) / (float)F;
    float sq = 0.f;
    for (int T = 0; T < KT; ++T) {
        const KTile kt = sal_ktile(sm, T);
        const f32x4 x = kfeat(km, kt, src, valid, last, net);
        for (int q = 0; q < 4; ++q)
            if (q < kt.nv) { const float d = x[q] - mu; sq = fmaf(d, d, sq); }
    }
    const float rstd = 1.0f / sqrtf(group_sum(sq) / (float)F + 1e-5f);

    // ---- pass 3: fc1; operands from the fragment-major pack (iplan_ac_pack_fc1) or from the arena in place
    const float* __restrict__ pkw = which ? a.packed_critic : a.packed_actor;
    if (pkw) pkw += (int64_t)net * a.packed_s_net;
    const float* __restrict__ pkg = pkw ? pkw + (int64_t)KT * 1024 : nullptr;
    const float* __restrict__ pkb = pkw ? pkg + (int64_t)KT * 16 : nullptr;
    const float* fnw = P + nw.off[IPLAN_AC_FN_W];
    const float* fnb = P + nw.off[IPLAN_AC_FN_B];
    const float* W1 = P + nw.off[IPLAN_AC_FC1_W];
    f32x4 acc[ST], part[ST];
    for (int o = 0; o < ST; ++o) { acc[o] = splat4(0.f); part[o] = splat4(0.f); }
    for (int T = 0; T < KT; ++T) {
        const KTile kt = sal_ktile(sm, T);
        const f32x4 x = kfeat(km, kt, src, valid, last, net);
        f32x4 gm, bt, wf[ST];
        if (pkw) {
            gm = *reinterpret_cast<const f32x4*>(pkg + T * 16 + 4 * g);
            bt = *reinterpret_cast<const f32x4*>(pkb + T * 16 + 4 * g);
            for (int oo = 0; oo < ST; ++oo) wf[oo] = *reinterpret_cast<const f32x4*>(pkw + ((int64_t)(T * ST + oo) * 64 + l) * 4);
        } else {
            gm = kcols(kt, fnw);
            bt = kcols(kt, fnb);
            for (int oo = 0; oo < ST; ++oo) wf[oo] = kcols(kt, W1 + (int64_t)(16 * oo + n) * F);
        }
        f32x4 xn;
        for (int q = 0; q < 4; ++q) xn[q] = (valid && q < kt.nv) ? fmaf((x[q] - mu) * rstd, gm[q], bt[q]) : 0.f;
        for (int oo = 0; oo < ST; ++oo) part[oo] = mma_block(wf[oo], xn, part[oo]);
        if ((T + 1) % SAL_GROUP == 0 || T + 1 == KT)
            for (int oo = 0; oo < ST; ++oo) { acc[oo] += part[oo]; part[oo] = splat4(0.f); }
    }

    // ---- the 64-wide layers forward; a1, a2, hn are kept as the values the three LayerNorms normalise
    f32x4 a1[ST], a2[ST], f[ST];
    float mu1, rs1, mu2, rs2, mu3, rs3;
    for (int t = 0; t < ST; ++t) f[t] = a1[t] = sal_act4(acc[t] + bfrag_a(P + nw.off[IPLAN_AC_FC1_B], t), tanh);
    layer_norm_tiles<ST>(f, P + nw.off[IPLAN_AC_LN1_W], P + nw.off[IPLAN_AC_LN1_B], &mu1, &rs1);
    for (int t = 0; t < ST; ++t)
        a2[t] = sal_act4(dense_tile_ga<ST>(P + nw.off[IPLAN_AC_FC2_W], SM, SM, 16 * t, f, bfrag_a(P + nw.off[IPLAN_AC_FC2_B], t)), tanh);
    for (int t = 0; t < ST; ++t) f[t] = a2[t];
    layer_norm_tiles<ST>(f, P + nw.off[IPLAN_AC_LN2_W], P + nw.off[IPLAN_AC_LN2_B], &mu2, &rs2);
    float* act1 = which ? a.act1_critic : a.act1_actor;
    float* act2 = which ? a.act2_critic : a.act2_actor;
    for (int t = 0; t < ST; ++t) {
        if (act1) vstore_a(act1 + orow * SM, valid, t, a1[t]);
        if (act2) vstore_a(act2 + orow * SM, valid, t, a2[t]);
    }

    // the GRU cell from the given state: gi = W_ih f + b_ih, gh = W_hh h + b_hh, the gates of wave_tile.h
    const float* hsrc = which ? a.h_critic : a.h_actor;
    const float* hrow = hsrc + (int64_t)net * a.hs_net + ec * a.hs_chain + sc * a.hs_step;
    f32x4 h[ST], gr[ST], gz[ST], gn[ST], ghn[ST], hn[ST];
    for (int t = 0; t < ST; ++t) h[t] = vload(hrow, valid, SM, t);
    for (int t = 0; t < ST; ++t) {
        f32x4 gi[3], gh[3];
        for (int k = 0; k < 3; ++k) {
            gi[k] = dense_tile_ga<ST>(P + nw.off[IPLAN_AC_WIH], SM, 3 * SM, k * SM + 16 * t, f, bfrag_a(P + nw.off[IPLAN_AC_BIH], k * ST + t));
            gh[k] = dense_tile_ga<ST>(P + nw.off[IPLAN_AC_WHH], SM, 3 * SM, k * SM + 16 * t, h, bfrag_a(P + nw.off[IPLAN_AC_BHH], k * ST + t));
        }
        const GruGates o = gru_gates(gi[0] + gh[0], gi[1] + gh[1], gi[2], gh[2], h[t]);
        gr[t] = o.r; gz[t] = o.z; gn[t] = o.n; ghn[t] = o.hn; hn[t] = o.h;
    }
    for (int t = 0; t < ST; ++t) f[t] = hn[t];
    layer_norm_tiles<ST>(f, P + nw.off[IPLAN_AC_LN3_W], P + nw.off[IPLAN_AC_LN3_B], &mu3, &rs3);
    const int n_out = nw.n_out;
    f32x4 lg = bfrag(P + nw.off[IPLAN_AC_HEAD_B], n_out, 0);
    for (int t = 0; t < ST; ++t) lg = mma_block(wfrag_a(P + nw.off[IPLAN_AC_HEAD_W], SM, n_out, 0, 16 * t), f[t], lg);

    // ---- y and d y / d logits (lane (n, g) holds outputs 4 g .. 4 g + 3 of row n)
    f32x4 dl = splat4(0.f);
    if (which == 1) {
        if (g == 0) dl[0] = 1.0f;
        if (valid && g == 0 && a.values) a.values[orow] = lg[0];
    } else {
        // masked categorical, the conventions of iplan_ac_trace (distributions.py:64-68)
        const int32_t* av = (a.avail && valid) ? a.avail + (int64_t)net * a.av_s_net + ec * a.av_s_chain + sc * a.av_s_step : nullptr;
        f32x4 x;
        bool off[4];
        float m = -INFINITY;
        for (int q = 0; q < 4; ++q) {
            const int idx = 4 * g + q;
            x[q] = lg[q];
            off[q] = idx >= n_out;
            if (idx < n_out) {
                if (av && av[idx] == 0) { x[q] = -1e10f; off[q] = true; }
                m = fmaxf(m, x[q]);
            }
        }
        m = fmaxf(m, __shfl_xor(m, 16));
        m = fmaxf(m, __shfl_xor(m, 32));
        f32x4 ex;
        float se = 0.f;
        for (int q = 0; q < 4; ++q) { ex[q] = (4 * g + q < n_out) ? expf(x[q] - m) : 0.f; se += ex[q]; }
        se = group_sum(se);
        const float lse = m + logf(se);
        f32x4 lp, pb;
        for (int q = 0; q < 4; ++q) { lp[q] = x[q] - lse; pb[q] = ex[q] / se; }
        // argmax of the probabilities, lowest index on ties
        float best = -INFINITY;
        for (int q = 0; q < 4; ++q)
            if (4 * g + q < n_out) best = fmaxf(best, pb[q]);
        best = fmaxf(best, __shfl_xor(best, 16));
        best = fmaxf(best, __shfl_xor(best, 32));
        int cand = 1 << 30;
        for (int q = 3; q >= 0; --q)
            if (4 * g + q < n_out && pb[q] == best) cand = 4 * g + q;
        int oc = __shfl_xor(cand, 16); cand = oc < cand ? oc : cand;
        oc = __shfl_xor(cand, 32); cand = oc < cand ? oc : cand;
        int64_t want = a.target_all;
        if (a.target && valid) want = a.target[(int64_t)net * a.tg_s_net + ec * a.tg_s_chain + sc * a.tg_s_step];
        const int action = (want >= 0 && want < n_out) ? (int)want : cand;
        float sel = 0.f;
        for (int q = 0; q < 4; ++q) {
            const int idx = 4 * g + q;
            if (idx == action) sel += lp[q];
            if (!off[q]) dl[q] = (idx == action ? 1.0f : 0.0f) - pb[q];
        }
        sel = group_sum(sel);
        if (valid && g == 0) {
            if (a.logp) a.logp[orow] = sel;
            if (a.target_out) a.target_out[orow] = (int64_t)action;
        }
    }

    // ---- backward through the 64-wide layers: d[] ends as delta = d y / d z1
    f32x4 d[ST];
    {
        const f32x4 dlt[1] = {dl};
        for (int t = 0; t < ST; ++t) d[t] = dense_tile_gt<1>(P + nw.off[IPLAN_AC_HEAD_W], SM, n_out, SM, 16 * t, dlt, splat4(0.f));
    }
    sal_ln_bwd(d, hn, mu3, rs3, P + nw.off[IPLAN_AC_LN3_W]);
    f32x4 dgi[3 * ST];                                                       // d y / d gi: r | z | n
    for (int t = 0; t < ST; ++t) {
        const GruGrads o = gru_gates_bwd(d[t], gr[t], gz[t], gn[t], ghn[t], h[t]);
        dgi[t] = o.dr; dgi[ST + t] = o.dz; dgi[2 * ST + t] = o.dni;
    }
    for (int t = 0; t < ST; ++t) d[t] = sal_dense_t<3 * ST>(P + nw.off[IPLAN_AC_WIH], t, dgi);
    sal_ln_bwd(d, a2, mu2, rs2, P + nw.off[IPLAN_AC_LN2_W]);
    f32x4 dz[ST];
    for (int t = 0; t < ST; ++t) dz[t] = sal_dact4(d[t], a2[t], tanh);
    for (int t = 0; t < ST; ++t) d[t] = sal_dense_t<ST>(P + nw.off[IPLAN_AC_FC2_W], t, dz);
    sal_ln_bwd(d, a1, mu1, rs1, P + nw.off[IPLAN_AC_LN1_W]);
    for (int t = 0; t < ST; ++t) d[t] = sal_dact4(d[t], a1[t], tanh);

    // ---- passes 4, 5: fc1^T and the LayerNorm(F) backward
    auto ktile_bwd = [&](int T) {
        SalTile o;
        o.kt = sal_ktile(sm, T);
        o.x = kfeat(km, o.kt, src, valid, last, net);
        // A = W1^T: this lane's output row is entry m = n of the k-tile; its column of fc1.weight, and whether the entry exists
        f32x4 wt[ST];
        if (pkw) {
            const float* p = pkw + ((int64_t)T * ST * 64 + 4 * g + 16 * (n >> 2)) * 4 + (n & 3);
            for (int t = 0; t < ST; ++t)
                for (int q = 0; q < 4; ++q) wt[t][q] = as_global(p)[(t * 64 + q) * 4];
        } else {
            const KTile km_ = sal_ktile_at(sm, T, 4 * (n >> 2));
            const int qm = n & 3;
            const bool ok = qm < km_.nv;
            const int cm = qm == 0 ? km_.c[0] : (qm == 1 ? km_.c[1] : (qm == 2 ? km_.c[2] : km_.c[3]));
            const float* p = W1 + (ok ? cm : 0) + (int64_t)(4 * g) * F;
            for (int t = 0; t < ST; ++t)
                for (int q = 0; q < 4; ++q) wt[t][q] = keep_if(ok, as_global(p)[(int64_t)(16 * t + q) * F]);
        }
        f32x4 u = splat4(0.f);
        for (int t = 0; t < ST; ++t) u = mma_block(wt[t], d[t], u);
        const f32x4 gm = pkw ? *reinterpret_cast<const f32x4*>(pkg + T * 16 + 4 * g) : kcols(o.kt, fnw);
        for (int q = 0; q < 4; ++q) {
            o.xh[q] = (o.x[q] - mu) * rstd;
            o.gh[q] = gm[q] * u[q];
        }
        return o;
    };
    float s1 = 0.f, s2 = 0.f;
    for (int T = 0; T < KT; ++T) {
        const SalTile o = ktile_bwd(T);
        for (int q = 0; q < 4; ++q)
            if (valid && q < o.kt.nv) { s1 += o.gh[q]; s2 = fmaf(o.gh[q], o.xh[q], s2); }
    }
    const float m1 = group_sum(s1) / (float)F, m2 = group_sum(s2) / (float)F;

    float* ig = which ? a.input_grad_critic : a.input_grad_actor;
    float* ent = which ? a.entity_critic : a.entity_actor;
    const int n_src = (sm.w0 > 0) + (sm.w1 > 0) + (sm.w2 > 0);
    float* igrow = ig ? ig + orow * F : nullptr;
    float* entrow = ent ? ent + orow * ft.N * n_src * 2 : nullptr;
    const int b_kt0 = sm.kt00, b_kt1 = sm.kt01, b_kt2 = sm.kt02, b_w0 = sm.w0, b_w1 = sm.w1, b_w2 = sm.w2, b_len0 = sm.len0, b_len1 = sm.len1, b_len2 = sm.len2;
    float ax = 0.f, al = 0.f;                                                // the running sums of the entity being added (lanes g = 0)
    int ej = 0, ee = 0;                                                      // columns of it added so far; the entity
    for (int T = 0; T < KT; ++T) {
        const SalTile o = ktile_bwd(T);
        f32x4 dx;
        for (int q = 0; q < 4; ++q) dx[q] = (valid && q < o.kt.nv) ? (o.gh[q] - m1 - o.xh[q] * m2) * rstd : 0.f;
        if (igrow && valid)
            for (int q = 0; q < 4; ++q)
                if (q < o.kt.nv) igrow[o.kt.c[q]] = dx[q];
        const int s = o.kt.s;                                                // (uniform: the block depends on T alone)
        if (!entrow || s == 3) continue;
        f32x4 px, pl;
        for (int q = 0; q < 4; ++q) { px[q] = dx[q] * o.x[q]; pl[q] = fabsf(dx[q]); }
        *reinterpret_cast<f32x4*>(&sh.v[w][0][n][4 * g]) = px;
        *reinterpret_cast<f32x4*>(&sh.v[w][1][n][4 * g]) = pl;
        IPLAN_WAVE_SYNC();
        if (g == 0) {
            const int t0 = T - (s == 0 ? b_kt0 : (s == 1 ? b_kt1 : b_kt2));
            const int ws = s == 0 ? b_w0 : (s == 1 ? b_w1 : b_w2);
            const int ls = s == 0 ? b_len0 : (s == 1 ? b_len1 : b_len2);
            if (t0 == 0) { ax = al = 0.f; ej = ee = 0; }
            const int cnt = imin(16, ls - 16 * t0);
            const int si = s == 0 ? 0 : (s == 1 ? (b_w0 > 0) : (b_w0 > 0) + (b_w1 > 0));
            f32x4 vx[4], vl[4];
            for (int k = 0; k < 4; ++k) {
                vx[k] = *reinterpret_cast<const f32x4*>(&sh.v[w][0][n][4 * k]);
                vl[k] = *reinterpret_cast<const f32x4*>(&sh.v[w][1][n][4 * k]);
            }
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                if (i >= cnt) continue;
                ax += vx[i >> 2][i & 3];
                al += vl[i >> 2][i & 3];
                if (++ej == ws) {
                    if (valid) {
                        float* p = entrow + ((int64_t)ee * n_src + si) * 2;
                        p[0] = ax;
                        p[1] = al;
                    }
                    ax = al = 0.f;
                    ej = 0;
                    ++ee;
                }
            }
        }
        IPLAN_WAVE_SYNC();
    }
}

int ac_saliency_launch(const IplanAcSaliencyArgs& a, hipStream_t stream) {
    const int64_t rows = (int64_t)a.E * a.S, tiles = (rows + 15) / 16;
    const unsigned nz = a.which == 2 ? 2u : 1u;
    hipLaunchKernelGGL(ac_saliency_kernel, dim3((unsigned)((tiles + SAL_WAVES - 1) / SAL_WAVES), (unsigned)a.n_agents, nz), dim3(64 * SAL_WAVES), 0, stream, a);
    return check_launch("iplan_ac_saliency");
}

}  // namespace iplan
