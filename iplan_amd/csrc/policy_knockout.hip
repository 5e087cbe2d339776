// Policy knock-out: "would this agent have acted differently, and would its critic have valued the state differently, if vehicle j had
// not been there?" (include/iplan_hip.h: IplanAcKnockoutArgs).  Every row (e, s, agent) of a recorded batch runs one actor and / or
// critic step per JOB of a list, forward only, the GRU state given and held:
//
//   LN(F) -> fc1 -> act -> LN -> fc2 -> act -> LN -> GRU cell (h given) -> LN -> head -> masked softmax | V
//
// A job is an entity index, or -1 for "nothing knocked".  The job's entity loses its entries of the selected sources AS THE FEATURES
// ARE GATHERED (kfeat_ko, ac_kmap_ko.h): the batch is read in place, nothing is copied, and LayerNorm(F) sees the modified row.
//
// Shape: the forward half of policy_saliency.hip -- one wave per 16-column tile, four tiles per workgroup, grid = ceil(tiles / 4) x
// n_agents x nets, fc1 on v_mfma_f32_16x16x4_f32 in the same k-tile order with the same partial sums of every 8 k-tiles, packed or
// in-place operands, the 64-wide layers from L2-resident weights, everything 64 wide in registers in the D layout.  The 16 columns of
// a tile are VIRTUAL rows of ONE recorded row: columns 0 .. 14 are the jobs 15 jt .. 15 jt + 14, column 15 is the row's base result
// (nothing knocked), which every tile carries.  So the feature loads of a tile hit the same cache lines (the J-fold extra reads stay
// in L2), and the differences to the base are formed inside the wave: no second kernel, no workspace, ceil(J / 15) tiles per row.
//
// Per column, lanes g = 0: dvalue = V_ko - V_base, dlogp = logp_ko - logp_base and
//   kl = sum over the available actions, ascending, of p_base * (logp_base - logp_ko)
// with all 16 log-probabilities of the column and of column 15 brought to the lane by shuffles; every difference, product and sum is
// rounded on its own (knock_kl is compiled with contraction off).  A column whose gathered values equal the row's own repeats the base
// column's arithmetic bit for bit, so its kl, dlogp and dvalue are exactly 0.
//
// Determinism: a column's arithmetic is lane-local apart from the MFMAs (column n of the product depends on column n of B only), the
// fixed xor butterflies over the column's four lanes and the reads of column 15, which holds the same bits in every tile of the row.
// No atomics, no LDS, no sums across columns.  Writes: the requested outputs only; parameter and batch memory is read.
#include "sal_body.h"
#include "ac_kmap_ko.h"

namespace iplan {

__global__ __launch_bounds__(64 * SAL_WAVES) void ac_knockout_kernel(IplanAcKnockoutArgs ka) {
    const IplanAcSaliencyArgs& a = ka.base;
    const int net = (int)blockIdx.y, which = a.which == 2 ? (int)blockIdx.z : a.which;
    const IplanAcNet& nw = which ? a.critic : a.actor;
    const float* __restrict__ P = nw.params + (int64_t)net * nw.params_s_net;
    const IplanAcFeatures& ft = a.feat;
    const int l = lane_id(), w = uniform_i(wave_id()), n = l & 15, g = l >> 4;
    const int64_t rows = (int64_t)a.E * a.S;
    const int J = ka.J, JT = (J + KO_JOBS - 1) / KO_JOBS;
    const int64_t tile = (int64_t)blockIdx.x * SAL_WAVES + w;
    if (tile >= rows * JT) return;                                           // (whole wave; the kernel has no barrier)
    const int64_t r = tile / JT;                                             // the recorded row all 16 columns share
    const int jt = (int)(tile - r * JT);
    const int slot = KO_JOBS * jt + n;                                       // this column's entry of jobs[]
    const bool is_base = n == KO_JOBS;
    const bool valid = is_base || slot < J;
    const int64_t ec = r / a.S, sc = r % a.S;
    const int64_t pr = ec * ft.T_phys + sc;
    const int64_t brow = (int64_t)net * rows + r;                            // the row's base outputs
    const int64_t orow = brow * J + (valid && !is_base ? slot : 0);          // the column's outputs
    const float* const p0 = ft.w[0] > 0 ? ft.src[0] + (int64_t)net * ft.s_net[0] + pr * ft.s_row[0] : nullptr;
    const float* const p1 = ft.w[1] > 0 ? ft.src[1] + (int64_t)net * ft.s_net[1] + pr * ft.s_row[1] : nullptr;
    const float* const p2 = ft.w[2] > 0 ? ft.src[2] + (int64_t)net * ft.s_net[2] + pr * ft.s_row[2] : nullptr;
    int last = -1;
    if (ft.n_actions > 0) {
        if (ft.last_action) last = ft.last_action[(int64_t)net * ft.la_s_net + pr * ft.la_s_row];
        else if (ft.last_action64) last = (int)ft.last_action64[(int64_t)net * ft.la64_s_net + pr * ft.la64_s_row];
    }
    // what this column gathers: the base column the row itself; a job column its own vector of an overridden source, and of the others
    // the row with the job's entity replaced where the source is to be knocked
    const bool jobcol = valid && !is_base;
    const int job = jobcol ? ka.jobs[slot] : -1;
    KnockCol kc;
    auto own = [&](int s) -> const float* {                                 // (s is a literal at every call)
        return (jobcol && ka.override_src[s] && ft.w[s] > 0)
                   ? ka.override_src[s] + (int64_t)slot * ka.ov_s_job[s] + (int64_t)net * ka.ov_s_net[s] + ec * ka.ov_s_chain[s] + sc * ka.ov_s_step[s]
                   : nullptr;
    };
    auto knocked = [&](int s) { return (ka.knock[s] && ft.w[s] > 0 && !ka.override_src[s]) ? job : -1; };
    kc.ent0 = knocked(0); kc.ent1 = knocked(1); kc.ent2 = knocked(2);
    kc.bl0 = ka.baseline[0]; kc.bl1 = ka.baseline[1]; kc.bl2 = ka.baseline[2];
    kc.ov0 = own(0); kc.ov1 = own(1); kc.ov2 = own(2);
    kc.se0 = ka.ov_s_ent[0]; kc.se1 = ka.ov_s_ent[1]; kc.se2 = ka.ov_s_ent[2];
    const KMap km = make_kmap(ft);                                           // (kfeat reads the one-hot widths from it)
    const SalMap sm = sal_make_map(ft);
    const int F = sm.NW + ft.n_actions + ft.n_id, KT = sm.KT;
    const int bw0 = sm.w0, bw1 = sm.w1, bw2 = sm.w2;
    const bool tanh = a.act_tanh != 0;
    auto feat = [&](const KTile& kt) {
        const int ws = kt.s == 0 ? bw0 : (kt.s == 1 ? bw1 : bw2);
        return kfeat_ko(km, kt, p0, p1, p2, kc, ws, valid, last, net);
    };

    // ---- passes 1, 2: LayerNorm(F) statistics of the modified row
    float sum = 0.f;
    for (int T = 0; T < KT; ++T) {
        const f32x4 x = feat(sal_ktile(sm, T));
        sum += (x[0] + x[1]) + (x[2] + x[3]);
    }
    const float mu = group_sum(sum) / (float)F;
    float sq = 0.f;
    for (int T = 0; T < KT; ++T) {
        const KTile kt = sal_ktile(sm, T);
        const f32x4 x = feat(kt);
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
        const f32x4 x = feat(kt);
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

    // ---- the 64-wide layers
    f32x4 f[ST], f2[ST];
    for (int t = 0; t < ST; ++t) f[t] = sal_act4(acc[t] + bfrag_a(P + nw.off[IPLAN_AC_FC1_B], t), tanh);
    layer_norm_tiles<ST>(f, P + nw.off[IPLAN_AC_LN1_W], P + nw.off[IPLAN_AC_LN1_B], nullptr, nullptr);
    for (int t = 0; t < ST; ++t)
        f2[t] = sal_act4(dense_tile_ga<ST>(P + nw.off[IPLAN_AC_FC2_W], SM, SM, 16 * t, f, bfrag_a(P + nw.off[IPLAN_AC_FC2_B], t)), tanh);
    layer_norm_tiles<ST>(f2, P + nw.off[IPLAN_AC_LN2_W], P + nw.off[IPLAN_AC_LN2_B], nullptr, nullptr);

    // the GRU cell from the given state: gi = W_ih f + b_ih, gh = W_hh h + b_hh, the gates of wave_tile.h
    const float* hsrc = which ? a.h_critic : a.h_actor;
    const float* hrow = hsrc + (int64_t)net * a.hs_net + ec * a.hs_chain + sc * a.hs_step;
    f32x4 h[ST], hn[ST];
    for (int t = 0; t < ST; ++t) h[t] = vload(hrow, valid, SM, t);
    for (int t = 0; t < ST; ++t) {
        f32x4 gi[3], gh[3];
        for (int k = 0; k < 3; ++k) {
            gi[k] = dense_tile_ga<ST>(P + nw.off[IPLAN_AC_WIH], SM, 3 * SM, k * SM + 16 * t, f2, bfrag_a(P + nw.off[IPLAN_AC_BIH], k * ST + t));
            gh[k] = dense_tile_ga<ST>(P + nw.off[IPLAN_AC_WHH], SM, 3 * SM, k * SM + 16 * t, h, bfrag_a(P + nw.off[IPLAN_AC_BHH], k * ST + t));
        }
        hn[t] = gru_gates(gi[0] + gh[0], gi[1] + gh[1], gi[2], gh[2], h[t]).h;
    }
    layer_norm_tiles<ST>(hn, P + nw.off[IPLAN_AC_LN3_W], P + nw.off[IPLAN_AC_LN3_B], nullptr, nullptr);
    const int n_out = nw.n_out;
    f32x4 lg = bfrag(P + nw.off[IPLAN_AC_HEAD_B], n_out, 0);
    for (int t = 0; t < ST; ++t) lg = mma_block(wfrag_a(P + nw.off[IPLAN_AC_HEAD_W], SM, n_out, 0, 16 * t), hn[t], lg);

    const bool base_out = is_base && jt == 0;                                // one tile of the row writes the base outputs
    if (which == 1) {
        const float vb = __shfl(lg[0], KO_JOBS);
        if (g != 0) return;
        if (base_out && a.values) a.values[brow] = lg[0];
        if (jobcol) {
            if (ka.values_ko) ka.values_ko[orow] = lg[0];
            if (ka.dvalue) ka.dvalue[orow] = lg[0] - vb;
        }
        return;
    }
    // masked categorical, the conventions of iplan_ac_trace (distributions.py:64-68)
    const int32_t* av = a.avail ? a.avail + (int64_t)net * a.av_s_net + ec * a.av_s_chain + sc * a.av_s_step : nullptr;
    f32x4 x;
    int offm = 0;
    float m = -INFINITY;
    for (int q = 0; q < 4; ++q) {
        const int idx = 4 * g + q;
        x[q] = lg[q];
        if (idx < n_out) {
            if (av && av[idx] == 0) { x[q] = -1e10f; offm |= 1 << q; }
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
    // a*: the row's target, or the BASE column's argmax -- one action for every job of the row
    const int cand_b = __shfl(cand, KO_JOBS);
    int64_t want = a.target_all;
    if (a.target) want = a.target[(int64_t)net * a.tg_s_net + ec * a.tg_s_chain + sc * a.tg_s_step];
    const int action = (want >= 0 && want < n_out) ? (int)want : cand_b;
    float sel = 0.f;
    for (int q = 0; q < 4; ++q)
        if (4 * g + q == action) sel += lp[q];
    sel = group_sum(sel);
    const float sel_b = __shfl(sel, KO_JOBS);
    const float kl = knock_kl(pb, lp, offm, n, n_out);
    if (base_out && ka.probs_base)
        for (int q = 0; q < 4; ++q)
            if (4 * g + q < n_out) ka.probs_base[brow * n_out + 4 * g + q] = pb[q];
    if (jobcol && ka.probs_ko)
        for (int q = 0; q < 4; ++q)
            if (4 * g + q < n_out) ka.probs_ko[orow * n_out + 4 * g + q] = pb[q];
    if (g != 0) return;
    if (base_out) {
        if (a.logp) a.logp[brow] = sel;
        if (a.target_out) a.target_out[brow] = (int64_t)action;
        if (ka.greedy_base) ka.greedy_base[brow] = (int64_t)cand;
    }
    if (jobcol) {
        if (ka.logp_ko) ka.logp_ko[orow] = sel;
        if (ka.greedy_ko) ka.greedy_ko[orow] = (int64_t)cand;
        if (ka.kl) ka.kl[orow] = kl;
        if (ka.dlogp) ka.dlogp[orow] = sel - sel_b;
    }
}

int ac_knockout_launch(const IplanAcKnockoutArgs& a, hipStream_t stream) {
    const int64_t rows = (int64_t)a.base.E * a.base.S, tiles = rows * ((a.J + KO_JOBS - 1) / KO_JOBS);
    const unsigned nz = a.base.which == 2 ? 2u : 1u;
    hipLaunchKernelGGL(ac_knockout_kernel, dim3((unsigned)((tiles + SAL_WAVES - 1) / SAL_WAVES), (unsigned)a.base.n_agents, nz), dim3(64 * SAL_WAVES), 0,
                       stream, a);
    return check_launch("iplan_ac_knockout");
}

}  // namespace iplan
