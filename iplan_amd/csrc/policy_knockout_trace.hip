// Policy knock-out through time: "vehicle j was hidden from this agent for D steps and then shown again -- for how many steps do its
// actions and its critic's values still differ?" (include/iplan_hip.h: IplanAcKnockoutTraceArgs).  E recorded chains are walked over
// H = base.S consecutive steps once per JOB of a list, forward only, each job with a GRU state of its own from a common start state.
// In steps 0 .. D-1 the job's entity loses its entries of the selected sources AS THE FEATURES ARE GATHERED (kfeat_ko, ac_kmap_ko.h);
// steps D .. H-1 see the recorded inputs again, and all that is left of the knock is the job's own state: the echo.  Two kernels, the
// split of policy_trace.hip:
//
//   LN(F) -> fc1 -> act -> LN -> fc2 -> act -> LN -> [ gi = W_ih x + b_ih ]   |   W_hh h, gates -> LN -> head -> kl, dlogp, dvalue, shift
//   -------------- phase 1: knocked trunk, steps < D only ------------------   ------------------- phase 2: knocked walk -----------
//
// Phase 1 (ac_knockout_trace_trunk_kernel): one wave per 16-column tile of one recorded row (e, s < D), four tiles per workgroup.  The
// columns are policy_knockout.hip's: 0 .. 14 the jobs 15 jt .. 15 jt + 14, column 15 the row with nothing knocked.  The body is
// ac_trace_trunk_kernel's, the same text (trace_trunk_impl.h) with the knocked gather, so column 15 holds that kernel's bits; the 192
// gate pre-activations of every column go to gi_ko [2, n_agents, E, D, JT, 16, 192].  The echo steps need the rows' base gi only, once
// per row: base.gi as iplan_ac_trace with phases = 1 leaves it -- the caller runs that first; this file does not repeat it.
//
// Phase 2 (ac_knockout_trace_walk_kernel): one 320-thread workgroup per (net, chain e, job tile jt) walks h = 0 .. H-1; its 16 columns
// are the 15 job chains of ONE chain and, in column 15, its base chain.  Wave roles, W_hh fragments in registers, the double-buffered
// LDS state and the one barrier per step are ac_trace_walk_kernel's.  A column reads its own gi while h < D and the row's base gi
// after (one address for the 16 columns).  The head wave forms, per step and column, against column 15: kl (knock_kl), dlogp, dvalue,
// the column's greedy action and shift_sq = sum over the 64 units, ascending, of (h_col - h_base)^2 read from the LDS state, every
// difference, product and sum rounded on its own.  The base chain's outputs are written by tile jt = 0.
//
// Determinism: a column's arithmetic is lane-local apart from the MFMAs (column n of the product depends on column n of B only), the
// fixed xor butterflies over its four lanes and the reads of column 15, which holds the same bits in every tile.  No atomics, no sums
// across columns.  A column whose gathered values equal the row's own repeats column 15's arithmetic at every step: its kl, dlogp,
// dvalue and shift_sq are exactly 0.  A step's results depend on the steps before it only, so a shorter H gives a prefix.
#include "trace_body.h"
#include "sal_body.h"
#include "ac_kmap_ko.h"

namespace iplan {

__device__ __forceinline__ int64_t ko_trace_tiles(const IplanAcKnockoutTraceArgs& k) { return (k.J + KO_JOBS - 1) / KO_JOBS; }

// ---- phase 1 -----------------------------------------------------------------------------------------------------------------------
#define TRUNK_KTILE(T) sal_ktile(sm, T)
#define TRUNK_FEAT(kt) feat(kt)
#define TRUNK_GI_ROW ka.gi_ko + ((((((int64_t)which * a.n_agents + net) * a.E + ec) * D + sc) * JT + jt) * 16 + n) * PGI
__global__ __launch_bounds__(64 * TRUNK_WAVES) void ac_knockout_trace_trunk_kernel(IplanAcKnockoutTraceArgs ka) {
    const IplanAcTraceArgs& a = ka.base;
    const int net = (int)blockIdx.y, which = trace_which(a);
    const IplanAcNet& nw = which ? a.critic : a.actor;
    const float* __restrict__ P = nw.params + (int64_t)net * nw.params_s_net;
    const IplanAcFeatures& ft = a.feat;
    const int l = lane_id(), w = uniform_i(wave_id()), n = l & 15, g = l >> 4;
    const int D = ka.D, J = ka.J, JT = (int)ko_trace_tiles(ka);
    const int64_t rows = (int64_t)a.E * D;                                   // the knocked rows
    const int64_t tile = (int64_t)blockIdx.x * TRUNK_WAVES + w;
    if (tile >= rows * JT) return;                                           // (whole wave; the kernel has no barrier)
    const int64_t r = tile / JT;                                             // the recorded row all 16 columns share
    const int jt = (int)(tile - r * JT);
    const int slot = KO_JOBS * jt + n;                                       // this column's entry of jobs[]
    const bool is_base = n == KO_JOBS;
    const bool valid = is_base || slot < J;
    const int64_t ec = r / D, sc = r % D;
    const int64_t pr = ec * ft.T_phys + sc;
    const float* const p0 = ft.w[0] > 0 ? ft.src[0] + (int64_t)net * ft.s_net[0] + pr * ft.s_row[0] : nullptr;
    const float* const p1 = ft.w[1] > 0 ? ft.src[1] + (int64_t)net * ft.s_net[1] + pr * ft.s_row[1] : nullptr;
    const float* const p2 = ft.w[2] > 0 ? ft.src[2] + (int64_t)net * ft.s_net[2] + pr * ft.s_row[2] : nullptr;
    int last = -1;
    if (ft.n_actions > 0) {
        if (ft.last_action) last = ft.last_action[(int64_t)net * ft.la_s_net + pr * ft.la_s_row];
        else if (ft.last_action64) last = (int)ft.last_action64[(int64_t)net * ft.la64_s_net + pr * ft.la64_s_row];
    }
    // what this column gathers: the base column the row itself, a job column the row with the job's entity replaced in the knocked sources
    const int job = (valid && !is_base) ? ka.jobs[slot] : -1;
    KnockCol kc;
    kc.ent0 = (ka.knock[0] && ft.w[0] > 0) ? job : -1;
    kc.ent1 = (ka.knock[1] && ft.w[1] > 0) ? job : -1;
    kc.ent2 = (ka.knock[2] && ft.w[2] > 0) ? job : -1;
    kc.bl0 = ka.baseline[0]; kc.bl1 = ka.baseline[1]; kc.bl2 = ka.baseline[2];
    kc.ov0 = nullptr; kc.ov1 = nullptr; kc.ov2 = nullptr;
    kc.se0 = 0; kc.se1 = 0; kc.se2 = 0;
    const KMap km = make_kmap(ft);                                           // (kfeat_ko reads the one-hot widths from it)
    const SalMap sm = sal_make_map(ft);                                      // (the K map as scalars: sal_body.h)
    const int F = sm.NW + ft.n_actions + ft.n_id, KT = sm.KT;
    const int bw0 = sm.w0, bw1 = sm.w1, bw2 = sm.w2;
    auto feat = [&](const KTile& kt) {
        const int ws = kt.s == 0 ? bw0 : (kt.s == 1 ? bw1 : bw2);
        return kfeat_ko(km, kt, p0, p1, p2, kc, ws, valid, last, net);
    };

#include "trace_trunk_impl.h"
}
#undef TRUNK_KTILE
#undef TRUNK_FEAT
#undef TRUNK_GI_ROW

// ---- phase 2 -----------------------------------------------------------------------------------------------------------------------
// sum over the 64 units, ascending, of (col - base)^2: the host's fp32 loop, nothing fused
__device__ __forceinline__ float knock_shift_sq(const float* col, const float* base) {
#pragma clang fp contract(off)
    float acc = 0.f;
    for (int u = 0; u < PM; ++u) {
        const float d = col[u] - base[u];
        const float t = d * d;
        acc = acc + t;
    }
    return acc;
}

__global__ __launch_bounds__(64 * WALK_WAVES) void ac_knockout_trace_walk_kernel(IplanAcKnockoutTraceArgs ka) {
    __shared__ __attribute__((aligned(16))) WalkShared sh;
    const IplanAcTraceArgs& a = ka.base;
    const int net = (int)blockIdx.y, which = trace_which(a);
    const IplanAcNet& nw = which ? a.critic : a.actor;
    const float* __restrict__ P = nw.params + (int64_t)net * nw.params_s_net;
    const int l = lane_id(), w = uniform_i(wave_id()), n = l & 15, g = l >> 4;
    const int E = a.E, S = a.S, D = ka.D, J = ka.J, n_out = nw.n_out, JT = (int)ko_trace_tiles(ka);
    const int64_t ec = (int64_t)blockIdx.x / JT;                             // the chain all 16 columns walk
    const int jt = (int)((int64_t)blockIdx.x - ec * JT);
    const int slot = KO_JOBS * jt + n;
    const bool is_base = n == KO_JOBS;
    const bool valid = is_base || slot < J;
    const bool jobcol = valid && !is_base;
    const bool base_out = is_base && jt == 0;                                // one tile of the chain writes the base outputs
    const bool gru = w < PT;

    // the common start state
    const float* h0 = which ? a.hidden0_critic : a.hidden0_actor;
    f32x4 h[PT];
    for (int t = 0; t < PT; ++t) h[t] = h0 ? vload(h0 + (int64_t)net * a.h0_s_net + ec * a.h0_s_chain, valid, PM, t) : splat4(0.f);

    // step s of this column: its own gi while the knock lasts, the row's base gi after
    const int64_t chain = ((int64_t)which * a.n_agents + net) * E + ec;
    const float* gi_own = ka.gi_ko + ((chain * D * JT + jt) * 16 + n) * PGI;   // step s: + s * JT * 16 * PGI
    const float* gi_row = a.gi + chain * S * PGI;                               // step s: + s * PGI
    auto gi_at = [&](int s) -> const float* { return s < D ? gi_own + (int64_t)s * JT * 16 * PGI : gi_row + (int64_t)s * PGI; };

    // loop invariants.  GRU waves: W_hh rows of this wave's hidden units, gate by gate, and their bias tiles
    f32x4 wf[3][PT], bh[3], gi[3];
    // head wave: rnn.norm and the head
    f32x4 gm[PT], bt[PT], hw[PT], hb = splat4(0.f);
    if (gru) {
        for (int k = 0; k < 3; ++k) {
            for (int T = 0; T < PT; ++T) wf[k][T] = wfrag_a(P + nw.off[IPLAN_AC_WHH], PM, 3 * PM, k * PM + 16 * w, 16 * T);
            bh[k] = bfrag_a(P + nw.off[IPLAN_AC_BHH], k * PT + w);
            gi[k] = vload_a(gi_at(0), valid, k * PT + w);
        }
    } else {
        for (int t = 0; t < PT; ++t) {
            gm[t] = bfrag_a(P + nw.off[IPLAN_AC_LN3_W], t);
            bt[t] = bfrag_a(P + nw.off[IPLAN_AC_LN3_B], t);
            hw[t] = wfrag_a(P + nw.off[IPLAN_AC_HEAD_W], PM, n_out, 0, 16 * t);
        }
        hb = bfrag(P + nw.off[IPLAN_AC_HEAD_B], n_out, 0);
    }
    float* h_ko = which ? ka.h_ko_critic : ka.h_ko_actor;
    float* shift = which ? ka.shift_sq_critic : ka.shift_sq_actor;

    for (int s = 0; s < S; ++s) {
        f32x4 gin[3];
        if (gru) {
            const bool more = valid && s + 1 < S;
            for (int k = 0; k < 3; ++k) gin[k] = vload_a(gi_at(s + 1), more, k * PT + w);
            f32x4 acc[3] = {bh[0], bh[1], bh[2]};
            for (int T = 0; T < PT; ++T)
                for (int q = 0; q < 4; ++q)
                    for (int k = 0; k < 3; ++k) acc[k] = mfma4(wf[k][T][q], h[T][q], acc[k]);
            const f32x4 hown = w == 0 ? h[0] : (w == 1 ? h[1] : (w == 2 ? h[2] : h[3]));
            const GruGates o = gru_gates(gi[0] + acc[0], gi[1] + acc[1], gi[2], acc[2], hown);
            *reinterpret_cast<f32x4*>(&sh.h[s & 1][n][16 * w + 4 * g]) = o.h;
        }
        IPLAN_LDS_BARRIER();
        for (int t = 0; t < PT; ++t) h[t] = *reinterpret_cast<const f32x4*>(&sh.h[s & 1][n][16 * t + 4 * g]);
        if (gru) {
            for (int k = 0; k < 3; ++k) gi[k] = gin[k];
            continue;
        }
        // ---- head wave: the results of step s.  Buffer s & 1 is next written behind the barrier of step s + 1, which waits for this wave
        const int64_t brow = ((int64_t)net * E + ec) * S + s;                 // the base chain's outputs
        const int64_t orow = brow * J + (jobcol ? slot : 0);                  // the column's outputs
        if (h_ko) for (int t = 0; t < PT; ++t) vstore_a(h_ko + orow * PM, jobcol, t, h[t]);
        if (shift) {
            const float sq = knock_shift_sq(&sh.h[s & 1][n][0], &sh.h[s & 1][KO_JOBS][0]);
            if (jobcol && g == 0) shift[orow] = sq;
        }
        f32x4 f[PT];
        for (int t = 0; t < PT; ++t) f[t] = h[t];
        layer_norm_tiles_f<PT>(f, gm, bt, nullptr, nullptr);
        f32x4 lg = hb;
        for (int t = 0; t < PT; ++t) lg = mma_block(hw[t], f[t], lg);
        if (which == 1) {
            const float vb = __shfl(lg[0], KO_JOBS);
            if (g == 0) {
                if (base_out && a.values) a.values[brow] = lg[0];
                if (jobcol) {
                    if (ka.values_ko) ka.values_ko[orow] = lg[0];
                    if (ka.dvalue) ka.dvalue[orow] = lg[0] - vb;
                }
            }
            continue;
        }
        // masked categorical, the conventions of iplan_ac_trace (distributions.py:64-68); the columns share the row's avail
        const int64_t pr = ec * a.feat.T_phys + s;
        f32x4 x;
        int offm = 0;
        float m = -INFINITY;
        for (int q = 0; q < 4; ++q) {
            const int idx = 4 * g + q;
            x[q] = lg[q];
            if (idx < n_out) {
                if (a.avail && a.avail[(int64_t)net * a.av_s_net + pr * a.av_s_row + idx] == 0) { x[q] = -1e10f; offm |= 1 << q; }
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
        // argmax of the probabilities, lowest index on ties (mode 0 of iplan_ac_fwd)
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
        // a*: the row's entry of actions_in, or the BASE chain's argmax of this step -- one action for every job
        const int cand_b = __shfl(cand, KO_JOBS);
        const int64_t want = a.actions_in ? a.actions_in[(int64_t)net * a.act_s_net + pr * a.act_s_row] : -1;
        const int action = (want >= 0 && want < n_out) ? (int)want : cand_b;
        float sel = 0.f;
        for (int q = 0; q < 4; ++q)
            if (4 * g + q == action) sel += lp[q];
        sel = group_sum(sel);
        const float sel_b = __shfl(sel, KO_JOBS);
        const float kl = knock_kl(pb, lp, offm, n, n_out);
        if (base_out && a.probs)
            for (int q = 0; q < 4; ++q)
                if (4 * g + q < n_out) a.probs[brow * n_out + 4 * g + q] = pb[q];
        if (jobcol && ka.probs_ko)
            for (int q = 0; q < 4; ++q)
                if (4 * g + q < n_out) ka.probs_ko[orow * n_out + 4 * g + q] = pb[q];
        if (jobcol && ka.logp_all_ko)
            for (int q = 0; q < 4; ++q)
                if (4 * g + q < n_out) ka.logp_all_ko[orow * n_out + 4 * g + q] = lp[q];
        if (g != 0) continue;
        if (base_out) {
            if (a.logp) a.logp[brow] = sel;
            if (a.greedy) a.greedy[brow] = (int64_t)cand;
            if (ka.target_out) ka.target_out[brow] = (int64_t)action;
        }
        if (jobcol) {
            if (ka.logp_ko) ka.logp_ko[orow] = sel;
            if (ka.greedy_ko) ka.greedy_ko[orow] = (int64_t)cand;
            if (ka.kl) ka.kl[orow] = kl;
            if (ka.dlogp) ka.dlogp[orow] = sel - sel_b;
        }
    }
}

}  // namespace iplan

extern "C" int iplan_ac_knockout_trace(const IplanAcKnockoutTraceArgs* k, iplan_stream_t stream) {
    using namespace iplan;
    if (!k) return fail(IPLAN_EINVAL, "iplan_ac_knockout_trace: null args");
    const IplanAcTraceArgs* a = &k->base;
    if (a->which < 0 || a->which > 2 || a->n_agents < 1)
        return fail(IPLAN_EINVAL, "iplan_ac_knockout_trace: bad which=%d / n_agents=%d", a->which, a->n_agents);
    if (a->E < 1) return fail(IPLAN_EINVAL, "iplan_ac_knockout_trace: E=%d, at least one chain is needed", a->E);
    if (a->S < 1) return fail(IPLAN_EINVAL, "iplan_ac_knockout_trace: H=%d, at least one step is needed", a->S);
    if (k->D < 1 || k->D > a->S) return fail(IPLAN_EINVAL, "iplan_ac_knockout_trace: D=%d outside [1, H=%d]", k->D, a->S);
    if (a->phases < 0 || a->phases > 2) return fail(IPLAN_EINVAL, "iplan_ac_knockout_trace: phases must be 0, 1 or 2 (got %d)", a->phases);
    const IplanAcFeatures& ft = a->feat;
    if (ft.N < 1 || ft.N > IPLAN_MAX_ENTITIES) return fail(IPLAN_EINVAL, "iplan_ac_knockout_trace: N=%d outside [1,%d]", ft.N, IPLAN_MAX_ENTITIES);
    if (ft.T != a->S || ft.T_phys < ft.T)
        return fail(IPLAN_EINVAL, "iplan_ac_knockout_trace: feat.T=%d must equal H=%d and T_phys=%d must not be smaller", ft.T, a->S, ft.T_phys);
    if (ft.n_actions < 0 || ft.n_id < 0 || ft.w[0] < 0 || ft.w[1] < 0 || ft.w[2] < 0 || ft.N * (ft.w[0] + ft.w[1] + ft.w[2]) + ft.n_actions + ft.n_id < 1)
        return fail(IPLAN_EINVAL, "iplan_ac_knockout_trace: bad feature widths");
    for (int s = 0; s < 3; ++s)
        if (ft.w[s] > 0 && !ft.src[s]) return fail(IPLAN_EINVAL, "iplan_ac_knockout_trace: feature source %d is null", s);
    if (k->J < 1) return fail(IPLAN_EINVAL, "iplan_ac_knockout_trace: J=%d, at least one job is needed", k->J);
    if (!k->jobs || !k->jobs_host) return fail(IPLAN_EINVAL, "iplan_ac_knockout_trace: the job list is missing (device and host copy)");
    for (int s = 0; s < k->J; ++s)
        if (k->jobs_host[s] < -1 || k->jobs_host[s] >= ft.N)
            return fail(IPLAN_EINVAL, "iplan_ac_knockout_trace: job %d = %d outside [-1,%d)", s, k->jobs_host[s], ft.N);
    const int64_t JT = (k->J + KO_JOBS - 1) / KO_JOBS;
    if ((int64_t)a->E * a->S * JT > 0x7fffffff / 16)
        return fail(IPLAN_EINVAL, "iplan_ac_knockout_trace: E * H * ceil(J / 15) = %lld tiles are too many", (long long)a->E * a->S * JT);
    for (int s = 0; s < 3; ++s) {
        if (k->knock[s] && ft.w[s] == 0) return fail(IPLAN_EINVAL, "iplan_ac_knockout_trace: source %d is to be knocked, but it is absent", s);
        if (k->baseline[s] && ft.w[s] == 0) return fail(IPLAN_EINVAL, "iplan_ac_knockout_trace: a baseline for the absent source %d", s);
    }
    if (a->entropy || a->h_all_actor || a->h_all_critic || a->h_last_actor || a->h_last_critic)
        return fail(IPLAN_EINVAL, "iplan_ac_knockout_trace: of base's outputs only probs, greedy, logp and values (the base chain) are written");
    bool any = false;
    if (a->which != 1) {
        if (a->actor.n_out < 1 || a->actor.n_out > 16) return fail(IPLAN_EINVAL, "iplan_ac_knockout_trace: n_actions=%d outside [1,16]", a->actor.n_out);
        if (!a->actor.params) return fail(IPLAN_EINVAL, "iplan_ac_knockout_trace: actor parameters missing");
        any = any || a->probs || a->greedy || a->logp || k->target_out || k->probs_ko || k->logp_ko || k->greedy_ko || k->kl || k->dlogp ||
              k->shift_sq_actor || k->h_ko_actor || k->logp_all_ko;
    }
    if (a->which != 0) {
        if (a->critic.n_out != 1) return fail(IPLAN_EINVAL, "iplan_ac_knockout_trace: the critic's head has one output (got %d)", a->critic.n_out);
        if (!a->critic.params) return fail(IPLAN_EINVAL, "iplan_ac_knockout_trace: critic parameters missing");
        any = any || a->values || k->values_ko || k->dvalue || k->shift_sq_critic || k->h_ko_critic;
    }
    if (a->phases != 1 && !any) return fail(IPLAN_EINVAL, "iplan_ac_knockout_trace: no output of the selected nets was asked for");
    if (!k->gi_ko)
        return fail(IPLAN_EINVAL, "iplan_ac_knockout_trace: the gi_ko workspace [2, n_agents, E, D, ceil(J / 15), 16, %d] is missing", IPLAN_AC_TRACE_GI);
    if (k->D < a->S && !a->gi)
        return fail(IPLAN_EINVAL, "iplan_ac_knockout_trace: D=%d < H=%d, the echo steps need base.gi as iplan_ac_trace (phases = 1) leaves it", k->D, a->S);
    if (!aligned16(k->gi_ko) || !aligned16(a->gi) || !aligned16(k->h_ko_actor) || !aligned16(k->h_ko_critic) || !aligned16(a->packed_actor) ||
        !aligned16(a->packed_critic) || (a->packed_s_net & 3))
        return fail(IPLAN_EALIGN, "iplan_ac_knockout_trace: gi_ko, base.gi, h_ko and the packed operands must be 16-byte aligned");
    const unsigned nz = a->which == 2 ? 2u : 1u;
    const int64_t tiles = (int64_t)a->E * k->D * JT;
    if (a->phases != 2)
        hipLaunchKernelGGL(ac_knockout_trace_trunk_kernel, dim3((unsigned)((tiles + TRUNK_WAVES - 1) / TRUNK_WAVES), (unsigned)a->n_agents, nz),
                           dim3(64 * TRUNK_WAVES), 0, (hipStream_t)stream, *k);
    if (a->phases != 1)
        hipLaunchKernelGGL(ac_knockout_trace_walk_kernel, dim3((unsigned)((int64_t)a->E * JT), (unsigned)a->n_agents, nz), dim3(64 * WALK_WAVES), 0,
                           (hipStream_t)stream, *k);
    return check_launch("iplan_ac_knockout_trace");
}
