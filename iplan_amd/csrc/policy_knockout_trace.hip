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
#include "knock_trunk.h"

namespace iplan {

// ---- phase 1 (knock_trunk.h: the body, shared with policy_knockout_chain.hip) ---------------------------------------------------------
__global__ __launch_bounds__(64 * TRUNK_WAVES) void ac_knockout_trace_trunk_kernel(IplanAcKnockoutTraceArgs ka) {
    const IplanAcKnockoutTraceArgs& tk = ka;                                 // (no override)
    const int steps = ka.D;                                                  // the knocked rows
#include "knock_trunk_impl.h"
}

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

    // loop invariants.  GRU waves: walk_gru_load (trace_body.h); head wave: rnn.norm and the head
    WalkGru u;
    f32x4 gm[PT], bt[PT], hw[PT], hb = splat4(0.f);
    if (gru) {
        walk_gru_load(u, P, nw, w, gi_at(0), valid);
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
        walk_step(u, gru, h, sh, s, w, gi_at(s + 1), valid && s + 1 < S);
        if (gru) continue;
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
        // the column's results against column 15 (knock_results, ac_kmap_ko.h); the columns share the row's avail and a*: the row's
        // entry of actions_in, or the BASE chain's argmax of this step
        const int64_t pr = ec * a.feat.T_phys + s;
        const int32_t* av = a.avail ? a.avail + (int64_t)net * a.av_s_net + pr * a.av_s_row : nullptr;
        const int64_t want = (which == 0 && a.actions_in) ? a.actions_in[(int64_t)net * a.act_s_net + pr * a.act_s_row] : -1;
        const KnockBaseOut bo = {a.values, a.probs, a.logp, a.greedy, ka.target_out};
        const f32x4 lp = knock_results(ka, bo, which, lg, av, want, n_out, n, g, base_out, jobcol, brow, orow);
        if (which == 0 && jobcol && ka.logp_all_ko)
            for (int q = 0; q < 4; ++q)
                if (4 * g + q < n_out) ka.logp_all_ko[orow * n_out + 4 * g + q] = lp[q];
    }
}

// The argument checks of iplan_ac_knockout_trace, and of iplan_ac_knockout_chain (`chain`), whose trunk covers all H steps: its gi_ko is
// H deep and base.gi is not read.
int ac_knockout_trace_check(const char* who, const IplanAcKnockoutTraceArgs* k, bool chain) {
    const IplanAcTraceArgs* a = &k->base;
    if (a->E < 1) return fail(IPLAN_EINVAL, "%s: E=%d, at least one chain is needed", who, a->E);
    if (a->S < 1) return fail(IPLAN_EINVAL, "%s: H=%d, at least one step is needed", who, a->S);
    if (k->D < 1 || k->D > a->S) return fail(IPLAN_EINVAL, "%s: D=%d outside [1, H=%d]", who, k->D, a->S);
    if (a->phases < 0 || a->phases > 2) return fail(IPLAN_EINVAL, "%s: phases must be 0, 1 or 2 (got %d)", who, a->phases);
    if (const int rc = ac_rows_check(who, "H", a->feat, a->which, a->n_agents, a->S, a->actor, a->critic)) return rc;
    if (const int rc = ac_jobs_check(who, "H", a->feat, a->E, a->S, k->J, k->jobs, k->jobs_host, k->knock, k->baseline)) return rc;
    if (a->entropy || a->h_all_actor || a->h_all_critic || a->h_last_actor || a->h_last_critic)
        return fail(IPLAN_EINVAL, "%s: of base's outputs only probs, greedy, logp and values (the base chain) are written", who);
    bool any = false;
    if (a->which != 1)
        any = any || a->probs || a->greedy || a->logp || k->target_out || k->probs_ko || k->logp_ko || k->greedy_ko || k->kl || k->dlogp ||
              k->shift_sq_actor || k->h_ko_actor || k->logp_all_ko;
    if (a->which != 0) any = any || a->values || k->values_ko || k->dvalue || k->shift_sq_critic || k->h_ko_critic;
    if (a->phases != 1 && !any) return fail(IPLAN_EINVAL, "%s: no output of the selected nets was asked for", who);
    if (!k->gi_ko)
        return fail(IPLAN_EINVAL, "%s: the gi_ko workspace [2, n_agents, E, %s, ceil(J / 15), 16, %d] is missing", who, chain ? "H" : "D", IPLAN_AC_TRACE_GI);
    if (chain && a->gi) return fail(IPLAN_EINVAL, "%s: base.gi is given, but it is not read: every step's gi is the column's own gi_ko row", who);
    if (!chain && k->D < a->S && !a->gi)
        return fail(IPLAN_EINVAL, "%s: D=%d < H=%d, the echo steps need base.gi as iplan_ac_trace (phases = 1) leaves it", who, k->D, a->S);
    if (!aligned16(k->gi_ko) || !aligned16(a->gi) || !aligned16(k->h_ko_actor) || !aligned16(k->h_ko_critic) || !aligned16(a->packed_actor) ||
        !aligned16(a->packed_critic) || (a->packed_s_net & 3))
        return fail(IPLAN_EALIGN, "%s: gi_ko, base.gi, h_ko and the packed operands must be 16-byte aligned", who);
    return IPLAN_OK;
}

// phase 2 alone.  With k.D = H no step reads base.gi: the chain's walk (policy_knockout_chain.hip)
int ac_knockout_trace_walk_launch(const IplanAcKnockoutTraceArgs& k, hipStream_t stream) {
    const IplanAcTraceArgs& a = k.base;
    hipLaunchKernelGGL(ac_knockout_trace_walk_kernel, dim3((unsigned)((int64_t)a.E * ko_trace_tiles(k)), (unsigned)a.n_agents, a.which == 2 ? 2u : 1u),
                       dim3(64 * WALK_WAVES), 0, stream, k);
    return IPLAN_OK;
}

}  // namespace iplan

extern "C" int iplan_ac_knockout_trace(const IplanAcKnockoutTraceArgs* k, iplan_stream_t stream) {
    using namespace iplan;
    if (!k) return fail(IPLAN_EINVAL, "iplan_ac_knockout_trace: null args");
    if (const int rc = ac_knockout_trace_check("iplan_ac_knockout_trace", k, false)) return rc;
    const IplanAcTraceArgs* a = &k->base;
    const int64_t tiles = (int64_t)a->E * k->D * ko_trace_tiles(*k);
    if (a->phases != 2)
        hipLaunchKernelGGL(ac_knockout_trace_trunk_kernel, dim3((unsigned)((tiles + TRUNK_WAVES - 1) / TRUNK_WAVES), (unsigned)a->n_agents, a->which == 2 ? 2u : 1u),
                           dim3(64 * TRUNK_WAVES), 0, (hipStream_t)stream, *k);
    if (a->phases != 1) ac_knockout_trace_walk_launch(*k, (hipStream_t)stream);
    return check_launch("iplan_ac_knockout_trace");
}

