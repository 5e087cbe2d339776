// The knock-out tile (policy_knockout.hip: ac_knockout_kernel; policy_knockout_trace.hip: both of its kernels), stated once:
//   kfeat_ko        the knocked form of kfeat (ac_kmap.h): one column gathers its row's features with one entity's entries of the
//                   selected sources replaced, or with a whole source read from the column's own vector
//   knock_tile      tile index -> the recorded row, the job tile, the column's slot and flags, the row's source pointers and last
//                   action, and what the column gathers (KnockCol); knock_feat is the gather of one k-tile from it
//   knock_results   what a column forms against column 15 behind the head -- the critic's dvalue, the actor's masked categorical
//                   (ac_categorical.h), a*, dlogp and knock_kl -- and where it goes
// The argument structs (IplanAcKnockoutArgs, IplanAcKnockoutTraceArgs; IplanAcKnockoutChainArgs through its kt: knock_core) name the
// fields read here alike; the functions are templates over them.
#pragma once
#include <type_traits>

#include "sal_body.h"

namespace iplan {

constexpr int KO_JOBS = 15;                // jobs per tile; column 15 carries the base

// What one column (row, job) gathers instead of the row's own values.  Scalars, not arrays: the block is a run-time value, and an
// array indexed by it ends in private memory (sal_body.h: SalMap).
struct KnockCol {
    int ent0, ent1, ent2;                  // per source: the entity whose entries are replaced, or -1
    const float *bl0, *bl1, *bl2;          // its replacement row [w] (nullptr: zeros)
    const float *ov0, *ov1, *ov2;          // the column's own vector of the source (nullptr: the row's), entity e at ov + e * se
    int64_t se0, se1, se2;
};

// this lane's 4 features of one column for a k-tile: kfeat's values (the plain loads, the one-hots) wherever the replacement does not
// reach; `w`: the width per entity of the tile's block (unused for the one-hots), p0 .. p2 the row's own source vectors (scalars for
// the reason above).  In K order entry f of a source block belongs to entity f / w.
__device__ __forceinline__ f32x4 kfeat_ko(const KMap& k, const KTile& kt, const float* p0, const float* p1, const float* p2, const KnockCol& c, int w,
                                          bool valid, int last, int net) {
    const int e0 = c.ent0, e1 = c.ent1, e2 = c.ent2;
    const float *b0 = c.bl0, *b1 = c.bl1, *b2 = c.bl2, *o0 = c.ov0, *o1 = c.ov1, *o2 = c.ov2;
    const int64_t s0 = c.se0, s1 = c.se1, s2 = c.se2;
    const int s = kt.s;
    f32x4 v = splat4(0.f);
    if (!valid || kt.nv == 0) return v;
    if (s == 3) {
        for (int q = 0; q < 4; ++q) {
            const int idx = kt.f0 + q;
            if (q < kt.nv) v[q] = idx < k.n_actions ? (idx == last ? 1.0f : 0.0f) : (idx - k.n_actions == net ? 1.0f : 0.0f);
        }
        return v;
    }
    const int ke = s == 0 ? e0 : (s == 1 ? e1 : e2);
    const float* bl = s == 0 ? b0 : (s == 1 ? b1 : b2);
    const float* ov = s == 0 ? o0 : (s == 1 ? o1 : o2);
    const int64_t se = s == 0 ? s0 : (s == 1 ? s1 : s2);
    const float* p = (s == 0 ? p0 : (s == 1 ? p1 : p2)) + kt.f0;
    const int lo = ke * w;
    if (!ov && (ke < 0 || kt.f0 + kt.nv <= lo || kt.f0 >= lo + w)) {          // untouched: the row's own values
        if (kt.nv == 4) v = ldu4(p);
        else for (int q = 0; q < 4; ++q) if (q < kt.nv) v[q] = as_global(p)[q];
        return v;
    }
    for (int q = 0; q < 4; ++q) {
        if (q >= kt.nv) continue;
        const int f = kt.f0 + q, e = f / w, r = f - e * w;
        if (ov) v[q] = as_global(ov)[(int64_t)e * se + r];
        else if (e == ke) v[q] = bl ? as_global(bl)[r] : 0.0f;
        else v[q] = as_global(p)[q];
    }
    return v;
}

// One column of a knock-out tile.  The 16 columns are VIRTUAL rows of ONE recorded row r = (chain ec, step sc): columns 0 .. 14 are the
// jobs 15 jt .. 15 jt + 14, column 15 is the row with nothing knocked, which every tile carries.
struct KnockTile {
    int64_t ec, sc;                        // the recorded row all 16 columns share
    int jt, slot;                          // the job tile; this column's entry of jobs[]
    bool is_base, valid, jobcol;           // column 15; a column that exists; a job's column
    const float *p0, *p1, *p2;             // the row's own source vectors (nullptr: absent)
    int last;                              // the row's last action, or -1
    KnockCol kc;                           // what the column gathers instead
};

// The struct that carries J, jobs, knock and baseline: the argument struct itself, or the chain's walk description.
__device__ __forceinline__ const IplanAcKnockoutArgs& knock_core(const IplanAcKnockoutArgs& k) { return k; }
__device__ __forceinline__ const IplanAcKnockoutTraceArgs& knock_core(const IplanAcKnockoutTraceArgs& k) { return k; }
__device__ __forceinline__ const IplanAcKnockoutTraceArgs& knock_core(const IplanAcKnockoutChainArgs& k) { return k.kt; }

// tile = r * JT + jt over rows r = ec * steps + sc; n: the lane's column.  The base column gathers the row itself; a job column its own
// vector of an overridden source (IplanAcKnockoutArgs, IplanAcKnockoutChainArgs) and, of the others, the row with the job's entity
// replaced where the source is to be knocked.  The chain (IplanAcKnockoutChainArgs) walks every step of the window: its entity knock
// ends with step D (kt.D), and a source with a base override is read from there by column 15 and by a job of entity -1 that has no
// vector of its own.
template <class KA>
__device__ __forceinline__ KnockTile knock_tile(const KA& ka, const IplanAcFeatures& ft, int64_t tile, int JT, int64_t steps, int net, int n) {
    constexpr bool is_chain = std::is_same<KA, IplanAcKnockoutChainArgs>::value;
    constexpr bool has_override = std::is_same<KA, IplanAcKnockoutArgs>::value || is_chain;
    const auto& kk = knock_core(ka);
    KnockTile t;
    const int64_t r = tile / JT;
    t.jt = (int)(tile - r * JT);
    t.slot = KO_JOBS * t.jt + n;
    t.is_base = n == KO_JOBS;
    t.valid = t.is_base || t.slot < kk.J;
    t.jobcol = t.valid && !t.is_base;
    t.ec = r / steps; t.sc = r % steps;
    const int64_t pr = t.ec * ft.T_phys + t.sc;
    t.p0 = ft.w[0] > 0 ? ft.src[0] + (int64_t)net * ft.s_net[0] + pr * ft.s_row[0] : nullptr;
    t.p1 = ft.w[1] > 0 ? ft.src[1] + (int64_t)net * ft.s_net[1] + pr * ft.s_row[1] : nullptr;
    t.p2 = ft.w[2] > 0 ? ft.src[2] + (int64_t)net * ft.s_net[2] + pr * ft.s_row[2] : nullptr;
    t.last = -1;
    if (ft.n_actions > 0) {
        if (ft.last_action) t.last = ft.last_action[(int64_t)net * ft.la_s_net + pr * ft.la_s_row];
        else if (ft.last_action64) t.last = (int)ft.last_action64[(int64_t)net * ft.la64_s_net + pr * ft.la64_s_row];
    }
    const int job = t.jobcol ? kk.jobs[t.slot] : -1;
    auto from_base = [&](int s) {                                            // (s is a literal at every call)
        if constexpr (is_chain) return t.valid && job < 0 && ka.override_base[s] && ft.w[s] > 0 && !(t.jobcol && ka.override_src[s]);
        return false;
    };
    auto own = [&](int s) -> const float* {
        if constexpr (has_override)
            if (t.jobcol && ka.override_src[s] && ft.w[s] > 0)
                return ka.override_src[s] + (int64_t)t.slot * ka.ov_s_job[s] + (int64_t)net * ka.ov_s_net[s] + t.ec * ka.ov_s_chain[s] + t.sc * ka.ov_s_step[s];
        if constexpr (is_chain)
            if (from_base(s)) return ka.override_base[s] + (int64_t)net * ka.ovb_s_net[s] + t.ec * ka.ovb_s_chain[s] + t.sc * ka.ovb_s_step[s];
        return nullptr;
    };
    auto knocked = [&](int s) {
        if constexpr (has_override)
            if (ka.override_src[s]) return -1;
        if constexpr (is_chain)
            if (t.sc >= kk.D) return -1;
        return (kk.knock[s] && ft.w[s] > 0) ? job : -1;
    };
    KnockCol& kc = t.kc;
    kc.ent0 = knocked(0); kc.ent1 = knocked(1); kc.ent2 = knocked(2);
    kc.bl0 = kk.baseline[0]; kc.bl1 = kk.baseline[1]; kc.bl2 = kk.baseline[2];
    kc.ov0 = own(0); kc.ov1 = own(1); kc.ov2 = own(2);
    kc.se0 = kc.se1 = kc.se2 = 0;
    if constexpr (has_override) { kc.se0 = ka.ov_s_ent[0]; kc.se1 = ka.ov_s_ent[1]; kc.se2 = ka.ov_s_ent[2]; }
    if constexpr (is_chain) {
        if (from_base(0)) kc.se0 = ka.ovb_s_ent[0];
        if (from_base(1)) kc.se1 = ka.ovb_s_ent[1];
        if (from_base(2)) kc.se2 = ka.ovb_s_ent[2];
    }
    return t;
}

// this lane's 4 raw features of its column for a k-tile (km: kfeat_ko reads the one-hot widths from it; sm: the K map as scalars)
__device__ __forceinline__ f32x4 knock_feat(const KMap& km, const SalMap& sm, const KTile& kt, const KnockTile& t, int net) {
    const int w0 = sm.w0, w1 = sm.w1, w2 = sm.w2;
    return kfeat_ko(km, kt, t.p0, t.p1, t.p2, t.kc, kt.s == 0 ? w0 : (kt.s == 1 ? w1 : w2), t.valid, t.last, net);
}

// KL(base || column) of this lane's column, summed in ascending action order: lane (n, gg) holds actions 4 gg .. 4 gg + 3 of column n.
// offm: bit q set = action 4 g + q of this lane is unavailable (the same for every column: they share the row).
__device__ __forceinline__ float knock_kl(const f32x4& pb, const f32x4& lp, int offm, int n, int n_out) {
#pragma clang fp contract(off)
    float kl = 0.f;
#pragma unroll
    for (int gg = 0; gg < 4; ++gg) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float p_b = __shfl(pb[q], 15 + 16 * gg), l_b = __shfl(lp[q], 15 + 16 * gg), l_k = __shfl(lp[q], n + 16 * gg);
            const int om = __shfl(offm, n + 16 * gg);
            if (4 * gg + q < n_out && !((om >> q) & 1)) {
                const float d = l_b - l_k;
                const float t = p_b * d;
                kl = kl + t;
            }
        }
    }
    return kl;
}

// Where the row's base result (column 15 of the tile with base_out) goes; each may be null.
struct KnockBaseOut {
    float *values, *probs, *logp;
    int64_t *greedy, *target_out;
};

// A column's results against column 15, from the head's output lg (lane (n, g): outputs 4 g .. 4 g + 3 of column n).  brow: the row's
// slot of the base outputs, orow: the column's slot of the per-job outputs; av: the row's availability or nullptr; want: the row's
// target, or anything outside [0, n_out) for "the BASE column's argmax" -- one action a* for every job of the row.  Returns the
// column's log-probabilities (the critic: zeros).  Stores by lanes g = 0, the probabilities by every lane its four.
template <class KA>
__device__ __forceinline__ f32x4 knock_results(const KA& ka, const KnockBaseOut& b, int which, const f32x4& lg, const int32_t* av, int64_t want, int n_out,
                                               int n, int g, bool base_out, bool jobcol, int64_t brow, int64_t orow) {
    if (which == 1) {
        const float vb = __shfl(lg[0], KO_JOBS);
        if (g == 0) {
            if (base_out && b.values) b.values[brow] = lg[0];
            if (jobcol) {
                if (ka.values_ko) ka.values_ko[orow] = lg[0];
                if (ka.dvalue) ka.dvalue[orow] = lg[0] - vb;
            }
        }
        return splat4(0.f);
    }
    const MaskedCat c = masked_categorical(lg, av, g, n_out);
    const int cand_b = __shfl(c.cand, KO_JOBS);
    const int action = (want >= 0 && want < n_out) ? (int)want : cand_b;
    float sel = 0.f;
    for (int q = 0; q < 4; ++q)
        if (4 * g + q == action) sel += c.lp[q];
    sel = group_sum(sel);
    const float sel_b = __shfl(sel, KO_JOBS);
    const float kl = knock_kl(c.pb, c.lp, c.offm, n, n_out);
    if (base_out && b.probs)
        for (int q = 0; q < 4; ++q)
            if (4 * g + q < n_out) b.probs[brow * n_out + 4 * g + q] = c.pb[q];
    if (jobcol && ka.probs_ko)
        for (int q = 0; q < 4; ++q)
            if (4 * g + q < n_out) ka.probs_ko[orow * n_out + 4 * g + q] = c.pb[q];
    if (g == 0) {
        if (base_out) {
            if (b.logp) b.logp[brow] = sel;
            if (b.target_out) b.target_out[brow] = (int64_t)action;
            if (b.greedy) b.greedy[brow] = (int64_t)c.cand;
        }
        if (jobcol) {
            if (ka.logp_ko) ka.logp_ko[orow] = sel;
            if (ka.greedy_ko) ka.greedy_ko[orow] = (int64_t)c.cand;
            if (ka.kl) ka.kl[orow] = kl;
            if (ka.dlogp) ka.dlogp[orow] = sel - sel_b;
        }
    }
    return c.lp;
}

}  // namespace iplan
