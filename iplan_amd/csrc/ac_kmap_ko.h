// The knocked form of kfeat (ac_kmap.h): one column of a knock-out tile gathers its row's features with one entity's entries of the
// selected sources replaced, or with a whole source read from the column's own vector (policy_knockout.hip, policy_knockout_trace.hip);
// and what a job column of such a tile forms against the base column, knock_kl.
#pragma once
#include "ac_kmap.h"

namespace iplan {

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

constexpr int KO_JOBS = 15;                // jobs per tile; column 15 carries the base

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

}  // namespace iplan
