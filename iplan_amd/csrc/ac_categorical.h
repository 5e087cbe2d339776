// The masked categorical of the inspection kernels (policy_trace.hip, sal_body_impl.h, policy_knockout.hip, policy_knockout_trace.hip):
// one statement of distributions.py:64-68 and act.py:81-83,159-164 with the conventions of iplan_ac_fwd, so that the four give the
// same bits on the same logits.  (ac_fwd_body.h and actor_critic_bwd.hip keep their own: they sample, and they are benchmarked.)
#pragma once
#include "wave_tile.h"

namespace iplan {

struct MaskedCat {
    f32x4 lp, pb;                          // log-probabilities and probabilities of this lane's four actions
    int offm;                              // bit q set: action 4 g + q is below n_out and unavailable
    int cand;                              // argmax of the probabilities, lowest index on ties (mode 0 of iplan_ac_fwd): the same in the 4 lanes
};

// lane (n, g) holds the logits 4 g .. 4 g + 3 of row n in lg; av: the row's availability [n_out], or nullptr (everything available).
// An unavailable action's logit is -1e10; entries at or past n_out take no part (their pb is 0, their lp is not to be read).
__device__ __forceinline__ MaskedCat masked_categorical(const f32x4& lg, const int32_t* av, int g, int n_out) {
    MaskedCat o;
    f32x4 x;
    o.offm = 0;
    float m = -INFINITY;
    for (int q = 0; q < 4; ++q) {
        const int idx = 4 * g + q;
        x[q] = lg[q];
        if (idx < n_out) {
            if (av && av[idx] == 0) { x[q] = -1e10f; o.offm |= 1 << q; }
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
    for (int q = 0; q < 4; ++q) { o.lp[q] = x[q] - lse; o.pb[q] = ex[q] / se; }
    float best = -INFINITY;
    for (int q = 0; q < 4; ++q)
        if (4 * g + q < n_out) best = fmaxf(best, o.pb[q]);
    best = fmaxf(best, __shfl_xor(best, 16));
    best = fmaxf(best, __shfl_xor(best, 32));
    o.cand = 1 << 30;
    for (int q = 3; q >= 0; --q)
        if (4 * g + q < n_out && o.pb[q] == best) o.cand = 4 * g + q;
    int oc = __shfl_xor(o.cand, 16); o.cand = oc < o.cand ? oc : o.cand;
    oc = __shfl_xor(o.cand, 32); o.cand = oc < o.cand ? oc : o.cand;
    return o;
}

}  // namespace iplan
