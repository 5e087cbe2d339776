// The trace kernels (policy_trace.hip: ac_trace_trunk_kernel / ac_trace_walk_kernel; policy_knockout_trace.hip: their knocked forms;
// policy_knockout.hip: ac_knockout_kernel, whose trunk is the same): the helpers here, the statements of the trunk's body in
// trace_trunk_impl.h -- one source for the three, included as TEXT into each kernel (sal_body.h says why not called), so that the base
// column of a knocked tile is the plain trunk's arithmetic.  What differs between them is the gather, and the includer names it:
//   TRUNK_KTILE(T)   this lane's KTile of k-tile T
//   TRUNK_FEAT(kt)   this lane's 4 raw features of its column for that k-tile
//   TRUNK_GI_ROW     where the column's 192 gate pre-activations go; not defined: the body ends where f2, the GRU's input, is complete
//                    (ac_knockout_kernel, which runs the cell from a given state in the same wave)
// The body reads, from the kernel around it: a (IplanAcTraceArgs, or IplanAcSaliencyArgs: act_tanh and packed_* are named alike), which,
// net, nw, P, l, n, g, valid, F, KT.
// The two walk kernels share the GRU waves' half of a step: WalkGru, walk_gru_load and walk_step below; what differs is where a
// column's gi of a step lies, and the caller passes the address.
#pragma once
#include "api_util.h"
#include "wave_tile.h"
#include "gru_tile.h"
#include "ac_kmap.h"
#include "ac_categorical.h"

namespace iplan {

constexpr int PM = IPLAN_AC_HIDDEN;        // 64
constexpr int PT = PM / 16;                // 4 tiles
constexpr int PGI = IPLAN_AC_TRACE_GI;     // 192
constexpr int TRUNK_WAVES = 4;             // row tiles per workgroup of phase 1
constexpr int TRUNK_GROUP = 8;             // k-tiles per partial sum
constexpr int WALK_WAVES = 5;              // four GRU waves and the head wave
constexpr int HLD = PM + 8;                // LDS row stride of the state

// MLPBase activation (utils/mappo_utils/mlp.py:10); `tanh` is uniform
__device__ __forceinline__ f32x4 trace_act4(f32x4 v, bool tanh) {
    f32x4 r;
    for (int q = 0; q < 4; ++q) r[q] = tanh ? tanh_f(v[q]) : (v[q] > 0.0f ? v[q] : 0.0f);
    return r;
}

__device__ __forceinline__ int trace_which(const IplanAcTraceArgs& a) { return a.which == 2 ? (int)blockIdx.z : a.which; }

struct TrunkOps {                          // operands of one k-tile
    KTile kt;
    f32x4 x, gm, bt, wf[PT];
};

struct WalkShared {
    __attribute__((aligned(16))) float h[2][16][HLD];
};

// The GRU half of a walk kernel's step (policy_trace.hip describes the roles and the hand-off).  What a GRU wave w < PT keeps for the
// S steps: the W_hh rows of its hidden units 16 w .. 16 w + 15, gate by gate, their bias tiles, and the gi tiles of the step to come.
struct WalkGru {
    f32x4 wf[3][PT], bh[3], gi[3];
};
// gi0: the column's gi row of step 0
__device__ __forceinline__ void walk_gru_load(WalkGru& u, const float* __restrict__ P, const IplanAcNet& nw, int w, const float* gi0, bool valid) {
    for (int k = 0; k < 3; ++k) {
        for (int T = 0; T < PT; ++T) u.wf[k][T] = wfrag_a(P + nw.off[IPLAN_AC_WHH], PM, 3 * PM, k * PM + 16 * w, 16 * T);
        u.bh[k] = bfrag_a(P + nw.off[IPLAN_AC_BHH], k * PT + w);
        u.gi[k] = vload_a(gi0, valid, k * PT + w);
    }
}
// Step s up to the hand-off: the GRU waves (gru) request the gi tiles of step s + 1 (gi_next, read if `more`), take h -> h_s on their
// slice and put it into buffer s & 1; ONE barrier; every wave picks the whole of h_s up.  What differs between the walks is where a
// column's gi of a step lies, and the caller says it.
__device__ __forceinline__ void walk_step(WalkGru& u, bool gru, f32x4 (&h)[PT], WalkShared& sh, int s, int w, const float* gi_next, bool more) {
    const int n = lane_id() & 15, g = lane_id() >> 4;
    f32x4 gin[3];
    if (gru) {
        for (int k = 0; k < 3; ++k) gin[k] = vload_a(gi_next, more, k * PT + w);
        f32x4 acc[3] = {u.bh[0], u.bh[1], u.bh[2]};
        for (int T = 0; T < PT; ++T)
            for (int q = 0; q < 4; ++q)
                for (int k = 0; k < 3; ++k) acc[k] = mfma4(u.wf[k][T][q], h[T][q], acc[k]);
        const f32x4 hown = w == 0 ? h[0] : (w == 1 ? h[1] : (w == 2 ? h[2] : h[3]));
        const GruGates o = gru_gates(u.gi[0] + acc[0], u.gi[1] + acc[1], u.gi[2], acc[2], hown);
        *reinterpret_cast<f32x4*>(&sh.h[s & 1][n][16 * w + 4 * g]) = o.h;
    }
    IPLAN_LDS_BARRIER();
    for (int t = 0; t < PT; ++t) h[t] = *reinterpret_cast<const f32x4*>(&sh.h[s & 1][n][16 * t + 4 * g]);
    if (gru)
        for (int k = 0; k < 3; ++k) u.gi[k] = gin[k];
}

}  // namespace iplan
