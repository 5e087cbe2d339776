// The trace kernels (policy_trace.hip: ac_trace_trunk_kernel / ac_trace_walk_kernel; policy_knockout_trace.hip: their knocked forms):
// the helpers here, the statements of the trunk's body in trace_trunk_impl.h -- one source for both, included as TEXT into each kernel
// (sal_body.h says why not called), so that the base column of a knocked tile is the plain trunk's arithmetic.  What differs between
// the two is the gather, and the includer names it:
//   TRUNK_KTILE(T)   this lane's KTile of k-tile T
//   TRUNK_FEAT(kt)   this lane's 4 raw features of its column for that k-tile
//   TRUNK_GI_ROW     where the column's 192 gate pre-activations go
// The body reads, from the kernel around it: a (IplanAcTraceArgs), which, net, nw, P, l, n, g, valid, F, KT.
#pragma once
#include "api_util.h"
#include "wave_tile.h"
#include "gru_tile.h"
#include "ac_kmap.h"

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

}  // namespace iplan
