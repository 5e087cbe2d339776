// Attention inspection: the GAT forward pass (gat_body.h) walked over S consecutive steps of an episode inside ONE launch, forward
// only, with the attention it computes written out.
//
// One 512-thread workgroup owns one (net, env) scene for the whole launch:  h_s = GAT(x_s, h_{s-1}),  s = 0 .. S-1, h_{-1} =
// hidden0 (or zero).  x_s is read in place through the step strides of the episode fields.  The arithmetic of a step is
// gat_fwd_block<false, true> -- the folded-gate form of the rollout -- so the latents carry the rollout's bits.
// Besides the latent after every step the launch can store, per step, the soft-attention weights, the gumbel gate and their
// product as ENTITY-indexed [N, N] maps (element [i, j] = what ego i gives entity j, diagonal 0; the kernel scatters the N-1
// neighbour slots s -> j = s + [s >= i]) and six partial sums per scene-step (include/iplan_hip.h), reduced inside the workgroup
// in a fixed order: lane-local over the lane's 8 pairs, butterfly over the wave, then the 8 waves in wave order.  No atomics;
// every scene-step's sums are written by its own workgroup only.
//
// Hidden-state hand-off: phase 4's wave (dir, tile) produces columns 16 dir .. 16 dir + 15 of its tile's rows and needs all 32
// columns of the previous latent.  The new latent is parked in the scene's x table (LDS; dead once phase 4 has read the two
// partial aggregates -- a barrier of its own separates those reads from the parking stores) and read from there at the top of the
// next step's phase 3, before that phase's mid barrier lets anyone write the table again.  The barrier that ends phase 1 of step
// s + 1 (every wave passes it between its parking store of step s and its read in step s + 1) makes the stores visible.  The same
// barriers order the re-use of the B / q / k / v / logit tables, the presence flags and the per-wave partial sums by the next step.
//
// Loop invariants: none is hoisted.  The split-bf16 W_hh pieces, the hard-encoding fragment and the GRUCell fragments are fetched
// once per STEP (from L2 after the first), not once per launch: the block makes the parameter pointer and the lane index opaque
// per step, because with the fetches of all four phases lifted out of the loop the kernel spills, and phase 2 reads its W_b h_j rows
// where it uses them instead of a pair-step ahead: with both the resource report shows no scratch -- DESIGN.md section 4.
#include "api_util.h"
#include "wave_tile.h"
#include "gat_body.h"

namespace iplan {

struct GatTraceShared {
    GatShared gat;
    float pres[NP];                     // 1 = entity present at this step
    float part[8][IPLAN_GAT_TRACE_NSTAT];   // per wave: partial sums of this scene-step
};
static_assert(sizeof(GatTraceShared) <= 160 * 1024, "one CU's LDS");

// `a`: the scene's descriptor as iplan_gat_fwd takes it (the launcher fills it: h_prev = hidden0, out = latent, nothing saved);
// the step's offsets and outputs ride in GatTraceStep
__global__ __launch_bounds__(512) void gat_trace_kernel(IplanGatFwdArgs a, IplanGatTraceArgs t) {
    __shared__ __attribute__((aligned(16))) GatTraceShared sh;
    const int block = (int)blockIdx.x;
    const int net = block / t.B, b = block % t.B;
    const int N = t.N, S = t.S;
    const int64_t sb = (int64_t)net * t.B + b;
    GatTraceStep tr;
    tr.pres = sh.pres;
    tr.part = t.stats ? &sh.part[0][0] : nullptr;
    for (int s = 0; s < S; ++s) {
        tr.src0_off = (int64_t)s * t.src0_s_step;
        tr.src1_off = (int64_t)s * t.src1_s_step;
        tr.out_off = (int64_t)s * t.lat_s_step;
        tr.noise = t.noise ? t.noise + (sb * S + s) * N * (N - 1) * 2 : nullptr;
        tr.h_in_lds = s > 0;
        tr.park = s + 1 < S;
        tr.soft = t.soft ? t.soft + (int64_t)net * t.soft_s_net + (int64_t)b * t.soft_s_b + (int64_t)s * t.soft_s_step : nullptr;
        tr.hard = t.hard ? t.hard + (int64_t)net * t.hard_s_net + (int64_t)b * t.hard_s_b + (int64_t)s * t.hard_s_step : nullptr;
        tr.attn = t.attn ? t.attn + (int64_t)net * t.attn_s_net + (int64_t)b * t.attn_s_b + (int64_t)s * t.attn_s_step : nullptr;
        if (t.stats && threadIdx.x < NP) {
            // (the previous step read the flags in phase 3, in front of barriers every wave has passed since)
            const int i = (int)threadIdx.x;
            float p = 0.f;
            if (i < N)
                p = t.presence_col < 0 ? 1.f
                                       : (t.src0[(int64_t)net * t.src0_s_net + (int64_t)b * t.src0_s_b + tr.src0_off + (int64_t)i * t.d0 + t.presence_col] != 0.f ? 1.f : 0.f);
            sh.pres[i] = p;
        }
        gat_fwd_block<false, true, true>(a, block, sh.gat, &tr);
        if (t.stats && threadIdx.x < IPLAN_GAT_TRACE_NSTAT) {
            // the waves' partials were stored in front of the barrier that ends phase 3; wave order
            float v = 0.f;
            for (int w = 0; w < 8; ++w) v += sh.part[w][threadIdx.x];
            const float wt = t.weight ? t.weight[sb * S + s] : 1.f;
            t.stats[(sb * S + s) * IPLAN_GAT_TRACE_NSTAT + threadIdx.x] = wt * v;
        }
    }
}

}  // namespace iplan

extern "C" int iplan_gat_trace(const IplanGatTraceArgs* a, iplan_stream_t stream) {
    using namespace iplan;
    if (!a) return fail(IPLAN_EINVAL, "iplan_gat_trace: null args");
    if (a->N < 2 || a->N > IPLAN_MAX_ENTITIES)
        return fail(IPLAN_EINVAL, "iplan_gat_trace: N=%d outside [2,%d]", a->N, IPLAN_MAX_ENTITIES);
    if (a->S < 1) return fail(IPLAN_EINVAL, "iplan_gat_trace: S=%d, at least one step is needed", a->S);
    if (a->n_nets < 1 || a->B < 1 || a->d0 < 1 || a->d1 < 0 || a->presence_col >= a->d0 ||
        (int64_t)a->n_nets * a->B > 0x7fffffff)
        return fail(IPLAN_EINVAL, "iplan_gat_trace: bad dims n_nets=%d B=%d d0=%d d1=%d presence_col=%d", a->n_nets, a->B, a->d0, a->d1,
                    a->presence_col);
    if (!a->src0 || (a->d1 > 0 && !a->src1) || !a->params) return fail(IPLAN_EINVAL, "iplan_gat_trace: null tensor pointer");
    if (!a->latent && !a->soft && !a->hard && !a->attn && !a->stats) return fail(IPLAN_EINVAL, "iplan_gat_trace: no output asked for");
    if (a->hidden0 && (!aligned16(a->hidden0) || (a->h_s_net & 3) || (a->h_s_b & 3)))
        return fail(IPLAN_EALIGN, "iplan_gat_trace: hidden0 must be 16-byte aligned with strides %% 4 == 0");
    if (a->latent && (!aligned16(a->latent) || (a->lat_s_net & 3) || (a->lat_s_b & 3) || (a->lat_s_step & 3)))
        return fail(IPLAN_EALIGN, "iplan_gat_trace: latent must be 16-byte aligned with strides %% 4 == 0");
    IplanGatFwdArgs f = {};                                   // nothing saved, no clocks
    f.n_nets = a->n_nets; f.B = a->B; f.N = a->N; f.d0 = a->d0; f.d1 = a->d1;
    f.src0 = a->src0; f.src0_s_net = a->src0_s_net; f.src0_s_b = a->src0_s_b;
    f.src1 = a->d1 > 0 ? a->src1 : nullptr; f.src1_s_net = a->src1_s_net; f.src1_s_b = a->src1_s_b;
    f.h_prev = a->hidden0; f.h_s_net = a->h_s_net; f.h_s_b = a->h_s_b;
    f.out = a->latent; f.out_s_net = a->lat_s_net; f.out_s_b = a->lat_s_b;
    f.params = a->params; f.params_s_net = a->params_s_net;
    for (int i = 0; i < IPLAN_GAT_NPARAM; ++i) f.off[i] = a->off[i];
    f.tau = a->tau;
    hipLaunchKernelGGL(gat_trace_kernel, dim3((unsigned)(a->n_nets * a->B)), dim3(512), 0, (hipStream_t)stream, f, *a);
    return check_launch("iplan_gat_trace");
}
