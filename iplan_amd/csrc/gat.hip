// GAT-RNN instant-incentive encoder: forward pass of GAT_Net (nova/GAT_Net.py:41-142) for every
// (net, env) scene in one launch.
//
// One 512-thread workgroup (8 waves) owns one scene = N <= 64 entities of one (agent-net, env):
//   phase 1  node encode + per-node projections (MFMA): h = ReLU(W_enc x + b); the bi-GRU input
//            projection is separable, W_ih [h_i ; h_j] = W_a h_i + W_b h_j, so the
//            [N-1, B*N, 2H] pair tensor the reference materialises (GAT_Net.py:57-75, 55 % of its
//            CPU time) never exists: W_a h_i stays in registers of the wave that owns chain i,
//            W_b h_j goes to LDS.  q, k, v also go to LDS.
//   phase 2  hard-attention bi-GRU: wave (dir, tile) runs 16 ego chains for N-1 steps; W_hh lives in
//            registers as MFMA A fragments, the hidden state never leaves the D layout, gates are
//            lane-local.  At step s every chain needs W_b h_j for j = s + [s >= i], i.e. one of two
//            LDS rows -> near-broadcast reads.  Each step's contribution to the 2 hard logits is
//            reduced over the 4 lane groups and parked in LDS.
//   phase 3  per 16-ego tile (one wave each): scaled dot-product scores and the gated aggregation of v as two
//            small MFMA products with the ego as the column of the D layout (the softmax over the N-1
//            neighbours and the gumbel-softmax gate, tau = 0.01, are then lane-local).
//   phase 4  output GRUCell (MFMA) -> new attention latent.
// HBM traffic per scene is the compulsory obs + h_prev + noise + out (~1.4 MB per net at cfg3);
// everything else lives in the 150 KB of LDS / registers.  Training launches additionally stream
// the activations the backward pass needs.
#include "api_util.h"
#include "wave_tile.h"
#include "enc_body.h"
#include "ac_fwd_body.h"
#include "gat_body.h"

namespace iplan {

template <bool FOLD>
__global__ __launch_bounds__(512) void gat_fwd_kernel(IplanGatFwdArgs a) {
    __shared__ __attribute__((aligned(16))) GatShared sh;
    gat_fwd_block<false, FOLD>(a, (int)blockIdx.x, sh);
}

// The rollout's vector step: GAT_latent_update and the behaviour encoder's latent_update read the PREVIOUS latents, are
// independent of each other and were two launches on two streams -- whose workgroups the hardware dispatched in either order:
// when the encoder's 140 small workgroups got onto the CUs first, GAT's 160 whole-CU workgroups waited for them (139 us
// instead of 108 us in the kernel trace), and every step paid two cross-stream event round trips.  One launch instead: the
// first n_nets * B workgroups are the GAT scenes (dispatched first, one CU each), the following ones run the encoder, eight
// 16-row tiles each, on the CUs that are left (its LDS is the head of the same allocation).
template <bool FOLD>
__global__ __launch_bounds__(512) void gat_enc_fwd_kernel(IplanGatFwdArgs a, IplanEncFwdArgs e, int n_gat, int enc_blocks_per_net) {
    __shared__ __attribute__((aligned(16))) GatShared sh;
    static_assert(sizeof(GatShared) >= sizeof(float) * ENC_LDS_FLOATS, "encoder LDS must fit into the scene's");
    const int block = (int)blockIdx.x;
    if (block < n_gat) {
        gat_fwd_block<false, FOLD>(a, block, sh);
    } else {
        const int j = block - n_gat, net = j / enc_blocks_per_net, tb = j - net * enc_blocks_per_net;
        enc_fwd_block(e, net, tb * 8 + wave_id(), reinterpret_cast<float*>(&sh));
    }
}

// ... and the NEXT step's action selection behind both (runners/ippo_parallel_runner.py:166-268: select_actions of step t + 1
// reads exactly what the latent updates of step t write, and nothing sits between them -- the environment steps AFTER the
// action selection).  The actor/critic workgroups are the last ones of the grid: they stage their tail weights, compute
// W_hh h and the history block of the fc1 contraction while the scenes run, wait until every scene and encoder workgroup has
// counted itself into sync[0] (ac_fwd_body.h), and go on with the latent blocks.  One launch boundary per vector step instead of
// two, and the action selection's prologue off the critical path.
union GatAcShared {
    GatShared gat;
    AcShared<1> ac;
};

template <bool FOLD>
__global__ __launch_bounds__(512) void gat_enc_ac_fwd_kernel(IplanGatFwdArgs a, IplanEncFwdArgs e, IplanAcFwdArgs c, int n_gat, int enc_blocks_per_net,
                                                             int n_enc, int ac_gx, int32_t* sync) {
    __shared__ __attribute__((aligned(16))) GatAcShared sh;
    static_assert(sizeof(GatShared) >= sizeof(float) * ENC_LDS_FLOATS, "encoder LDS must fit into the scene's");
    const int block = (int)blockIdx.x;
    if (block < n_gat) {
        gat_fwd_block<true, FOLD>(a, block, sh.gat);
        ac_signal_producer_done(sync);
    } else if (block < n_gat + n_enc) {
        const int j = block - n_gat, net = j / enc_blocks_per_net, tb = j - net * enc_blocks_per_net;
        enc_fwd_block<true>(e, net, tb * 8 + wave_id(), reinterpret_cast<float*>(&sh));
        ac_signal_producer_done(sync);
    } else {
        const int j = block - n_gat - n_enc, gy = c.n_agents, gz = c.which == 2 ? 2 : 1;
        const AcGrid gp = {j % ac_gx, (j / ac_gx) % gy, j / (ac_gx * gy), ac_gx, gy, gz};
        ac_fwd_body<1, false, true>(c, gp, sh.ac, AcProducers{sync, n_gat + n_enc, ac_gx * gy * gz});
    }
}

}  // namespace iplan

static int check_gat(const IplanGatFwdArgs* a, const char* what);

extern "C" int iplan_gat_enc_fwd(const IplanGatFwdArgs* a, const IplanEncFwdArgs* e, iplan_stream_t stream) {
    using namespace iplan;
    if (int rc = check_gat(a, "iplan_gat_enc_fwd")) return rc;
    if (!e) return fail(IPLAN_EINVAL, "iplan_gat_enc_fwd: null encoder args");
    if (e->d < 1 || e->d > 16 || e->Z < 1 || e->Z > 16 || e->L < 1 || e->n_nets < 1 || e->B < 1 || e->N < 1)
        return fail(IPLAN_EINVAL, "iplan_gat_enc_fwd: unsupported encoder dims d=%d Z=%d L=%d", e->d, e->Z, e->L);
    if (!e->x || !e->h0 || !e->hL || !e->latent_out || !e->params)
        return fail(IPLAN_EINVAL, "iplan_gat_enc_fwd: null encoder tensor pointer");
    const int n_gat = a->n_nets * a->B, per_net = (e->B * e->N + 127) / 128;
    if (a->saved.gru) hipLaunchKernelGGL(gat_enc_fwd_kernel<false>, dim3((unsigned)(n_gat + per_net * e->n_nets)), dim3(512), 0, (hipStream_t)stream, *a, *e, n_gat, per_net);
    else hipLaunchKernelGGL(gat_enc_fwd_kernel<true>, dim3((unsigned)(n_gat + per_net * e->n_nets)), dim3(512), 0, (hipStream_t)stream, *a, *e, n_gat, per_net);
    return check_launch("iplan_gat_enc_fwd");
}

extern "C" int iplan_gat_enc_ac_fwd(const IplanGatFwdArgs* a, const IplanEncFwdArgs* e, const IplanAcFwdArgs* c, int32_t* sync, iplan_stream_t stream) {
    using namespace iplan;
    if (int rc = check_gat(a, "iplan_gat_enc_ac_fwd")) return rc;
    if (!e || !c || !sync) return fail(IPLAN_EINVAL, "iplan_gat_enc_ac_fwd: null encoder / actor-critic args or sync");
    if (e->d < 1 || e->d > 16 || e->Z < 1 || e->Z > 16 || e->L < 1 || e->n_nets < 1 || e->B < 1 || e->N < 1)
        return fail(IPLAN_EINVAL, "iplan_gat_enc_ac_fwd: unsupported encoder dims d=%d Z=%d L=%d", e->d, e->Z, e->L);
    if (!e->x || !e->h0 || !e->hL || !e->latent_out || !e->params)
        return fail(IPLAN_EINVAL, "iplan_gat_enc_ac_fwd: null encoder tensor pointer");
    if (int rc = ac_fwd_check(c, "iplan_gat_enc_ac_fwd")) return rc;
    if (c->ksplit != 8 || c->saved || c->fc1_pre || c->ln_stats_mode != 0)
        return fail(IPLAN_EINVAL, "iplan_gat_enc_ac_fwd: the actor/critic part must be a rollout-shaped launch (ksplit 8, one-pass "
                                  "LayerNorm statistics, nothing saved)");
    const int n_gat = a->n_nets * a->B, per_net = (e->B * e->N + 127) / 128, n_enc = per_net * e->n_nets;
    const int tiles = (c->rows + 15) / 16, ac_gx = tiles * (c->ksplit_wg > 1 ? c->ksplit_wg : 1);
    const int n_ac = ac_gx * c->n_agents * (c->which == 2 ? 2 : 1);
    if (a->saved.gru) hipLaunchKernelGGL(gat_enc_ac_fwd_kernel<false>, dim3((unsigned)(n_gat + n_enc + n_ac)), dim3(512), 0, (hipStream_t)stream, *a, *e, *c, n_gat, per_net, n_enc, ac_gx, sync);
    else hipLaunchKernelGGL(gat_enc_ac_fwd_kernel<true>, dim3((unsigned)(n_gat + n_enc + n_ac)), dim3(512), 0, (hipStream_t)stream, *a, *e, *c, n_gat, per_net, n_enc, ac_gx, sync);
    return check_launch("iplan_gat_enc_ac_fwd");
}

static int check_gat(const IplanGatFwdArgs* a, const char* what) {
    using namespace iplan;
    if (!a) return fail(IPLAN_EINVAL, "%s: null args", what);
    if (a->N < 2 || a->N > IPLAN_MAX_ENTITIES)
        return fail(IPLAN_EINVAL, "%s: N=%d outside [2,%d]", what, a->N, IPLAN_MAX_ENTITIES);
    if (a->n_nets < 1 || a->B < 1 || a->d0 < 1 || a->d1 < 0)
        return fail(IPLAN_EINVAL, "%s: bad dims n_nets=%d B=%d d0=%d d1=%d", what, a->n_nets, a->B, a->d0, a->d1);
    if (!a->src0 || (a->d1 > 0 && !a->src1) || !a->h_prev || !a->out || !a->noise || !a->params)
        return fail(IPLAN_EINVAL, "%s: null tensor pointer", what);
    if (!aligned16(a->h_prev) || !aligned16(a->out) || (a->h_s_net & 3) || (a->h_s_b & 3) ||
        (a->out_s_net & 3) || (a->out_s_b & 3))
        return fail(IPLAN_EALIGN, "%s: h_prev/out must be 16-byte aligned with strides %% 4 == 0", what);
    return IPLAN_OK;
}

extern "C" int iplan_gat_fwd(const IplanGatFwdArgs* a, iplan_stream_t stream) {
    using namespace iplan;
    if (int rc = check_gat(a, "iplan_gat_fwd")) return rc;
    if (a->saved.gru) hipLaunchKernelGGL(gat_fwd_kernel<false>, dim3((unsigned)(a->n_nets * a->B)), dim3(512), 0, (hipStream_t)stream, *a);
    else hipLaunchKernelGGL(gat_fwd_kernel<true>, dim3((unsigned)(a->n_nets * a->B)), dim3(512), 0, (hipStream_t)stream, *a);
    return check_launch("iplan_gat_fwd");
}
