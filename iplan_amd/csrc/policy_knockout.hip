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
// in-place operands, the 64-wide layers from L2-resident weights, everything 64 wide in registers in the D layout.  The trunk up to
// the GRU's input is the trace kernels' text (trace_trunk_impl.h) with the knocked gather; the tile's columns and what they form
// against column 15 are stated in ac_kmap_ko.h (knock_tile, knock_results), for this kernel and policy_knockout_trace.hip's.  The 16 columns of
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
#include "trace_body.h"
#include "sal_body.h"
#include "ac_kmap_ko.h"

namespace iplan {

#define TRUNK_KTILE(T) sal_ktile(sm, T)
#define TRUNK_FEAT(kt) knock_feat(km, sm, kt, col, net)
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
    const KnockTile col = knock_tile(ka, ft, tile, JT, a.S, net, n);         // (ac_kmap_ko.h)
    const bool valid = col.valid, jobcol = col.jobcol;
    const int64_t ec = col.ec, sc = col.sc;
    const int64_t brow = (int64_t)net * rows + ec * a.S + sc;                // the row's base outputs
    const int64_t orow = brow * J + (jobcol ? col.slot : 0);                 // the column's outputs
    const KMap km = make_kmap(ft);
    const SalMap sm = sal_make_map(ft);
    const int F = sm.NW + ft.n_actions + ft.n_id, KT = sm.KT;

    // the trunk up to f2: trace_trunk_impl.h's text with the knocked gather (no TRUNK_GI_ROW: gi stays in registers)
#include "trace_trunk_impl.h"

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

    // the column's results against column 15 (knock_results, ac_kmap_ko.h); one tile of the row writes the base outputs
    const int32_t* av = a.avail ? a.avail + (int64_t)net * a.av_s_net + ec * a.av_s_chain + sc * a.av_s_step : nullptr;
    int64_t want = a.target_all;
    if (which == 0 && a.target) want = a.target[(int64_t)net * a.tg_s_net + ec * a.tg_s_chain + sc * a.tg_s_step];
    const KnockBaseOut bo = {a.values, ka.probs_base, a.logp, ka.greedy_base, a.target_out};
    knock_results(ka, bo, which, lg, av, want, n_out, n, g, col.is_base && col.jt == 0, jobcol, brow, orow);
}

#undef TRUNK_KTILE
#undef TRUNK_FEAT

int ac_knockout_launch(const IplanAcKnockoutArgs& a, hipStream_t stream) {
    const int64_t rows = (int64_t)a.base.E * a.base.S, tiles = rows * ((a.J + KO_JOBS - 1) / KO_JOBS);
    const unsigned nz = a.base.which == 2 ? 2u : 1u;
    hipLaunchKernelGGL(ac_knockout_kernel, dim3((unsigned)((tiles + SAL_WAVES - 1) / SAL_WAVES), (unsigned)a.base.n_agents, nz), dim3(64 * SAL_WAVES), 0,
                       stream, a);
    return check_launch("iplan_ac_knockout");
}

}  // namespace iplan
