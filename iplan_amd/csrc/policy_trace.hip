// Policy inspection: R_Actor / R_Critic walked over the S consecutive steps of E recorded chains, forward only, with the GRU state
// carried from step to step by the nets under inspection (include/iplan_hip.h: IplanAcTraceArgs).  Two kernels per call:
//
//   LN(F) -> fc1 -> act -> LN -> fc2 -> act -> LN -> [ gi = W_ih x + b_ih ]   |   W_hh h, gates -> LN -> head
//   ------------------------- phase 1: trunk -------------------------------   ------ phase 2: walk ------
//
// Phase 1 (ac_trace_trunk_kernel) is row-parallel: with the last action taken from the batch, nothing in front of the recurrent
// matrix depends on the state, so every row (chain e, step s) of every net is worked at once -- one wave per 16-row tile, four tiles
// per workgroup, grid = ceil(tiles / 4) x n_agents x nets.  The wave gathers its rows in place through the K map (ac_kmap.h), takes the
// LayerNorm(F) statistics in two passes, contracts fc1 on v_mfma_f32_16x16x4_f32 (k-tile operands requested one tile ahead; the
// partial sums of every 8 k-tiles are added to the running sum, so an accumulation chain is <= 32 MFMAs + F / 128 adds), runs the two
// 64-wide layers from L2-resident weights and stores the 192 input-side gate pre-activations of each row.  Nothing else is recorded.
//
// Phase 2 (ac_trace_walk_kernel): one 320-thread workgroup owns a 16-chain tile of one net and walks s = 0 .. S-1.
//   waves 0..3  wave w owns hidden units 16 w .. 16 w + 15 of all three gates: its 3 x 4 fragments of W_hh (48 registers) are loaded
//               once and stay in registers for the S steps; per step 48 MFMAs in three independent chains, the gate math on its slice,
//               and the slice goes to LDS.  The next step's gi tiles are requested before the chain starts.
//   wave 4      everything behind the state: it picks the full state up from LDS with the others and, while they run step s + 1,
//               stores h_s, normalises it, applies the head and the masked softmax and writes the row's results of step s.
// The recommended shape has one of the four GRU waves do that work; with a wave of its own the per-step critical path is the
// recurrent product and the gates alone (the head of step s overlaps the product of step s + 1), at the price of a fifth wave.
// Hand-off: the state lives in LDS twice (buffers s & 1).  Step s writes buffer s & 1, ONE barrier, everybody reads it; the writes
// of step s + 1 go to the other buffer, and buffer s & 1 is next written in step s + 2, behind the barrier of step s + 1 that every
// reader of step s has passed.  Rows are padded to 72 floats: the 16-byte reads of lane (n, g) at row n, column 16 t + 4 g are
// conflict-free.  The barrier waits for LDS traffic only, so the gi prefetch and wave 4's stores stay in flight across it.
//
// Determinism: a row's arithmetic is lane-local apart from the MFMAs (column n of the product depends on column n of B only) and the
// fixed xor butterflies over the four lane groups; no atomics, no cross-row sums.  The state crosses calls and steps as fp32 values,
// so a walk split into several calls, a chain moved to another lane or tile, and a tile with fewer chains give the same bits.
// Packed and in-place fc1 operands hold the same values (zeros past a block's end in both) and feed the same instructions: the
// normalisation is written with explicit fmaf so that no contraction choice can differ -- same bits either way.
#include "trace_body.h"

namespace iplan {

// ---- phase 1 -----------------------------------------------------------------------------------------------------------------------
#define TRUNK_KTILE(T) ktile(km, T)
#define TRUNK_FEAT(kt) kfeat(km, kt, src, valid, last, net)
#define TRUNK_GI_ROW a.gi + (((int64_t)which * a.n_agents + net) * rows + (valid ? r : 0)) * PGI
__global__ __launch_bounds__(64 * TRUNK_WAVES) void ac_trace_trunk_kernel(IplanAcTraceArgs a) {
    const int net = (int)blockIdx.y, which = trace_which(a);
    const IplanAcNet& nw = which ? a.critic : a.actor;
    const float* __restrict__ P = nw.params + (int64_t)net * nw.params_s_net;
    const IplanAcFeatures& ft = a.feat;
    const int l = lane_id(), w = uniform_i(wave_id()), n = l & 15, g = l >> 4;
    const int64_t rows = (int64_t)a.E * a.S;
    const int64_t tile = (int64_t)blockIdx.x * TRUNK_WAVES + w;
    if (tile * 16 >= rows) return;                                           // (whole wave; the kernel has no barrier)
    const int64_t r = tile * 16 + n;
    const bool valid = r < rows;
    const int64_t pr = valid ? (r / ft.T) * ft.T_phys + r % ft.T : 0;
    const float* src[3];
    for (int s = 0; s < 3; ++s) src[s] = ft.w[s] > 0 ? ft.src[s] + (int64_t)net * ft.s_net[s] + pr * ft.s_row[s] : nullptr;
    int last = -1;
    if (valid && ft.n_actions > 0) {
        if (ft.last_action) last = ft.last_action[(int64_t)net * ft.la_s_net + pr * ft.la_s_row];
        else if (ft.last_action64) last = (int)ft.last_action64[(int64_t)net * ft.la64_s_net + pr * ft.la64_s_row];
    }
    const KMap km = make_kmap(ft);
    const int F = km.NW + km.n_actions + km.n_id, KT = km.kt0[4];

#include "trace_trunk_impl.h"
}
#undef TRUNK_KTILE
#undef TRUNK_FEAT
#undef TRUNK_GI_ROW

// ---- phase 2 -----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64 * WALK_WAVES) void ac_trace_walk_kernel(IplanAcTraceArgs a) {
    __shared__ __attribute__((aligned(16))) WalkShared sh;
    const int net = (int)blockIdx.y, which = trace_which(a);
    const IplanAcNet& nw = which ? a.critic : a.actor;
    const float* __restrict__ P = nw.params + (int64_t)net * nw.params_s_net;
    const int l = lane_id(), w = uniform_i(wave_id()), n = l & 15, g = l >> 4;
    const int E = a.E, S = a.S, n_out = nw.n_out;
    const int e = (int)blockIdx.x * 16 + n;
    const bool valid = e < E;
    const int64_t ec = valid ? e : 0;
    const bool gru = w < PT;

    // the state the walk starts from
    const float* h0 = which ? a.hidden0_critic : a.hidden0_actor;
    f32x4 h[PT];
    for (int t = 0; t < PT; ++t) h[t] = h0 ? vload(h0 + (int64_t)net * a.h0_s_net + ec * a.h0_s_chain, valid, PM, t) : splat4(0.f);

    // loop invariants.  GRU waves: walk_gru_load (trace_body.h); head wave: rnn.norm and the head
    WalkGru u;
    const float* girow = a.gi + (((int64_t)which * a.n_agents + net) * E + ec) * S * PGI;     // step s: + s * PGI
    f32x4 gm[PT], bt[PT], hw[PT], hb = splat4(0.f);
    const bool want_head = which ? a.values != nullptr : (a.probs || a.entropy || a.greedy || a.logp);
    if (gru) {
        walk_gru_load(u, P, nw, w, girow, valid);
    } else {
        for (int t = 0; t < PT; ++t) {
            gm[t] = bfrag_a(P + nw.off[IPLAN_AC_LN3_W], t);
            bt[t] = bfrag_a(P + nw.off[IPLAN_AC_LN3_B], t);
            hw[t] = wfrag_a(P + nw.off[IPLAN_AC_HEAD_W], PM, n_out, 0, 16 * t);
        }
        hb = bfrag(P + nw.off[IPLAN_AC_HEAD_B], n_out, 0);
    }
    float* h_all = which ? a.h_all_critic : a.h_all_actor;
    float* h_last = which ? a.h_last_critic : a.h_last_actor;

    for (int s = 0; s < S; ++s) {
        walk_step(u, gru, h, sh, s, w, girow + (int64_t)(s + 1) * PGI, valid && s + 1 < S);
        if (gru) continue;
        // ---- head wave: the results of step s
        const int64_t orow = ((int64_t)net * E + ec) * S + s;
        if (h_all) for (int t = 0; t < PT; ++t) vstore_a(h_all + orow * PM, valid, t, h[t]);
        if (s + 1 == S) for (int t = 0; t < PT; ++t) vstore_a(h_last + ((int64_t)net * E + ec) * PM, valid, t, h[t]);
        if (!want_head) continue;
        f32x4 f[PT];
        for (int t = 0; t < PT; ++t) f[t] = h[t];
        layer_norm_tiles_f<PT>(f, gm, bt, nullptr, nullptr);
        f32x4 lg = hb;
        for (int t = 0; t < PT; ++t) lg = mma_block(hw[t], f[t], lg);
        if (which == 1) {
            if (valid && g == 0) a.values[orow] = lg[0];
            continue;
        }
        // the masked categorical of ac_categorical.h
        const int64_t pr = ec * a.feat.T_phys + s;
        const MaskedCat c = masked_categorical(lg, (a.avail && valid) ? a.avail + (int64_t)net * a.av_s_net + pr * a.av_s_row : nullptr, g, n_out);
        const int action = (a.actions_in && valid) ? (int)a.actions_in[(int64_t)net * a.act_s_net + pr * a.act_s_row] : -1;
        float sel = 0.f, ent = 0.f;
        for (int q = 0; q < 4; ++q) {
            const int idx = 4 * g + q;
            if (idx < n_out) {
                if (idx == action) sel += c.lp[q];
                ent -= c.pb[q] * c.lp[q];
                if (a.probs && valid) a.probs[orow * n_out + idx] = c.pb[q];
            }
        }
        sel = group_sum(sel);
        ent = group_sum(ent);
        if (valid && g == 0) {
            if (a.greedy) a.greedy[orow] = (int64_t)c.cand;
            if (a.logp) a.logp[orow] = sel;
            if (a.entropy) a.entropy[orow] = ent;
        }
    }
}

}  // namespace iplan

extern "C" int iplan_ac_trace(const IplanAcTraceArgs* a, iplan_stream_t stream) {
    using namespace iplan;
    if (!a) return fail(IPLAN_EINVAL, "iplan_ac_trace: null args");
    if (a->E < 1) return fail(IPLAN_EINVAL, "iplan_ac_trace: E=%d, at least one chain is needed", a->E);
    if (a->S < 1) return fail(IPLAN_EINVAL, "iplan_ac_trace: S=%d, at least one step is needed", a->S);
    if ((int64_t)a->E * a->S > 0x7fffffff / 16) return fail(IPLAN_EINVAL, "iplan_ac_trace: E * S = %lld rows are too many", (long long)a->E * a->S);
    if (a->phases < 0 || a->phases > 2) return fail(IPLAN_EINVAL, "iplan_ac_trace: phases must be 0, 1 or 2 (got %d)", a->phases);
    if (const int rc = ac_rows_check("iplan_ac_trace", "S", a->feat, a->which, a->n_agents, a->S, a->actor, a->critic)) return rc;
    if (a->which != 1) {
        if (!a->h_last_actor) return fail(IPLAN_EINVAL, "iplan_ac_trace: h_last_actor missing");
        if (a->logp && !a->actions_in) return fail(IPLAN_EINVAL, "iplan_ac_trace: logp needs actions_in");
    }
    if (a->which != 0 && !a->h_last_critic) return fail(IPLAN_EINVAL, "iplan_ac_trace: h_last_critic missing");
    if (!a->gi) return fail(IPLAN_EINVAL, "iplan_ac_trace: the gi workspace [2, n_agents, E * S, %d] is missing", IPLAN_AC_TRACE_GI);
    if (!aligned16(a->gi) || !aligned16(a->h_all_actor) || !aligned16(a->h_all_critic) || !aligned16(a->h_last_actor) || !aligned16(a->h_last_critic) ||
        !aligned16(a->packed_actor) || !aligned16(a->packed_critic) || (a->packed_s_net & 3))
        return fail(IPLAN_EALIGN, "iplan_ac_trace: gi, the state outputs and the packed operands must be 16-byte aligned");
    const int64_t rows = (int64_t)a->E * a->S, tiles = (rows + 15) / 16;
    const unsigned nz = a->which == 2 ? 2u : 1u;
    if (a->phases != 2)
        hipLaunchKernelGGL(ac_trace_trunk_kernel, dim3((unsigned)((tiles + TRUNK_WAVES - 1) / TRUNK_WAVES), (unsigned)a->n_agents, nz), dim3(64 * TRUNK_WAVES), 0,
                           (hipStream_t)stream, *a);
    if (a->phases != 1)
        hipLaunchKernelGGL(ac_trace_walk_kernel, dim3((unsigned)((a->E + 15) / 16), (unsigned)a->n_agents, nz), dim3(64 * WALK_WAVES), 0, (hipStream_t)stream, *a);
    return check_launch("iplan_ac_trace");
}
