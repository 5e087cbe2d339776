// The social knock-out chain through time: "vehicle j was out of sight for D steps -- how long do this agent's actions and its critic's
// values stay different because its SOCIAL CONTEXT still remembers?" (include/iplan_hip.h: IplanAcKnockoutChainArgs).  This is
// policy_knockout_trace.hip with a per-job source: job q reads an overridden source from a vector of its own at EVERY step of the
// window (the attention latent a knocked GAT walk produced, say), and column 15 -- the base chain -- may read its own from a base
// override (the same walk with nothing knocked).  An overridden source is taken as given and never knocked as well; the other sources
// selected by knock[] are replaced for steps s < D only.
//
// A job's inputs therefore differ from the base's at every step, not only while s < D, and there is no row whose gi all columns share:
//
//   phase 1 (ac_knockout_chain_trunk_kernel)  the knocked trunk over ALL E x H x ceil(J / 15) tiles.  The body is
//       ac_knockout_trace_trunk_kernel's, the same text (knock_trunk_impl.h: trace_trunk_impl.h's text, k-tile order and partial sums)
//       with steps = H; the gather is knock_tile's (ac_kmap_ko.h) with the override pointers set, the base override for column 15 and
//       the entity knock masked off for s >= D.  It writes gi_ko [2, n_agents, E, H, ceil(J / 15), 16, 192].
//   phase 2  IS ac_knockout_trace_walk_kernel (policy_knockout_trace.hip), launched with its D set to H: every column reads its own
//       gi_ko row at every step, column 15 carries the base chain.  No iplan_ac_trace launch, no base.gi.
//
// Determinism, the exact zeros and what is written: policy_knockout_trace.hip's.  The override pointers and strides are wave-uniform;
// a column's address differs by its slot's stride only.  No atomics, no LDS in the trunk, no sums across columns.
#include "knock_trunk.h"

namespace iplan {

__global__ __launch_bounds__(64 * TRUNK_WAVES) void ac_knockout_chain_trunk_kernel(IplanAcKnockoutChainArgs ka) {
    const IplanAcKnockoutTraceArgs& tk = ka.kt;
    const int steps = tk.base.S;                                             // every step of the window has tiles of its own
#include "knock_trunk_impl.h"
}

}  // namespace iplan

extern "C" int iplan_ac_knockout_chain(const IplanAcKnockoutChainArgs* c, iplan_stream_t stream) {
    using namespace iplan;
    const char* who = "iplan_ac_knockout_chain";
    if (!c) return fail(IPLAN_EINVAL, "%s: null args", who);
    const IplanAcKnockoutTraceArgs* k = &c->kt;
    const IplanAcTraceArgs* a = &k->base;
    if (const int rc = ac_knockout_trace_check(who, k, true)) return rc;
    bool any = false;
    for (int s = 0; s < 3; ++s) {
        if ((c->override_src[s] || c->override_base[s]) && a->feat.w[s] == 0)
            return fail(IPLAN_EINVAL, "%s: an override for the absent source %d", who, s);
        if (c->override_src[s] && (c->ov_s_job[s] < 0 || c->ov_s_net[s] < 0 || c->ov_s_chain[s] < 0 || c->ov_s_step[s] < 0 || c->ov_s_ent[s] < 0))
            return fail(IPLAN_EINVAL, "%s: negative override stride of source %d", who, s);
        if (c->override_base[s] && (c->ovb_s_net[s] < 0 || c->ovb_s_chain[s] < 0 || c->ovb_s_step[s] < 0 || c->ovb_s_ent[s] < 0))
            return fail(IPLAN_EINVAL, "%s: negative base override stride of source %d", who, s);
        any = any || c->override_src[s];
    }
    if (!any)
        return fail(IPLAN_EINVAL, "%s: no source has a per-job override; iplan_ac_knockout_trace is the entry for the batch's own sources", who);
    const int64_t tiles = (int64_t)a->E * a->S * ko_trace_tiles(*k);
    if (a->phases != 2)
        hipLaunchKernelGGL(ac_knockout_chain_trunk_kernel, dim3((unsigned)((tiles + TRUNK_WAVES - 1) / TRUNK_WAVES), (unsigned)a->n_agents, a->which == 2 ? 2u : 1u),
                           dim3(64 * TRUNK_WAVES), 0, (hipStream_t)stream, *c);
    if (a->phases != 1) {
        IplanAcKnockoutTraceArgs walk = *k;                                  // the walk with no echo step: gi_ko at every step
        walk.D = a->S;
        ac_knockout_trace_walk_launch(walk, (hipStream_t)stream);
    }
    return check_launch(who);
}
