// The knocked trunk of the knock-out kernels through time (policy_knockout_trace.hip: ac_knockout_trace_trunk_kernel;
// policy_knockout_chain.hip: ac_knockout_chain_trunk_kernel), stated once: one wave per 16-column tile of one recorded row (e, s <
// steps), four tiles per workgroup; columns 0 .. 14 the jobs 15 jt .. 15 jt + 14, column 15 the base.  The body is ac_trace_trunk_kernel's,
// the same text (trace_trunk_impl.h) with the knocked gather (knock_tile / knock_feat, ac_kmap_ko.h); the 192 gate pre-activations of
// every column go to tk.gi_ko [2, n_agents, E, steps, JT, 16, 192].  The kernel's body is knock_trunk_impl.h: statements (sal_body.h says
// why text and not a call), included where these are in scope:
//   ka      what the gather reads: the kernel's own argument struct
//   tk      const IplanAcKnockoutTraceArgs&: its walk description
//   steps   const int: the rows per chain with tiles of their own -- D for the trace (the echo steps read base.gi), H for the chain
// The macros below are the trunk's (trace_body.h) for that body and stay defined for the includer's kernel.
#pragma once
#include "trace_body.h"
#include "sal_body.h"
#include "ac_kmap_ko.h"

namespace iplan {

__host__ __device__ __forceinline__ int64_t ko_trace_tiles(const IplanAcKnockoutTraceArgs& k) { return (k.J + KO_JOBS - 1) / KO_JOBS; }

#define TRUNK_KTILE(T) sal_ktile(sm, T)
#define TRUNK_FEAT(kt) knock_feat(km, sm, kt, col, net)
#define TRUNK_GI_ROW tk.gi_ko + ((((((int64_t)which * a.n_agents + net) * a.E + ec) * steps + sc) * JT + jt) * 16 + n) * PGI

// host side, policy_knockout_trace.hip: the checks both entries share, and phase 2 alone
int ac_knockout_trace_check(const char* who, const IplanAcKnockoutTraceArgs* k, bool chain);
int ac_knockout_trace_walk_launch(const IplanAcKnockoutTraceArgs& k, hipStream_t stream);

}  // namespace iplan
