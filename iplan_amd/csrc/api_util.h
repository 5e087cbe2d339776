// Error reporting + launch checking shared by the C-ABI entry points.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>

#include "iplan_hip.h"

namespace iplan {

char* error_buffer();   // thread-local, defined in api.cpp

inline int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(error_buffer(), 512, fmt, ap);
    va_end(ap);
    return code;
}

inline int check_launch(const char* what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(IPLAN_EHIP, "%s: %s", what, hipGetErrorString(e));
    return IPLAN_OK;
}

int ac_fwd_check(const IplanAcFwdArgs* a, const char* what = "iplan_ac_fwd");   // argument checks of iplan_ac_fwd (actor_critic.hip), also used by iplan_gat_enc_ac_fwd: ``what`` names the refusing entry point

// The checks the policy inspection entries share (api.cpp); `who`: the entry's name as its messages begin, `steps`: its name for S.
// Rows, features and nets: which / n_agents, N, feat.T = S <= T_phys, the widths, the sources, n_out and the parameters of the selected
// nets (iplan_ac_saliency and what builds on it, iplan_ac_trace, iplan_ac_knockout_trace).
int ac_rows_check(const char* who, const char* steps, const IplanAcFeatures& ft, int which, int n_agents, int S, const IplanAcNet& actor,
                  const IplanAcNet& critic);
// The job list, the tile count and knock / baseline of the two policy knock-out entries.
int ac_jobs_check(const char* who, const char* steps, const IplanAcFeatures& ft, int E, int S, int J, const int32_t* jobs, const int32_t* jobs_host,
                  const int32_t* knock, const float* const* baseline);

__host__ __device__ inline bool aligned16(const void* p) { return (((size_t)p) & 15) == 0; }

}  // namespace iplan
