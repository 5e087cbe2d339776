// Neighbour knock-out: the GAT forward pass (gat_body.h) of a scene run once per JOB of a list, forward only, with the input row
// of one entity replaced as it is loaded -- "what becomes of ego i's social context if vehicle j were not there?".
//
// One 512-thread workgroup owns one (net, scene, job slot): workgroup = (net * B + b) * J + slot.  A job is an entity index j, or
// -1 for "nothing knocked".  The arithmetic is gat_fwd_block<false, true, true, true> -- the folded-gate form of the rollout, as
// gat_trace.hip instantiates it, plus the row override of phase 1 (KNOCK) -- so the knocked latent carries the bits the rollout's
// launch gives on a copy of the inputs with row j replaced.  src0 / src1 are read in place through net / scene strides; the
// previous latent is the scene's `hidden`, read from global memory and NOT knocked; the gumbel samples are the scene's, the same for
// every job (common random numbers).
//
// Outputs per slot: the knocked latent, the entity-indexed soft * hard map (the trace form's `attn`), and
//   shift_sq[i] = sum_c (latent_ko[i][c] - base[i][c])^2,   c = 0 .. 31 ascending, one lane per ego,
// with the knocked latent read from the x table the block parks it in (LDS) and `base` -- the scene's latent with nothing knocked,
// written by an EARLIER launch -- from global memory: GatShared leaves no room for it.  Every difference, product and sum is rounded
// on its own (no fma), so the plain fp32 host loop gives the same bits.  No atomics, no sums across workgroups: a slot's bits depend
// on its scene, its job and the arguments only.
#include "api_util.h"
#include "wave_tile.h"
#include "gat_body.h"
#include "knock_shift.h"

namespace iplan {

static_assert(sizeof(GatShared) <= 160 * 1024, "one CU's LDS");

// what the kernel itself reads of IplanGatKnockoutArgs: the scene's inputs travel in IplanGatFwdArgs, jobs_host stays on the host
struct GatKnockoutDev {
    int32_t B, N, J, knock0, knock1;
    const int32_t* jobs;
    const float *noise, *baseline0, *baseline1, *base;
    int64_t base_s_net, base_s_b;
    int64_t lat_s_job;
    float* attn_ko;
    int64_t attn_s_net, attn_s_b, attn_s_job;
    float* shift_sq;
    int64_t shift_s_net, shift_s_b, shift_s_job;
};

// `a`: the scene's descriptor as iplan_gat_fwd takes it (the launcher fills it: h_prev = hidden, out = latent_ko, nothing saved)
__global__ __launch_bounds__(512) void gat_knockout_kernel(IplanGatFwdArgs a, GatKnockoutDev k) {
    __shared__ __attribute__((aligned(16))) GatShared sh;
    const int slot = (int)(blockIdx.x % (unsigned)k.J);
    const int scene = (int)(blockIdx.x / (unsigned)k.J);
    const int net = scene / k.B, b = scene % k.B;
    const int N = k.N;
    GatKnock ko;
    ko.j = k.jobs[slot];
    ko.k0 = k.knock0 != 0;
    ko.k1 = k.knock1 != 0;
    ko.base0 = k.baseline0;
    ko.base1 = k.baseline1;
    GatTraceStep tr;
    tr.src0_off = 0;
    tr.src1_off = 0;
    tr.out_off = (int64_t)slot * k.lat_s_job;
    tr.noise = k.noise ? k.noise + (int64_t)scene * N * (N - 1) * 2 : nullptr;
    tr.h_in_lds = false;
    tr.park = k.shift_sq != nullptr;                         // the epilogue reads the knocked latent from the x table
    tr.soft = nullptr;
    tr.hard = nullptr;
    tr.attn = k.attn_ko ? k.attn_ko + (int64_t)net * k.attn_s_net + (int64_t)b * k.attn_s_b + (int64_t)slot * k.attn_s_job : nullptr;
    tr.pres = nullptr;
    tr.part = nullptr;
    gat_fwd_block<false, true, true, true>(a, scene, sh, &tr, &ko);
    if (k.shift_sq) {
        __syncthreads();                                     // the parking stores of both direction waves of every ego tile
        const int i = (int)threadIdx.x;
        if (i < N) {
            const float* base = k.base + (int64_t)net * k.base_s_net + (int64_t)b * k.base_s_b + (int64_t)i * GH;
            const float s = knock_shift_sq(&sh.x[i][0], base);
            k.shift_sq[(int64_t)net * k.shift_s_net + (int64_t)b * k.shift_s_b + (int64_t)slot * k.shift_s_job + i] = s;
        }
    }
}

}  // namespace iplan

extern "C" int iplan_gat_knockout(const IplanGatKnockoutArgs* a, iplan_stream_t stream) {
    using namespace iplan;
    if (!a) return fail(IPLAN_EINVAL, "iplan_gat_knockout: null args");
    if (a->N < 2 || a->N > IPLAN_MAX_ENTITIES)
        return fail(IPLAN_EINVAL, "iplan_gat_knockout: N=%d outside [2,%d]", a->N, IPLAN_MAX_ENTITIES);
    if (a->J < 1) return fail(IPLAN_EINVAL, "iplan_gat_knockout: J=%d, at least one job is needed", a->J);
    if (a->n_nets < 1 || a->B < 1 || a->d0 < 1 || a->d1 < 0)
        return fail(IPLAN_EINVAL, "iplan_gat_knockout: bad dims n_nets=%d B=%d d0=%d d1=%d", a->n_nets, a->B, a->d0, a->d1);
    if ((int64_t)a->n_nets * a->B * a->J > 0x7fffffff)
        return fail(IPLAN_EINVAL, "iplan_gat_knockout: n_nets * B * J = %lld workgroups exceed 2^31 - 1", (long long)a->n_nets * a->B * a->J);
    if (a->knock1 && a->d1 == 0) return fail(IPLAN_EINVAL, "iplan_gat_knockout: source 1 is to be knocked, but d1 == 0");
    if (!a->src0 || (a->d1 > 0 && !a->src1) || !a->params || !a->jobs || !a->jobs_host)
        return fail(IPLAN_EINVAL, "iplan_gat_knockout: null tensor pointer");
    if (!a->latent_ko && !a->attn_ko && !a->shift_sq) return fail(IPLAN_EINVAL, "iplan_gat_knockout: no output asked for");
    if (a->shift_sq && !a->base) return fail(IPLAN_EINVAL, "iplan_gat_knockout: shift_sq needs base, the latent with nothing knocked");
    for (int s = 0; s < a->J; ++s)
        if (a->jobs_host[s] < -1 || a->jobs_host[s] >= a->N)
            return fail(IPLAN_EINVAL, "iplan_gat_knockout: job %d = %d outside [-1,%d]", s, a->jobs_host[s], a->N - 1);
    if (a->hidden && (!aligned16(a->hidden) || (a->h_s_net & 3) || (a->h_s_b & 3)))
        return fail(IPLAN_EALIGN, "iplan_gat_knockout: hidden must be 16-byte aligned with strides %% 4 == 0");
    if (a->latent_ko && (!aligned16(a->latent_ko) || (a->lat_s_net & 3) || (a->lat_s_b & 3) || (a->lat_s_job & 3)))
        return fail(IPLAN_EALIGN, "iplan_gat_knockout: latent_ko must be 16-byte aligned with strides %% 4 == 0");
    IplanGatFwdArgs f = {};                                   // nothing saved, no clocks
    f.n_nets = a->n_nets; f.B = a->B; f.N = a->N; f.d0 = a->d0; f.d1 = a->d1;
    f.src0 = a->src0; f.src0_s_net = a->src0_s_net; f.src0_s_b = a->src0_s_b;
    f.src1 = a->d1 > 0 ? a->src1 : nullptr; f.src1_s_net = a->src1_s_net; f.src1_s_b = a->src1_s_b;
    f.h_prev = a->hidden; f.h_s_net = a->h_s_net; f.h_s_b = a->h_s_b;
    f.out = a->latent_ko; f.out_s_net = a->lat_s_net; f.out_s_b = a->lat_s_b;
    f.params = a->params; f.params_s_net = a->params_s_net;
    for (int i = 0; i < IPLAN_GAT_NPARAM; ++i) f.off[i] = a->off[i];
    f.tau = a->tau;
    GatKnockoutDev k = {};
    k.B = a->B; k.N = a->N; k.J = a->J; k.knock0 = a->knock0; k.knock1 = a->knock1;
    k.jobs = a->jobs; k.noise = a->noise; k.baseline0 = a->baseline0; k.baseline1 = a->baseline1;
    k.base = a->base; k.base_s_net = a->base_s_net; k.base_s_b = a->base_s_b;
    k.lat_s_job = a->lat_s_job;
    k.attn_ko = a->attn_ko; k.attn_s_net = a->attn_s_net; k.attn_s_b = a->attn_s_b; k.attn_s_job = a->attn_s_job;
    k.shift_sq = a->shift_sq; k.shift_s_net = a->shift_s_net; k.shift_s_b = a->shift_s_b; k.shift_s_job = a->shift_s_job;
    hipLaunchKernelGGL(gat_knockout_kernel, dim3((unsigned)(a->n_nets * a->B * a->J)), dim3(512), 0, (hipStream_t)stream, f, k);
    return check_launch("iplan_gat_knockout");
}
