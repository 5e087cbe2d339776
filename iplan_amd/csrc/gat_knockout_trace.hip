// Neighbour knock-out through time: gat_trace.hip's walk over consecutive steps of an episode, run once per JOB of a list with the
// input row of one entity replaced in the first D steps of the window -- "vehicle j was out of sight for D steps and is visible again;
// for how many steps afterwards is every ego's social context still different?".
//
// One 512-thread workgroup owns one (net, env, job slot) for the whole launch: workgroup = (net * B + b) * J + slot.  A job is an
// entity index j, or -1 for "nothing knocked".  It walks steps start .. start + H - 1 of the episode fields, read in place through
// net / env / step strides:  h_s = GAT(x_s, h_{s-1}),  h_{start-1} = hidden0 (or zero).  Every step is gat_fwd_block<false, true,
// true, true>, the form gat_knockout.hip instantiates: in the first D steps ko.j is the slot's job, in the later ones -1 -- those see
// the recorded rows, and the only trace of the knock is the slot's own carried latent (the echo).  Entity j's hidden row is never
// overwritten: it is whatever the knocked chain computed.  The gumbel samples of a (net, env, step) are the same for every job
// (common random numbers).  So the latent of job j at every step carries the bits iplan_gat_trace gives on a copy of the fields
// with row j replaced in the knocked steps only.
//
// Hidden-state hand-off: as in gat_trace.hip -- the new latent is parked in the scene's x table (LDS) behind a barrier of its own
// (inside the block: it separates phase 4's reads of the partial aggregates from the parking stores) and read from there at the top
// of the next step's phase 3.
//
// Distance epilogue, per step:  shift_sq[i] = sum_c (latent_ko[i][c] - base[i][c])^2,  c ascending, one lane per ego (wave 0), the
// chain's latent read from the x table, `base` -- the walk with nothing knocked over the same window, written by an EARLIER launch of
// iplan_gat_trace -- from global memory (knock_shift.h: no fma, the plain fp32 host loop gives the same bits).  With shift_sq wanted
// the last step parks its latent too.  Two barriers keep a fast wave from overwriting a row that a slow lane is still differencing:
//   parking stores -> epilogue reads:         the __syncthreads() in front of the epilogue, below;
//   epilogue reads -> next step's x writes:   the barrier that ends phase 1 of the next step.  Wave 0 passes it only after its
//                                             epilogue, and nothing writes the x table before phase 3's mid barrier, two barriers
//                                             further on (phase 1 and phase 2 do not touch it; the top of phase 3 only reads it).
// No atomics, no sums across workgroups: a slot's bits depend on its scene, its job and the arguments only.
//
// Loop invariants: none is hoisted, for gat_trace.hip's reason (the block makes the parameter pointer and the lane index opaque
// per step; with the fetches lifted out of the loop the kernel spills).
#include "api_util.h"
#include "wave_tile.h"
#include "gat_body.h"
#include "knock_shift.h"

namespace iplan {

static_assert(sizeof(GatShared) <= 160 * 1024, "one CU's LDS");

// what the kernel itself reads of IplanGatKnockoutTraceArgs: the scene's inputs travel in IplanGatFwdArgs, jobs_host stays on the host
struct GatKnockoutTraceDev {
    int32_t B, N, J, H, D, start, knock0, knock1;
    int64_t src0_s_step, src1_s_step;
    const int32_t* jobs;
    const float *noise, *baseline0, *baseline1, *base;
    int64_t base_s_net, base_s_b, base_s_step;
    int64_t lat_s_job, lat_s_step;
    float* attn_ko;
    int64_t attn_s_net, attn_s_b, attn_s_job, attn_s_step;
    float* shift_sq;
    int64_t shift_s_net, shift_s_b, shift_s_job, shift_s_step;
};

// `a`: the scene's descriptor as iplan_gat_fwd takes it (the launcher fills it: h_prev = hidden0, out = latent_ko, nothing saved)
__global__ __launch_bounds__(512) void gat_knockout_trace_kernel(IplanGatFwdArgs a, GatKnockoutTraceDev k) {
    __shared__ __attribute__((aligned(16))) GatShared sh;
    const int slot = (int)(blockIdx.x % (unsigned)k.J);
    const int scene = (int)(blockIdx.x / (unsigned)k.J);
    const int net = scene / k.B, b = scene % k.B;
    const int N = k.N, H = k.H;
    const int job = k.jobs[slot];
    GatKnock ko;
    ko.k0 = k.knock0 != 0;
    ko.k1 = k.knock1 != 0;
    ko.base0 = k.baseline0;
    ko.base1 = k.baseline1;
    GatTraceStep tr;
    tr.soft = nullptr;
    tr.hard = nullptr;
    tr.pres = nullptr;
    tr.part = nullptr;
    for (int h = 0; h < H; ++h) {
        ko.j = h < k.D ? job : -1;                              // the later steps see the recorded rows: the echo
        tr.src0_off = (int64_t)(k.start + h) * k.src0_s_step;
        tr.src1_off = (int64_t)(k.start + h) * k.src1_s_step;
        tr.out_off = (int64_t)slot * k.lat_s_job + (int64_t)h * k.lat_s_step;
        tr.noise = k.noise ? k.noise + ((int64_t)scene * H + h) * N * (N - 1) * 2 : nullptr;
        tr.h_in_lds = h > 0;
        tr.park = h + 1 < H || k.shift_sq != nullptr;           // the epilogue reads the chain's latent from the x table
        tr.attn = k.attn_ko ? k.attn_ko + (int64_t)net * k.attn_s_net + (int64_t)b * k.attn_s_b + (int64_t)slot * k.attn_s_job +
                                  (int64_t)h * k.attn_s_step
                            : nullptr;
        gat_fwd_block<false, true, true, true>(a, scene, sh, &tr, &ko);
        if (k.shift_sq) {
            // the parking stores of both direction waves of every ego tile; the reads below are separated from the next step's
            // first writes to the x table by the barrier that ends that step's phase 1 (the header)
            __syncthreads();
            const int i = (int)threadIdx.x;
            if (i < N) {
                const float* base = k.base + (int64_t)net * k.base_s_net + (int64_t)b * k.base_s_b + (int64_t)h * k.base_s_step + (int64_t)i * GH;
                const float s = knock_shift_sq(&sh.x[i][0], base);
                k.shift_sq[(int64_t)net * k.shift_s_net + (int64_t)b * k.shift_s_b + (int64_t)slot * k.shift_s_job + (int64_t)h * k.shift_s_step + i] = s;
            }
        }
    }
}

}  // namespace iplan

extern "C" int iplan_gat_knockout_trace(const IplanGatKnockoutTraceArgs* a, iplan_stream_t stream) {
    using namespace iplan;
    if (!a) return fail(IPLAN_EINVAL, "iplan_gat_knockout_trace: null args");
    if (a->N < 2 || a->N > IPLAN_MAX_ENTITIES)
        return fail(IPLAN_EINVAL, "iplan_gat_knockout_trace: N=%d outside [2,%d]", a->N, IPLAN_MAX_ENTITIES);
    if (a->J < 1) return fail(IPLAN_EINVAL, "iplan_gat_knockout_trace: J=%d, at least one job is needed", a->J);
    if (a->H < 1) return fail(IPLAN_EINVAL, "iplan_gat_knockout_trace: H=%d, at least one step is needed", a->H);
    if (a->D < 1 || a->D > a->H) return fail(IPLAN_EINVAL, "iplan_gat_knockout_trace: D=%d outside [1,%d]", a->D, a->H);
    if (a->n_nets < 1 || a->B < 1 || a->d0 < 1 || a->d1 < 0 || a->start < 0)
        return fail(IPLAN_EINVAL, "iplan_gat_knockout_trace: bad dims n_nets=%d B=%d d0=%d d1=%d start=%d", a->n_nets, a->B, a->d0, a->d1, a->start);
    if ((int64_t)a->n_nets * a->B * a->J > 0x7fffffff)
        return fail(IPLAN_EINVAL, "iplan_gat_knockout_trace: n_nets * B * J = %lld workgroups exceed 2^31 - 1", (long long)a->n_nets * a->B * a->J);
    if (a->knock1 && a->d1 == 0) return fail(IPLAN_EINVAL, "iplan_gat_knockout_trace: source 1 is to be knocked, but d1 == 0");
    if (!a->src0 || (a->d1 > 0 && !a->src1) || !a->params || !a->jobs || !a->jobs_host)
        return fail(IPLAN_EINVAL, "iplan_gat_knockout_trace: null tensor pointer");
    if (!a->latent_ko && !a->attn_ko && !a->shift_sq) return fail(IPLAN_EINVAL, "iplan_gat_knockout_trace: no output asked for");
    if (a->shift_sq && !a->base)
        return fail(IPLAN_EINVAL, "iplan_gat_knockout_trace: shift_sq needs base, the latents of the window with nothing knocked");
    for (int s = 0; s < a->J; ++s)
        if (a->jobs_host[s] < -1 || a->jobs_host[s] >= a->N)
            return fail(IPLAN_EINVAL, "iplan_gat_knockout_trace: job %d = %d outside [-1,%d]", s, a->jobs_host[s], a->N - 1);
    if (a->hidden0 && (!aligned16(a->hidden0) || (a->h_s_net & 3) || (a->h_s_b & 3)))
        return fail(IPLAN_EALIGN, "iplan_gat_knockout_trace: hidden0 must be 16-byte aligned with strides %% 4 == 0");
    if (a->latent_ko && (!aligned16(a->latent_ko) || (a->lat_s_net & 3) || (a->lat_s_b & 3) || (a->lat_s_job & 3) || (a->lat_s_step & 3)))
        return fail(IPLAN_EALIGN, "iplan_gat_knockout_trace: latent_ko must be 16-byte aligned with strides %% 4 == 0");
    IplanGatFwdArgs f = {};                                   // nothing saved, no clocks
    f.n_nets = a->n_nets; f.B = a->B; f.N = a->N; f.d0 = a->d0; f.d1 = a->d1;
    f.src0 = a->src0; f.src0_s_net = a->src0_s_net; f.src0_s_b = a->src0_s_b;
    f.src1 = a->d1 > 0 ? a->src1 : nullptr; f.src1_s_net = a->src1_s_net; f.src1_s_b = a->src1_s_b;
    f.h_prev = a->hidden0; f.h_s_net = a->h_s_net; f.h_s_b = a->h_s_b;
    f.out = a->latent_ko; f.out_s_net = a->lat_s_net; f.out_s_b = a->lat_s_b;
    f.params = a->params; f.params_s_net = a->params_s_net;
    for (int i = 0; i < IPLAN_GAT_NPARAM; ++i) f.off[i] = a->off[i];
    f.tau = a->tau;
    GatKnockoutTraceDev k = {};
    k.B = a->B; k.N = a->N; k.J = a->J; k.H = a->H; k.D = a->D; k.start = a->start; k.knock0 = a->knock0; k.knock1 = a->knock1;
    k.src0_s_step = a->src0_s_step; k.src1_s_step = a->src1_s_step;
    k.jobs = a->jobs; k.noise = a->noise; k.baseline0 = a->baseline0; k.baseline1 = a->baseline1;
    k.base = a->base; k.base_s_net = a->base_s_net; k.base_s_b = a->base_s_b; k.base_s_step = a->base_s_step;
    k.lat_s_job = a->lat_s_job; k.lat_s_step = a->lat_s_step;
    k.attn_ko = a->attn_ko; k.attn_s_net = a->attn_s_net; k.attn_s_b = a->attn_s_b; k.attn_s_job = a->attn_s_job; k.attn_s_step = a->attn_s_step;
    k.shift_sq = a->shift_sq; k.shift_s_net = a->shift_s_net; k.shift_s_b = a->shift_s_b; k.shift_s_job = a->shift_s_job;
    k.shift_s_step = a->shift_s_step;
    hipLaunchKernelGGL(gat_knockout_trace_kernel, dim3((unsigned)(a->n_nets * a->B * a->J)), dim3(512), 0, (hipStream_t)stream, f, k);
    return check_launch("iplan_gat_knockout_trace");
}
