// C-ABI bookkeeping: version + thread-local error string; the argument checks of iplan_ppo_eval (kernels: ppo_eval.hip) and of
// iplan_ac_saliency (kernel: policy_saliency.hip), of iplan_ac_saliency_lag (kernels: policy_saliency_lag.hip) and of iplan_ac_knockout
// (kernel: policy_knockout.hip).
#include <cstring>

#include "api_util.h"

namespace iplan {
char* error_buffer() {
    static thread_local char buf[512] = {0};
    return buf;
}
int ppo_eval_launch(const IplanPpoEvalArgs& a, hipStream_t stream);   // ppo_eval.hip
int ac_saliency_launch(const IplanAcSaliencyArgs& a, hipStream_t stream);   // policy_saliency.hip
int ac_saliency_lag_launch(const IplanAcSaliencyLagArgs& a, hipStream_t stream);   // policy_saliency_lag.hip
int ac_knockout_launch(const IplanAcKnockoutArgs& a, hipStream_t stream);   // policy_knockout.hip
}  // namespace iplan

extern "C" const char* iplan_last_error(void) { return iplan::error_buffer(); }
extern "C" int iplan_version(void) { return 100; }

extern "C" size_t iplan_sizeof(const char* name) {
    if (!name) return 0;
#define IPLAN_SZ(T) if (!strcmp(name, #T)) return sizeof(T);
    IPLAN_SZ(IplanGatSaved) IPLAN_SZ(IplanGatFwdArgs) IPLAN_SZ(IplanGatBwdArgs) IPLAN_SZ(IplanEncFwdArgs) IPLAN_SZ(IplanAcNet)
    IPLAN_SZ(IplanAcFeatures) IPLAN_SZ(IplanAcFwdArgs) IPLAN_SZ(IplanAcBwdArgs) IPLAN_SZ(IplanAdamArgs) IPLAN_SZ(IplanWgradProblem)
    IPLAN_SZ(IplanWgradArgs) IPLAN_SZ(IplanPpoPrepareArgs) IPLAN_SZ(IplanPpoLossArgs) IPLAN_SZ(IplanPdecArgs) IPLAN_SZ(IplanBehArgs) IPLAN_SZ(IplanMlp3Args) IPLAN_SZ(IplanAdvNormArgs) IPLAN_SZ(IplanSeq2SeqArgs) IPLAN_SZ(IplanAcPackArgs) IPLAN_SZ(IplanP2pArgs) IPLAN_SZ(IplanIpcHandle) IPLAN_SZ(IplanAcXhatArgs) IPLAN_SZ(IplanAcFc1SplitArgs) IPLAN_SZ(IplanObsHistArgs) IPLAN_SZ(IplanSeq2SeqBwdArgs)
    IPLAN_SZ(IplanPredictArgs) IPLAN_SZ(IplanBehEvalArgs) IPLAN_SZ(IplanGatTraceArgs) IPLAN_SZ(IplanAcTraceArgs) IPLAN_SZ(IplanPpoEvalArgs)
    IPLAN_SZ(IplanAcSaliencyArgs) IPLAN_SZ(IplanAcSaliencyLagArgs) IPLAN_SZ(IplanEncSaliencyArgs) IPLAN_SZ(IplanGatSaliencyArgs)
    IPLAN_SZ(IplanPdecSaliencyArgs) IPLAN_SZ(IplanGatKnockoutArgs) IPLAN_SZ(IplanAcKnockoutArgs)
    IPLAN_SZ(IplanAcKnockoutTraceArgs) IPLAN_SZ(IplanGatKnockoutTraceArgs) IPLAN_SZ(IplanAcKnockoutChainArgs)
    IPLAN_SZ(IplanEncKnockoutArgs) IPLAN_SZ(IplanPredictKnockoutArgs) IPLAN_SZ(IplanGatSaliencyTraceArgs)
#undef IPLAN_SZ
    return 0;
}

extern "C" int64_t iplan_ppo_eval_workspace_bytes(int32_t n_agents, int64_t row_stride) {
    if (n_agents < 1 || row_stride < 1 || row_stride > 0x7fffffff) return 0;
    const int64_t chunks = (row_stride + IPLAN_PPO_EVAL_CHUNK - 1) / IPLAN_PPO_EVAL_CHUNK;
    return (int64_t)n_agents * chunks * IPLAN_PPO_EVAL_WS * (int64_t)sizeof(double);
}

extern "C" int iplan_ppo_eval(const IplanPpoEvalArgs* a, iplan_stream_t stream) {
    using namespace iplan;
    if (!a) return fail(IPLAN_EINVAL, "iplan_ppo_eval: null args");
    if (a->n_agents < 1) return fail(IPLAN_EINVAL, "iplan_ppo_eval: n_agents=%d, at least one agent is needed", a->n_agents);
    if (a->T < 1 || a->rows < 1) return fail(IPLAN_EINVAL, "iplan_ppo_eval: rows=%d and T=%d must be positive", a->rows, a->T);
    if (a->rows % a->T) return fail(IPLAN_EINVAL, "iplan_ppo_eval: rows=%d is not a multiple of T=%d", a->rows, a->T);
    if (a->row_stride < a->rows) return fail(IPLAN_EINVAL, "iplan_ppo_eval: rows=%d > row_stride=%lld", a->rows, (long long)a->row_stride);
    if (a->row_stride < 2 || a->row_stride > 0x7fffffff)
        return fail(IPLAN_EINVAL, "iplan_ppo_eval: row_stride=%lld outside [2, 2^31): the unbiased std needs two entries", (long long)a->row_stride);
    if (!a->logp || !a->entropy || !a->values || !a->old_logp || !a->adv || !a->value_preds || !a->returns || !a->mask)
        return fail(IPLAN_EINVAL, "iplan_ppo_eval: a per-row input is null");
    if (!a->stats || !a->step_stats || !a->workspace) return fail(IPLAN_EINVAL, "iplan_ppo_eval: stats, step_stats or workspace is null");
    if (a->n_parts < 0) return fail(IPLAN_EINVAL, "iplan_ppo_eval: n_parts=%d is negative", a->n_parts);
    if (a->flags & ~(IPLAN_PPO_MSE | IPLAN_PPO_NO_VCLIP | IPLAN_PPO_VALUE_MEAN | IPLAN_PPO_POLICY_MEAN))
        return fail(IPLAN_EINVAL, "iplan_ppo_eval: unknown flag bits in %d", a->flags);
    if (a->adv_norm == a->adv) return fail(IPLAN_EINVAL, "iplan_ppo_eval: adv_norm must not alias adv");
    if (((size_t)a->workspace) & 7) return fail(IPLAN_EALIGN, "iplan_ppo_eval: workspace must be 8-byte aligned");
    return ppo_eval_launch(*a, (hipStream_t)stream);
}

__attribute__((visibility("hidden"))) int iplan::ac_rows_check(const char* who, const char* steps, const IplanAcFeatures& ft, int which, int n_agents, int S,
                                                               const IplanAcNet& actor, const IplanAcNet& critic) {
    if (which < 0 || which > 2 || n_agents < 1) return fail(IPLAN_EINVAL, "%s: bad which=%d / n_agents=%d", who, which, n_agents);
    if (ft.N < 1 || ft.N > IPLAN_MAX_ENTITIES) return fail(IPLAN_EINVAL, "%s: N=%d outside [1,%d]", who, ft.N, IPLAN_MAX_ENTITIES);
    if (ft.T != S || ft.T_phys < ft.T)
        return fail(IPLAN_EINVAL, "%s: feat.T=%d must equal %s=%d and T_phys=%d must not be smaller", who, ft.T, steps, S, ft.T_phys);
    if (ft.n_actions < 0 || ft.n_id < 0 || ft.w[0] < 0 || ft.w[1] < 0 || ft.w[2] < 0 || ft.N * (ft.w[0] + ft.w[1] + ft.w[2]) + ft.n_actions + ft.n_id < 1)
        return fail(IPLAN_EINVAL, "%s: bad feature widths", who);
    for (int s = 0; s < 3; ++s)
        if (ft.w[s] > 0 && !ft.src[s]) return fail(IPLAN_EINVAL, "%s: feature source %d is null", who, s);
    if (which != 1) {
        if (actor.n_out < 1 || actor.n_out > 16) return fail(IPLAN_EINVAL, "%s: n_actions=%d outside [1,16]", who, actor.n_out);
        if (!actor.params) return fail(IPLAN_EINVAL, "%s: actor parameters missing", who);
    }
    if (which != 0) {
        if (critic.n_out != 1) return fail(IPLAN_EINVAL, "%s: the critic's head has one output (got %d)", who, critic.n_out);
        if (!critic.params) return fail(IPLAN_EINVAL, "%s: critic parameters missing", who);
    }
    return IPLAN_OK;
}

__attribute__((visibility("hidden"))) int iplan::ac_jobs_check(const char* who, const char* steps, const IplanAcFeatures& ft, int E, int S, int J,
                                                               const int32_t* jobs, const int32_t* jobs_host, const int32_t* knock,
                                                               const float* const* baseline) {
    if (J < 1) return fail(IPLAN_EINVAL, "%s: J=%d, at least one job is needed", who, J);
    if (!jobs || !jobs_host) return fail(IPLAN_EINVAL, "%s: the job list is missing (device and host copy)", who);
    for (int s = 0; s < J; ++s)
        if (jobs_host[s] < -1 || jobs_host[s] >= ft.N) return fail(IPLAN_EINVAL, "%s: job %d = %d outside [-1,%d)", who, s, jobs_host[s], ft.N);
    const int64_t tiles_per_row = (J + 14) / 15;
    if ((int64_t)E * S * tiles_per_row > 0x7fffffff / 16)
        return fail(IPLAN_EINVAL, "%s: E * %s * ceil(J / 15) = %lld tiles are too many", who, steps, (long long)E * S * tiles_per_row);
    for (int s = 0; s < 3; ++s) {
        if (knock[s] && ft.w[s] == 0) return fail(IPLAN_EINVAL, "%s: source %d is to be knocked, but it is absent", who, s);
        if (baseline[s] && ft.w[s] == 0) return fail(IPLAN_EINVAL, "%s: a baseline for the absent source %d", who, s);
    }
    return IPLAN_OK;
}

// the checks iplan_ac_saliency and iplan_ac_saliency_lag share; `outputs`: at least one output must be asked for
static int saliency_check(const IplanAcSaliencyArgs* a, bool outputs) {
    using namespace iplan;
    if (a->E < 1 || a->S < 1) return fail(IPLAN_EINVAL, "iplan_ac_saliency: E=%d x S=%d rows, at least one row is needed", a->E, a->S);
    if ((int64_t)a->E * a->S > 0x7fffffff / 16) return fail(IPLAN_EINVAL, "iplan_ac_saliency: E * S = %lld rows are too many", (long long)a->E * a->S);
    if (const int rc = ac_rows_check("iplan_ac_saliency", "S", a->feat, a->which, a->n_agents, a->S, a->actor, a->critic)) return rc;
    bool any = false;
    if (a->which != 1) {
        if (!a->h_actor) return fail(IPLAN_EINVAL, "iplan_ac_saliency: the actors' GRU state h_actor is missing");
        if (!a->target && (a->target_all < -1 || a->target_all >= a->actor.n_out))
            return fail(IPLAN_EINVAL, "iplan_ac_saliency: target action %d outside [-1,%d)", a->target_all, a->actor.n_out);
        any = any || a->logp || a->target_out || a->entity_actor || a->input_grad_actor || a->act1_actor || a->act2_actor;
    }
    if (a->which != 0) {
        if (!a->h_critic) return fail(IPLAN_EINVAL, "iplan_ac_saliency: the critics' GRU state h_critic is missing");
        any = any || a->values || a->entity_critic || a->input_grad_critic || a->act1_critic || a->act2_critic;
    }
    if (outputs && !any) return fail(IPLAN_EINVAL, "iplan_ac_saliency: no output was asked for");
    if (!aligned16(a->act1_actor) || !aligned16(a->act2_actor) || !aligned16(a->act1_critic) || !aligned16(a->act2_critic) ||
        !aligned16(a->packed_actor) || !aligned16(a->packed_critic) || (a->packed_s_net & 3))
        return fail(IPLAN_EALIGN, "iplan_ac_saliency: act1, act2 and the packed operands must be 16-byte aligned");
    return IPLAN_OK;
}

extern "C" int iplan_ac_saliency(const IplanAcSaliencyArgs* a, iplan_stream_t stream) {
    using namespace iplan;
    if (!a) return fail(IPLAN_EINVAL, "iplan_ac_saliency: null args");
    if (const int rc = saliency_check(a, true)) return rc;
    return ac_saliency_launch(*a, (hipStream_t)stream);
}

extern "C" int iplan_ac_saliency_lag(const IplanAcSaliencyLagArgs* x, iplan_stream_t stream) {
    using namespace iplan;
    if (!x) return fail(IPLAN_EINVAL, "iplan_ac_saliency_lag: null args");
    const IplanAcSaliencyArgs* a = &x->base;
    if (const int rc = saliency_check(a, false)) return rc;                  // (the row description: iplan_ac_saliency's rules)
    if (x->n_lags < 1 || x->n_lags > a->S) return fail(IPLAN_EINVAL, "iplan_ac_saliency_lag: n_lags=%d outside [1, S=%d]", x->n_lags, a->S);
    if (x->lag < 0 || x->lag >= x->n_lags) return fail(IPLAN_EINVAL, "iplan_ac_saliency_lag: lag=%d outside [0, n_lags=%d)", x->lag, x->n_lags);
    if (x->seed_s_row < 0 || x->carry_s_row < 0) return fail(IPLAN_EINVAL, "iplan_ac_saliency_lag: negative seed / carry stride");
    bool any = false;
    for (int net = 0; net < 2; ++net) {
        if (a->which == 1 - net) continue;
        const float* seed = net ? x->seed_critic : x->seed_actor;
        const float* carry = net ? x->carry_critic : x->carry_actor;
        const char* who = net ? "critics" : "actors";
        if (x->lag >= 1 && !seed) return fail(IPLAN_EINVAL, "iplan_ac_saliency_lag: lag=%d needs the %s' seed (the carry of lag %d)", x->lag, who, x->lag - 1);
        if (x->lag + 1 < x->n_lags && !carry) return fail(IPLAN_EINVAL, "iplan_ac_saliency_lag: lag %d follows, the %s' carry is needed", x->lag + 1, who);
        if (x->lag >= 1 && seed && x->seed_s_row < IPLAN_AC_HIDDEN) return fail(IPLAN_EINVAL, "iplan_ac_saliency_lag: seed_s_row=%lld < 64", (long long)x->seed_s_row);
        if (carry && x->carry_s_row < IPLAN_AC_HIDDEN) return fail(IPLAN_EINVAL, "iplan_ac_saliency_lag: carry_s_row=%lld < 64", (long long)x->carry_s_row);
        any = any || carry || (net ? a->entity_critic || a->input_grad_critic : a->entity_actor || a->input_grad_actor);
        if (x->lag == 0) any = any || (net ? a->values || a->act1_critic || a->act2_critic : a->logp || a->target_out || a->act1_actor || a->act2_actor);
    }
    if (!any) return fail(IPLAN_EINVAL, "iplan_ac_saliency_lag: no output of lag %d was asked for", x->lag);
    if (!aligned16(x->seed_actor) || !aligned16(x->seed_critic) || !aligned16(x->carry_actor) || !aligned16(x->carry_critic) || (x->seed_s_row & 3) ||
        (x->carry_s_row & 3))
        return fail(IPLAN_EALIGN, "iplan_ac_saliency_lag: seed and carry must be 16-byte aligned, their row strides multiples of 4");
    return ac_saliency_lag_launch(*x, (hipStream_t)stream);
}

extern "C" int iplan_ac_knockout(const IplanAcKnockoutArgs* k, iplan_stream_t stream) {
    using namespace iplan;
    if (!k) return fail(IPLAN_EINVAL, "iplan_ac_knockout: null args");
    const IplanAcSaliencyArgs* a = &k->base;
    if (const int rc = saliency_check(a, false)) return rc;                  // (the row description: iplan_ac_saliency's rules)
    if (a->entity_actor || a->entity_critic || a->input_grad_actor || a->input_grad_critic || a->act1_actor || a->act2_actor || a->act1_critic ||
        a->act2_critic)
        return fail(IPLAN_EINVAL, "iplan_ac_knockout: of base's outputs only logp, values and target_out (the base result) are written");
    if (const int rc = ac_jobs_check("iplan_ac_knockout", "S", a->feat, a->E, a->S, k->J, k->jobs, k->jobs_host, k->knock, k->baseline)) return rc;
    for (int s = 0; s < 3; ++s) {
        if (k->override_src[s] && a->feat.w[s] == 0) return fail(IPLAN_EINVAL, "iplan_ac_knockout: an override for the absent source %d", s);
        if (k->override_src[s] && (k->ov_s_job[s] < 0 || k->ov_s_net[s] < 0 || k->ov_s_chain[s] < 0 || k->ov_s_step[s] < 0 || k->ov_s_ent[s] < 0))
            return fail(IPLAN_EINVAL, "iplan_ac_knockout: negative override stride of source %d", s);
    }
    bool any = false;
    if (a->which != 1) any = any || a->logp || a->target_out || k->probs_base || k->greedy_base || k->probs_ko || k->logp_ko || k->greedy_ko || k->kl || k->dlogp;
    if (a->which != 0) any = any || a->values || k->values_ko || k->dvalue;
    if (!any) return fail(IPLAN_EINVAL, "iplan_ac_knockout: no output of the selected nets was asked for");
    return ac_knockout_launch(*k, (hipStream_t)stream);
}
