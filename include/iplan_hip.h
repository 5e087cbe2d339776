/* iplan_hip.h -- C ABI of libiplan_hip.so, the MI355X (gfx950) implementation of the iPLAN
 * multi-agent forward/backward hot path.
 *
 * The reference (wuxiyang1996/iPLAN) is pure Python on PyTorch: it has no FFI of its own, so the
 * "binding a maintainer would add" is a ctypes stub under the reference's nn.Module / policy
 * classes.  Each entry point below names the reference code it replaces
 * (file:line relative to the reference root).
 *
 * Conventions
 *   - plain C, no C++/torch types; every pointer is a DEVICE pointer to contiguous fp32 unless
 *     stated; int64 strides are in ELEMENTS.
 *   - the caller owns all memory (PyTorch caching allocator in the shipped host code); the
 *     library allocates nothing (one documented exception: iplan_p2p_alloc), keeps no global mutable state, and
 *     enqueues every kernel on the stream handed in (no implicit synchronisation) -> thread-safe and stream-ordered.
 *   - return value: 0 on success, a negative IPLAN_E* code otherwise; iplan_last_error() returns
 *     a thread-local human-readable description of the last failure on the calling thread.
 *   - "nets": the reference keeps one private network set per learning agent and loops over
 *     agents in Python (controllers/dcntrl_controller.py:34, nova/prediction_policy.py:101,
 *     nova/stable_behavior_policy.py:101).  Here the n_nets parameter sets are stacked in one
 *     parameter arena (net stride `params_s_net`, per-tensor element offsets `off[]` in
 *     state_dict order) and ONE launch covers every (net, env) pair.
 */
#ifndef IPLAN_HIP_H
#define IPLAN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* iplan_stream_t; /* hipStream_t */

enum {
    IPLAN_OK = 0,
    IPLAN_EINVAL = -1,      /* unsupported dimension / null pointer            */
    IPLAN_EALIGN = -2,      /* pointer not 16-byte aligned                     */
    IPLAN_EHIP = -3         /* HIP runtime error at launch                     */
};

const char* iplan_last_error(void);
int iplan_version(void);
/* sizeof() of an argument struct by name ("IplanGatFwdArgs", ...), 0 if unknown: lets a foreign-language binding check
 * its own struct mirror against the library it loaded. */
size_t iplan_sizeof(const char* struct_name);

/* Limits of this build (compile-time tile sizes). */
#define IPLAN_MAX_ENTITIES 64      /* N  : entities per (env, agent) scene             */
#define IPLAN_GAT_HIDDEN 32        /* H == A == 32 (config/default.yaml:89-90)         */

/* ------------------------------------------------------------------------------------------
 * GAT_Net.forward  (nova/GAT_Net.py:41-142)  --  K1..K7 of SURVEY.md §2b, all nets, one launch.
 * Parameter tensors in state_dict order:
 */
enum {
    IPLAN_GAT_ENC_W = 0,    /* encoding.weight                [H, D]   */
    IPLAN_GAT_ENC_B,        /* encoding.bias                  [H]      */
    IPLAN_GAT_F_WIH,        /* hard_bi_GRU.weight_ih_l0       [3H, 2H] */
    IPLAN_GAT_F_WHH,        /* hard_bi_GRU.weight_hh_l0       [3H, H]  */
    IPLAN_GAT_F_BIH,        /* hard_bi_GRU.bias_ih_l0         [3H]     */
    IPLAN_GAT_F_BHH,        /* hard_bi_GRU.bias_hh_l0         [3H]     */
    IPLAN_GAT_R_WIH,        /* ..._reverse                             */
    IPLAN_GAT_R_WHH,
    IPLAN_GAT_R_BIH,
    IPLAN_GAT_R_BHH,
    IPLAN_GAT_HARD_W,       /* hard_encoding.weight           [2, 2H]  */
    IPLAN_GAT_HARD_B,       /* hard_encoding.bias             [2]      */
    IPLAN_GAT_Q_W,          /* q.weight                       [A, H]   */
    IPLAN_GAT_K_W,          /* k.weight                       [A, H]   */
    IPLAN_GAT_V_W,          /* v.weight                       [A, H]   */
    IPLAN_GAT_V_B,          /* v.bias                         [A]      */
    IPLAN_GAT_C_WIH,        /* rnn.weight_ih (GRUCell)        [3A, A]  */
    IPLAN_GAT_C_WHH,        /* rnn.weight_hh                  [3A, A]  */
    IPLAN_GAT_C_BIH,        /* rnn.bias_ih                    [3A]     */
    IPLAN_GAT_C_BHH,        /* rnn.bias_hh                    [3A]     */
    IPLAN_GAT_NPARAM
};

/* Activations kept for the backward pass (contiguous; NULL = inference).  Rows are (b, i) = b*N + i. */
typedef struct {
    float* h_enc;   /* [n_nets, B*N, H]              ReLU(encoding(obs))                          */
    float* gru;     /* [n_nets, 2, B, ceil(N/16), N-1, 8, 16, 16]  per direction, scene, 16-ego tile and pair step: eight 16-column
                       groups (h h r r z z n n) of [16 egos][16 columns] -- 1 KiB blocks, one per wave store / load; the
                       backward recomputes gh_n = W_hn h_prev + b_hn                                                    */
    float* qkv;     /* [n_nets, B*N, 3A]             q | k | v                                    */
    float* soft;    /* [n_nets, B*N, N-1]            soft attention weights                       */
    float* hard;    /* [n_nets, B*N, N-1]            gumbel-softmax class-1 weights               */
    float* x;       /* [n_nets, B*N, A]              aggregated neighbour feature                 */
    float* cell;    /* [n_nets, B*N, 4A]             GRUCell r, z, n, hn                          */
} IplanGatSaved;

typedef struct {
    int32_t n_nets, B, N;     /* N <= IPLAN_MAX_ENTITIES                                   */
    int32_t d0, d1;           /* GAT input = [src0 (d0 floats) || src1 (d1 floats)] per entity */
    const float* src0;        /* element (net,b,i,c) at src0 + net*src0_s_net + b*src0_s_b + i*d0 + c */
    int64_t src0_s_net, src0_s_b;
    const float* src1;        /* may be NULL iff d1 == 0 (GAT_use_behavior False)           */
    int64_t src1_s_net, src1_s_b;
    const float* h_prev;      /* previous attention latent, rows of A floats: (net,b,i)     */
    int64_t h_s_net, h_s_b;
    float* out;               /* new attention latent, same addressing                      */
    int64_t out_s_net, out_s_b;
    const float* noise;       /* gumbel samples [n_nets,B,N,N-1,2] contiguous               */
    const float* params;      /* parameter arena                                            */
    int64_t params_s_net;
    int64_t off[IPLAN_GAT_NPARAM];
    float tau;                /* 0.01 (nova/GAT_Net.py:93)                                  */
    IplanGatSaved saved;      /* all-NULL for inference                                     */
    int64_t* phase_clocks;    /* optional profiling aid: [n_nets*B, 5] wall_clock64 at kernel entry and after each
                                 of the 4 phases (written by thread 0 of each workgroup); NULL = off          */
} IplanGatFwdArgs;

int iplan_gat_fwd(const IplanGatFwdArgs* args, iplan_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * EncoderRNN.forward + soft latent update (nova/behavior_net.py:17-22,
 * nova/stable_behavior_policy.py:83-123): Linear(d->R)+ReLU -> GRU(R) over the L-step window from
 * the carried hidden state -> Linear(R->Z) -> softmax -> new = (1-c)*prev + c*latent.
 * Rows are (net, b, i) with i < N; R == 32, d <= 16, Z <= 16 in this build.
 */
enum {
    IPLAN_ENC_LIN_W = 0,    /* linear.weight      [R, d]  */
    IPLAN_ENC_LIN_B,        /* linear.bias        [R]     */
    IPLAN_ENC_WIH,          /* rnn.weight_ih_l0   [3R, R] */
    IPLAN_ENC_WHH,          /* rnn.weight_hh_l0   [3R, R] */
    IPLAN_ENC_BIH,          /* rnn.bias_ih_l0     [3R]    */
    IPLAN_ENC_BHH,          /* rnn.bias_hh_l0     [3R]    */
    IPLAN_ENC_OUT_W,        /* out.weight         [Z, R]  */
    IPLAN_ENC_OUT_B,        /* out.bias           [Z]     */
    IPLAN_ENC_NPARAM
};

typedef struct {
    int32_t n_nets, B, N, L, d, Z;
    const float* x;            /* window element (net,b,i,t,c) at x + net*x_s_net + b*x_s_b + i*x_s_i + t*x_s_t + c */
    int64_t x_s_net, x_s_b;
    const float* h0;           /* carried hidden, rows of 32 floats */
    int64_t h0_s_net, h0_s_b;
    float* hL;                 /* new hidden */
    int64_t hL_s_net, hL_s_b;
    const float* prev_latent;  /* rows of Z floats; NULL -> latent_out = softmax only */
    int64_t pl_s_net, pl_s_b;
    float* latent_out;         /* rows of Z floats */
    int64_t lo_s_net, lo_s_b;
    float one_minus_c, c;      /* soft_update_coef (config/default.yaml:75) */
    const float* params;
    int64_t params_s_net;
    int64_t off[IPLAN_ENC_NPARAM];
    int64_t x_s_i, x_s_t;      /* 0, 0 = the contiguous default (L*d, d); lets a sliding window over a time-major
                                  observation log be read in place                                          */
} IplanEncFwdArgs;

int iplan_enc_fwd(const IplanEncFwdArgs* args, iplan_stream_t stream);
/* iplan_gat_fwd and iplan_enc_fwd of one rollout vector step (ippo_parallel_runner.py:223-230: both read the previous
 * latents) as ONE launch: the GAT scenes' workgroups first, the encoder's behind them on the remaining CUs. */
int iplan_gat_enc_fwd(const IplanGatFwdArgs* gat, const IplanEncFwdArgs* enc, iplan_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * R_Actor / R_Critic forward (modules/agents/ippo_actor.py:43-102, modules/critics/ippo_critic.py:47-65,
 * utils/mappo_utils/{mlp,rnn,act,distributions,popart}.py) fused with the feature assembly of
 * DcntrlMAC._build_inputs / _build_inputs_ippo (controllers/dcntrl_controller.py:187-213, 87-115):
 *   x = [ per entity i<N: src0[i] || src1[i] || src2[i] ] || onehot(last_action) || onehot(agent)
 *   LN(F) -> Linear(F->M)+ReLU -> LN -> Linear(M->M)+ReLU -> LN -> GRU(M) one step -> LN -> head
 * for every agent (grid.y) and for actor and critic (grid.z) in one launch.  M == 64.
 * The [rows, F] input matrix the reference materialises (231 MB per agent in PPO) never exists.
 */
enum {
    IPLAN_AC_FN_W = 0,      /* base.feature_norm.weight   [F]     */
    IPLAN_AC_FN_B,          /* base.feature_norm.bias     [F]     */
    IPLAN_AC_FC1_W,         /* base.mlp.fc1.0.weight      [M, F]  */
    IPLAN_AC_FC1_B,         /* base.mlp.fc1.0.bias        [M]     */
    IPLAN_AC_LN1_W,         /* base.mlp.fc1.2.weight      [M]     */
    IPLAN_AC_LN1_B,         /* base.mlp.fc1.2.bias        [M]     */
    IPLAN_AC_FC2_W,         /* base.mlp.fc2.0.0.weight    [M, M]  */
    IPLAN_AC_FC2_B,         /* base.mlp.fc2.0.0.bias      [M]     */
    IPLAN_AC_LN2_W,         /* base.mlp.fc2.0.2.weight    [M]     */
    IPLAN_AC_LN2_B,         /* base.mlp.fc2.0.2.bias      [M]     */
    IPLAN_AC_WIH,           /* rnn.rnn.weight_ih_l0       [3M, M] */
    IPLAN_AC_WHH,           /* rnn.rnn.weight_hh_l0       [3M, M] */
    IPLAN_AC_BIH,           /* rnn.rnn.bias_ih_l0         [3M]    */
    IPLAN_AC_BHH,           /* rnn.rnn.bias_hh_l0         [3M]    */
    IPLAN_AC_LN3_W,         /* rnn.norm.weight            [M]     */
    IPLAN_AC_LN3_B,         /* rnn.norm.bias              [M]     */
    IPLAN_AC_HEAD_W,        /* act.action_out.linear.weight [n_act, M]  |  v_out.weight [1, M] */
    IPLAN_AC_HEAD_B,        /* act.action_out.linear.bias   [n_act]     |  v_out.bias   [1]    */
    IPLAN_AC_NPARAM
};
#define IPLAN_AC_HIDDEN 64
#define IPLAN_AC_SAVE_FLOATS (10 * IPLAN_AC_HIDDEN + 8)
#define IPLAN_AC_KS_SLOT_FLOATS (16 * IPLAN_AC_HIDDEN + 32)   /* a workgroup's partial fc1 sums of one row tile + row sums, row sums of squares */

typedef struct {
    const float* params;        /* arena of the actors (or critics) */
    int64_t params_s_net;
    int64_t off[IPLAN_AC_NPARAM];
    int32_t n_out;              /* n_actions for actors, 1 for critics */
} IplanAcNet;

/* Row r (< rows) of agent `net` lives at physical row  pr = (r / T) * T_phys + r % T  of each
 * source; entity i of source k at  src[k] + net*s_net[k] + pr*s_row[k] + i*w[k]. */
typedef struct {
    int32_t N;
    int32_t w[3];               /* widths per entity (0 = source absent) */
    const float* src[3];
    int64_t s_net[3], s_row[3];
    int32_t n_actions;          /* width of the last-action one-hot (0 = obs_last_action False) */
    const int32_t* last_action; /* hot index per row or -1 (all zeros): last_action[net*la_s_net + pr*la_s_row] */
    int64_t la_s_net, la_s_row;
    int32_t n_id;               /* width of the agent-id one-hot (0 = obs_agent_id False); hot index = net */
    int32_t T, T_phys;          /* logical / physical steps per episode (equal when rows are contiguous) */
    const int64_t* last_action64; /* alternative to last_action: int64 indices read in place (e.g. EpisodeBatch "actions"), */
    int64_t la64_s_net, la64_s_row; /* last_action64[net*la64_s_net + pr*la64_s_row]; used when last_action == NULL      */
} IplanAcFeatures;

typedef struct {
    int32_t n_agents, rows;
    int32_t which;              /* 0 = actors only, 1 = critics only, 2 = both */
    int32_t ksplit;             /* 1 or 8: waves cooperating on the F-contraction of one 16-row tile */
    IplanAcFeatures feat;
    IplanAcNet actor, critic;
    const float* h_actor;       /* GRU state rows of M floats: h + net*hs_net + pr*hs_row */
    const float* h_critic;
    int64_t hs_net, hs_row;
    float* h_actor_out;         /* [n_agents, rows, M] contiguous (NULL = discard) */
    float* h_critic_out;
    /* actor head */
    const int32_t* avail;       /* [.., n_actions] int32, avail + net*av_s_net + pr*av_s_row; NULL = all available */
    int64_t av_s_net, av_s_row;
    int32_t mode;               /* 0 = argmax(probs), 1 = sample argmax(probs / q), 2 = evaluate given actions */
    const float* q_noise;       /* mode 1: Exp(1) samples [n_agents, rows, n_actions] (torch.multinomial's trick) */
    const int64_t* actions_in;  /* mode 2: actions_in[net*act_s_net + pr*act_s_row] */
    int64_t act_s_net, act_s_row;
    int64_t* actions_out;       /* [n_agents, rows] (modes 0,1) */
    float* logp;                /* [n_agents, rows] log-prob of the chosen / given action */
    float* entropy;             /* [n_agents, rows] per-row entropy (NULL = skip) */
    float* probs;               /* [n_agents, rows, n_actions] (NULL = skip) */
    /* critic head */
    float* values;              /* [n_agents, rows] */
    /* activations for the backward pass, [2, n_agents, rows, IPLAN_AC_SAVE_FLOATS] (NULL = inference) */
    float* saved;
    /* optional strided destinations (all-zero strides = the contiguous defaults above) so that a rollout step
     * writes straight into the episode buffer: h_*_out rows at net*ho_s_net + r*ho_s_row, actions_out at
     * net*ao_s_net + r*ao_s_row, and the action's one-hot (n_actions floats) at onehot_out + net*oh_s_net + r*oh_s_row */
    int64_t ho_s_net, ho_s_row;
    int64_t ao_s_net, ao_s_row;
    float* onehot_out;
    int64_t oh_s_net, oh_s_row;
    /* LayerNorm(F) statistics (mean, rstd) per (net, physical row): the features do not change across PPO
     * epochs, so they are computed once (mode 1 = compute + store) and re-read (mode 2); mode 0 = private.   */
    float* ln_stats;
    int64_t ln_stats_s_net;
    int32_t ln_stats_mode;
    int64_t* phase_clocks;      /* optional profiling aid: wall_clock64 of workgroup (0,0,0) at entry, after the
                                   LayerNorm statistics, after the fc1 contraction, at the end of the tail; NULL = off */
    /* optional pre-packed fc1 operands (iplan_ac_pack_fc1): fc1.weight and feature_norm.{weight,bias} of every net in the
     * kernels' own K order and MFMA fragment order, so that a wave's fragment load is ONE contiguous 1 KiB block instead of
     * 64 scattered 64-byte pieces of a row-major [64, F] matrix (the rollout contraction was bound by exactly that:
     * profiles/r02b_notes.md).  NULL = read the arena in place.  The caller repacks after every weight update.          */
    const float* packed_actor;
    const float* packed_critic;
    int64_t packed_s_net;
    /* optional (which = 2, ksplit = 1, ln_stats_mode = 2): fc1's pre-activation  W LN_F(x)  (WITHOUT fc1.bias) of every row, as
     * iplan_ac_fc1_split_fwd leaves it, [2, n_agents, rows, 64]; the launch then skips the F-wide contraction and runs the
     * 64-wide tail only.  NULL = contract here.                                                                            */
    const float* fc1_pre;
    /* optional, rollout shape only (ksplit = 8, ln_stats_mode = 0, packed operands, saved = NULL): the F-wide contraction of a
     * (row tile, net) unit is split over ksplit_wg (2 .. 8) workgroups; their partial sums meet in ks_scratch
     * [units, ksplit_wg, IPLAN_AC_KS_SLOT_FLOATS] and the last arrival (ticket in ks_count [units], zero before the first
     * launch, left zero by every launch) adds them in workgroup order and runs the tail.  units = ceil(rows / 16) * n_agents *
     * (which == 2 ? 2 : 1).  0 / 1 = off.                                                                                   */
    int32_t ksplit_wg;
    float* ks_scratch;
    int32_t* ks_count;
    int32_t act_tanh;           /* MLPBase activation (mlp.py:10, args.use_ReLU): 0 = ReLU (shipped), 1 = tanh -- forward and, through
                                   IplanAcBwdArgs.fwd, the backward tail (round 4: the second activation of this kernel family) */
    int32_t fc1_pre_parts;      /* 0 / 1: fc1_pre is one array; > 1: that many arrays [2, n_agents, rows, 64] back to back
                                   (iplan_ac_fc1_split_fwd with kparts), added in order                                       */
} IplanAcFwdArgs;

int iplan_ac_fwd(const IplanAcFwdArgs* args, iplan_stream_t stream);
/* One rollout vector step as ONE launch (runners/ippo_parallel_runner.py:166-268, controllers/dcntrl_controller.py:27-58): the
 * latent updates of step t (iplan_gat_enc_fwd) and, behind them in the same grid, select_actions_ippo of step t + 1, which reads
 * exactly what they write (the environment steps after the action selection, not between the two).  `ac` must be a rollout-shaped
 * iplan_ac_fwd argument set (ksplit 8, nothing saved).  `sync`: 3 int32 counters owned by the caller, zero before the first use,
 * private to one stream; [0] / [1] are back at zero when the launch ends, [2] != 0 reports a wait that gave up (poll limit). */
int iplan_gat_enc_ac_fwd(const IplanGatFwdArgs* gat, const IplanEncFwdArgs* enc, const IplanAcFwdArgs* ac, int32_t* sync, iplan_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Gumbel(0, 1) samples  g = -log(-log(u)),  u uniform on (0, 1): the noise F.gumbel_softmax draws inside
 * GAT_Net.forward (nova/GAT_Net.py:93, `-empty_like(logits).exponential_().log()`), for a whole rollout in one launch
 * (one pass over `out` instead of the three of the torch expression).  Counter based: out[i] depends on (seed, i) only, so
 * any partition of the range gives the same samples.  n % 4 == 0, out 16-byte aligned.
 */
int iplan_gumbel_noise(float* out, int64_t n, uint64_t seed, iplan_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * clip_grad_norm_ + torch.optim.Adam on flat arenas (learners/ippo_learner.py:204-221,
 * nova/prediction_policy.py:231-241, nova/stable_behavior_policy.py:252-262), all nets per launch.
 */
#define IPLAN_MAX_NETS 16

/* out[net*out_stride + slot] = sum of squares of grad[net*stride + off .. + n) (fixed order). */
int iplan_grad_sqnorm(const float* grad, int64_t stride, int64_t off, int64_t n, int32_t n_nets,
                      float* out, int32_t out_stride, int32_t slot, iplan_stream_t stream);

typedef struct {
    float* param;               /* arena base; net k slice at + k*stride + off, n elements        */
    float* grad;
    float* exp_avg;
    float* exp_avg_sq;
    int64_t stride, off, n;
    int32_t n_nets;
    const float* sqnorm;        /* squared grad norms (iplan_grad_sqnorm output); NULL = no clip  */
    int32_t sqnorm_stride, sqnorm_slot;
    float max_norm;             /* grads scaled by min(1, max_norm / (norm + 1e-6))               */
    int32_t write_clipped;      /* store the clipped gradient back (clip_grad_norm_ is in place)  */
    float lr, beta1, beta2, eps;
    float bc1[IPLAN_MAX_NETS];      /* 1 - beta1^step   per net                                   */
    float bc2_sqrt[IPLAN_MAX_NETS]; /* sqrt(1 - beta2^step)                                       */
    float weight_decay;         /* torch.optim.Adam's L2 form: g <- g + weight_decay * p, after the clip (0 = off) */
} IplanAdamArgs;

int iplan_adam_step(const IplanAdamArgs* args, iplan_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Weight-gradient contraction (the autograd of every nn.Linear / nn.GRU / nn.GRUCell weight on the
 * path: torch's addmm/GRU backward under loss.backward() at nova/prediction_policy.py:228,
 * nova/stable_behavior_policy.py:249, learners/ippo_learner.py:202,216):
 *     dW[o][k] = scale * sum_rows dY[row][ocol(o)] * X[row'][x_col0 + k],   db[o] = scale * sum_rows dY[row][ocol(o)]
 * rows = (outer, inner), outer < n_outer, inner < n_inner;  row' = (outer, inner + x_shift); when
 * inner + x_shift falls outside [0, n_inner) the row x0[outer] is used (zeros if x0 == NULL).
 * ocol(o) = o < seg_split ? seg_c0 + o : seg_c1 + (o - seg_split)  selects the columns of dY.
 * Results are written (beta = 0) or accumulated (beta = 1) into the gradient arena of each net at
 * dw_off + o*dw_ld + dw_col0 + k  /  db_off + o  (offset -1 = not wanted).  Fixed summation order.
 */
#define IPLAN_WGRAD_MAX 16
#define IPLAN_WGRAD_MAX_CHUNKS 128

typedef struct {
    const float* dy;
    int64_t dy_s_net, dy_s_outer, dy_s_inner;
    const float* x;
    int64_t x_s_net, x_s_outer, x_s_inner;
    const float* x0;
    int64_t x0_s_net, x0_s_outer;
    int64_t dw_off, db_off;
    int64_t ws_off;             /* filled by the library */
    int32_t O, K;
    int32_t seg_split, seg_c0, seg_c1;
    int32_t x_col0, x_shift;
    int32_t n_outer, n_inner;
    int32_t dw_ld, dw_col0;
    float beta, scale;
    /* Column-grouped operands (0 = plain rows): column c of dY / X lives at element (c >> 4) * cg_stride + (c & 15) of its row
     * -- the behaviour decoder's records are stored [chain tile][16-column group][step][chain][16] so that a row's 16-column
     * group is contiguous over (step, chain) (rows = (tile, step * 16 + chain), row stride 16).  dY columns are then addressed
     * through seg_c0 / seg_c1 and X columns through x_col0 (not by offsetting the pointers).                                */
    int32_t dy_cg_stride, x_cg_stride;
    /* x_shift < 0 only: the |x_shift| rows in front of every outer index's first row exist in memory (the previous steps of a
     * window range that does not start at step 0) and are read in place instead of x0 / zeros.                              */
    int32_t x_pre_valid;
} IplanWgradProblem;

typedef struct {
    int32_t n_problems, n_nets;
    float* grad;                /* gradient arena base */
    int64_t grad_s_net;
    float* workspace;           /* >= iplan_wgrad_workspace_floats() floats */
    int64_t workspace_floats;
    IplanWgradProblem p[IPLAN_WGRAD_MAX];
} IplanWgradArgs;

size_t iplan_wgrad_workspace_floats(const IplanWgradArgs* args);
int iplan_wgrad(IplanWgradArgs* args, iplan_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Backward of the recurrent actor / critic (autograd of R_Actor.evaluate_actions /
 * R_Critic.forward under learners/ippo_learner.py:202,216).  Launch order:
 *   iplan_ac_fwd(mode 2, saved != NULL) -> loss gradients per row -> iplan_ac_bwd_tail ->
 *   iplan_wgrad problems for the 64-wide layers (host assembles them from `dsave` / `saved`) and
 *   iplan_ac_bwd_fc1 -> iplan_ac_bwd_fc1_finalize (needs fc1.bias' gradient from iplan_wgrad).
 */
#define IPLAN_AC_DSAVE_FLOATS (6 * IPLAN_AC_HIDDEN + 16) /* dz1 | dz2 | dr dz dn_i dn_h | dhead(16) */
#define IPLAN_AC_LNPART_FLOATS (6 * IPLAN_AC_HIDDEN)     /* [rnn.norm w,b | fc2.0.2 w,b | fc1.2 w,b] */

typedef struct {
    IplanAcFwdArgs fwd;         /* the descriptor of the forward launch (mode 2, saved != NULL)        */
    const float* g_logp;        /* [n_agents, rows] dLoss/dlogp                                          */
    const float* g_entropy;     /* [n_agents, rows] dLoss/d(entropy of the row); NULL -> g_entropy_const */
    float g_entropy_const;
    const float* g_values;      /* [n_agents, rows] dLoss/dvalue                                         */
    float* dsave;               /* [2, n_agents, rows, IPLAN_AC_DSAVE_FLOATS]                            */
    float* ln_part;             /* [2, n_agents, ceil(rows/16), IPLAN_AC_LNPART_FLOATS]                  */
    float* g_part;              /* [2, n_agents, fc1_chunks, 64, Kpad] partial G tiles, Kpad = iplan_ac_kpad()  */
    int32_t fc1_chunk_rows;     /* rows per chunk, multiple of 16                                        */
    int32_t fc1_chunks;
    float* actor_grad;          /* gradient arenas (fc1.weight, feature_norm.* are written by finalize)  */
    float* critic_grad;
    int64_t actor_grad_s_net, critic_grad_s_net;
    const float* xb;            /* iplan_ac_bwd_fc1_split only: the row-major-K fragments of iplan_ac_xhat_pack  */
} IplanAcBwdArgs;

/* iplan_ac_pack_fc1: packed[net] = { Wp [KT][4 o-tiles][64 lanes][4] | gamma_p [KT][16] | beta_p [KT][16] | W gamma [64] | W beta [64] },
 * KT = iplan_ac_kpad / 16 (the last two: fc1.weight x feature_norm.{weight, bias}, operands of the folded LayerNorm(F)):
 * Wp[T][oo][lane (n, g)][q] = fc1.weight[16 oo + n][column of k-order position 16 T + 4 g + q] (0 past a block's end).      */
typedef struct {
    int32_t n_nets;
    IplanAcFeatures feat;        /* only N, w[], n_actions, n_id are read                             */
    const float* params;
    int64_t params_s_net, off_w1, off_fn_w, off_fn_b;
    float* packed;
    int64_t packed_s_net;        /* >= iplan_ac_packed_floats(feat)                                   */
    int32_t parts;               /* 0 = everything; 1 = Wp | gamma_p | beta_p only (all the streaming forward of a PPO
                                    epoch reads); 2 = W gamma | W beta only (operands of the rollout's folded form)    */
} IplanAcPackArgs;
int64_t iplan_ac_packed_floats(const IplanAcFeatures* feat);
int iplan_ac_pack_fc1(const IplanAcPackArgs* args, iplan_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * fc1 of the PPO epochs on the bf16 matrix cores (learners/ippo_learner.py:190-221: the 15 epochs evaluate the same stored
 * rows, only the weights move).  The normalised feature rows  xhat = (x - mean) * rstd  (LayerNorm(F) without its affine
 * part, which is folded into the weights:  fc1(LN(x)) = (W o gamma) xhat + W beta + b)  are gathered ONCE per train() into
 * two fp32 fragment-major copies -- `xf` for the forward (K = features), `xb` for the weight gradient (K = rows) -- and every
 * epoch runs
 *    iplan_ac_fc1_split_fwd    z1 = (W o gamma) xhat + W beta     for the actor and the critic of every agent, one pass over xf
 *    iplan_ac_fwd(fc1_pre=z1)  the 64-wide tail
 *    iplan_ac_bwd_fc1_split    G = dz1^T xhat  for both nets, one pass over xb  (then iplan_ac_bwd_fc1_finalize as before)
 * with every fp32 operand split into three bf16 pieces in registers (x = p0 + p1 + p2 exactly) and the six largest piece
 * products accumulated in fp32 on v_mfma_f32_16x16x32_bf16: the result agrees with the fp32 contraction to fp32 round-off.
 * Fragment layouts (KT = iplan_ac_kpad / 16 k-tiles of the source-major feature order, KS = ceil(KT / 2) k-steps of 32):
 *    xf [n_agents, 2 * RB, KS, 64 lanes, 8]   lane (n, g) of row tile t, slot j: xhat[16 t + n][k-tile 2 ks + (j >> 2)][4 g + (j & 3)]
 *    xb [n_agents, RB, KT, 64 lanes, 8]       lane (f, g) of 32-row block b, slot j: xhat[32 b + 8 g + j][k-tile T][f]
 * RB = ceil(rows / 32); rows past `rows` and features past F are zeros.                                                    */
typedef struct {
    int32_t n_agents, rows;
    IplanAcFeatures feat;
    const float* ln_stats;      /* (mean, rstd) per (net, physical row), as iplan_ac_fwd(ln_stats_mode = 1) stored them */
    int64_t ln_stats_s_net;
    float* xf;
    float* xb;
} IplanAcXhatArgs;
int64_t iplan_ac_xhat_floats(const IplanAcFeatures* feat, int32_t rows, int32_t which);   /* per agent: which 0 = xf, 1 = xb */
int iplan_ac_xhat_pack(const IplanAcXhatArgs* args, iplan_stream_t stream);

typedef struct {
    int32_t n_agents, rows;
    IplanAcFeatures feat;        /* only N, w[], n_actions, n_id are read                                               */
    IplanAcNet actor, critic;
    const float* xf;
    void* wsplit;                /* workspace, n_agents * KS * 24576 bytes: the bf16 pieces of W o gamma in fragment order */
    float* wbeta;                /* workspace [2, n_agents, 64]: W beta                                                  */
    float* z1;                   /* out [kparts][2, n_agents, rows, 64]: part p holds the contribution of K-step range p (part 0 + W beta) */
    int32_t kparts;              /* 0 / 1: one part (the whole K loop in one workgroup).  > 1 -- small batches only (<= iplan_ac_fc1_split_parts):
                                    a data-parallel rank's 2 880 rows are 113 workgroups of one 79-step K chain each; the chain is dealt
                                    to `kparts` workgroups and iplan_ac_fwd(fc1_pre, fc1_pre_parts) adds the parts in order            */
} IplanAcFc1SplitArgs;
/* the number of parts the host layer should ask for at this size (1 = the full-buffer shape) */
int iplan_ac_fc1_split_parts(int32_t n_agents, int32_t rows);
int iplan_ac_fc1_split_fwd(const IplanAcFc1SplitArgs* args, iplan_stream_t stream);
/* args->xb set, fwd.which = 2, fc1_chunk_rows a multiple of 32; g_part as for iplan_ac_bwd_fc1.  iplan_ac_fc1_split_chunks:
 * the row chunking that fills the chip once (returns fc1_chunks, writes fc1_chunk_rows). */
int iplan_ac_fc1_split_chunks(const IplanAcFeatures* feat, int32_t n_agents, int32_t rows, int32_t* chunk_rows);
int iplan_ac_bwd_fc1_split(const IplanAcBwdArgs* args, iplan_stream_t stream);

int iplan_ac_kpad(const IplanAcFeatures* feat);   /* padded length of the kernels' source-major feature order */
int iplan_ac_fc1_groups(const IplanAcFeatures* feat); /* wave jobs along the feature axis of iplan_ac_bwd_fc1 (the caller
                                                          sizes fc1_chunks so that groups x chunks x nets fill the chip:
                                                          2048 waves, two per SIMD) */
int iplan_ac_bwd_tail(const IplanAcBwdArgs* args, iplan_stream_t stream);
int iplan_ac_bwd_fc1(const IplanAcBwdArgs* args, iplan_stream_t stream);
int iplan_ac_bwd_fc1_finalize(const IplanAcBwdArgs* args, iplan_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * PPO bookkeeping of IPPOLearner.train (learners/ippo_learner.py).
 * iplan_ppo_prepare: compute_returns (:344-365, GAE) + advantage normalisation (:273-279):
 *   mask_t = 1 - terminated_t;  delta_t = r_t + gamma V_{t+1} mask_{t+1} - V_t;
 *   gae_t = delta_t + gamma lam mask_{t+1} gae_{t+1};  ret_t = gae_t + V_t;
 *   adv = (ret - V) zeroed where mask == 0, then (adv - mean) / (unbiased std + 1e-5) over all bs*T.
 */
typedef struct {
    int32_t n_agents, bs, T;
    const float* reward;         /* reward[net*rw_s_net + b*rw_s_ep + t*rw_s_t], t < T              */
    int64_t rw_s_net, rw_s_ep, rw_s_t;
    const uint8_t* terminated;   /* same addressing, t <= T                                          */
    int64_t tm_s_net, tm_s_ep, tm_s_t;
    const float* values;         /* [n_agents, bs, T+1] critic values of every stored step           */
    float gamma, lam;
    float* returns;              /* [n_agents, bs, T]                                                */
    float* adv;                  /* [n_agents, bs, T] normalised advantages                          */
    float* mask;                 /* [n_agents, bs, T] 1 - terminated                                 */
    float* value_preds;          /* [n_agents, bs, T] = values[:, :, :T]                             */
    int32_t skip_norm;           /* 1 = leave adv un-normalised (data-parallel callers normalise with the
                                    mean / std over ALL ranks' rows between this call and iplan_ppo_loss)      */
    int32_t no_gae;              /* 1 = use_gae False (:360-362): ret_T = V_T, ret_t = ret_{t+1} gamma mask_{t+1} + r_t */
} IplanPpoPrepareArgs;

int iplan_ppo_prepare(const IplanPpoPrepareArgs* args, iplan_stream_t stream);

/* iplan_ppo_adv_norm: the advantage normalisation of ippo_learner.py:276-279 over the rows of ALL data-parallel ranks, in
 * three launches around two sum all-reduces (the caller only moves bytes between them; every arithmetic step is here):
 *   phase 0:  sum[net]   = sum_i adv[net, i]                              (this rank's rows)       -> all-reduce sum
 *   phase 1:  sqdev[net] = sum_i (adv[net, i] - sum[net] / count)^2        (sum = global)           -> all-reduce sqdev
 *   phase 2:  adv[net, i] = (adv[net, i] - mean) / (sqrt(sqdev[net] / (count - 1)) + 1e-5)
 * count = rows of all ranks.  With one rank this reproduces iplan_ppo_prepare's own normalisation.                    */
typedef struct {
    int32_t n_agents, n;         /* n = this rank's rows per agent; 1 <= n <= row_stride (refused otherwise) */
    int64_t row_stride;          /* per-agent stride of adv; entries [n, row_stride) are left alone  */
    float* adv;                  /* [n_agents, row_stride]                                           */
    float* sum;                  /* [n_agents]                                                       */
    float* sqdev;                /* [n_agents]                                                       */
    float count;                 /* rows per agent over all ranks                                    */
    int32_t phase;
} IplanAdvNormArgs;

int iplan_ppo_adv_norm(const IplanAdvNormArgs* args, iplan_stream_t stream);

/* iplan_ppo_loss: ppo_update's losses (:185-197) and cal_value_loss (:128-159) over the first
 * `rows` rows of every agent, plus dLoss/dlogp and d(value_loss_coef * value_loss)/dvalue per row.
 * stats[net][0..4] = policy_loss, value_loss, mean ratio, mean entropy, sum(mask).              */
typedef struct {
    int32_t n_agents, rows;      /* 1 <= rows <= row_stride (refused otherwise)                      */
    int64_t row_stride;          /* per-agent stride of the [n_agents, bs*T] inputs below; their entries
                                    [rows, row_stride) are never read                                */
    const float* logp;           /* [n_agents, rows] current log-probs (iplan_ac_fwd output)         */
    const float* entropy;        /* [n_agents, rows]                                                 */
    const float* values;         /* [n_agents, rows] current values                                  */
    const float* old_logp;       /* [n_agents, row_stride]                                           */
    const float* adv;
    const float* value_preds;
    const float* returns;
    const float* mask;
    float clip, huber_delta, value_loss_coef;
    float* g_logp;               /* [n_agents, rows]                                                 */
    float* g_values;             /* [n_agents, rows]                                                 */
    float* stats;                /* [n_agents, 8]                                                    */
    const float* mask_sum;       /* optional [n_agents]: sum(mask) over the rows of ALL data-parallel ranks -- the
                                    losses' denominator (NULL = this launch's own rows)                        */
    int32_t flags;               /* IPLAN_PPO_* bits below; 0 = config/algs/ippo.yaml as shipped                 */
    float row_count;             /* rows of ALL data-parallel ranks, the denominator of the *_MEAN forms (0 = rows) */
    int32_t n_parts;             /* 0 / 1: one workgroup per agent (stats as above).  P > 1: the rows of an agent are dealt to P
                                    workgroups (contiguous ranges); REQUIRES mask_sum (every workgroup needs the denominator up
                                    front); stats is [n_agents, P, 8] and holds each range's SHARE of the five values -- the caller
                                    adds the P shares (fixed order: reproducible).  22 950 rows: 46.5 -> ~10 us per launch.     */
} IplanPpoLossArgs;
#define IPLAN_PPO_MSE 1          /* use_huber_loss False: e^2 / 2 (:145-147)                                     */
#define IPLAN_PPO_NO_VCLIP 2     /* use_clipped_value_loss False: the unclipped value loss alone (:149-152)      */
#define IPLAN_PPO_VALUE_MEAN 4   /* use_value_active_masks False: plain mean over the rows (:154-157)            */
#define IPLAN_PPO_POLICY_MEAN 8  /* use_policy_active_masks False: plain mean over the rows (:190-196)           */

int iplan_ppo_loss(const IplanPpoLossArgs* args, iplan_stream_t stream);

/* iplan_ppo_eval: how a recorded batch scores under the nets, forward only -- the five statistics of iplan_ppo_loss plus the
 * numbers a PPO user reads first, per agent and per episode step, with no gradient and nothing stepped
 * (IPPOLearner.evaluate).  Inputs are addressed exactly as in IplanPpoLossArgs: the first `rows` rows of every agent are
 * scored, row r = b * T + t; `adv` is the RAW advantage iplan_ppo_prepare(skip_norm = 1) leaves and is normalised HERE as
 * iplan_ppo_prepare normalises it: mean and unbiased std + 1e-5 over ALL row_stride entries of the agent (two passes).
 * With m = mask, ratio = exp(logp - old_logp), sums over the first `rows` rows, S = sum m:
 *   stats[net][ 0.. 4] policy_loss, value_loss, mean ratio, mean entropy, S        (iplan_ppo_loss's definitions, flags included;
 *                                                                                   the value loss is NOT scaled by value_loss_coef)
 *   stats[net][ 5]     approx_kl (k1)    = sum m (old_logp - logp) / S
 *   stats[net][ 6]     approx_kl_k3      = sum m ((ratio - 1) - (logp - old_logp)) / S
 *   stats[net][ 7]     clip_fraction     = sum m [|ratio - 1| > clip] / S
 *   stats[net][ 8, 9]  largest and smallest ratio over the rows with m != 0
 *   stats[net][10]     explained_variance = 1 - Var_m(returns - value_preds) / Var_m(returns), masked population variances taken
 *                      in two passes (NaN or -inf when Var_m(returns) == 0, as the formula gives)
 *   stats[net][11]     value_clip_fraction = sum m [|values - value_preds| > clip] / S
 *   stats[net][12,13]  mean and unbiased std of the raw advantage over the row_stride entries: the normaliser's two numbers
 *   stats[net][14]     sum m returns / S
 *   stats[net][15]     sum m |returns - values| / S
 *   step_stats[net][t][0..5], over the episodes b < rows / T in episode order: live count c = sum_b m, then sum_b m x / c for
 *                      x = raw advantage, |returns - values|, ratio, entropy, [|ratio - 1| > clip]; exact zeros where c == 0.
 * Reduction order (no atomics; every bit of every output is the same for any n_parts and from call to call): the row axis is
 * cut into chunks of IPLAN_PPO_EVAL_CHUNK rows.  A chunk is reduced by one 256-thread workgroup -- a row per thread, fp32
 * xor-butterfly per wave, the four waves added in wave order in fp64 -- into one fp64 partial per quantity in `workspace`;
 * whoever needs a total adds the chunk partials in chunk order in fp64.  Four launches on the stream, a launch boundary
 * between a phase that writes partials and the one that reads them:
 *   1. per chunk: sum adv, S, sum m returns, sum m (returns - value_preds)
 *   2. per chunk, around the means of 1: sum (adv - mean)^2, sum m (returns - mean)^2, sum m (residual - mean)^2
 *   3. per chunk, with S and the advantage's mean / std of 1 and 2: the loss terms, KLs, fractions, extrema; ratio, adv_norm
 *   4. one workgroup per agent adds up -> stats;  one thread per (agent, t) walks b = 0, 1, ... -> step_stats
 * n_parts workgroups per agent take the chunks p, p + n_parts, ...: it changes who computes a chunk, never what is added. */
#define IPLAN_PPO_EVAL_CHUNK 256     /* rows per chunk = threads per workgroup                                     */
#define IPLAN_PPO_EVAL_STATS 16
#define IPLAN_PPO_EVAL_STEP_STATS 6
#define IPLAN_PPO_EVAL_WS 18         /* fp64 workspace slots per (agent, chunk)                                    */
typedef struct {
    int32_t n_agents, rows;
    int64_t row_stride;          /* per-agent stride of the [n_agents, bs*T] inputs below; >= 2, >= rows, < 2^31   */
    const float* logp;           /* [n_agents, rows] current log-probs (iplan_ac_fwd output)                       */
    const float* entropy;        /* [n_agents, rows]                                                               */
    const float* values;         /* [n_agents, rows] current values                                                */
    const float* old_logp;       /* [n_agents, row_stride]                                                         */
    const float* adv;            /* [n_agents, row_stride] RAW advantages, read over all row_stride entries        */
    const float* value_preds;
    const float* returns;
    const float* mask;
    float clip, huber_delta, value_loss_coef;   /* (value_loss_coef: carried with the other two; no statistic uses it) */
    int32_t flags;               /* IPLAN_PPO_* bits                                                               */
    int32_t T;                   /* steps per episode; rows must be a multiple of it                               */
    int32_t n_parts;             /* workgroups per agent, 0 / 1 = one; clamped to the number of chunks and to 1024 */
    float* stats;                /* [n_agents, IPLAN_PPO_EVAL_STATS]                                               */
    float* step_stats;           /* [n_agents, T, IPLAN_PPO_EVAL_STEP_STATS]                                       */
    float* ratio;                /* optional [n_agents, rows]                     (NULL = skip)                    */
    float* adv_norm;             /* optional [n_agents, row_stride] normalised advantages; must not alias adv      */
    void* workspace;             /* iplan_ppo_eval_workspace_bytes(n_agents, row_stride) bytes, 8-byte aligned; scratch */
} IplanPpoEvalArgs;

int64_t iplan_ppo_eval_workspace_bytes(int32_t n_agents, int64_t row_stride);
int iplan_ppo_eval(const IplanPpoEvalArgs* args, iplan_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Backward of GAT_Net.forward (autograd under loss.backward() at nova/prediction_policy.py:228) for
 * every (net, env) scene in one launch: GRUCell', gated soft attention', gumbel gate', BPTT through
 * the bidirectional pair GRU (its recurrent weight / bias gradients accumulated in-kernel), node
 * projections'.  Emits node-level pre-activation gradients; their weight gradients are iplan_wgrad
 * contractions over them (host assembles the problem list).
 * node_dy row layout (floats): ENC 0 (H) | DA_fwd 32 | DB_fwd 128 | DA_rev 224 | DB_rev 320 (3H each)
 *                              | DQ 416 | DK 448 | DV 480 (A each) | CELL 512 (dr dz dn_i dn_h, 4A).
 * hard_part row (per scene): [dir][tile<4][H] partial sums of dDelta * h, then sum(dDelta) at 8H.
 */
#define IPLAN_GAT_NODE_DY 640
#define IPLAN_GAT_HARD_PART (8 * IPLAN_GAT_HIDDEN + 16)
#define IPLAN_GAT_WHH_PART (3 * IPLAN_GAT_HIDDEN * IPLAN_GAT_HIDDEN + 3 * IPLAN_GAT_HIDDEN)   /* dW_hh [3H, H] | db_hh [3H] */

typedef struct {
    IplanGatFwdArgs fwd;        /* descriptor of the forward launch (saved.* all non-NULL)           */
    const float* g_out;         /* dLoss/d out, rows of A floats: (net,b,i)                          */
    int64_t g_s_net, g_s_b;
    float* dgru;                /* scratch [n_nets, 2, B, ceil(N/16), N-1, 2, 3H] (kernel-private)   */
    float* node_dy;             /* [n_nets, B*N, IPLAN_GAT_NODE_DY]                                  */
    float* hard_part;           /* [n_nets, B, IPLAN_GAT_HARD_PART]                                  */
    float* whh_part;            /* scratch [n_nets, B, 2, 4, IPLAN_GAT_WHH_PART]                     */
    float* grad;                /* gradient arena: hard_bi_GRU.weight_hh_l0{,_reverse} and bias_hh_l0{,_reverse} are
                                   WRITTEN here (at fwd.off[...]); all other GAT gradients are iplan_wgrad contractions
                                   over node_dy / hard_part assembled by the host                                    */
    int64_t grad_s_net;
} IplanGatBwdArgs;

int iplan_gat_bwd(const IplanGatBwdArgs* args, iplan_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Prediction_Decoder.forward (nova/prediction_net.py:40-63; DecoderRNN :6-26) + the masked-L1 loss
 * of Prediction_policy.learn (nova/prediction_policy.py:223-225), and their backward.
 * Rows are (sample s, entity i) = s*N + i; hidden size == 32; d <= 16.
 * Parameter tensors of DecoderRNN in state_dict order (also used by the behaviour decoder):
 */
enum {
    IPLAN_DEC_LIN_W = 0,    /* decoder.linear.weight      [Hd, In]   */
    IPLAN_DEC_LIN_B,        /* decoder.linear.bias        [Hd]       */
    IPLAN_DEC_WIH,          /* decoder.rnn.weight_ih_l0   [3Hd, Hd]  */
    IPLAN_DEC_WHH,          /* decoder.rnn.weight_hh_l0   [3Hd, Hd]  */
    IPLAN_DEC_BIH,          /* decoder.rnn.bias_ih_l0     [3Hd]      */
    IPLAN_DEC_BHH,          /* decoder.rnn.bias_hh_l0     [3Hd]      */
    IPLAN_DEC_OUT_W,        /* decoder.out.weight         [d, Hd]    */
    IPLAN_DEC_OUT_B,        /* decoder.out.bias           [d]        */
    IPLAN_DEC_NPARAM
};
#define IPLAN_PDEC_SAVE 256   /* per (row, step): xin 0 (16) | u 16 | r 48 | z 80 | n 112 | hn 144 | h 176 | a 208 (32 each) | y 240 (16) */
#define IPLAN_PDEC_DSAVE 176  /* per (row, step): dy 0 (16) | du 16 | dr 48 | dz 80 | dn_i 112 | dn_h 144 (32 each)                      */

typedef struct {
    int32_t n_nets, rows, N, P, d;
    const float* x0;            /* [n_nets, rows, d]     current state (decoder input of step 0)        */
    const float* h0;            /* [n_nets, rows, 32]    GAT output = initial hidden state              */
    const float* target;        /* [n_nets, rows, P, d]  actual next states                             */
    const float* mask;          /* [n_nets, rows / N]    per-sample mask                                */
    const float* keep;          /* [n_nets, P, rows, 32] dropout keep flags {0,1}; NULL = no dropout    */
    float drop_p;
    const int32_t* teacher;     /* [n_nets, P] 1 = feed the actual state to the next step; NULL = never */
    const float* params;
    int64_t params_s_net;
    int64_t off[IPLAN_DEC_NPARAM];
    float* pred;                /* [n_nets, rows, P, d]                                                 */
    float* saved;               /* [n_nets, rows, P, IPLAN_PDEC_SAVE]                                   */
    float* loss_part;           /* [n_nets, ceil(rows/16)]                                              */
    float* loss;                /* [n_nets]  sum|target-pred|*m / (sum m + 1e-10) * d * P               */
    float* dsave;               /* backward: [n_nets, rows, P, IPLAN_PDEC_DSAVE]                        */
    float* g_h0;                /* backward: [n_nets, rows, 32] dLoss/d h0                              */
    const float* mask_sum;      /* optional [n_nets]: sum(mask) over the samples of ALL data-parallel ranks (the
                                   loss normaliser); NULL = this launch's own samples                       */
} IplanPdecArgs;

int iplan_pdec_fwd(const IplanPdecArgs* args, iplan_stream_t stream);
int iplan_pdec_bwd(const IplanPdecArgs* args, iplan_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Trajectory-prediction inference: Prediction_Decoder.forward(last_state, None, hidden) under .eval()
 * (nova/prediction_net.py:40-63) -- the chain of iplan_pdec_fwd without teacher forcing and without
 * dropout, forward only: nothing is recorded for a backward pass.
 * Rows are (sample s, entity i) = s*N + i; hidden size == 32; d <= 16; n_nets <= IPLAN_MAX_NETS.
 * The start state and the targets are read in place from an episode buffer: the row of entity i of sample s
 * of net n starts at element  offset[n][s] + i * ent_stride  of x0 (the start state) and, for the target of
 * horizon step p < P, at element  offset[n][s] + i * ent_stride + (p + 1) * step_stride  of target; its d
 * features are contiguous.  The caller guarantees that all of these lie inside the buffers.
 * Outputs, each optional (NULL = not wanted; at least one is):
 *   pred     the predicted states
 *   metrics  per (net, step): sum w * ||delta pos||_2 over columns pos_first .. pos_first + pos_count - 1,
 *            sum w * sum_c |delta_c| over all d columns, sum w, with delta = target - pred and
 *            w(row, p) = weight[n][s] * [x0 row's presence column != 0] * [target_p row's presence column != 0]
 *            (the presence factors are dropped when presence_col < 0).  Reduced in a fixed order: per-tile
 *            partials in part, then one pass over the tiles -- bit-identical from launch to launch.
 * Without metrics neither target nor weight is read (target may be NULL).
 */
typedef struct {
    int32_t n_nets, S, N, P, d;
    const float* x0;            /* base of the start states (e.g. the episode buffer's history field)     */
    const float* target;        /* base of the targets (usually == x0); only read with metrics            */
    const int64_t* offset;      /* [n_nets, S] element offset of (sample, entity 0, feature 0)             */
    int64_t ent_stride;         /* elements between entities                                               */
    int64_t step_stride;        /* elements between time steps                                             */
    const float* h0;            /* [n_nets, S*N, 32] GAT output = initial hidden state                     */
    const float* weight;        /* [n_nets, S] sample weights; NULL = 1                                    */
    int32_t presence_col;       /* < 0: no presence factors                                                */
    int32_t pos_first, pos_count;
    const float* params;        /* decoder arena, IPLAN_DEC_* offsets                                      */
    int64_t params_s_net;
    int64_t off[IPLAN_DEC_NPARAM];
    float* pred;                /* [n_nets, S*N, P, d] or NULL                                             */
    float* metrics;             /* [n_nets, P, 3] or NULL                                                  */
    float* part;                /* scratch [n_nets, P, 3, ceil(S*N/16)], needed with metrics               */
} IplanPredictArgs;

int iplan_predict(const IplanPredictArgs* args, iplan_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Behavior_policy.learn, soft update (nova/stable_behavior_policy.py:161-279): the whole episode of
 * every (env, entity) chain of every agent-net in one forward and one backward launch.
 * Encoder parameters: IPLAN_ENC_* (EncoderRNN); decoder parameters: IPLAN_DEC_* of
 * behavior_decoder[i].decoder (DecoderRNN, input d + Z, hidden 64).  rows = E * N, J = T - 1 - L.
 * Per-step records (floats):
 *   saved_dec  [x_t || latent] 0 (d+Z <= 16 cols) | 16 (16, unused) | u 32 | r 96 | z 160 | n 224 | hn 288 | h 352 | a 416 (64 each) | y 480 (16)
 *   saved_enc  u 0 | r 32 | z 64 | n 96 | hn 128 | h 160 (32 each)
 *   dsave_dec  dy 0 (16) | du 16 | dr 80 | dz 144 | dn_i 208 | dn_h 272 (64 each)
 * The three per-step records are stored column-grouped: [n_nets, ceil(rows / 16) chain tiles, columns / 16 groups, J * L steps,
 * 16 chains, 16 floats] -- column c of (chain, step) at group c >> 4, float c & 15.  A wave's access to one 16-column group of
 * its 16 chains is then one contiguous 1 KiB block, and a group's rows are contiguous over (step, chain): the weight-gradient
 * contraction reads them as rows (tile, step * 16 + chain) with IplanWgradProblem.dy_cg_stride / x_cg_stride = J * L * 256.
 * The chain slots of a ragged last tile are never written: the caller zeroes them in the decoder records (nothing reads them in
 * saved_enc, which is stored the same way: 12 groups).
 */
#define IPLAN_BEH_SAVE_DEC 496
#define IPLAN_BEH_SAVE_ENC 192
#define IPLAN_BEH_SAVE_LAT 32        /* per (row, window): softmax output 0 (16) | latent used by the decoder 16 (16) */
#define IPLAN_BEH_DSAVE_DEC 336
#define IPLAN_BEH_DSAVE_LAT 16
#define IPLAN_BEH_DEC_THIN_PART 2144 /* per workgroup of the BPTT's second form: out.weight [16][64] | out.bias [16] | linear.weight [64][16] | linear.bias [64] */
#define IPLAN_BEH_ENC_PART 7408       /* per-wave encoder weight-gradient partial: W_ih 0 | W_hh 3072 | b_ih 6144 | b_hh 6240
                                         | lin.W [32][16] 6336 | lin.b 6848 | out.W [16][32] 6880 | out.b 7392          */

typedef struct {
    int32_t n_nets, E, N, T, L, d, Z;  /* T = stored steps used (= episode_limit)                      */
    const float* hist;          /* x(net,e,t,i,c) = hist[net*h_s_net + e*h_s_e + t*h_s_t + i*d + c]     */
    int64_t h_s_net, h_s_e, h_s_t;
    const float* mask;          /* [n_nets, E, T] loss mask (env-dependent polarity applied by caller)  */
    const uint8_t* keep;        /* [n_nets, J, rows, L, 64] dropout keep flags; NULL = drawn in-kernel  */
    uint64_t seed;              /* seed of the in-kernel counter-based Bernoulli draw                   */
    float drop_p, coef, thres;  /* decoder_dropout, soft_update_coef, thres_small_variation             */
    const float* enc_params;
    int64_t enc_s_net;
    int64_t enc_off[IPLAN_ENC_NPARAM];
    const float* dec_params;
    int64_t dec_s_net;
    int64_t dec_off[IPLAN_DEC_NPARAM];
    float* saved_dec;           /* column-grouped (above): n_nets * ceil(rows/16)*16 * J * L * IPLAN_BEH_SAVE_DEC floats */
    float* saved_enc;           /* column-grouped: n_nets * ceil(rows/16)*16 * J * L * IPLAN_BEH_SAVE_ENC floats       */
    float* saved_lat;           /* [n_nets, rows, J, IPLAN_BEH_SAVE_LAT]  softmax output of window j    */
    float* loss_part;           /* [n_nets, ceil(rows/16), 2]                                           */
    float* loss;                /* [n_nets, 2]  behaviour error, stability error                        */
    float* dsave_dec;           /* backward: column-grouped like saved_dec, IPLAN_BEH_DSAVE_DEC columns               */
    float* dsave_lat;           /* backward: [n_nets, rows, J, IPLAN_BEH_DSAVE_LAT] d(loss)/d(latent_j) through
                                   the decoder inputs of window j (decoder BPTT -> encoder BPTT hand-off) */
    /* single-window decoder mode = Behavior_Latent_Decoder.forward (nova/behavior_net.py:55-69): set T = L + 2 (one
     * window) and pass the window, latent and hidden state explicitly; the encoder and the loss are skipped.     */
    const float* win;           /* [n_nets, rows, L, d] or NULL                                          */
    const float* lat_in;        /* [n_nets, rows, Z]                                                     */
    const float* hd_in;         /* [n_nets, rows, 64]                                                    */
    float* pred_out;            /* [n_nets, rows, L, d]                                                  */
    float* hd_out;              /* [n_nets, rows, 64]                                                    */
    /* hard = 1: the iPLAN-Hard ablation (nova/behavior_policy.py:119-215): non-overlapping windows
     * (window j = steps j*L .. j*L+L-1, J = T/L - 1), the latent is REPLACED by the encoder output, one global
     * normaliser sum(mask[:, :J*L]) for the whole loss and the mask taken at the window's own steps.            */
    int32_t hard;
    float* enc_part;            /* backward: [n_nets, ceil(rows/16), IPLAN_BEH_ENC_PART] per-wave partials */
    float* enc_grad;            /* backward: encoder gradient arena (written at enc_off[])               */
    int64_t enc_grad_s_net;
    int32_t bwd_phase;          /* iplan_beh_bwd: 0 = decoder then encoder, 1 = decoder BPTT only, 2 = encoder BPTT only
                                   (lets the host run the encoder's BPTT on a second stream beside the decoder's
                                   weight-gradient contractions; phase 2 needs phase 1's dsave_lat)               */
    /* BPTT in pieces (bwd_phase 1 or 2): windows [bwd_j_lo, bwd_j_hi) only, processed from the top down;
     * bwd_j_hi == 0 means all windows.  A piece that does not end at window 0 leaves d(loss)/d(h) of its last
     * step in dec_carry (decoder) / enc_carry (encoder, plus d(loss)/d(latent)), the next piece (bwd_j_hi = the
     * previous bwd_j_lo) picks it up -- so the weight-gradient contraction of the rows a decoder piece produced and
     * the encoder piece of the same windows can run beside the next decoder piece.  Encoder pieces accumulate
     * their weight-gradient partials in enc_part; the piece with bwd_j_lo == 0 reduces them into enc_grad.      */
    int32_t bwd_j_lo, bwd_j_hi;
    float* dec_carry;           /* [n_nets, ceil(rows/16), 2, 512]; needed when the decoder runs in pieces */
    /* The forward in pieces, same idea (the encoder of the next windows runs beside the decoder of the current
     * ones): fwd_phase 0 = encoder, decoder and loss reduction; 1 = encoder only; 2 = decoder only; 3 = loss
     * reduction only.  Windows [fwd_j_lo, fwd_j_hi), bottom up; fwd_j_hi == 0 means all.  Hidden states / latent
     * cross the pieces in enc_carry [n_nets, ceil(rows/16), 768] and dec_carry; loss partials accumulate.      */
    int32_t fwd_phase, fwd_j_lo, fwd_j_hi;
    float* enc_carry;
    const float* win_norm;      /* optional [n_nets, J]: per window, sum of the mask over the window's target steps and
                                   the envs of ALL data-parallel ranks (hard update: the one global sum, repeated);
                                   NULL = summed in-kernel over this launch's envs                              */
    float enc_grad_beta;        /* backward: enc_grad = enc_grad_beta * enc_grad + sum of the wave partials (1 = accumulate
                                   over several launches on disjoint env chunks, 0 = overwrite)                  */
    float penalty;              /* backward: behavior_variation_penalty -- weight of the stability term
                                   mean_j sum_{chain, t} max(||x_t - y_t||_2 - thres, 0) / (E_norm L) in the differentiated loss
                                   (nova/stable_behavior_policy.py:238-246); 0 = the shipped configuration       */
    int32_t E_norm;             /* envs the stability term is averaged over (all chunks / ranks); 0 = E           */
    /* Round 4 (decoder BPTT, second form): the THIN decoder weight gradients -- out.weight / out.bias (d x 64) and
     * linear.weight / linear.bias (64 x (d + Z)) -- accumulated IN the BPTT kernel (its waves hold dy, the output-layer input
     * and the Linear's gradient in registers) instead of from row gradients by iplan_wgrad: dec_thin_part != NULL switches it
     * on, the kernel then does NOT store the dy / du columns of dsave_dec, window-range pieces accumulate in the partials, and
     * the piece with bwd_j_lo == 0 reduces them (workgroup order: reproducible) into dec_grad at dec_off[] as
     * dec_grad_beta * old + sum.  Only the second form supports it (iplan_beh_bwd fails if it cannot run that form).   */
    float* dec_thin_part;       /* [n_nets, ceil(ceil(rows/16) / 3), IPLAN_BEH_DEC_THIN_PART] or NULL              */
    float* dec_grad;            /* decoder gradient arena                                                          */
    int64_t dec_grad_s_net;
    float dec_grad_beta;
    int32_t fwd_skip_act;       /* forward (second form): do not store the output layer's input (record columns 416..479) --
                                   only the out.weight contraction of iplan_wgrad reads it, and with dec_thin_part the BPTT
                                   re-forms it from the hidden state it holds anyway: 64 of the 480 floats a chain-step stores */
} IplanBehArgs;

int iplan_beh_fwd(const IplanBehArgs* args, iplan_stream_t stream);
int iplan_beh_bwd(const IplanBehArgs* args, iplan_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Behaviour-model inference: the chain of iplan_beh_fwd (soft update) without dropout, forward only -- nothing is
 * recorded for a backward pass, no seed is consumed.  Every (env, entity) chain of every agent-net starts with
 * latent = 0, encoder hidden = 0, decoder hidden = 0 and walks the windows j < J = T - 1 - L:
 *   curr = steps j-L+1 .. j (right-aligned, zero-padded), next = steps j+1 .. j+L
 *   recon_j = Linear(tanh(GRU64(ReLU(Linear([curr_t, latent_{j-1}]))))),  decoder hidden carried across windows
 *   latent_j = (1 - coef) latent_{j-1} + coef softmax(out(GRU32(ReLU(Linear(curr_t))))),  encoder hidden carried
 * rows = E * N; d >= 1, Z >= 1, d + Z <= 16; L >= 1; J >= 1; n_nets <= IPLAN_MAX_NETS.  The history is read in place
 * through its net / env / step strides (IplanBehArgs' layout).
 * Outputs, each optional (NULL = not wanted; at least one is):
 *   latent  the latent after window j's update
 *   recon   the decoder's output
 *   sums    per (net, window j, look-ahead step t):  sum_rows mask[e, j+1+t] * sum_c |next - recon|  and
 *           sum_rows max(||curr - recon||_2 - thres, 0).  Reduced in a fixed order: per-tile partials in part, then one
 *           pass over the tiles -- bit-identical from launch to launch, no floating-point atomics.
 * Without sums neither the next steps nor mask are read (mask and part may be NULL).
 */
typedef struct {
    int32_t n_nets, E, N, T, L, d, Z;
    const float* hist;          /* x(net,e,t,i,c) = hist[net*h_s_net + e*h_s_e + t*h_s_t + i*d + c]      */
    int64_t h_s_net, h_s_e, h_s_t;
    const float* mask;          /* [n_nets, E, T]; only read with sums                                   */
    float coef, thres;          /* soft_update_coef, thres_small_variation                               */
    const float* enc_params;    /* encoder arena, IPLAN_ENC_* offsets                                    */
    int64_t enc_s_net;
    int64_t enc_off[IPLAN_ENC_NPARAM];
    const float* dec_params;    /* decoder arena, IPLAN_DEC_* offsets                                    */
    int64_t dec_s_net;
    int64_t dec_off[IPLAN_DEC_NPARAM];
    float* latent;              /* [n_nets, rows, J, Z] or NULL                                          */
    float* recon;               /* [n_nets, rows, J, L, d] or NULL                                       */
    float* sums;                /* [n_nets, J, L, 2] or NULL                                             */
    float* part;                /* scratch [n_nets, J, L, 2, ceil(rows/16)], needed with sums            */
} IplanBehEvalArgs;

int iplan_beh_eval(const IplanBehEvalArgs* args, iplan_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Intent saliency: the derivative of the intent latent with respect to the RAW history, by BPTT through the encoder chain
 * iplan_beh_eval walks (no decoder is involved):
 *   he_{-1} = 0, lat_{-1} = 0;  window j < J = T - 1 - L:  h = he_{j-1};  t < L:  s = j-L+1+t, x~ = x_s (0 where s < 0),
 *   u = ReLU(W_lin x~ + b_lin), h = GRU32(u, h);  he_j = h, p_j = softmax(W_out he_j + b_out), lat_j = (1 - coef) lat_{j-1} + coef p_j
 * For every chain (net, row = e*N + i) and every target window j = windows[w], w < nW (sorted, distinct, in [0, J)):
 *   y = <v, lat_j>,  v = seed[net, row, w, :] or, with seed == NULL, the one-hot of seed_index (>= 0) or of the chain's own
 *   argmax_z lat_j (seed_index == -1; lowest index on ties);
 *   windows j - Kj .. j are unrolled, Kj = min(K, j); he_{j-Kj-1} and lat_{j-Kj-1} are constants (both 0 when Kj == j: the result is
 *   then the exact total derivative);   G[r, c] = d y / d x_{j-r, c},  r < R = K + L  (a step read by several windows: the sum).
 * G[r] is 0.0 where j - r < 0 (zero padding) and where r > Kj + L - 1.  rows = E * N; 1 <= d <= 16, 1 <= Z <= 16;
 * 1 <= L <= IPLAN_ENC_SAL_MAX_L; J >= 1; K >= 0; nW >= 1; n_nets <= IPLAN_MAX_NETS.  Outputs, each optional (at least one is asked for):
 *   grad         [n_nets, rows, nW, R, d]   G
 *   step_l1      [n_nets, rows, nW, R]      sum_c |G[r, c]|
 *   step_gxi     [n_nets, rows, nW, R]      sum_c G[r, c] x_{j-r, c}
 *   feature_l1   [n_nets, rows, nW, d]      sum_r |G[r, c]|, r ascending
 *   carry_l2     [n_nets, rows, nW]         || d y / d he_{j-Kj-1} ||_2; 0.0 where Kj == j
 *   latent       [n_nets, rows, nW, Z]      lat_j
 *   target_index [n_nets, rows, nW] int32   the component the one-hot v selects (seed == NULL only)
 *   active       [n_nets, rows, nW, K+1, L] uint32: bit m = unit m of the input Linear has u > 0 at window j - k, position t, as the
 *                backward pass recomputed it; 0 where k > Kj
 * Two passes: a forward walk over windows 0 .. max(windows) that keeps he_j and the argmax in `scratch`, then one wave per (16-chain
 * tile, target window) that walks windows j .. j - Kj backwards, restarting each from he_{w-1} and recomputing the gates; a step's
 * gradient is complete once the window that ends at it has been walked, so at most L rows are pending at a time (in LDS).
 * scratch: at least 32 * n_nets * rows * (max(windows) + 1) + n_nets * rows * nW floats, 16-byte aligned -- it does not grow with K.
 * No atomics, no cross-chain sums: a slot's bits do not depend on its lane, tile, workgroup or on the other entries of `windows`;
 * two launches give the same bits; padding lanes of a ragged last tile write nothing; parameters and history are only read.
 * With Z == 1 every gradient and the carry are exactly 0.0 (the softmax is constant).
 */
#define IPLAN_ENC_SAL_MAX_L 30      /* the window's L hidden states and L pending rows of one wave beside the weights in LDS */
typedef struct {
    int32_t n_nets, E, N, T, L, d, Z, K, nW;
    const float* hist;          /* x(net,e,t,i,c) = hist[net*h_s_net + e*h_s_e + t*h_s_t + i*d + c]      */
    int64_t h_s_net, h_s_e, h_s_t;
    const int32_t* windows;     /* [nW] device memory                                                    */
    const int32_t* windows_host;/* the same values in host memory (argument checks, grid size)           */
    const float* seed;          /* [n_nets, rows, nW, Z] or NULL                                         */
    int32_t seed_index;         /* seed == NULL: -1 = argmax of lat_j, >= 0 = that component             */
    float coef;                 /* soft_update_coef                                                      */
    const float* enc_params;    /* encoder arena, IPLAN_ENC_* offsets                                    */
    int64_t enc_s_net;
    int64_t enc_off[IPLAN_ENC_NPARAM];
    float* scratch;
    int64_t scratch_floats;
    float* grad;
    float* step_l1;
    float* step_gxi;
    float* feature_l1;
    float* carry_l2;
    float* latent;
    int32_t* target_index;
    uint32_t* active;
} IplanEncSaliencyArgs;

int iplan_enc_saliency(const IplanEncSaliencyArgs* args, iplan_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Intent knock-out through time: the finite change of the intent latent when the encoder does not see some steps of the RAW
 * history, on the chain iplan_enc_saliency differentiates (stated above; no decoder is involved).  With J = T - 1 - L, for every
 * chain (net, row = e*N + i) and every job q < Q with start s = starts[q] (sorted, distinct, in [0, J)):
 *   the columns c with bit c of col_mask set, of steps s .. s+D-1, are replaced by baseline[net, c] (0.0 with baseline == NULL) or,
 *   with hold == 1, by the chain's own x_{s-1, c} (0.0 when s == 0);  the knocked chain starts from the base chain's he_{s-1},
 *   lat_{s-1} (zeros when s == 0) and walks windows s + h, h < H.  Windows s + h >= J do not exist: their slots are NOT written.
 * rows = E * N; 1 <= d <= 16, 1 <= Z <= 16; 1 <= L <= IPLAN_ENC_SAL_MAX_L; J >= 1; Q, D, H >= 1; n_nets <= IPLAN_MAX_NETS;
 * Jn = min(J, starts[Q-1] + H).  Outputs (latent is required, every other one optional):
 *   latent          [n_nets, rows, Jn, Z]       lat_j of the base chain, the bits iplan_beh_eval's latent has on [0, Jn)
 *   intent_base     [n_nets, rows, Jn] int32    argmax_z lat_j, lowest index on ties
 *   latent_ko       [n_nets, rows, Q, H, Z]     the knocked chain's latent after window s + h: the bits iplan_beh_eval gives on an
 *                                               explicitly modified copy of the history
 *   hidden_ko       [n_nets, rows, Q, H, 32]    the knocked chain's he after window s + h
 *   intent          [n_nets, rows, Q, H] int32  argmax_z of latent_ko
 *   latent_shift_sq [n_nets, rows, Q, H]        sum_z (lat_ko - lat)^2, z ascending, one lane per chain, every difference, product and
 *   state_shift_sq  [n_nets, rows, Q, H]        sum rounded on its own (the plain fp32 host loop's bits); the same over the 32 units of he
 * Two kernels: the base walk over windows 0 .. Jn-1 (one wave per 16-chain tile), which records every he_j in `workspace`, then -- when
 * a per-job output is asked for -- one wave per (tile, job).  The history is read in place through its strides and never copied.
 * workspace: at least 32 * n_nets * rows * Jn floats, 16-byte aligned.
 * No atomics, no cross-chain sums: a slot's bits do not depend on its lane, tile, workgroup, on Q or on the other entries of `starts`;
 * two launches give the same bits; padding lanes of a ragged last tile write nothing; parameters and history are only read.
 */
typedef struct {
    int32_t n_nets, E, N, T, L, d, Z, Q, D, H;
    const float* hist;          /* x(net,e,t,i,c) = hist[net*h_s_net + e*h_s_e + t*h_s_t + i*d + c]      */
    int64_t h_s_net, h_s_e, h_s_t;
    const int32_t* starts;      /* [Q] device memory                                                     */
    const int32_t* starts_host; /* the same values in host memory (argument checks, Jn)                  */
    uint32_t col_mask;          /* bit c: column c is replaced; at least one, none at or beyond d        */
    int32_t hold;               /* 1: the replacement is the chain's own row of step s-1                 */
    const float* baseline;      /* [n_nets, d] or NULL (zeros); NULL with hold                           */
    float coef;                 /* soft_update_coef                                                      */
    const float* enc_params;    /* encoder arena, IPLAN_ENC_* offsets                                    */
    int64_t enc_s_net;
    int64_t enc_off[IPLAN_ENC_NPARAM];
    float* workspace;
    int64_t workspace_floats;
    float* latent;
    int32_t* intent_base;
    float* latent_ko;
    float* hidden_ko;
    int32_t* intent;
    float* latent_shift_sq;
    float* state_shift_sq;
} IplanEncKnockoutArgs;

int iplan_enc_knockout(const IplanEncKnockoutArgs* args, iplan_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Attention inspection: GAT_Net.forward walked over S >= 1 consecutive steps in one launch, forward only,
 *   h_s = GAT([src0_s || src1_s], h_{s-1}),   s = 0 .. S-1,   h_{-1} = hidden0 (NULL: zeros),
 * one workgroup per (net, env) scene; a step's arithmetic is the inference form of iplan_gat_fwd (nothing saved), so the
 * latents are the ones S successive iplan_gat_fwd launches give.  src0 / src1 are read in place: element (net, b, s, i, c) at
 * src + net*s_net + b*s_b + s*s_step + i*d + c (views of [E, S, nA, N, .] episode fields).
 * Outputs, each optional (NULL = not wanted; at least one is), element (net, b, s) at base + net*s_net + b*s_b + s*s_step:
 *   latent            [N, A]  the attention latent after step s
 *   soft, hard, attn  [N, N]  ENTITY-indexed maps: [i, j] = softmax weight / gumbel gate / their product that ego i gives
 *                             entity j (slot j - [j > i] of the backward record's [N, N-1] layout); the diagonal is written as 0
 *   stats             [n_nets, B, S, 6] contiguous: the scene-step's own sums, with pres(i) = src0 column presence_col of entity i
 *                     is non-zero at step s (presence_col < 0: every entity), w = weight[net, b, s] (NULL: 1):
 *                       [0] w * #{i pres}                         [1] w * #{(i, j): i pres, j != i, j pres}
 *                       [2] w * sum over those pairs of hard      [3] w * sum over those pairs of soft * hard
 *                       [4] w * sum over those pairs of soft      [5] w * sum_{i pres} -sum_{j != i} soft log soft  (0 log 0 = 0)
 *                     summed inside the workgroup in a fixed order, no atomics: bit-identical from launch to launch.
 * noise: gumbel samples [n_nets, B, S, N, N-1, 2] contiguous, or NULL = none (the deterministic gate sigmoid((l1 - l0) / tau)).
 * hidden0 and latent: 16-byte aligned, strides % 4 == 0.  2 <= N <= IPLAN_MAX_ENTITIES.
 */
#define IPLAN_GAT_TRACE_NSTAT 6
typedef struct {
    int32_t n_nets, B, N, d0, d1, S;
    const float* src0;
    int64_t src0_s_net, src0_s_b, src0_s_step;
    const float* src1;          /* may be NULL iff d1 == 0                                                 */
    int64_t src1_s_net, src1_s_b, src1_s_step;
    const float* hidden0;       /* rows of A floats: (net, b, i) at hidden0 + net*h_s_net + b*h_s_b + i*A; or NULL */
    int64_t h_s_net, h_s_b;
    const float* noise;
    const float* params;        /* parameter arena, IPLAN_GAT_* offsets                                    */
    int64_t params_s_net;
    int64_t off[IPLAN_GAT_NPARAM];
    float tau;
    int32_t presence_col;
    const float* weight;        /* [n_nets, B, S] or NULL                                                  */
    float* latent;
    int64_t lat_s_net, lat_s_b, lat_s_step;
    float* soft;
    int64_t soft_s_net, soft_s_b, soft_s_step;
    float* hard;
    int64_t hard_s_net, hard_s_b, hard_s_step;
    float* attn;
    int64_t attn_s_net, attn_s_b, attn_s_step;
    float* stats;
} IplanGatTraceArgs;

int iplan_gat_trace(const IplanGatTraceArgs* args, iplan_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Policy inspection: R_Actor / R_Critic (the comment above IplanAcNet) walked over S >= 1 consecutive steps of E >= 1 recorded
 * chains in one call, forward only, with the GRU state carried by the nets under inspection:
 *   h_s = GRU(trunk(x_s), h_{s-1}),   s = 0 .. S-1,   h_{-1} = hidden0 (NULL: zeros),   results of step s from LN(h_s) -> head.
 * Row r = e*S + s (chain e, step s) is described by `feat` exactly as for iplan_ac_fwd (feat.T must equal S, so the row sits at
 * physical row e*T_phys + s); its last action comes from feat.last_action / last_action64 (-1: all zeros), i.e. it is teacher-forced
 * from the batch, so everything in front of the recurrent matrix is row-parallel.  One call enqueues two kernels on the stream:
 *   phase 1 (trunk)  every net, every row: LN(F) (two passes), fc1 on v_mfma_f32_16x16x4_f32, act, LN, fc2, act, LN and
 *                    gi = W_ih x + b_ih -> `gi`, a caller-provided workspace [2 (actor | critic), n_agents, E*S, IPLAN_AC_TRACE_GI];
 *   phase 2 (walk)   one workgroup per 16-chain tile of one net steps s = 0 .. S-1 with W_hh in registers: W_hh h + b_hh, the gates,
 *                    LN, head, masked softmax.
 * which: 0 = actors, 1 = critics, 2 = both.  hidden0_*: rows of 64 floats at hidden0 + net*h0_s_net + e*h0_s_chain.  avail and
 * actions_in are addressed by physical row as in IplanAcFwdArgs (avail NULL = all available).  packed_*: optional fc1 operands as
 * iplan_ac_pack_fc1 leaves them (parts 0 or 1 suffice), NULL = read the arena in place; both give the same bits.
 * Outputs, each optional (NULL = skip) and contiguous [n_agents, E, S, ...]:
 *   probs   [.., n_actions]  unavailable actions exactly 0 (the masking of iplan_ac_fwd)
 *   entropy, logp            as iplan_ac_fwd's entropy / logp of actions_in (mode 2); logp needs actions_in
 *   greedy  int64            argmax of the row's own probs, lowest index on ties (mode 0 of iplan_ac_fwd)
 *   values                   critic head
 *   h_all_actor, h_all_critic  [.., 64]  the state after every step
 * and always h_last_actor / h_last_critic [n_agents, E, 64] (of the nets `which` selects): the state after step S-1, which a
 * following call takes as hidden0 -- a walk split into several calls gives the bits of the single call.
 * fp32 throughout, fixed reduction order, no atomics: a row's results do not depend on the lane or tile its chain falls in, on how
 * many chains share the tile, or on the split into calls.  1 <= n_actions <= 16, N <= IPLAN_MAX_ENTITIES; gi, the state outputs
 * and the packed operands 16-byte aligned.  phases: 0 = both kernels; 1 = phase 1 only, 2 = phase 2 only (gi as a previous call
 * left it) -- a timing aid for the phase split, nothing else uses it.
 */
#define IPLAN_AC_TRACE_GI (3 * IPLAN_AC_HIDDEN)
typedef struct {
    int32_t n_agents, E, S;
    int32_t which;
    int32_t act_tanh;           /* MLPBase activation: 0 = ReLU, 1 = tanh                                  */
    int32_t phases;
    IplanAcFeatures feat;
    IplanAcNet actor, critic;
    const float* hidden0_actor;
    const float* hidden0_critic;
    int64_t h0_s_net, h0_s_chain;
    const int32_t* avail;
    int64_t av_s_net, av_s_row;
    const int64_t* actions_in;
    int64_t act_s_net, act_s_row;
    const float* packed_actor;
    const float* packed_critic;
    int64_t packed_s_net;
    float* gi;
    float* probs;
    float* entropy;
    int64_t* greedy;
    float* logp;
    float* values;
    float* h_all_actor;
    float* h_all_critic;
    float* h_last_actor;
    float* h_last_critic;
} IplanAcTraceArgs;

int iplan_ac_trace(const IplanAcTraceArgs* args, iplan_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Policy saliency: the gradient of an actor's log-probability and of a critic's value with respect to the INPUT row
 *   x = [ per entity: hist || att || beh ] || onehot(last action) || onehot(agent)      (the comment above IplanAcNet)
 * for E*S independent rows in one launch, forward + input-backward.  Row r = e*S + s is described by `feat` as for iplan_ac_trace
 * (feat.T must equal S; features at physical row e*T_phys + s; last action from feat.last_action / last_action64, -1 = none).  The
 * row's GRU state is GIVEN -- 64 floats at h + net*hs_net + e*hs_chain + s*hs_step -- and held constant: nothing is differentiated
 * through time.  Differentiated is
 *   actor   y = log_softmax(masked logits)[a*]   masked logits are the constant -1e10 and carry no gradient; a* = the row's entry of
 *               `target` (target[net*tg_s_net + e*tg_s_chain + s*tg_s_step]; NULL: target_all for every row), or the row's own
 *               argmax -- lowest index on ties, as iplan_ac_trace's greedy -- where that entry is -1.  target_all is checked on the
 *               host against [-1, n_actions); the entries of `target` live on the device: one outside [0, n_actions) is read as -1.
 *   critic  y = V
 * back through head, LN, the GRU cell with respect to its input only (d gi -> W_ih^T), LN, act', fc2^T, LN, act', fc1^T and the
 * whole LayerNorm(F):  dx = (g^ - mean g^ - x^ mean(g^ x^)) / sigma,  g^ = gamma * (W1^T delta).  One wave per 16-row tile, four
 * tiles per workgroup; fc1 and fc1^T on v_mfma_f32_16x16x4_f32; the F axis is passed over five times (mean, variance, fc1, the two
 * means of g^, dx) with W1^T delta recomputed in the last pass -- nothing F-wide is kept.  avail: int32 at avail + net*av_s_net +
 * e*av_s_chain + s*av_s_step (NULL = all available).  packed_*: as in IplanAcTraceArgs (same bits as the arena in place).
 * Outputs, each optional (NULL = not written), contiguous, of the nets `which` selects; at least one must be asked for:
 *   logp, values  [n_agents, E*S]            y of the actors / the critics
 *   target_out    [n_agents, E*S] int64      the a* that was used
 *   entity_*      [n_agents, E*S, N, n_src, 2]   per entity and ENABLED source (w[k] > 0, in order): sum_k g_k x_k and sum_k |g_k|
 *                                            over the source's w[k] columns of that entity, added one by one in column order
 *   input_grad_*  [n_agents, E*S, F]         the whole gradient in the reference's entity-major column order, one-hots included
 *   act1_*, act2_* [n_agents, E*S, 64]       the two post-activation tiles of the trunk (the ReLU branch taken; for tests)
 * No atomics, no cross-row sums: a row's results do not depend on the lane, tile or workgroup it falls in.  Parameter and gradient
 * memory is only read.  N <= IPLAN_MAX_ENTITIES, 1 <= n_actions <= 16; act1 / act2 and the packed operands 16-byte aligned.
 */
typedef struct {
    int32_t n_agents, E, S;
    int32_t which;              /* 0 = actors, 1 = critics, 2 = both                                       */
    int32_t act_tanh;           /* MLPBase activation: 0 = ReLU, 1 = tanh                                  */
    int32_t target_all;         /* used when target == NULL: -1 = greedy, else one action for every row    */
    IplanAcFeatures feat;
    IplanAcNet actor, critic;
    const float* h_actor;
    const float* h_critic;
    int64_t hs_net, hs_chain, hs_step;
    const int32_t* avail;
    int64_t av_s_net, av_s_chain, av_s_step;
    const int64_t* target;
    int64_t tg_s_net, tg_s_chain, tg_s_step;
    const float* packed_actor;
    const float* packed_critic;
    int64_t packed_s_net;
    float* logp;
    float* values;
    int64_t* target_out;
    float* entity_actor;
    float* entity_critic;
    float* input_grad_actor;
    float* input_grad_critic;
    float* act1_actor;
    float* act2_actor;
    float* act1_critic;
    float* act2_critic;
} IplanAcSaliencyArgs;

int iplan_ac_saliency(const IplanAcSaliencyArgs* args, iplan_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Policy saliency through time (BPTT over the recurrent state): d y_s / d x_{s-k}, the sensitivity of the output of step s to the
 * inputs of step s - k, for every slot (e, s) of E chains x S consecutive steps; one launch is ONE lag k for all slots, agents and
 * selected nets.  `base` describes the rows exactly as for iplan_ac_saliency, with the state ENTERING step s of chain e at
 * h + net*hs_net + e*hs_chain + s*hs_step -- the caller's self-consistent chain, h_s = GRU(trunk(x_s), h_{s-1}) before rnn.norm (what
 * iplan_ac_trace's h_all_* holds, shifted by one step behind hidden0).  Slot r = e*S + s:
 *   lag == 0   iplan_ac_saliency's arithmetic, bit for bit (head seed, target / avail handling, logp / values / target_out / act1 / act2
 *              [n_agents, E*S, ..] as there), and additionally
 *                carry = delta^(0) = d y_s / d h_{s-1} = z * d y / d h' + W_hh^T [dr | dz | r * dn]
 *   lag k >= 1 the slot reads the input row, the last action and the entering state of step s - k, and takes seed = delta^(k-1) of the
 *              SAME slot as d y_s / d h_{s-k} at the GRU output: no rnn.norm, head or softmax, nothing of logp / values / target_out /
 *              act1 / act2 is written.  It writes the lag-k gradient and carry = delta^(k) = (d h_{s-k} / d h_{s-k-1})^T seed.
 *              Slots with s < k write NOTHING.
 * entity_* and input_grad_* carry a lag axis of n_lags entries: [n_agents, E*S, n_lags, N, n_src, 2] and [n_agents, E*S, n_lags, F];
 * this launch writes entry `lag` of it.  seed_* / carry_*: 64 floats per slot at ptr + (net*E*S + r) * seed_s_row / carry_s_row; a
 * slot reads its seed before it writes its carry and touches no other slot's, so seed and carry may be the same memory (in place) or
 * two entries of one [.., n_lags, 64] buffer.  carry_* may be NULL only when lag + 1 == n_lags (nothing follows).
 * Determinism and memory rules of iplan_ac_saliency: no atomics, no cross-row sums, a slot's results do not depend on its lane, tile or
 * workgroup; parameter, gradient and batch memory is only read.  0 <= lag < n_lags <= S; seed, carry, act1 / act2 and the packed
 * operands 16-byte aligned, seed_s_row and carry_s_row multiples of 4.
 */
typedef struct {
    IplanAcSaliencyArgs base;
    int32_t lag, n_lags;
    const float* seed_actor;    /* lag >= 1: delta^(lag-1) of the nets `base.which` selects                   */
    const float* seed_critic;
    int64_t seed_s_row;
    float* carry_actor;         /* delta^(lag)                                                             */
    float* carry_critic;
    int64_t carry_s_row;
} IplanAcSaliencyLagArgs;

int iplan_ac_saliency_lag(const IplanAcSaliencyLagArgs* args, iplan_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Three-layer perceptron of the FC behaviour ablation (nova/behavior_FC_net.py:6-37, Encoder_3FC / Decoder_3FC):
 *   out = [softmax] (W3 tanh(W2 tanh(W1 x + b1) + b2) + b3)   for n_nets stacked nets, rows per net.
 * off[0..5] = linear_1.weight [H,K0], linear_1.bias, linear_2.weight [H,H], linear_2.bias, out.weight [O,H], out.bias.
 * Forward: writes out, saved = [tanh1 (H) | tanh2 (H)] per row and, when `target` is given, the per-wave sums of
 * |target - out| (L1 loss numerator) in loss_part [n_nets, 4 * ceil(rows/64)].
 * Backward: d(out) = g_out, or -sign(target - out) * g_scale when g_out is NULL; writes dsave = [d pre1 (H) | d pre2 (H) |
 * d pre3 (16 * ceil(O/16))] per row (operands of iplan_wgrad) and dx [n_nets, rows, K0] if not NULL.
 */
typedef struct {
    int32_t n_nets, K0, H, O, softmax;
    int64_t rows;
    const float* x;             /* [n_nets, rows, K0]                                                   */
    const float* params;
    int64_t params_s_net;
    int64_t off[6];
    float* out;                 /* [n_nets, rows, O]                                                    */
    float* saved;               /* [n_nets, rows, 2H] (forward: optional)                               */
    const float* target;        /* [n_nets, rows, O] or NULL                                            */
    float* loss_part;
    const float* g_out;         /* backward: [n_nets, rows, O] or NULL                                  */
    float g_scale;
    float* dsave;               /* backward: [n_nets, rows, 2H + 16*ceil(O/16)]                         */
    float* dx;                  /* backward: [n_nets, rows, K0] or NULL                                 */
} IplanMlp3Args;

int iplan_mlp3_fwd(const IplanMlp3Args* args, iplan_stream_t stream);
int iplan_mlp3_bwd(const IplanMlp3Args* args, iplan_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * nova/Seq2Seq.py:41-70 -- Seq2Seq.forward (encoder GRU over the input sequence from a zero state, then pred_length
 * autoregressive decoder steps  y_t = Linear(Dropout(tanh(GRU(y_{t-1}, h))))  from last_location, optionally teacher forced).
 * nn.GRU semantics, batch_first, `layers` stacked layers (1..4) of width H in {32, 64}; rows = N*V.  Inference only.
 * enc_off / dec_off: per layer l  [4l + 0..3] = weight_ih_l<l> [3H, In_l], weight_hh_l<l> [3H, H], bias_ih_l<l>, bias_hh_l<l>
 * (In_0 = input_size for the encoder, output_size for the decoder; In_l = H above); lin_off = decoder.linear.weight [O, H], .bias.
 * Alignment: `params` is 16-byte aligned and every weight_hh offset (enc_off / dec_off [4l + 1], l < layers) is a multiple of 4 floats
 * -- their fragments are unconditional 16-byte loads; refused otherwise.  Every other offset, and the base of x, last, teacher, keep,
 * out, hidden_out, save, g_out and dsave, needs only the 4 bytes of a float: where an address is not 16-byte aligned the kernels take
 * their scalar path and move the same values.  Offsets are not range-checked against the block.
 * Refused with IPLAN_EINVAL (both entry points check the forward's descriptor alike): dims outside 1 <= In <= 64, 1 <= O <= 16,
 * H in {32, 64}, 1 <= layers <= 4, rows, T_in, P >= 1; a NULL x, last, params or out (the backward: save, params, g_out, dsave);
 * `keep` with drop_p outside [0, 1) or NaN; `teacher` without `coins` or `coins` without `teacher`.
 * Not refused: drop_p is ignored (any value) when `keep` is NULL; teacher[:, t] is read only where coins[t] != 0, and the cell of the
 * last step feeds nothing; nothing behind the last row of any tensor is read or written.
 */
#define IPLAN_S2S_MAX_LAYERS 4
typedef struct {
    int32_t rows, T_in, In, H, layers, P, O;
    const float* x;             /* [rows, T_in, In]                                                     */
    const float* last;          /* [rows, O]   last_location                                            */
    const float* teacher;       /* [rows, P, O] or NULL                                                 */
    const int32_t* coins;       /* [P] 1 = feed teacher[:, t] into step t + 1 (teacher != NULL), or NULL */
    const float* keep;          /* [P, rows, H] dropout keep flags of the decoder output, or NULL (no dropout) */
    float drop_p;
    const float* params;
    int64_t enc_off[4 * IPLAN_S2S_MAX_LAYERS], dec_off[4 * IPLAN_S2S_MAX_LAYERS], lin_off[2];
    float* out;                 /* [rows, P, O]                                                         */
    float* hidden_out;          /* optional [layers, rows, H]: the decoder's final hidden state         */
    float* save;                /* optional (training): the record iplan_seq2seq_bwd reads,
                                   [T_in + P, layers, rows, 6H] = h_prev | r | z | n | gh_n | h_new per GRU step (encoder steps first),
                                   followed by [P, rows, 16 + H] = the decoder step's input (O <= 16 columns) | the output layer's input */
} IplanSeq2SeqArgs;

int iplan_seq2seq_fwd(const IplanSeq2SeqArgs* args, iplan_stream_t stream);

/* iplan_seq2seq_bwd: the autograd of the above (nova/Seq2Seq.py:52-70 under loss.backward()) for a loss on `out` (BPTT through the decoder's feedback -- a step whose
 * input was the previous prediction passes its input gradient on to it -- and through both GRU stacks).  It walks the
 * data gradients and writes the row-level pre-activation gradients; the weight gradients are dY^T X contractions over them
 * (iplan_wgrad; iplan_amd/nova/Seq2Seq.py lists the problems):
 *   dsave [T_in + P, layers, rows, 4H] = dr | dz | dn_i | dn_h per GRU step, followed by [P, rows, 16] = d out (first O columns).
 * No gradient is returned for in_data / last_location / teacher_location (data).                                          */
typedef struct {
    IplanSeq2SeqArgs fwd;       /* the forward launch's arguments (its `save` filled)                   */
    const float* g_out;         /* [rows, P, O] dLoss/d out                                             */
    float* dsave;
} IplanSeq2SeqBwdArgs;

int iplan_seq2seq_bwd(const IplanSeq2SeqBwdArgs* args, iplan_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * One-shot peer-to-peer sum all-reduce of a gradient arena over xGMI (the reference has no
 * multi-GPU path -- this replaces the torch.distributed all-reduce behind parallel.DataParallel.all_reduce_grads when
 * IPLAN_P2P_ALLREDUCE=1).  Arenas are 0.3-4 MB: a ring's 2 (n - 1) latency-bound steps cost more than every rank reading
 * its peers' buffers directly.  Protocol, per collective `seq` (same on all ranks, +1 per call, >= 1):
 *   publish: copy `data` into this rank's staging half (seq & 1), then store `seq` into flags[peer][rank] of EVERY rank
 *            (system-scope release);
 *   reduce : wait until flags[rank][p] >= seq for all p (system-scope acquire), then data[i] = sum over p = 0 .. world-1, in
 *            that order on every rank (bit-identical replicas), of stage[p][half][i].
 * Double-buffered staging needs no second barrier: a rank can only publish seq + 2 (the same half) after it finished
 * seq + 1, which needed every peer's seq + 1, published only after that peer finished reading seq.
 * The ONLY entry points that allocate: staging / flag buffers must be shareable between processes, so they come from
 * hipMalloc directly (a caching allocator's sub-allocations cannot be exported); iplan_p2p_free releases them.
 */
#define IPLAN_P2P_MAX_RANKS 8
typedef struct {
    unsigned char bytes[64];                    /* hipIpcMemHandle_t */
} IplanIpcHandle;
int iplan_p2p_alloc(size_t bytes, void** dev_ptr);               /* zero-filled device memory of the current device */
int iplan_p2p_free(void* dev_ptr);
int iplan_p2p_export(void* dev_ptr, IplanIpcHandle* out);        /* hipIpcGetMemHandle */
int iplan_p2p_open(const IplanIpcHandle* handle, void** dev_ptr); /* hipIpcOpenMemHandle (another process' allocation) */
int iplan_p2p_close(void* dev_ptr);
typedef struct {
    int32_t world, rank;
    int64_t count;                              /* floats to reduce, <= capacity, multiple of 4                         */
    float* data;                                /* in / out, 16-byte aligned                                            */
    float* stage[IPLAN_P2P_MAX_RANKS];          /* staging buffers of all ranks (own: local, peers: opened), 2 * capacity floats each */
    uint32_t* flags[IPLAN_P2P_MAX_RANKS];       /* flag arrays of all ranks, IPLAN_P2P_MAX_RANKS words each              */
    int64_t capacity;                           /* floats per staging half, multiple of 4                               */
    uint32_t seq;
    int32_t* error;                             /* device int, set to 1 when the wait gives up after spin_limit polls    */
    int64_t spin_limit;                         /* 0 = wait for ever                                                     */
} IplanP2pArgs;
int iplan_p2p_publish(const IplanP2pArgs* args, iplan_stream_t stream);
int iplan_p2p_reduce(const IplanP2pArgs* args, iplan_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * iplan_obs_history_step: one environment step of the id -> slot history wrapper on the device
 * (observation_wrapper.py:68-141: obs_history_create + obs_history_output + obs_single_history_output).
 * State (caller-owned device memory, zeroed / -1-filled at the head of an episode -- agent_obs_profile_init,
 * observation_wrapper.py:26-46, stays on the host: it runs once per episode):
 *   slot_id[k][i][s] = vehicle id of slot s of (thread k, registered agent i), -1 = free; n_slots[k][i];
 *   win[k][i][s] = the slot's last L entries, right-aligned (the deque views the reference rebuilds every step).
 * A step appends this step's observed rows to the slots of their ids (new ids take the next free slot in row order) and a
 * zero entry to every known slot the agent did not observe; `win` IS obs_history_output(), `single` receives
 * obs_single_history_output() (any strides: it is written straight into the episode container's history field).
 * Values are copied bit for bit.  err: 0 ok; |1 an ego id that was never registered (the reference raises ValueError);
 * |2 more than N vehicles observed by one agent (IndexError).  One wave per (thread, registered agent).            */
typedef struct {
    int32_t K, nA, N, L, d, obs_num;
    const float* obs;            /* [K, nA, obs_num, 1 + d]: id column first; an all-zero row is padding            */
    const int32_t* agent_ids;    /* [K, nA] ego ids in order of first appearance (unused entries: INT32_MIN)         */
    int32_t* slot_id;            /* [K, nA, N]                                                                       */
    int32_t* n_slots;            /* [K, nA]                                                                          */
    float* win;                  /* [K, nA, N, L, d]                                                                 */
    float* single;               /* optional: element (k, i, s, c) at k * single_s_k + i * single_s_a + s * d + c    */
    int64_t single_s_k, single_s_a;
    int32_t* err;                /* [1] device int, OR-ed                                                            */
} IplanObsHistArgs;
int iplan_obs_history_step(const IplanObsHistArgs* args, iplan_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Attention saliency: the input backward of GAT_Net.forward with the egos kept apart (csrc/gat_saliency.hip).  For every scene
 * (net, b) and every ego i:  y_i = <v_i, latent_i>,  latent = GAT([src0 || src1], h_prev) as the training-form forward launch
 * described by `fwd` computed it (its `saved` record filled; h_prev is held constant), and
 *   G[i, j, c] = d y_i / d obs[j, c]     for every entity j of the scene, the ego included, and every column c < d0 + d1.
 * v: rows of A floats, (net, b, i) at v + net*v_s_net + b*v_s_b + i*A.
 * gate_through: 1 = the exact derivative, through the gumbel gate and the bidirectional pair GRU (1/tau included); 0 = the gate is
 * held constant: only the soft attention, the values and the output cell are differentiated, saved.gru and scratch are not read.
 * Outputs, each optional (NULL = not wanted; at least one is), scene (net, b) at base + net*s_net + b*s_b, contiguous inside:
 *   grad        [N, N, d0 + d1]   G, indexed [ego i, entity j, column]
 *   pair_gl1    [N, N, n_src]     sum_c |G[i, j, c]| over the columns of source 0 (src0) / 1 (src1); n_src = 2 if d1 > 0 else 1
 *   pair_gxi    [N, N, n_src]     sum_c G[i, j, c] obs[j, c]                           (both share pair_s_net / pair_s_b)
 *   input_grad  [N, d0 + d1]      sum_i G[i, j, :]: a running fp32 sum over the egos in ascending order, one rounded add each
 *   hidden_grad [N, A]            d y_i / d h_prev_i
 * scratch (gate_through == 1): at least n_nets * B * 2 * N * N * 3H floats, 16-byte aligned.
 * One workgroup per scene, no atomics, no sums across scenes: a scene's bits depend on its own operands only -- not on the other
 * scenes of the launch, its position among them, or on which outputs were asked for.  An ego with v_i == 0 gets exact zeros.
 * 2 <= N <= IPLAN_MAX_ENTITIES, d0 >= 1, d1 >= 0.  Parameters, the record and the inputs are only read.
 */
typedef struct {
    IplanGatFwdArgs fwd;
    const float* v;
    int64_t v_s_net, v_s_b;
    int32_t gate_through;
    float* scratch;
    int64_t scratch_floats;
    float* grad;
    int64_t grad_s_net, grad_s_b;
    float* pair_gl1;
    float* pair_gxi;
    int64_t pair_s_net, pair_s_b;
    float* input_grad;
    int64_t ig_s_net, ig_s_b;
    float* hidden_grad;
    int64_t hg_s_net, hg_s_b;
} IplanGatSaliencyArgs;

int iplan_gat_saliency(const IplanGatSaliencyArgs* args, iplan_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Attention saliency through time: iplan_gat_saliency chained over the past steps of the ego's own latent
 * (csrc/gat_saliency_trace.hip).  `fwd` describes ONE training-form forward launch (its `saved` record filled) over B * R rows per
 * net: row b * R + r is (env b, record step r), its h_prev the latent of record step r - 1 (the state the chain starts from for
 * r = 0).  The output GRUCell reads only the ego's own previous latent, so for every target t (record step r = targets[t]), ego i
 * and lag k = 0 .. min(K, r), with  y_i = <v_i, latent_{r,i}>  and  c_i^(-1) = v_i:
 *   lag k is iplan_gat_saliency on row r - k with the cotangent c_i^(k-1); its hidden_grad is the carry
 *   c_i^(k) = d y_i / d latent_{r-k-1,i},   and   G^(k)[i, j, c] = d y_i / d obs_{r-k}[j, c]   (total, through the ego's latent chain).
 * A lag's arithmetic is iplan_gat_saliency's, statement for statement: a slot's bits are that entry point's bits.
 * targets: T record steps in [0, R), any order, duplicates allowed; `targets` is the device copy the kernel reads, `targets_host`
 * the host copy the entry point checks.  v: rows of A floats, (net, b, t, i) at v + net*v_s_net + b*v_s_b + t*v_s_t + i*A.
 * gate_through: as in IplanGatSaliencyArgs.
 * Outputs, each optional (NULL = not wanted; at least one is), slot (net, b, t, k) at base + net*s_net + b*s_b + t*s_t + k*s_k,
 * contiguous inside, k = 0 .. K:
 *   grad        [N, N, d0 + d1]   G^(k), indexed [ego i, entity j, column]
 *   pair_gl1    [N, N, n_src]     sum_c |G^(k)[i, j, c]| per source; n_src = 2 if d1 > 0 else 1
 *   pair_gxi    [N, N, n_src]     sum_c G^(k)[i, j, c] obs_{r-k}[j, c]                 (both share the pair_s_* strides)
 *   input_grad  [N, d0 + d1]      sum_i G^(k)[i, j, :]: a running fp32 sum over the egos in ascending order, one rounded add each
 *   carry       [N, A]            c^(k)
 *   carry_sq    [N]               sum_c c^(k)[i][c]^2: one lane per ego, columns ascending, every product and sum rounded on its own
 * The slots of lags that do not exist (k > r) are written +0.0 by the kernel: the outputs need no prefill.
 * scratch (gate_through == 1): at least n_nets * B * T * 2 * N * N * 3H floats, 16-byte aligned; a workgroup reuses its part for
 * every lag.  One workgroup per (net, b, t) (grid n_nets * B * T), no atomics, no sums across workgroups: a slot's bits depend on
 * its own operands only -- not on the other targets, scenes or nets, on K, or on which outputs were asked for.  A zero v_i gives
 * exact zeros at every lag.  2 <= N <= IPLAN_MAX_ENTITIES, d0 >= 1, d1 >= 0, K >= 0.  Parameters, the record and the inputs are
 * only read.
 */
typedef struct {
    IplanGatFwdArgs fwd;
    int32_t B, R, T, K;
    const int32_t* targets;
    const int32_t* targets_host;
    const float* v;
    int64_t v_s_net, v_s_b, v_s_t;
    int32_t gate_through;
    float* scratch;
    int64_t scratch_floats;
    float* grad;
    int64_t grad_s_net, grad_s_b, grad_s_t, grad_s_k;
    float* pair_gl1;
    float* pair_gxi;
    int64_t pair_s_net, pair_s_b, pair_s_t, pair_s_k;
    float* input_grad;
    int64_t ig_s_net, ig_s_b, ig_s_t, ig_s_k;
    float* carry;
    int64_t carry_s_net, carry_s_b, carry_s_t, carry_s_k;
    float* carry_sq;
    int64_t csq_s_net, csq_s_b, csq_s_t, csq_s_k;
} IplanGatSaliencyTraceArgs;

int iplan_gat_saliency_trace(const IplanGatSaliencyTraceArgs* args, iplan_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Prediction saliency: the input Jacobian of the chain iplan_predict walks (csrc/pdec_saliency.hip),
 *   x_0 = start state, h_{-1} = h0;  t < P:  u_t = ReLU(W_lin x_t + b_lin), h_t = GRU32(u_t, h_{t-1}), y_t = W_out tanh(h_t) + b_out, x_{t+1} = y_t
 * (Prediction_Decoder.forward(last_state, None, hidden) under .eval(): no teacher forcing, no dropout).  Rows, the start state read in
 * place through offset / ent_stride, h0 and the parameters are iplan_predict's.  A job k < K is the pair jobs[k] = (p, c): horizon step
 * p in [0, P) and the cotangent v on y_p -- the one-hot of column c in [0, d), or, with c == -1, the row v[net, row, p, :] of the tensor
 * `v` [n_nets, rows, P, d].  The job list is the same for every row.  For every row and job, by BPTT through steps p .. 0 with the gates
 * recomputed (nothing is recorded in global memory, whatever P is):
 *   state_grad  [n_nets, rows, K, d]    d <v, y_p> / d x_0
 *   latent_grad [n_nets, rows, K, 32]   d <v, y_p> / d h0
 *   state_l1, state_gxi   [n_nets, rows, K]   sum_c |state_grad[c]|,  sum_c state_grad[c] x_0[c]
 *   latent_l1, latent_gxi [n_nets, rows, K]   sum_c |latent_grad[c]|, sum_c latent_grad[c] h0[c]
 *               (one lane per row, c ascending, every product and sum rounded on its own: the plain fp32 loops over the stored gradient)
 * and, independent of the jobs,
 *   pred        [n_nets, rows, P, d]    y_t, bit for bit iplan_predict's
 *   active      [n_nets, rows, P] int32: bit m = unit m of the input Linear has u_t > 0
 * Each output is optional (NULL = not wanted and not written; at least one is asked for); the per-job ones need K >= 1, jobs (device
 * memory) and jobs_host (the same values in host memory: argument checks, LDS and grid size).
 * One wave per (16-row tile, job), one more per tile for pred / active; the weights sit in LDS in both orientations and a wave keeps
 * the state and input each step enters with in LDS (3 KB per step), which bounds P.  No atomics, no sums across rows: a slot's bits
 * do not depend on its lane, tile or workgroup, on the other rows, on P, on the other jobs or on which outputs were asked for; two
 * launches give the same bits; a zero cotangent gives exact zeros; padding lanes of a ragged last tile write nothing; parameters and
 * inputs are only read.  1 <= d <= 16, hidden == 32, 1 <= P <= IPLAN_PDEC_SAL_MAX_P, n_nets <= IPLAN_MAX_NETS.
 */
#define IPLAN_PDEC_SAL_MAX_P 30     /* 160 KB of LDS: 68 KB of weights + one wave's 3 KB per chain step */
typedef struct {
    int32_t n_nets, S, N, P, d, K;
    const float* x0;            /* base of the start states (e.g. the episode buffer's history field)     */
    const int64_t* offset;      /* [n_nets, S] element offset of (sample, entity 0, feature 0)             */
    int64_t ent_stride;         /* elements between entities                                               */
    const float* h0;            /* [n_nets, S*N, 32] GAT output = initial hidden state                     */
    const float* params;        /* decoder arena, IPLAN_DEC_* offsets                                      */
    int64_t params_s_net;
    int64_t off[IPLAN_DEC_NPARAM];
    const int32_t* jobs;        /* [K, 2] (p, c) in device memory                                          */
    const int32_t* jobs_host;   /* the same values in host memory                                          */
    const float* v;             /* [n_nets, S*N, P, d]; needed by jobs with c == -1, NULL otherwise        */
    float* state_grad;
    float* latent_grad;
    float* state_l1;
    float* state_gxi;
    float* latent_l1;
    float* latent_gxi;
    float* pred;
    int32_t* active;
} IplanPdecSaliencyArgs;

int iplan_pdec_saliency(const IplanPdecSaliencyArgs* args, iplan_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Neighbour knock-out (occlusion attribution of the GAT): every scene (net, b) is run once per JOB, forward only, with one entity's
 * input row replaced (csrc/gat_knockout.hip).  A job is an entity index j in [0, N) or -1 (nothing knocked); the list jobs[J] is
 * the same for every scene, duplicates are allowed, every slot is computed on its own by one 512-thread workgroup (grid n_nets*B*J).
 * A slot's arithmetic is the inference form of iplan_gat_fwd (iplan_gat_trace's step), so latent_ko of job j carries the bits
 * iplan_gat_fwd gives on a copy of the inputs with row j replaced; src0 / src1 are read in place and never written.
 *   knock0 / knock1   which sources of entity j are replaced: source 0 by baseline0[d0], source 1 by baseline1[d1] (NULL = zeros)
 *   hidden            the state every slot starts from, rows as iplan_gat_fwd's h_prev (NULL: zeros); entity j's row is NOT changed
 *   noise             gumbel samples [n_nets, B, N, N-1, 2] contiguous, the same for every job of a scene; NULL = none
 * Outputs, each optional (NULL = not wanted; at least one is), element (net, b, slot) at ptr + net*s_net + b*s_b + slot*s_job:
 *   latent_ko [N, A]  the attention latent of the knocked scene (16-byte aligned, strides % 4 == 0)
 *   attn_ko   [N, N]  the entity-indexed soft * hard map of the knocked scene, diagonal 0 (iplan_gat_trace's `attn`)
 *   shift_sq  [N]     sum_c (latent_ko[i, c] - base[i, c])^2, c = 0 .. A-1 ascending, one lane per ego, every difference, product
 *                     and sum rounded on its own (no fma; the plain fp32 host loop gives the same bits); no square root is taken.
 *                     Needs `base`: rows (net, b, i) at base + net*base_s_net + b*base_s_b + i*A, written by an EARLIER launch.
 * No atomics, no sums across workgroups: a slot's bits depend on its scene, its job and the arguments only.
 * Refused: N outside [2, IPLAN_MAX_ENTITIES], J < 1, a job outside [-1, N-1] (checked on jobs_host), knock1 with d1 == 0, null or
 * misaligned tensors, no output, shift_sq without base, more than 2^31 - 1 workgroups.
 */
typedef struct {
    int32_t n_nets, B, N, d0, d1, J;
    const float* src0;
    int64_t src0_s_net, src0_s_b;
    const float* src1;          /* may be NULL iff d1 == 0                                                 */
    int64_t src1_s_net, src1_s_b;
    const float* hidden;        /* or NULL                                                                 */
    int64_t h_s_net, h_s_b;
    const float* noise;
    const float* params;        /* parameter arena, IPLAN_GAT_* offsets                                    */
    int64_t params_s_net;
    int64_t off[IPLAN_GAT_NPARAM];
    float tau;
    int32_t knock0, knock1;
    const int32_t* jobs;        /* [J] device memory                                                       */
    const int32_t* jobs_host;   /* the same values in host memory (argument checks)                        */
    const float* baseline0;     /* [d0] or NULL                                                            */
    const float* baseline1;     /* [d1] or NULL                                                            */
    const float* base;          /* the latent of the scene with nothing knocked, or NULL                   */
    int64_t base_s_net, base_s_b;
    float* latent_ko;
    int64_t lat_s_net, lat_s_b, lat_s_job;
    float* attn_ko;
    int64_t attn_s_net, attn_s_b, attn_s_job;
    float* shift_sq;
    int64_t shift_s_net, shift_s_b, shift_s_job;
} IplanGatKnockoutArgs;

int iplan_gat_knockout(const IplanGatKnockoutArgs* args, iplan_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Neighbour knock-out through time: iplan_gat_trace's walk, run once per JOB with one entity's input row replaced in the first D
 * steps of the window (csrc/gat_knockout_trace.hip).  One 512-thread workgroup owns one (net, b, job slot) (grid n_nets*B*J) and
 * walks steps start .. start + H - 1 of the episode fields, read in place through net / b / step strides and never written:
 * h_s = GAT(x_s, h_{s-1}), h_{start-1} = hidden0 (NULL: zeros).  In steps start .. start + D - 1 the slot's job is knocked as
 * iplan_gat_knockout knocks it (knock0 / knock1, baseline0 / baseline1); the later steps see the recorded rows, and only the slot's
 * own carried latent remembers the knock.  Entity j's hidden row is never overwritten.  A slot's arithmetic is iplan_gat_trace's
 * step, so latent_ko of job j carries the bits iplan_gat_trace gives on a copy of the fields with row j replaced in the knocked steps.
 *   jobs / jobs_host  as in IplanGatKnockoutArgs: entity indices in [0, N) or -1 (nothing knocked), duplicates allowed
 *   noise             gumbel samples [n_nets, B, H, N, N-1, 2] contiguous (the window's), the same for every job; NULL = none
 * Outputs, each optional (NULL = not wanted; at least one is), element (net, b, slot, step h of the window) at
 * ptr + net*s_net + b*s_b + slot*s_job + h*s_step:
 *   latent_ko [N, A]  the attention latent of the knocked chain (16-byte aligned, strides % 4 == 0)
 *   attn_ko   [N, N]  the entity-indexed soft * hard map of the knocked chain, diagonal 0
 *   shift_sq  [N]     sum_c (latent_ko[i, c] - base[i, c])^2 as IplanGatKnockoutArgs forms it.  Needs `base`: rows (net, b, h, i) at
 *                     base + net*base_s_net + b*base_s_b + h*base_s_step + i*A, the walk with nothing knocked over the same window,
 *                     written by an EARLIER launch (iplan_gat_trace's `latent`).
 * No atomics, no sums across workgroups: a slot's bits depend on its scene, its job and the arguments only.
 * Refused: N outside [2, IPLAN_MAX_ENTITIES], J < 1, H < 1, D outside [1, H], start < 0, a job outside [-1, N-1] (checked on
 * jobs_host), knock1 with d1 == 0, null or misaligned tensors, no output, shift_sq without base, more than 2^31 - 1 workgroups.
 */
typedef struct {
    int32_t n_nets, B, N, d0, d1, J, H, D, start;
    const float* src0;
    int64_t src0_s_net, src0_s_b, src0_s_step;
    const float* src1;          /* may be NULL iff d1 == 0                                                 */
    int64_t src1_s_net, src1_s_b, src1_s_step;
    const float* hidden0;       /* the state step `start` starts from, or NULL                             */
    int64_t h_s_net, h_s_b;
    const float* noise;
    const float* params;        /* parameter arena, IPLAN_GAT_* offsets                                    */
    int64_t params_s_net;
    int64_t off[IPLAN_GAT_NPARAM];
    float tau;
    int32_t knock0, knock1;
    const int32_t* jobs;        /* [J] device memory                                                       */
    const int32_t* jobs_host;   /* the same values in host memory (argument checks)                        */
    const float* baseline0;     /* [d0] or NULL                                                            */
    const float* baseline1;     /* [d1] or NULL                                                            */
    const float* base;          /* the latents of the window with nothing knocked, or NULL                 */
    int64_t base_s_net, base_s_b, base_s_step;
    float* latent_ko;
    int64_t lat_s_net, lat_s_b, lat_s_job, lat_s_step;
    float* attn_ko;
    int64_t attn_s_net, attn_s_b, attn_s_job, attn_s_step;
    float* shift_sq;
    int64_t shift_s_net, shift_s_b, shift_s_job, shift_s_step;
} IplanGatKnockoutTraceArgs;

int iplan_gat_knockout_trace(const IplanGatKnockoutTraceArgs* args, iplan_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Forecasts of the knocked chains through time (csrc/predict_knockout.hip): iplan_predict's decoder chain
 *   y_p, h = Linear(tanh(GRU(ReLU(Linear(y_{p-1})), h))),  p < P,
 * run on the latents iplan_gat_knockout_trace wrote, reduced where it runs to P numbers per row.  A row is (net, b, job slot q, window
 * step h, entity i) -- the order of a contiguous latent_ko [n_nets, B, J, H, N, 32]; one wave walks 16 rows of one net.  Per row
 *   h_0    = latent_ko row (net, b, q, h, i)
 *   y_{-1} = history row (net, b, start + h, i): history + net*hist_s_net + b*hist_s_b + (start + h)*hist_s_step + i*hist_s_ent, d
 *            contiguous floats of any alignment, read in place.  It is NEVER knocked, whatever the job was: the result isolates the
 *            social path (Prediction_policy.attention_knockout's rule).
 * The job list itself is not an argument: the knock is in latent_ko already.
 * Outputs, each optional (NULL = not wanted; at least one is), element (net, b, q, h) at ptr + net*s_net + b*s_b + q*s_job + h*s_step:
 *   fshift_sq [N, P]    sum over k < n_pos of (y_p[pos[k]] - pred_base_p[pos[k]])^2, k ascending, every difference, product and sum
 *                       rounded on its own (no fma), so that the plain fp32 host loop gives the same bits.  Needs pred_base: rows
 *                       (net, b, h) [N, P, d] at pred_base + net*pb_s_net + b*pb_s_b + h*pb_s_step, the forecasts of the walk with
 *                       nothing knocked, written by an EARLIER launch (iplan_predict's pred on iplan_gat_trace's latent).
 *   ferr_sq   [N, P]    the same sum against the recorded future, history row (net, b, start + h + 1 + p, i).  Where that step is not
 *                       recorded (start + h + 1 + p >= S) the entry is +0.0 and nothing is read for it.  Needs S, the number of
 *                       recorded steps of `history`, with start + H <= S.
 *   pred_ko   [N, P, d] the forecasts themselves, bit for bit iplan_predict's on the same h_0 and start state.
 * No atomics, no sums across rows: a slot's bits depend on its row and the arguments only.
 * Refused: null args or tensors, no output, fshift_sq without pred_base, ferr_sq without a readable window (S < start + H), d outside
 * [1, 16], n_nets outside [1, IPLAN_MAX_NETS], B / J / H / N / P < 1, start < 0, B*J*H*N > 2^31 - 17, n_pos outside [1, 16] (with
 * fshift_sq or ferr_sq), a pos entry outside [0, d) or repeated, latent_ko misaligned (16 bytes, strides % 4 == 0).
 */
typedef struct {
    int32_t n_nets, B, J, H, N, P, d;
    int32_t S;                  /* recorded steps of `history`; only read with ferr_sq                     */
    int32_t start;              /* first step of the window                                                */
    int32_t n_pos;
    int32_t pos[16];            /* the columns of the distance, in the order they are added                */
    const float* history;
    int64_t hist_s_net, hist_s_b, hist_s_step, hist_s_ent;
    const float* latent_ko;     /* [N, 32] per (net, b, q, h)                                              */
    int64_t lat_s_net, lat_s_b, lat_s_job, lat_s_step;
    const float* pred_base;     /* [N, P, d] per (net, b, h), or NULL                                      */
    int64_t pb_s_net, pb_s_b, pb_s_step;
    const float* params;        /* decoder arena, IPLAN_DEC_* offsets                                      */
    int64_t params_s_net;
    int64_t off[IPLAN_DEC_NPARAM];
    float* fshift_sq;
    int64_t fs_s_net, fs_s_b, fs_s_job, fs_s_step;
    float* ferr_sq;
    int64_t fe_s_net, fe_s_b, fe_s_job, fe_s_step;
    float* pred_ko;
    int64_t pk_s_net, pk_s_b, pk_s_job, pk_s_step;
} IplanPredictKnockoutArgs;

int iplan_predict_knockout(const IplanPredictKnockoutArgs* args, iplan_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Policy knock-out (occlusion attribution of the actors and critics): every row (e, s, agent) of a recorded batch is run once per
 * JOB, forward only -- LN(F) -> fc1 -> act -> LN -> fc2 -> act -> LN -> GRU cell (state given, held) -> LN -> head -> masked softmax | V
 * -- with one entity's columns of the selected per-entity sources replaced AS THE FEATURES ARE GATHERED (csrc/policy_knockout.hip,
 * ac_kmap_ko.h); nothing is copied or modified in memory.  `base` describes the rows exactly as for iplan_ac_saliency (feat, nets, h_*,
 * avail, target, packed_*); of its outputs logp, values and target_out [n_agents, E*S] receive the row's BASE result (nothing knocked)
 * and the a* that was used, the others must be NULL.  A job is an entity index in [0, N) or -1 (nothing knocked); jobs[J] is the same
 * for every row, duplicates are allowed.
 *   knock[k]      source k's columns of the job's entity are replaced: entry f of the row's source block belongs to entity f / w[k] and
 *                 becomes baseline[k][f - e*w[k]] (baseline[k] NULL: 0).  The replacement precedes LayerNorm(F): the statistics are
 *                 those of the modified row.  The one-hots are never knocked.
 *   override[k]   instead of the row's own vector, job q of row (e, s) of agent `net` reads source k from
 *                 override[k] + q*ov_s_job[k] + net*ov_s_net[k] + e*ov_s_chain[k] + s*ov_s_step[k] + entity*ov_s_ent[k] + column
 *                 (innermost axis contiguous).  An overridden source is taken as given: it is not knocked as well, for any job.
 * a*: the row's entry of base.target (base.target_all), or the BASE result's argmax where that is -1 -- one action per row, the same
 * for every job of it.
 * Work: one wave per tile of 16 columns = the 15 jobs 15*jt .. 15*jt + 14 of ONE row and, in column 15, the row's base result, which
 * every tile carries; ceil(J / 15) tiles per row, four tiles per workgroup, grid over tiles x agents x nets.  The arithmetic of a
 * column is iplan_ac_saliency's forward half (fc1 on v_mfma_f32_16x16x4_f32, the same k-tile order and partial sums of 8 k-tiles).
 * Outputs, each optional, contiguous, of the nets base.which selects, slot (net, row, job) at index (net*E*S + row)*J + job:
 *   probs_ko  [.., n_actions]   logp_ko (of a*), values_ko, greedy_ko (int64, lowest index on ties)
 *   kl     = sum over the available actions, ascending, of p_base * (logp_base - logp_ko); every term rounded on its own (no fma)
 *   dlogp  = logp_ko - logp_base,  dvalue = V_ko - V_base      formed by one lane per (row, job) from its tile's base column
 *   probs_base [n_agents, E*S, n_actions], greedy_base [n_agents, E*S] int64    the base result (with base.logp / values / target_out)
 * At least one output must be asked for.  A slot whose gathered values equal the row's has kl = dlogp = dvalue = 0.0 and the base's
 * bits.  No atomics, no sums across columns: a slot's bits do not depend on its lane, tile, workgroup, the other jobs, J or on which
 * outputs were asked for.  Refused: what iplan_ac_saliency refuses of the rows, J < 1, a job outside [-1, N) (checked on jobs_host),
 * knock or override on an absent source, negative override strides, E*S*ceil(J/15) tiles beyond 2^31 / 16, a base output other than
 * logp / values / target_out.
 */
typedef struct {
    IplanAcSaliencyArgs base;
    int32_t J;
    int32_t knock[3];
    const int32_t* jobs;        /* [J] device memory                                                       */
    const int32_t* jobs_host;   /* the same values in host memory (argument checks)                        */
    const float* baseline[3];   /* [w[k]] or NULL (zeros)                                                  */
    const float* override_src[3];
    int64_t ov_s_job[3], ov_s_net[3], ov_s_chain[3], ov_s_step[3], ov_s_ent[3];
    float* probs_base;
    int64_t* greedy_base;
    float* probs_ko;
    float* logp_ko;
    float* values_ko;
    int64_t* greedy_ko;
    float* kl;
    float* dlogp;
    float* dvalue;
} IplanAcKnockoutArgs;

int iplan_ac_knockout(const IplanAcKnockoutArgs* args, iplan_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Policy knock-out through time: E recorded chains are walked over H = base.S consecutive steps once per JOB, forward only, every job
 * with a GRU state of its OWN, carried by the nets from the common start state base.hidden0_* (csrc/policy_knockout_trace.hip).  In
 * steps 0 .. D-1 the job's entity has its columns of the knocked sources replaced AS THE FEATURES ARE GATHERED (jobs, knock, baseline:
 * IplanAcKnockoutArgs' rules; no override); steps D .. H-1 see the recorded rows again, and only the job's state remembers the knock.
 * `base` describes the chains exactly as for iplan_ac_trace: n_agents, E, S = H, which, act_tanh, feat (feat.T = H; the last action is
 * teacher-forced from the batch for every job), the nets, hidden0_* and strides, avail, packed_*.  base.actions_in is the TARGET a*
 * of step (e, s) by physical row; NULL, or an entry outside [0, n_actions): the BASE chain's argmax of that step -- one action per
 * step, the same for every job.  Of base's outputs probs, greedy, logp (of a*) and values [n_agents, E, H, ..] receive the base chain
 * (nothing knocked), which equals iplan_ac_trace's bits; entropy, h_all_* and h_last_* must be NULL.
 *   phase 1 (knocked trunk)  steps < D only; one wave per tile of 16 columns = the jobs 15*jt .. 15*jt + 14 of ONE row and, in column 15,
 *                    the row with nothing knocked; iplan_ac_trace's trunk arithmetic (the same k-tile order and partial sums of 8
 *                    k-tiles) -> gi_ko, a caller-provided workspace [2 (actor | critic), n_agents, E, D, ceil(J/15), 16, IPLAN_AC_TRACE_GI]
 *   phase 2 (knocked walk)   one workgroup per (net, chain, job tile) steps s = 0 .. H-1 with W_hh in registers; a column reads its own
 *                    gi_ko row while s < D and base.gi of the row after: base.gi [2, n_agents, E*H, IPLAN_AC_TRACE_GI] as a call of
 *                    iplan_ac_trace with phases = 1 on the same rows leaves it (needed when D < H; this entry does not write it).
 * base.phases: 0 = both kernels, 1 = phase 1 only, 2 = phase 2 only (gi_ko as a previous call left it).
 * Outputs, each optional, contiguous, of the nets base.which selects, slot (net, e, s, job) at index ((net*E + e)*H + s)*J + job:
 *   probs_ko [.., n_actions]   logp_ko (of a*), values_ko, greedy_ko (int64, lowest index on ties)
 *   logp_all_ko [.., n_actions]  every log-probability of the job's distribution, the operands of kl (for tests)
 *   kl, dlogp, dvalue          as iplan_ac_knockout forms them, against the base chain's result of the same step
 *   shift_sq_actor / _critic   sum over the 64 units, ascending, of (h_job - h_base)^2 after the step; every difference, product and sum
 *                              rounded on its own (no fma)
 *   h_ko_actor / h_ko_critic   [.., 64] the job's state after the step
 *   target_out [n_agents, E, H] int64   the a* that was used
 * A job whose gathered values equal the rows' own has kl = dlogp = dvalue = shift_sq = 0.0 at every step.  No atomics, no sums across
 * columns: a slot's bits do not depend on its lane, tile, the other jobs, J, H (a shorter H gives a prefix), packed or in-place fc1 or
 * the outputs asked for.  Refused: what iplan_ac_trace refuses of the chains, D outside [1, H], J < 1, a job outside [-1, N) (checked
 * on jobs_host), knock or baseline on an absent source, E*H*ceil(J/15) tiles beyond 2^31 / 16, a base output other than probs / greedy
 * / logp / values, no output (unless phases = 1), a missing gi_ko, a missing base.gi with D < H; gi_ko, base.gi, h_ko_* and the packed
 * operands 16-byte aligned.
 */
typedef struct {
    IplanAcTraceArgs base;
    int32_t D, J;
    int32_t knock[3];
    const int32_t* jobs;        /* [J] device memory                                                       */
    const int32_t* jobs_host;   /* the same values in host memory (argument checks)                        */
    const float* baseline[3];   /* [w[k]] or NULL (zeros)                                                  */
    float* gi_ko;
    int64_t* target_out;
    float* probs_ko;
    float* logp_ko;
    float* values_ko;
    int64_t* greedy_ko;
    float* kl;
    float* dlogp;
    float* dvalue;
    float* shift_sq_actor;
    float* shift_sq_critic;
    float* h_ko_actor;
    float* h_ko_critic;
    float* logp_all_ko;
} IplanAcKnockoutTraceArgs;

int iplan_ac_knockout_trace(const IplanAcKnockoutTraceArgs* args, iplan_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * The knock-out chain through time: iplan_ac_knockout_trace with a per-job SOURCE (csrc/policy_knockout_chain.hip).  `kt` describes the
 * chains, the jobs, the window (H = kt.base.S, D = kt.D) and the outputs exactly as for iplan_ac_knockout_trace.  In addition
 *   override_src[k]   instead of the row's own vector, job q of step (e, s) of agent `net` reads source k from
 *                     override_src[k] + q*ov_s_job[k] + net*ov_s_net[k] + e*ov_s_chain[k] + s*ov_s_step[k] + entity*ov_s_ent[k] + column
 *                     at EVERY step of the window (IplanAcKnockoutArgs' rules: innermost axis contiguous, non-negative strides, read in
 *                     place).  An overridden source is taken as given: it is not knocked as well, for any job.
 *   override_base[k]  what column 15 of every tile -- the base chain -- reads for source k instead of the batch's, from
 *                     override_base[k] + net*ovb_s_net[k] + e*ovb_s_chain[k] + s*ovb_s_step[k] + entity*ovb_s_ent[k] + column;
 *                     NULL: the batch's own source.  A job of entity -1 reads it too where override_src[k] is NULL.
 * The other sources selected by kt.knock are replaced for steps s < D only, as iplan_ac_knockout_trace replaces them.  At least one
 * source must be overridden (without one iplan_ac_knockout_trace is the entry): a job's inputs then differ from the base's at every
 * step, so
 *   phase 1 (knocked trunk)  runs over all E x H x ceil(J/15) tiles: iplan_ac_knockout_trace's trunk, the same text, k-tile order and
 *                    partial sums, with the override pointers in the gather and the entity knock masked off for s >= D
 *                    -> kt.gi_ko [2 (actor | critic), n_agents, E, H, ceil(J/15), 16, IPLAN_AC_TRACE_GI]
 *   phase 2 (knocked walk)   IS iplan_ac_knockout_trace's walk kernel, launched with D = H: every column reads its own gi_ko row at
 *                    every step, column 15 carries the base chain.  kt.base.gi is not read and must be NULL.
 * kt.base.phases, the outputs and their layout, a*, the exact zeros (a job whose gathered values equal column 15's at every step) and
 * the independence of a slot's bits from lane, tile, the other jobs, J, H and the outputs asked for: iplan_ac_knockout_trace's.
 * Refused: what iplan_ac_knockout_trace refuses, an override or base override on an absent source, negative override strides, a base
 * override without any job override, no override at all, a missing or misaligned gi_ko, kt.base.gi given.
 */
typedef struct {
    IplanAcKnockoutTraceArgs kt;
    const float* override_src[3];
    int64_t ov_s_job[3], ov_s_net[3], ov_s_chain[3], ov_s_step[3], ov_s_ent[3];
    const float* override_base[3];
    int64_t ovb_s_net[3], ovb_s_chain[3], ovb_s_step[3], ovb_s_ent[3];
} IplanAcKnockoutChainArgs;

int iplan_ac_knockout_chain(const IplanAcKnockoutChainArgs* args, iplan_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* IPLAN_HIP_H */
