// Attention saliency: the input backward of GAT_Net.forward with the egos kept apart.
//
// For every scene (net, env) and every ego i the launch differentiates  y_i = <v_i, latent_i>  (latent = the GAT's new attention
// latent, v = a cotangent the caller hands over) with respect to the GAT's input rows [src0 || src1] of EVERY entity j of the scene,
// the ego's own row included:  G[i, j, c] = d y_i / d obs[j, c].  The training backward (gat_bwd.hip) sums over the egos that see an
// entity and stops at the node pre-activations; this kernel does neither.  It reads the record a training-form forward launch left
// (IplanGatSaved) and the parameters, and writes only its outputs and its scratch.
//
// One 512-thread workgroup per scene, as in gat_bwd.hip:
//   A  GRUCell'            rows of the scene -> dx_i, and d y_i / d hidden_i (hidden_grad)
//   B  per ego (wave):     t_s = dx_i . v_j ; softmax' -> d score ; gumbel-gate' (x 1/tau) -> d(l1 - l0) ; dq_i
//   D  BPTT of both directions of the pair GRU over each ego's chain (gat_bwd.hip's phase D without the dW_hh / db_hh sums): the
//      input-side gate gradients [dr dz dn_i] of every pair step go to the scratch, their sums over the steps beside them.
//      Skipped with gate_through == 0 (the gate is a constant then): the pair-GRU record and the scratch are never touched.
//   P  per 16-entity tile (one wave): for the egos i = 0 .. N-1 in ascending order, 16 pairs (i, j) at a time on the fp32 MFMA
//        dh_j^(i) = W_b,f^T g_f + W_b,r^T g_r + W_k^T (dscore_ij q_i) + W_v^T ((soft hard)_ij dx_i . [v_j > 0])          j != i
//        dh_i^(i) = W_a,f^T sum_s g_f + W_a,r^T sum_s g_r + W_q^T dq_i                                                  j == i
//        G[i, j, :] = (dh . [h_j > 0]) W_enc
//      grad, the two pair maps, and input_grad[j] = sum_i G[i, j, :] -- a running fp32 sum in registers, one plain add per ego.
// No atomics and no sums across scenes: a scene's bits depend on nothing but its own operands -- not on its workgroup, the other
// scenes, or on which outputs were asked for.
//
// RESTATED in gat_saliency_trace.hip: its lag loop holds the phases A, B, D, P below statement for statement, and its slots are
// tested to be this kernel's bits.  A change to the arithmetic here has to be made there too.  What differs there on purpose: the
// cotangent comes from an LDS table and the hidden gradient is always formed (it is the next lag's cotangent), the parameter pointer
// is made opaque once per lag as well, and phase P's per-source pair sums are scalars (the indexed pair went to scratch memory there).
#include "api_util.h"
#include "gru_tile.h"

namespace iplan {

constexpr int SH = IPLAN_GAT_HIDDEN;   // H == A == 32
constexpr int SNP = IPLAN_MAX_ENTITIES;
constexpr int SQS = 33;                // padded row stride of the q / k / v / dx / dq tables
constexpr int SG = 3 * SH;             // [dr dz dn_i] of one pair step
constexpr int SCT = 4;                 // column tiles of G a wave holds the running input_grad of at a time

// the parameter pointer as a value the compiler knows nothing about: phase P's weight fragments are fetched where they are used
// (L1 / L2 resident), not lifted out of the ego loop into registers that are not there
__device__ __forceinline__ const float* sal_opaque(const float* p) {
#ifndef IPLAN_HOST_EMULATION
    asm volatile("" : "+s"(p));
#endif
    return p;
}

__global__ __launch_bounds__(512) void gat_saliency_kernel(IplanGatSaliencyArgs a) {
    __shared__ float s_q[SNP][SQS];
    __shared__ float s_k[SNP][SQS];
    __shared__ float s_v[SNP][SQS];
    __shared__ float s_dx[SNP][SQS];
    __shared__ float s_dq[SNP][SQS];
    __shared__ float s_ds[SNP][SNP];                                // d score (1/sqrt(A) included) per (ego, slot)
    __shared__ float s_w[SNP][SNP];                                 // soft * hard
    __shared__ float s_dd[SNP][SNP];                                // d(l1 - l0)
    constexpr int WLD = 3 * SH + 8;                                 // W_hh^T [H][3H + 8]: conflict-free ds_read_b128 fragments
    __shared__ __attribute__((aligned(16))) float s_whh[2][SH * WLD];
    __shared__ __attribute__((aligned(16))) float s_bhn[2][SH];

    const IplanGatFwdArgs& f = a.fwd;
    const IplanGatSaved& sv = f.saved;
    const int net = (int)blockIdx.x / f.B;
    const int b = (int)blockIdx.x % f.B;
    const int N = f.N;
    const int D = f.d0 + f.d1;
    const float* __restrict__ P = f.params + (int64_t)net * f.params_s_net;
    const int l = lane_id(), w = wave_id();
    const int n = l & 15, g = l >> 4;
    const int tile = w & 3, dir = w >> 2;
    const int node = 16 * tile + n;
    const bool tile_live = 16 * tile < N;
    const bool valid = node < N;
    const int64_t sb = (int64_t)net * f.B + b;
    const bool through = a.gate_through != 0;
    // scratch of this scene: [2][N][N-1][3H] pair-step gate gradients, then [2][N][3H] their sums over the steps
    float* __restrict__ scr = through ? a.scratch + sb * (int64_t)(2 * N * N * SG) : nullptr;
    float* __restrict__ scr_sum = through ? scr + (int64_t)2 * N * (N - 1) * SG : nullptr;

    for (int idx = (int)threadIdx.x; idx < N * 3 * SH; idx += (int)blockDim.x) {
        const int nd = idx / (3 * SH), c = idx - nd * 3 * SH;
        const float val = sv.qkv[(sb * N + nd) * 3 * SH + c];
        if (c < SH) s_q[nd][c] = val;
        else if (c < 2 * SH) s_k[nd][c - SH] = val;
        else s_v[nd][c - 2 * SH] = val;
    }
    if (through) {
        stage_matrix_t(s_whh[0], WLD, SH, P + f.off[IPLAN_GAT_F_WHH], 3 * SH, SH);
        stage_matrix_t(s_whh[1], WLD, SH, P + f.off[IPLAN_GAT_R_WHH], 3 * SH, SH);
        if (threadIdx.x < 2 * SH)                                   // b_hn of both directions (the recomputed gh_n's bias)
            s_bhn[threadIdx.x >> 5][threadIdx.x & 31] = P[f.off[(threadIdx.x >> 5) ? IPLAN_GAT_R_BHH : IPLAN_GAT_F_BHH] + 2 * SH + (threadIdx.x & 31)];
    }
    // ---------------------------------------------------------------- A: output GRUCell backward
    if (tile_live && dir == 0) {
        const float* crow = sv.cell + (sb * N + node) * (4 * SH);
        const float* hrow = f.h_prev + (int64_t)net * f.h_s_net + (int64_t)b * f.h_s_b + (int64_t)node * SH;
        const float* vrow = a.v + (int64_t)net * a.v_s_net + (int64_t)b * a.v_s_b + (int64_t)node * SH;
        f32x4 dgi[6], dgh[6], dhd[2];
        for (int T = 0; T < 2; ++T) {
            const GruGrads o = gru_gates_bwd(vload(vrow, valid, SH, T), vload(crow, valid, SH, T), vload(crow + SH, valid, SH, T),
                                             vload(crow + 2 * SH, valid, SH, T), vload(crow + 3 * SH, valid, SH, T),
                                             vload(hrow, valid, SH, T));
            dgi[T] = o.dr; dgi[2 + T] = o.dz; dgi[4 + T] = o.dni;
            dgh[T] = o.dr; dgh[2 + T] = o.dz; dgh[4 + T] = o.dnh;
            dhd[T] = o.dh_direct;
        }
        const float* Wi = P + f.off[IPLAN_GAT_C_WIH];
        const float* Wc = P + f.off[IPLAN_GAT_C_WHH];
        float* grow = a.hidden_grad ? a.hidden_grad + (int64_t)net * a.hg_s_net + (int64_t)b * a.hg_s_b + (int64_t)node * SH : nullptr;
        for (int T = 0; T < 2; ++T) {
            const f32x4 dx = dense_tile_gt<6>(Wi, SH, 3 * SH, SH, 16 * T, dgi, splat4(0.f));
            if (valid)
                for (int q = 0; q < 4; ++q) s_dx[node][16 * T + 4 * g + q] = dx[q];
            if (grow) vstore(grow, valid, SH, T, dense_tile_gt<6>(Wc, SH, 3 * SH, SH, 16 * T, dgh, dhd[T]));
        }
    }
    __syncthreads();

    // ---------------------------------------------------------------- B: attention backward per ego
    for (int i = w; i < N; i += 8) {
        const int s = l;
        const bool live = s < N - 1;
        const int j = live ? s + (s >= i ? 1 : 0) : 0;
        float soft = 0.f, hard = 0.f;
        if (live) {
            soft = sv.soft[(sb * N + i) * (N - 1) + s];
            hard = sv.hard[(sb * N + i) * (N - 1) + s];
        }
        float t = 0.f;
        for (int c = 0; c < SH; ++c) t = fmaf(s_dx[i][c], s_v[j][c], t);
        const float dsoft = t * hard, dhard = t * soft;
        const float dot = wave_sum(live ? soft * dsoft : 0.f);
        const float ds = live ? soft * (dsoft - dot) / 5.656854249492381f : 0.f;                // d score, incl. 1/sqrt(A)
        const float dd = (live && through) ? dhard * hard * (1.0f - hard) / f.tau : 0.f;         // d(l1 - l0); a held gate has none
        if (live) {
            s_ds[i][s] = ds;
            s_w[i][s] = soft * hard;
            s_dd[i][s] = dd;
        }
        const int c = l & 31, hf = l >> 5;
        float acc = 0.f;
        for (int it = 0; 2 * it < N - 1; ++it) {
            const int s2 = 2 * it + hf;
            const float dsv = __shfl(ds, s2);
            const int j2 = s2 < N - 1 ? s2 + (s2 >= i ? 1 : 0) : 0;
            acc = fmaf(dsv, s_k[j2][c], acc);
        }
        acc += __shfl_xor(acc, 32);
        if (l < 32) s_dq[i][c] = acc;
    }
    __syncthreads();

    // ---------------------------------------------------------------- D: BPTT through the pair GRU, per ego chain
    // (gat_bwd.hip's phase D: the record layout, the step-ahead loads, the clones of the ragged last tile and the recomputed gh_n
    // are its own; what leaves a step here is the chain's own [dr dz dn_i], one 3H row per (direction, ego, slot))
    if (through && tile_live) {
        const float* swT = s_whh[dir];
        const float* Wh = P + f.off[IPLAN_GAT_HARD_W];                              // [2][2H]
        f32x4 wdiff[2];
        for (int T = 0; T < 2; ++T) wdiff[T] = bfrag(Wh + 2 * SH + dir * SH, SH, T) - bfrag(Wh + dir * SH, SH, T);
        const int cnode = imin(node, N - 1);
        const int NT = (N + 15) / 16;
        constexpr int REC = 8 * 256;
        const float* gbase = sv.gru + (((((int64_t)net * 2 + dir) * f.B + b) * NT + tile) * (int64_t)(N - 1)) * REC + (cnode & 15) * 16 + 4 * g;
        float* __restrict__ srow = scr + ((int64_t)dir * N + cnode) * (N - 1) * SG + 4 * g;
        struct PairIn {
            f32x4 hs[2], r[2], z[2], nn[2], hp[2];
            float dd;
            bool has_prev;
        };
        auto load_step = [&](int it, PairIn& o, bool first) {
            const int s = dir ? it : (N - 2 - it);                 // reverse of the forward visiting order
            const int sp = dir ? s + 1 : s - 1;                    // the step the forward came from
            o.has_prev = sp >= 0 && sp <= N - 2;
            const float* row = gbase + (int64_t)s * REC;
            const float* prow = gbase + (int64_t)(o.has_prev ? sp : s) * REC;
            for (int T = 0; T < 2; ++T) {
                if (first) o.hs[T] = *reinterpret_cast<const f32x4*>(row + 256 * T);
                o.r[T] = *reinterpret_cast<const f32x4*>(row + 256 * (2 + T));
                o.z[T] = *reinterpret_cast<const f32x4*>(row + 256 * (4 + T));
                o.nn[T] = *reinterpret_cast<const f32x4*>(row + 256 * (6 + T));
                o.hp[T] = *reinterpret_cast<const f32x4*>(prow + 256 * T);
            }
            o.dd = s_dd[cnode][s];
        };
        f32x4 dh[2], da[6];
        for (int T = 0; T < 2; ++T) dh[T] = splat4(0.f);
        for (int t = 0; t < 6; ++t) da[t] = splat4(0.f);
        PairIn cur;
        load_step(0, cur, true);
        for (int it = 0; it < N - 1; ++it) {
            const int s = dir ? it : (N - 2 - it);
            const float dd = cur.dd;
            f32x4 dgh[6], dhd[2], dni[2];
            f32x4 hpm[2], hnr[2];
            for (int T = 0; T < 2; ++T) hpm[T] = zero_unless(cur.has_prev, cur.hp[T]);
            for (int T = 0; T < 2; ++T) {                          // gh_n = W_hn h_prev + b_hn, recomputed (not in the record)
                f32x4 acc = *reinterpret_cast<const f32x4*>(&s_bhn[dir][16 * T + 4 * g]);
                for (int Tk = 0; Tk < 2; ++Tk) {
                    f32x4 wf;
                    for (int q = 0; q < 4; ++q) wf[q] = swT[(16 * Tk + 4 * g + q) * WLD + 2 * SH + 16 * T + n];
                    acc = mma_block(wf, hpm[Tk], acc);
                }
                hnr[T] = acc;
            }
            for (int T = 0; T < 2; ++T) {
                f32x4 dht;
                for (int q = 0; q < 4; ++q) dht[q] = fmaf(wdiff[T][q], dd, dh[T][q]);
                const GruGrads o2 = gru_gates_bwd(dht, cur.r[T], cur.z[T], cur.nn[T], hnr[T], hpm[T]);
                da[T] += o2.dr; da[2 + T] += o2.dz; da[4 + T] += o2.dni;
                dgh[T] = o2.dr; dgh[2 + T] = o2.dz; dgh[4 + T] = o2.dnh;
                dni[T] = o2.dni;
                dhd[T] = o2.dh_direct;
            }
            if (valid) {
                float* row = srow + (int64_t)s * SG;
                for (int t = 0; t < 4; ++t) *reinterpret_cast<f32x4*>(row + 16 * t) = dgh[t];
                for (int T = 0; T < 2; ++T) *reinterpret_cast<f32x4*>(row + 16 * (4 + T)) = dni[T];
            }
            IPLAN_SCHED_FENCE();
            for (int T = 0; T < 2; ++T) cur.hs[T] = cur.hp[T];
            load_step(it + 1 < N - 1 ? it + 1 : it, cur, false);
            IPLAN_SCHED_FENCE();
            for (int T = 0; T < 2; ++T) {
                f32x4 acc = dhd[T];
                for (int t = 0; t < 6; ++t) acc = mma_block(wfrag_lds(swT, WLD, 16 * T, 16 * t), dgh[t], acc);
                dh[T] = acc;
            }
        }
        if (valid) {
            float* row = scr_sum + ((int64_t)dir * N + node) * SG + 4 * g;
            for (int t = 0; t < 6; ++t) *reinterpret_cast<f32x4*>(row + 16 * t) = da[t];
        }
    }
    __syncthreads();                                                // the scratch rows are read by other waves below

    // ---------------------------------------------------------------- P: per (ego, entity) pair -> G[i, j, :]
    // wave jt owns the entities j = 16 jt + n (the MFMA's 16 chains) and walks the egos in ascending order
    const int NT_live = (N + 15) / 16;
    if (w < NT_live) {
        const int jt = w;
        const int j = 16 * jt + n;
        const bool jvalid = j < N;
        const int jc = imin(j, N - 1);
        const int KT = (D + 15) / 16;
        const int n_src = f.d1 > 0 ? 2 : 1;
        f32x4 hmask[2];                                             // [h_j > 0] as 1 / 0
        {
            const float* hrow = sv.h_enc + (sb * N + jc) * SH;
            for (int T = 0; T < 2; ++T) {
                const f32x4 he = vload(hrow, jvalid, SH, T);
                for (int q = 0; q < 4; ++q) hmask[T][q] = he[q] > 0.f ? 1.f : 0.f;
            }
        }
        const float* r0 = f.src0 + (int64_t)net * f.src0_s_net + (int64_t)b * f.src0_s_b + (int64_t)jc * f.d0;
        const float* r1 = f.d1 > 0 ? f.src1 + (int64_t)net * f.src1_s_net + (int64_t)b * f.src1_s_b + (int64_t)jc * f.d1 : nullptr;
        float* gbase = a.grad ? a.grad + (int64_t)net * a.grad_s_net + (int64_t)b * a.grad_s_b : nullptr;
        float* l1base = a.pair_gl1 ? a.pair_gl1 + (int64_t)net * a.pair_s_net + (int64_t)b * a.pair_s_b : nullptr;
        float* xibase = a.pair_gxi ? a.pair_gxi + (int64_t)net * a.pair_s_net + (int64_t)b * a.pair_s_b : nullptr;
        float* igrow = a.input_grad ? a.input_grad + (int64_t)net * a.ig_s_net + (int64_t)b * a.ig_s_b + (int64_t)jc * D : nullptr;
        for (int c0 = 0; c0 < KT; c0 += SCT) {                      // (one pass for D <= 64; wider inputs walk the egos again)
            f32x4 acc[SCT], xo[SCT];
            for (int ct = 0; ct < SCT; ++ct) {
                acc[ct] = splat4(0.f);
                xo[ct] = splat4(0.f);
                if (jvalid)
                    for (int q = 0; q < 4; ++q) {
                        const int c = 16 * (c0 + ct) + 4 * g + q;
                        if (c < f.d0) xo[ct][q] = r0[c];
                        else if (c < D) xo[ct][q] = r1[c - f.d0];
                    }
            }
            for (int i = 0; i < N; ++i) {
                const float* Pi = sal_opaque(P);
                const bool ok = jvalid && j != i;
                const int s = ok ? j - (j > i ? 1 : 0) : 0;
                f32x4 u[2];
                u[0] = splat4(0.f); u[1] = splat4(0.f);
                if (through) {
                    for (int d2 = 0; d2 < 2; ++d2) {
                        const float* Wih = Pi + f.off[d2 ? IPLAN_GAT_R_WIH : IPLAN_GAT_F_WIH];                // [3H][2H]
                        const float* grow = scr + (((int64_t)d2 * N + i) * (N - 1) + s) * SG + 4 * g;
                        for (int t = 0; t < 6; ++t) {
                            const f32x4 gv = zero_unless(ok, *reinterpret_cast<const f32x4*>(grow + 16 * t));
                            for (int T = 0; T < 2; ++T) u[T] = mma_block(wfrag_t(Wih, 2 * SH, 3 * SH, 2 * SH, SH + 16 * T, 16 * t), gv, u[T]);
                        }
                    }
                }
                {
                    const float ds = ok ? s_ds[i][s] : 0.f;
                    const float wv = ok ? s_w[i][s] : 0.f;
                    f32x4 dk[2], dv[2];
                    for (int T = 0; T < 2; ++T)
                        for (int q = 0; q < 4; ++q) {
                            const int c = 16 * T + 4 * g + q;
                            dk[T][q] = ds * s_q[i][c];
                            dv[T][q] = s_v[jc][c] > 0.f ? wv * s_dx[i][c] : 0.f;                            // v = ReLU(.)
                        }
                    for (int T = 0; T < 2; ++T) {
                        u[T] = dense_tile_gt<2>(Pi + f.off[IPLAN_GAT_K_W], SH, SH, SH, 16 * T, dk, u[T]);
                        u[T] = dense_tile_gt<2>(Pi + f.off[IPLAN_GAT_V_W], SH, SH, SH, 16 * T, dv, u[T]);
                    }
                }
                if ((i >> 4) == jt) {                               // the ego's own row is one of this tile's chains
                    const bool diag = j == i;
                    if (through) {
                        for (int d2 = 0; d2 < 2; ++d2) {
                            const float* Wih = Pi + f.off[d2 ? IPLAN_GAT_R_WIH : IPLAN_GAT_F_WIH];
                            const float* arow = scr_sum + ((int64_t)d2 * N + i) * SG + 4 * g;
                            for (int t = 0; t < 6; ++t) {
                                const f32x4 gv = zero_unless(diag, *reinterpret_cast<const f32x4*>(arow + 16 * t));
                                for (int T = 0; T < 2; ++T) u[T] = mma_block(wfrag_t(Wih, 2 * SH, 3 * SH, 2 * SH, 16 * T, 16 * t), gv, u[T]);
                            }
                        }
                    }
                    f32x4 dq[2];
                    for (int T = 0; T < 2; ++T)
                        for (int q = 0; q < 4; ++q) dq[T][q] = diag ? s_dq[i][16 * T + 4 * g + q] : 0.f;
                    for (int T = 0; T < 2; ++T) u[T] = dense_tile_gt<2>(Pi + f.off[IPLAN_GAT_Q_W], SH, SH, SH, 16 * T, dq, u[T]);
                }
                for (int T = 0; T < 2; ++T) u[T] *= hmask[T];       // encoding's ReLU
                float gl1[2] = {0.f, 0.f}, gxi[2] = {0.f, 0.f};
                const float* Wenc = Pi + f.off[IPLAN_GAT_ENC_W];     // [H][D]
                for (int ct = 0; ct < SCT; ++ct) {
                    if (c0 + ct >= KT) break;
                    const f32x4 G = dense_tile_gt<2>(Wenc, D, SH, D, 16 * (c0 + ct), u, splat4(0.f));
                    acc[ct] = acc[ct] + G;                          // input_grad: one rounded add per ego, ascending
                    for (int q = 0; q < 4; ++q) {
                        const int c = 16 * (c0 + ct) + 4 * g + q;
                        if (c < D) {
                            const int src = c < f.d0 ? 0 : 1;
                            gl1[src] += fabsf(G[q]);
                            gxi[src] = fmaf(G[q], xo[ct][q], gxi[src]);
                            if (gbase && jvalid) gbase[((int64_t)i * N + j) * D + c] = G[q];
                        }
                    }
                }
                if (l1base || xibase) {
                    for (int src = 0; src < n_src; ++src) {
                        const float t1 = group_sum(gl1[src]), t2 = group_sum(gxi[src]);
                        if (g == 0 && jvalid) {
                            const int64_t e = ((int64_t)i * N + j) * n_src + src;
                            // (a later column pass adds to what this lane stored in the pass before)
                            if (l1base) l1base[e] = c0 ? l1base[e] + t1 : t1;
                            if (xibase) xibase[e] = c0 ? xibase[e] + t2 : t2;
                        }
                    }
                }
            }
            if (igrow && jvalid)
                for (int ct = 0; ct < SCT; ++ct)
                    for (int q = 0; q < 4; ++q) {
                        const int c = 16 * (c0 + ct) + 4 * g + q;
                        if (c < D) igrow[c] = acc[ct][q];
                    }
        }
    }
}

}  // namespace iplan

extern "C" int iplan_gat_saliency(const IplanGatSaliencyArgs* a, iplan_stream_t stream) {
    using namespace iplan;
    if (!a) return fail(IPLAN_EINVAL, "iplan_gat_saliency: null args");
    const IplanGatFwdArgs& f = a->fwd;
    if (f.N < 2 || f.N > IPLAN_MAX_ENTITIES)
        return fail(IPLAN_EINVAL, "iplan_gat_saliency: N=%d outside [2,%d]", f.N, IPLAN_MAX_ENTITIES);
    if (f.n_nets < 1 || f.B < 1 || f.d0 < 1 || f.d1 < 0 || (int64_t)f.n_nets * f.B > 0x7fffffff)
        return fail(IPLAN_EINVAL, "iplan_gat_saliency: bad dims n_nets=%d B=%d d0=%d d1=%d", f.n_nets, f.B, f.d0, f.d1);
    if (a->gate_through != 0 && a->gate_through != 1)
        return fail(IPLAN_EINVAL, "iplan_gat_saliency: gate_through=%d is neither 0 (held) nor 1 (through)", a->gate_through);
    const IplanGatSaved& s = f.saved;
    if (!s.h_enc || !s.qkv || !s.soft || !s.hard || !s.cell || (a->gate_through && !s.gru))
        return fail(IPLAN_EINVAL, "iplan_gat_saliency: the forward launch did not save its activations");
    if (!a->v || !f.h_prev || !f.params || !f.src0 || (f.d1 > 0 && !f.src1))
        return fail(IPLAN_EINVAL, "iplan_gat_saliency: null tensor pointer");
    if (!a->grad && !a->pair_gl1 && !a->pair_gxi && !a->input_grad && !a->hidden_grad)
        return fail(IPLAN_EINVAL, "iplan_gat_saliency: no output asked for");
    if (a->gate_through) {
        if (!(f.tau > 0.f)) return fail(IPLAN_EINVAL, "iplan_gat_saliency: tau=%g must be positive", (double)f.tau);
        const int64_t need = (int64_t)f.n_nets * f.B * 2 * f.N * f.N * 3 * IPLAN_GAT_HIDDEN;
        if (!a->scratch || a->scratch_floats < need)
            return fail(IPLAN_EINVAL, "iplan_gat_saliency: scratch of %lld floats, %lld are needed", (long long)(a->scratch ? a->scratch_floats : 0),
                        (long long)need);
        if (!aligned16(a->scratch) || !aligned16(s.gru))
            return fail(IPLAN_EALIGN, "iplan_gat_saliency: scratch and the pair-GRU record must be 16-byte aligned");
    }
    hipLaunchKernelGGL(gat_saliency_kernel, dim3((unsigned)(f.n_nets * f.B)), dim3(512), 0, (hipStream_t)stream, *a);
    return check_launch("iplan_gat_saliency");
}
