// Attention saliency through time: gat_saliency.hip's input backward chained over the past steps of the ego's own latent.
//
// The GAT's output GRUCell reads only the ego's own previous latent, so through time the egos stay apart: with c_i^(-1) = v_i,
// lag k of target step s is the one-step saliency at step s - k with the cotangent c_i^(k-1), and its hidden gradient is
// c_i^(k) = d y_{s,i} / d latent_{s-k-1,i}.  The record is ONE training-form forward launch over the rows (env, record step); every
// target and lag that reaches a row reads it in place.
//
// One 512-thread workgroup per (net, env, target) walks the lags k = 0 .. min(K, r) (r = the target's record step).  Every lag runs
// the phases A, B, D, P of gat_saliency_kernel on the record row of step r - k, restated here statement for statement so that a
// lag's bits are that kernel's bits (both files are built with the same flags).  What differs:
//   - the cotangent rows live in an LDS table [N][33]: lag 0 fills it from v, phase A of lag k reads its row and writes c^(k) back
//     (every lane reads and rewrites its own four columns), so the carry never travels through global memory;
//   - the workgroup's pair-step scratch is reused by every lag;
//   - carry_sq[i] = sum_c c^(k)[i][c]^2, one lane per ego, columns ascending, every product and sum rounded on its own;
//   - the slots of lags that do not exist (k > r) are written +0.0 here, so the outputs need no prefill.
// No atomics and no sums across workgroups: a slot's bits depend on its own operands only.
#include "api_util.h"
#include "gru_tile.h"

namespace iplan {

constexpr int SH = IPLAN_GAT_HIDDEN;   // H == A == 32
constexpr int SNP = IPLAN_MAX_ENTITIES;
constexpr int SQS = 33;                // padded row stride of the q / k / v / dx / dq / cotangent tables
constexpr int SG = 3 * SH;             // [dr dz dn_i] of one pair step
constexpr int SCT = 4;                 // column tiles of G a wave holds the running input_grad of at a time

// the parameter pointer as a value the compiler knows nothing about (gat_saliency.hip's sal_opaque)
__device__ __forceinline__ const float* salt_opaque(const float* p) {
#ifndef IPLAN_HOST_EMULATION
    asm volatile("" : "+s"(p));
#endif
    return p;
}

// sum_c x[c]^2 over the SH columns, c ascending; contraction off, so the plain fp32 host loop gives the same bits (knock_shift.h)
__device__ __forceinline__ float carry_sq_row(const float* x) {
#pragma clang fp contract(off)
    float s = 0.f;
    for (int c = 0; c < SH; ++c) {
        const float p = x[c] * x[c];
        s = s + p;
    }
    return s;
}

// +0.0 into cnt floats at dst (the slot of a lag that does not exist)
__device__ __forceinline__ void zero_slot(float* dst, int cnt) {
    if (dst)
        for (int idx = (int)threadIdx.x; idx < cnt; idx += (int)blockDim.x) dst[idx] = 0.f;
}

__global__ __launch_bounds__(512) void gat_saliency_trace_kernel(IplanGatSaliencyTraceArgs a) {
    __shared__ float s_q[SNP][SQS];
    __shared__ float s_k[SNP][SQS];
    __shared__ float s_v[SNP][SQS];
    __shared__ float s_dx[SNP][SQS];
    __shared__ float s_dq[SNP][SQS];
    __shared__ float s_c[SNP][SQS];                                 // the cotangent rows: v at lag 0, then c^(k-1)
    __shared__ float s_ds[SNP][SNP];                                // d score (1/sqrt(A) included) per (ego, slot)
    __shared__ float s_w[SNP][SNP];                                 // soft * hard
    __shared__ float s_dd[SNP][SNP];                                // d(l1 - l0)
    constexpr int WLD = 3 * SH + 8;                                 // W_hh^T [H][3H + 8]: conflict-free ds_read_b128 fragments
    __shared__ __attribute__((aligned(16))) float s_whh[2][SH * WLD];
    __shared__ __attribute__((aligned(16))) float s_bhn[2][SH];

    const IplanGatFwdArgs& f = a.fwd;
    const IplanGatSaved& sv = f.saved;
    const int wg = (int)blockIdx.x;
    const int tgt = wg % a.T;
    const int b = (wg / a.T) % a.B;
    const int net = wg / (a.T * a.B);
    const int r = a.targets[tgt];                                   // the target's record step (checked on the host)
    const int N = f.N;
    const int D = f.d0 + f.d1;
    const int n_src = f.d1 > 0 ? 2 : 1;
    const float* __restrict__ P0 = f.params + (int64_t)net * f.params_s_net;
    const int l = lane_id(), w = wave_id();
    const int n = l & 15, g = l >> 4;
    const int tile = w & 3, dir = w >> 2;
    const int node = 16 * tile + n;
    const bool tile_live = 16 * tile < N;
    const bool valid = node < N;
    const bool through = a.gate_through != 0;
    // scratch of this workgroup, reused by every lag: [2][N][N-1][3H] pair-step gate gradients, then [2][N][3H] their sums
    float* __restrict__ scr = through ? a.scratch + (int64_t)wg * (int64_t)(2 * N * N * SG) : nullptr;
    float* __restrict__ scr_sum = through ? scr + (int64_t)2 * N * (N - 1) * SG : nullptr;

    if (through) {
        stage_matrix_t(s_whh[0], WLD, SH, P0 + f.off[IPLAN_GAT_F_WHH], 3 * SH, SH);
        stage_matrix_t(s_whh[1], WLD, SH, P0 + f.off[IPLAN_GAT_R_WHH], 3 * SH, SH);
        if (threadIdx.x < 2 * SH)                                   // b_hn of both directions (the recomputed gh_n's bias)
            s_bhn[threadIdx.x >> 5][threadIdx.x & 31] = P0[f.off[(threadIdx.x >> 5) ? IPLAN_GAT_R_BHH : IPLAN_GAT_F_BHH] + 2 * SH + (threadIdx.x & 31)];
    }
    {
        const float* vbase = a.v + (int64_t)net * a.v_s_net + (int64_t)b * a.v_s_b + (int64_t)tgt * a.v_s_t;
        for (int idx = (int)threadIdx.x; idx < N * SH; idx += (int)blockDim.x) s_c[idx / SH][idx % SH] = vbase[idx];
    }

    // lag 0's slot (net, b, target) of every output; lag k's is k * <its lag stride> further on
#define SALT_BASE(base, pre) ((base) ? (base) + (int64_t)net * a.pre##_s_net + (int64_t)b * a.pre##_s_b + (int64_t)tgt * a.pre##_s_t : nullptr)
#define SALT_SLOT(base, pre) ((base) ? (base) + (int64_t)k * a.pre##_s_k : nullptr)
    float* const grad_t = SALT_BASE(a.grad, grad);
    float* const l1_t = SALT_BASE(a.pair_gl1, pair);
    float* const xi_t = SALT_BASE(a.pair_gxi, pair);
    float* const ig_t = SALT_BASE(a.input_grad, ig);
    float* const carry_t = SALT_BASE(a.carry, carry);
    float* const csq_t = SALT_BASE(a.carry_sq, csq);
    const int k_end = imin(a.K, r);                                 // the last lag that exists
    for (int k = k_end + 1; k <= a.K; ++k) {                        // the others: +0.0
        zero_slot(SALT_SLOT(grad_t, grad), N * N * D);
        zero_slot(SALT_SLOT(l1_t, pair), N * N * n_src);
        zero_slot(SALT_SLOT(xi_t, pair), N * N * n_src);
        zero_slot(SALT_SLOT(ig_t, ig), N * D);
        zero_slot(SALT_SLOT(carry_t, carry), N * SH);
        zero_slot(SALT_SLOT(csq_t, csq), N);
    }

    for (int k = 0; k <= k_end; ++k) {
        const float* __restrict__ P = salt_opaque(P0);              // (nothing read through it is lifted out of the lag loop)
        const int brow = b * a.R + (r - k);                         // the record row of step r - k
        const int64_t sb = (int64_t)net * f.B + brow;

        for (int idx = (int)threadIdx.x; idx < N * 3 * SH; idx += (int)blockDim.x) {
            const int nd = idx / (3 * SH), c = idx - nd * 3 * SH;
            const float val = sv.qkv[(sb * N + nd) * 3 * SH + c];
            if (c < SH) s_q[nd][c] = val;
            else if (c < 2 * SH) s_k[nd][c - SH] = val;
            else s_v[nd][c - 2 * SH] = val;
        }
        __syncthreads();                                            // (also: lag 0's cotangent table and the staged weights)
        // ---------------------------------------------------------------- A: output GRUCell backward
        if (tile_live && dir == 0) {
            const float* crow = sv.cell + (sb * N + node) * (4 * SH);
            const float* hrow = f.h_prev + (int64_t)net * f.h_s_net + (int64_t)brow * f.h_s_b + (int64_t)node * SH;
            f32x4 dgi[6], dgh[6], dhd[2];
            for (int T = 0; T < 2; ++T) {
                f32x4 vv = splat4(0.f);
                if (valid)
                    for (int q = 0; q < 4; ++q) vv[q] = s_c[node][16 * T + 4 * g + q];
                const GruGrads o = gru_gates_bwd(vv, vload(crow, valid, SH, T), vload(crow + SH, valid, SH, T),
                                                 vload(crow + 2 * SH, valid, SH, T), vload(crow + 3 * SH, valid, SH, T),
                                                 vload(hrow, valid, SH, T));
                dgi[T] = o.dr; dgi[2 + T] = o.dz; dgi[4 + T] = o.dni;
                dgh[T] = o.dr; dgh[2 + T] = o.dz; dgh[4 + T] = o.dnh;
                dhd[T] = o.dh_direct;
            }
            const float* Wi = P + f.off[IPLAN_GAT_C_WIH];
            const float* Wc = P + f.off[IPLAN_GAT_C_WHH];
            float* cslot = SALT_SLOT(carry_t, carry);
            float* grow = cslot ? cslot + (int64_t)node * SH : nullptr;
            for (int T = 0; T < 2; ++T) {
                const f32x4 dx = dense_tile_gt<6>(Wi, SH, 3 * SH, SH, 16 * T, dgi, splat4(0.f));
                const f32x4 ck = dense_tile_gt<6>(Wc, SH, 3 * SH, SH, 16 * T, dgh, dhd[T]);
                if (valid)
                    for (int q = 0; q < 4; ++q) {
                        s_dx[node][16 * T + 4 * g + q] = dx[q];
                        s_c[node][16 * T + 4 * g + q] = ck[q];      // c^(k): the next lag's cotangent
                    }
                if (grow) vstore(grow, valid, SH, T, ck);
            }
        }
        __syncthreads();
        if (csq_t && (int)threadIdx.x < N) SALT_SLOT(csq_t, csq)[threadIdx.x] = carry_sq_row(s_c[threadIdx.x]);

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
        if (through && tile_live) {
            const float* swT = s_whh[dir];
            const float* Wh = P + f.off[IPLAN_GAT_HARD_W];                              // [2][2H]
            f32x4 wdiff[2];
            for (int T = 0; T < 2; ++T) wdiff[T] = bfrag(Wh + 2 * SH + dir * SH, SH, T) - bfrag(Wh + dir * SH, SH, T);
            const int cnode = imin(node, N - 1);
            const int NT = (N + 15) / 16;
            constexpr int REC = 8 * 256;
            const float* gbase = sv.gru + (((((int64_t)net * 2 + dir) * f.B + brow) * NT + tile) * (int64_t)(N - 1)) * REC + (cnode & 15) * 16 + 4 * g;
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
        __syncthreads();                                            // the scratch rows are read by other waves below

        // ---------------------------------------------------------------- P: per (ego, entity) pair -> G[i, j, :]
        // wave jt owns the entities j = 16 jt + n (the MFMA's 16 chains) and walks the egos in ascending order
        const int NT_live = (N + 15) / 16;
        if (w < NT_live) {
            const int jt = w;
            const int j = 16 * jt + n;
            const bool jvalid = j < N;
            const int jc = imin(j, N - 1);
            const int KT = (D + 15) / 16;
            f32x4 hmask[2];                                             // [h_j > 0] as 1 / 0
            {
                const float* hrow = sv.h_enc + (sb * N + jc) * SH;
                for (int T = 0; T < 2; ++T) {
                    const f32x4 he = vload(hrow, jvalid, SH, T);
                    for (int q = 0; q < 4; ++q) hmask[T][q] = he[q] > 0.f ? 1.f : 0.f;
                }
            }
            const float* r0 = f.src0 + (int64_t)net * f.src0_s_net + (int64_t)brow * f.src0_s_b + (int64_t)jc * f.d0;
            const float* r1 = f.d1 > 0 ? f.src1 + (int64_t)net * f.src1_s_net + (int64_t)brow * f.src1_s_b + (int64_t)jc * f.d1 : nullptr;
            float* gslot = SALT_SLOT(grad_t, grad);
            float* l1slot = SALT_SLOT(l1_t, pair);
            float* xislot = SALT_SLOT(xi_t, pair);
            float* igslot = SALT_SLOT(ig_t, ig);
            float* igrow = igslot ? igslot + (int64_t)jc * D : nullptr;
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
                    const float* Pi = salt_opaque(P);
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
                    float gl1_0 = 0.f, gl1_1 = 0.f, gxi_0 = 0.f, gxi_1 = 0.f;   // per source; scalars, not an indexed array: that went to scratch memory here
                    const float* Wenc = Pi + f.off[IPLAN_GAT_ENC_W];     // [H][D]
                    for (int ct = 0; ct < SCT; ++ct) {
                        if (c0 + ct >= KT) break;
                        const f32x4 G = dense_tile_gt<2>(Wenc, D, SH, D, 16 * (c0 + ct), u, splat4(0.f));
                        acc[ct] = acc[ct] + G;                          // input_grad: one rounded add per ego, ascending
                        for (int q = 0; q < 4; ++q) {
                            const int c = 16 * (c0 + ct) + 4 * g + q;
                            if (c < D) {
                                if (c < f.d0) {
                                    gl1_0 += fabsf(G[q]);
                                    gxi_0 = fmaf(G[q], xo[ct][q], gxi_0);
                                } else {
                                    gl1_1 += fabsf(G[q]);
                                    gxi_1 = fmaf(G[q], xo[ct][q], gxi_1);
                                }
                                if (gslot && jvalid) gslot[((int64_t)i * N + j) * D + c] = G[q];
                            }
                        }
                    }
                    if (l1slot || xislot) {
                        for (int src = 0; src < n_src; ++src) {
                            const float t1 = group_sum(src ? gl1_1 : gl1_0), t2 = group_sum(src ? gxi_1 : gxi_0);
                            if (g == 0 && jvalid) {
                                const int64_t e = ((int64_t)i * N + j) * n_src + src;
                                // (a later column pass adds to what this lane stored in the pass before)
                                if (l1slot) l1slot[e] = c0 ? l1slot[e] + t1 : t1;
                                if (xislot) xislot[e] = c0 ? xislot[e] + t2 : t2;
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
        __syncthreads();                                            // the tables and the scratch are the next lag's
    }
#undef SALT_SLOT
#undef SALT_BASE
}

}  // namespace iplan

extern "C" int iplan_gat_saliency_trace(const IplanGatSaliencyTraceArgs* a, iplan_stream_t stream) {
    using namespace iplan;
    if (!a) return fail(IPLAN_EINVAL, "iplan_gat_saliency_trace: null args");
    const IplanGatFwdArgs& f = a->fwd;
    if (f.N < 2 || f.N > IPLAN_MAX_ENTITIES)
        return fail(IPLAN_EINVAL, "iplan_gat_saliency_trace: N=%d outside [2,%d]", f.N, IPLAN_MAX_ENTITIES);
    if (f.n_nets < 1 || a->B < 1 || a->R < 1 || f.d0 < 1 || f.d1 < 0)
        return fail(IPLAN_EINVAL, "iplan_gat_saliency_trace: bad dims n_nets=%d B=%d R=%d d0=%d d1=%d", f.n_nets, a->B, a->R, f.d0, f.d1);
    if ((int64_t)a->B * a->R != f.B)
        return fail(IPLAN_EINVAL, "iplan_gat_saliency_trace: the record holds %d rows per net, B * R = %lld", f.B, (long long)a->B * a->R);
    if (a->T < 1) return fail(IPLAN_EINVAL, "iplan_gat_saliency_trace: T=%d, at least one target is needed", a->T);
    if (a->K < 0) return fail(IPLAN_EINVAL, "iplan_gat_saliency_trace: K=%d is negative", a->K);
    if ((int64_t)f.n_nets * a->B * a->T > 0x7fffffff)
        return fail(IPLAN_EINVAL, "iplan_gat_saliency_trace: n_nets * B * T = %lld workgroups exceed 2^31 - 1", (long long)f.n_nets * a->B * a->T);
    if (a->gate_through != 0 && a->gate_through != 1)
        return fail(IPLAN_EINVAL, "iplan_gat_saliency_trace: gate_through=%d is neither 0 (held) nor 1 (through)", a->gate_through);
    const IplanGatSaved& s = f.saved;
    if (!s.h_enc || !s.qkv || !s.soft || !s.hard || !s.cell || (a->gate_through && !s.gru))
        return fail(IPLAN_EINVAL, "iplan_gat_saliency_trace: the forward launch did not save its activations");
    if (!a->v || !f.h_prev || !f.params || !f.src0 || (f.d1 > 0 && !f.src1))
        return fail(IPLAN_EINVAL, "iplan_gat_saliency_trace: null tensor pointer");
    if (!a->targets || !a->targets_host) return fail(IPLAN_EINVAL, "iplan_gat_saliency_trace: the target list is missing (device and host copy)");
    for (int t = 0; t < a->T; ++t)
        if (a->targets_host[t] < 0 || a->targets_host[t] >= a->R)
            return fail(IPLAN_EINVAL, "iplan_gat_saliency_trace: target %d = step %d outside the record window [0,%d)", t, a->targets_host[t], a->R);
    if (!a->grad && !a->pair_gl1 && !a->pair_gxi && !a->input_grad && !a->carry && !a->carry_sq)
        return fail(IPLAN_EINVAL, "iplan_gat_saliency_trace: no output asked for");
    if (a->gate_through) {
        if (!(f.tau > 0.f)) return fail(IPLAN_EINVAL, "iplan_gat_saliency_trace: tau=%g must be positive", (double)f.tau);
        const int64_t need = (int64_t)f.n_nets * a->B * a->T * 2 * f.N * f.N * 3 * IPLAN_GAT_HIDDEN;
        if (!a->scratch || a->scratch_floats < need)
            return fail(IPLAN_EINVAL, "iplan_gat_saliency_trace: scratch of %lld floats, %lld are needed", (long long)(a->scratch ? a->scratch_floats : 0),
                        (long long)need);
        if (!aligned16(a->scratch) || !aligned16(s.gru))
            return fail(IPLAN_EALIGN, "iplan_gat_saliency_trace: scratch and the pair-GRU record must be 16-byte aligned");
    }
    hipLaunchKernelGGL(gat_saliency_trace_kernel, dim3((unsigned)(f.n_nets * a->B * a->T)), dim3(512), 0, (hipStream_t)stream, *a);
    return check_launch("iplan_gat_saliency_trace");
}
