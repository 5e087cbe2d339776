// The 32-wide chain  Linear(in <= 16 -> 32) -> ReLU -> GRU32 -> Linear(32 -> out <= 16)  with every weight in LDS in BOTH orientations: what
// the input-gradient kernels of the behaviour encoder (enc_saliency.hip) and of the prediction decoder (pdec_saliency.hip) share.  One wave
// walks a 16-row tile; each file keeps what follows the GRU (softmax and soft update there, tanh and the fed-back output here) to itself.
// Layout: the weights are staged once per workgroup (69 568 bytes), then one slab per wave of C_STEP_FLOATS per chain step: the state a
// step ENTERS with (16 rows x 32) and one more row of 16 x 16 (the encoder's pending gradient row, the decoder's input).  A slab is
// lane-private (every lane reads back only what it wrote: D layout in, D layout out), so a wave never waits for another; the 160 KB of
// a CU admit 30 steps of one wave beside the weights, and the number of waves per workgroup follows from the steps asked for.
#pragma once
#include "api_util.h"
#include "gru_tile.h"

namespace iplan {

constexpr int CH = 32, CHT = 2, CHLD = CH + 8;     // hidden width; leading dims: ld % 16 == 8 -> conflict-free fragment reads
constexpr int CLLD = 24;                           // leading dim of [.. x 16] matrices (in, out <= 16 real columns)
constexpr int CGLD = 3 * CH + 8;                   // leading dim of the transposed GRU weights [32 x 96]
constexpr int C_LIN = 0;                           // W_lin   [32 x in]
constexpr int C_LINT = C_LIN + CH * CLLD;          // W_lin^T [16 x 32]
constexpr int C_WIH = C_LINT + 16 * CHLD;          // W_ih    [96 x 32]
constexpr int C_WHH = C_WIH + 3 * CH * CHLD;       // W_hh    [96 x 32]
constexpr int C_WIHT = C_WHH + 3 * CH * CHLD;      // W_ih^T  [32 x 96]
constexpr int C_WHHT = C_WIHT + CH * CGLD;         // W_hh^T  [32 x 96]
constexpr int C_OUT = C_WHHT + CH * CGLD;          // W_out   [out x 32]
constexpr int C_OUTT = C_OUT + 16 * CHLD;          // W_out^T [32 x out]
constexpr int C_B = C_OUTT + CH * CLLD;            // biases: linear (32) | b_ih (96) | b_hh (96) | out (16)
constexpr int C_BIH = C_B + CH, C_BHH = C_BIH + 3 * CH, C_BOUT = C_BHH + 3 * CH;
constexpr int C_W_FLOATS = C_BOUT + 16;
constexpr int C_LDS_FLOATS = 160 * 1024 / 4;
constexpr int C_STEP_FLOATS = 16 * CH + 16 * 16;   // per wave and chain step
static_assert(C_W_FLOATS % 4 == 0 && C_B % 4 == 0 && C_LINT % 4 == 0 && C_OUTT % 4 == 0, "16-byte aligned fragments");
static_assert(IPLAN_ENC_LIN_W == IPLAN_DEC_LIN_W && IPLAN_ENC_LIN_B == IPLAN_DEC_LIN_B && IPLAN_ENC_WIH == IPLAN_DEC_WIH &&
                  IPLAN_ENC_WHH == IPLAN_DEC_WHH && IPLAN_ENC_BIH == IPLAN_DEC_BIH && IPLAN_ENC_BHH == IPLAN_DEC_BHH &&
                  IPLAN_ENC_OUT_W == IPLAN_DEC_OUT_W && IPLAN_ENC_OUT_B == IPLAN_DEC_OUT_B && IPLAN_ENC_NPARAM == IPLAN_DEC_NPARAM,
              "chain_stage reads an encoder's and a decoder's offset table by the same indices");

// one wave's slab of `steps` chain steps fits beside the weights
constexpr bool chain_fits(int steps) { return C_W_FLOATS + steps * C_STEP_FLOATS <= C_LDS_FLOATS; }

inline int chain_waves(int steps) { return imin(4, (C_LDS_FLOATS - C_W_FLOATS) / (steps * C_STEP_FLOATS)); }

// the weights of one net (`P`: its parameters, `off`: the offset table, IPLAN_ENC_* = IPLAN_DEC_* order) into LDS; all threads call it
__device__ __forceinline__ void chain_stage(float* lds, const float* __restrict__ P, const int64_t* off, int in_dim, int out_dim) {
    stage_matrix(lds + C_LIN, CLLD, CH, P + off[IPLAN_ENC_LIN_W], CH, in_dim);
    stage_matrix_t(lds + C_LINT, CHLD, 16, P + off[IPLAN_ENC_LIN_W], CH, in_dim);
    stage_matrix(lds + C_WIH, CHLD, 3 * CH, P + off[IPLAN_ENC_WIH], 3 * CH, CH);
    stage_matrix(lds + C_WHH, CHLD, 3 * CH, P + off[IPLAN_ENC_WHH], 3 * CH, CH);
    stage_matrix_t(lds + C_WIHT, CGLD, CH, P + off[IPLAN_ENC_WIH], 3 * CH, CH);
    stage_matrix_t(lds + C_WHHT, CGLD, CH, P + off[IPLAN_ENC_WHH], 3 * CH, CH);
    stage_matrix(lds + C_OUT, CHLD, 16, P + off[IPLAN_ENC_OUT_W], out_dim, CH);
    stage_matrix_t(lds + C_OUTT, CLLD, CH, P + off[IPLAN_ENC_OUT_W], out_dim, CH);
    stage_vector(lds + C_B, CH, P + off[IPLAN_ENC_LIN_B], CH);
    stage_vector(lds + C_BIH, 3 * CH, P + off[IPLAN_ENC_BIH], 3 * CH);
    stage_vector(lds + C_BHH, 3 * CH, P + off[IPLAN_ENC_BHH], 3 * CH);
    stage_vector(lds + C_BOUT, 16, P + off[IPLAN_ENC_OUT_B], out_dim);
}

// columns 4g .. 4g+3 of a d-wide row that need not be 16-byte aligned, zero past column d and where `ok` is false (the loads are
// clamped to the row and masked bitwise: a NaN in a float that is not the row's own never enters the arithmetic)
__device__ __forceinline__ f32x4 chain_row_load(const float* __restrict__ row, bool ok, int d, int g) {
    const IPLAN_GLOBAL_AS float* p = as_global(row);
    f32x4 v;
    for (int q = 0; q < 4; ++q) {
        const int i = 4 * g + q;
        v[q] = keep_if(ok && i < d, p[i < d ? i : d - 1]);
    }
    return v;
}

// the matching store: columns 4g .. 4g+3 below d, of valid rows
__device__ __forceinline__ void chain_row_store(float* __restrict__ row, bool valid, int d, int g, f32x4 v) {
    for (int q = 0; q < 4; ++q)
        if (valid && 4 * g + q < d) row[4 * g + q] = v[q];
}

// one chain step: u = ReLU(W_lin x + b_lin), h = GRU32(u, h); `keep`: the gate activations for the backward pass
__device__ __forceinline__ void chain_step(const float* lds, f32x4 x, f32x4 (&u)[CHT], f32x4 (&h)[CHT], GruGates* keep) {
    const f32x4 xin[1] = {x};
    for (int T = 0; T < CHT; ++T) u[T] = relu4(dense_tile<1>(lds + C_LIN, CLLD, 16 * T, xin, bfrag_lds(lds + C_B, T)));
    gru_step_lds<CHT, CHT>(lds + C_WIH, CHLD, lds + C_WHH, CHLD, lds + C_BIH, lds + C_BHH, u, h, keep);
}

// the lane's ReLU branches of a step: bit 16 T + 4 g + q is set where u[T][q] > 0
__device__ __forceinline__ uint32_t chain_relu_bits(const f32x4 (&u)[CHT], int g) {
    uint32_t bits = 0;
    for (int T = 0; T < CHT; ++T)
        for (int q = 0; q < 4; ++q) bits |= u[T][q] > 0.0f ? 1u << (16 * T + 4 * g + q) : 0u;
    return bits;
}

// a row's 32-bit branch word: the OR over its four lanes
__device__ __forceinline__ uint32_t chain_row_or(uint32_t bits) {
    int b = (int)bits;
    b |= __shfl_xor(b, 16);
    b |= __shfl_xor(b, 32);
    return (uint32_t)b;
}

// the same step backwards, from what chain_step kept and the state `hp` it entered with.  In: dh = the gradient on h_t (the caller has
// added what reads h_t beside the next step).  Out: dh = the gradient on h_{t-1}; returns dx_t; `bits` (may be null): chain_relu_bits(u),
// formed in the mask loop and not by that helper (with it the encoder's BPTT took 0.25 % longer: profiles/r19 notes).
//    [dr dz dn] from gru_gates_bwd,   dh = z dh + W_hh^T [dr | dz | r dn],   dx_t = W_lin^T (relu' . W_ih^T [dr | dz | dn])
__device__ __forceinline__ f32x4 chain_step_bwd(const float* lds, const GruGates (&keep)[CHT], const f32x4 (&hp)[CHT], const f32x4 (&u)[CHT],
                                                f32x4 (&dh)[CHT], int g, uint32_t* bits) {
    f32x4 di[3 * CHT], dg[3 * CHT], direct[CHT];
    for (int T = 0; T < CHT; ++T) {
        const GruGrads o = gru_gates_bwd(dh[T], keep[T].r, keep[T].z, keep[T].n, keep[T].hn, hp[T]);
        di[T] = dg[T] = o.dr;
        di[CHT + T] = dg[CHT + T] = o.dz;
        di[2 * CHT + T] = o.dni;
        dg[2 * CHT + T] = o.dnh;
        direct[T] = o.dh_direct;
    }
    f32x4 du[CHT];
    uint32_t b = 0;
    for (int T = 0; T < CHT; ++T) {
        du[T] = dense_tile<3 * CHT>(lds + C_WIHT, CGLD, 16 * T, di, splat4(0.f));
        dh[T] = dense_tile<3 * CHT>(lds + C_WHHT, CGLD, 16 * T, dg, direct[T]);
        for (int q = 0; q < 4; ++q) {
            const bool on = u[T][q] > 0.0f;
            du[T][q] = on ? du[T][q] : 0.0f;
            b |= on ? 1u << (16 * T + 4 * g + q) : 0u;
        }
    }
    if (bits) *bits = b;
    return dense_tile<CHT>(lds + C_LINT, CHLD, 0, du, splat4(0.f));
}

}  // namespace iplan
