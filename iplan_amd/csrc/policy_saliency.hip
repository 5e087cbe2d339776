// Policy saliency: d log pi(a* | x) / d x of the actors and d V / d x of the critics for E*S independent rows, the GRU state given and
// held constant (include/iplan_hip.h: IplanAcSaliencyArgs).  One row-parallel kernel, forward + input-backward:
//
//   LN(F) -> fc1 -> act -> LN -> fc2 -> act -> LN -> GRU cell (h given) -> LN -> head -> y      y = log_softmax(masked logits)[a*] | V
//   dx <- LN(F)' <- fc1^T <- act' <- LN' <- fc2^T <- act' <- LN' <- W_ih^T <- gates' <- LN' <- head^T <- dy = 1
//
// Shape: the trunk kernel of policy_trace.hip -- one wave per 16-row tile, four tiles per workgroup, grid = ceil(tiles / 4) x n_agents x
// nets, rows gathered in place through the K map (ac_kmap.h), the 64-wide layers from L2-resident weights.  The forward half is that
// kernel's arithmetic (same k-tile order, same partial sums of every 8 k-tiles) followed by the walk kernel's step with the recurrent
// product taken by this wave alone.  Everything 64 wide stays in registers in the D layout (wave_tile.h); a transposed layer is the
// same MFMA chain with the A fragment read down a column of the weight matrix (wfrag_ta).
//
// The F axis is passed over five times and nothing F wide is kept:
//   1, 2  mean, centred second moment of x                      (LayerNorm(F) statistics, as the trunk kernel takes them)
//   3     z1 = W1 LN(x) + b1                                     (fc1 on v_mfma_f32_16x16x4_f32)
//   4     u = W1^T delta, g^ = gamma u:  mean g^, mean g^ x^     (fc1^T on the same instruction: 16 MFMAs per k-tile)
//   5     u again, dx = (g^ - mean g^ - x^ mean(g^ x^)) / sigma  -> input_grad, and the per-entity sums
// fc1^T per k-tile: the tile's 16 K-order entries are the OUTPUT rows, the 64 hidden units the contraction.  A = W1^T: lane (m, g) reads
// W1[16 t + 4 g + q][column of entry m]; B = delta in the D layout; D: lane (n, g) gets u of entries 4 g .. 4 g + 3 of row n -- the very
// entries ktile() / kfeat() hand this lane, so x, gamma and u meet lane-locally.  From the fragment-major pack the same element is
// packed[((T * 4 + t) * 64 + (4 g + q) + 16 (m >> 2)) * 4 + (m & 3)]: same values (zeros past a block's end in both), same instructions.
//
// Per-entity sums (sum g x, sum |g| over one source's columns of one entity): an entity's columns straddle lanes and k-tiles (w = 5), so
// the tile's 16 products go through 2 x 16 x 16 floats of LDS per wave and ONE lane per row (g = 0) adds them in K order -- which inside
// a source block is the reference's column order -- carrying the running sum across k-tiles and storing it when the entity's last column
// has been added.  Hand-off inside the wave only (IPLAN_WAVE_SYNC), no barrier in the kernel.
//
// Determinism: a row's arithmetic is lane-local apart from the MFMAs (column n of the product depends on column n of B only), the fixed
// xor butterflies over the row's four lanes and the row's own LDS line; no atomics, no cross-row sums.  Writes: the requested outputs
// only; parameter, gradient and batch memory is read.
// The body is sal_body.h / sal_body_impl.h (MODE 0), shared with the BPTT kernel of policy_saliency_lag.hip.
#include "sal_body.h"

namespace iplan {

__global__ __launch_bounds__(64 * SAL_WAVES) void ac_saliency_kernel(IplanAcSaliencyArgs a) {
    __shared__ __attribute__((aligned(16))) SalShared sh;
    constexpr int MODE = 0;
    const IplanAcSaliencyLagArgs* const x_ = nullptr;
#include "sal_body_impl.h"
}

int ac_saliency_launch(const IplanAcSaliencyArgs& a, hipStream_t stream) {
    const int64_t rows = (int64_t)a.E * a.S, tiles = (rows + 15) / 16;
    const unsigned nz = a.which == 2 ? 2u : 1u;
    hipLaunchKernelGGL(ac_saliency_kernel, dim3((unsigned)((tiles + SAL_WAVES - 1) / SAL_WAVES), (unsigned)a.n_agents, nz), dim3(64 * SAL_WAVES), 0, stream, a);
    return check_launch("iplan_ac_saliency");
}

}  // namespace iplan
