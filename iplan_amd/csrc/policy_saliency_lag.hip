// Policy saliency through time: one lag of d y_s / d x_{s-k} for every slot (e, s) (include/iplan_hip.h: IplanAcSaliencyLagArgs).  The
// row kernel of policy_saliency.hip -- one wave per 16-row tile, fc1 and fc1^T on v_mfma_f32_16x16x4_f32, five passes over F, nothing
// F wide kept -- from the shared body (sal_body.h, sal_body_impl.h) in its two lag modes:
//
//   lag 0    LN(F) -> .. -> GRU cell -> LN -> head -> y;   dx <- .. <- W_ih^T <- gates' <- LN' <- head^T <- 1        (the plain kernel)
//                                                          carry = z * dh' + W_hh^T [dr | dz | r * dn]              (d y / d h_prev)
//   lag k    the forward of step s - k up to the GRU cell; dx <- .. <- W_ih^T <- gates' <- seed = carry of lag k - 1 of the same slot
//                                                          carry as above: the chain's next link
//
// carry is formed and stored right after the gate backward, before the trunk backward, so it is not live across passes 4-5; the seeded
// form is a separate instantiation without rnn.norm, head and softmax.  A slot's seed and carry are its own: no hand-off between rows,
// lanes of other rows or workgroups, no atomics -- the plain kernel's determinism.  Slots with s < k are masked like rows past the end.
#include "sal_body.h"

namespace iplan {

template <int MODE>
__global__ __launch_bounds__(64 * SAL_WAVES) void ac_saliency_lag_kernel(IplanAcSaliencyLagArgs xa) {
    __shared__ __attribute__((aligned(16))) SalShared sh;
    const IplanAcSaliencyArgs& a = xa.base;
    const IplanAcSaliencyLagArgs* const x_ = &xa;
#include "sal_body_impl.h"
}

int ac_saliency_lag_launch(const IplanAcSaliencyLagArgs& a, hipStream_t stream) {
    const int64_t rows = (int64_t)a.base.E * a.base.S, tiles = (rows + 15) / 16;
    const dim3 grid((unsigned)((tiles + SAL_WAVES - 1) / SAL_WAVES), (unsigned)a.base.n_agents, a.base.which == 2 ? 2u : 1u);
    if (a.lag == 0) hipLaunchKernelGGL(ac_saliency_lag_kernel<1>, grid, dim3(64 * SAL_WAVES), 0, stream, a);
    else hipLaunchKernelGGL(ac_saliency_lag_kernel<2>, grid, dim3(64 * SAL_WAVES), 0, stream, a);
    return check_launch("iplan_ac_saliency_lag");
}

}  // namespace iplan
