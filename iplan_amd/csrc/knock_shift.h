// The distance epilogue of the neighbour knock-out kernels (gat_knockout.hip: one step; gat_knockout_trace.hip: through time).
// Needs gat_body.h in front of it (GH).
#pragma once

namespace iplan {

// sum_c (x[c] - base[c])^2 over the GH columns, c ascending.  Every difference, product and sum is rounded on its own: the whole
// function is compiled with contraction off (the __fmul_rn / __fadd_rn of the HIP headers are plain operators compiled under the
// default -ffp-contract=fast and would fuse again once inlined), so the plain fp32 host loop gives the same bits.
__device__ __forceinline__ float knock_shift_sq(const float* x, const float* base) {
#pragma clang fp contract(off)
    float s = 0.f;
    for (int c = 0; c < GH; ++c) {
        const float d = x[c] - base[c];
        const float p = d * d;
        s = s + p;
    }
    return s;
}

}  // namespace iplan
