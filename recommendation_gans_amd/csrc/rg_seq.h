// What the sequence models' kernels (rg_seq.hip, rg_seq_cnn.hip) share: how an id is read and how
// a gradient row goes out to the [num_items][dim + 1] buffer.
#pragma once
#include "rg_common.h"

namespace rg {

// an id outside [0, num_items) is read as padding: no access outside the tables
__device__ __forceinline__ int64_t safe_id(int64_t id, int64_t num_items) {
    return (uint64_t)id < (uint64_t)num_items ? id : 0;
}

// grad[row] += dz * (x, 1): the row's dim elements from the lanes that own them, the bias
// column from the group's first lane
template <class L>
__device__ __forceinline__ void emit_row(float *grad, int64_t row, int D, int sub, float dz,
                                         const float (&x)[L::EPL]) {
    float *g = grad + row * (int64_t)(D + 1);
#pragma unroll
    for (int e = 0; e < L::EPL; ++e) {
        const int c = L::elem(sub, e);
        if (c < D) unsafeAtomicAdd(g + c, dz * x[e]);
    }
    if (sub == 0) unsafeAtomicAdd(g + D, dz);
}

}  // namespace rg
