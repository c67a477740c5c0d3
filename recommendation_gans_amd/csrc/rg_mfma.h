// What the MFMA kernels of rg_ncf_tile.hip, rg_ncf_wave.hip and rg_ncf_score.hip share: the
// 4-float vector of an MFMA operand / accumulator, the fp32 16x16x4 instruction and a compile-time loop.
#pragma once
#include <utility>

#include <hip/hip_runtime.h>

namespace rg {

typedef float v4f __attribute__((ext_vector_type(4)));

__device__ __forceinline__ v4f mfma(float a, float b, v4f c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

// f(integral_constant<int, 0>), ..., f(integral_constant<int, N - 1>): layer loops that
// contain barriers are not unrolled, which leaves every layer's shapes (and so the MFMA
// K loop) runtime values -- an LDS round trip between consecutive MFMA pairs
template <class F, int... I>
__device__ __forceinline__ void static_for_impl(F &&f, std::integer_sequence<int, I...>) {
    (f(std::integral_constant<int, I>{}), ...);
}
template <int N, class F>
__device__ __forceinline__ void static_for(F &&f) {
    static_for_impl(f, std::make_integer_sequence<int, N>{});
}

}  // namespace rg
