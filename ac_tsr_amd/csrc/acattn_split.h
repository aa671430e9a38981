// Exact three-plane bf16 split of fp32 operands, shared by the split-product kernels (acattn_ce_bf16.hip,
// acattn_proj.hip).  gfx950 has no fast fp32 matrix instruction: v_mfma_f32_16x16x4_f32 runs at the vector rate, 1/16
// of v_mfma_f32_16x16x32_bf16.  An fp32 operand x is split EXACTLY into three bf16 numbers,
//     x = x0 + x1 + x2,   x0 = bf16(x), x1 = bf16(x - x0), x2 = bf16(x - x0 - x1)      (3 x 8 = 24 significand bits)
// and a product a.b is evaluated as the six bf16 MFMAs with i + j <= 2 (ACATTN_SPLIT_TERMS), each exact in the fp32
// accumulator; what is dropped (a1 b2 + a2 b1 + a2 b2) is below 2^-23 |a||b|, one fp32 rounding of the product.
#pragma once

#include "acattn_common.h"

namespace {

typedef __bf16 b8 __attribute__((ext_vector_type(8)));

// product terms (plane of the first operand, plane of the second), smallest first
#define ACATTN_SPLIT_TERMS(X) X(0, 2) X(1, 1) X(2, 0) X(0, 1) X(1, 0) X(0, 0)

__device__ __forceinline__ f4 mfma_bf(const b8 a, const b8 b, const f4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}

// x = p0 + p1 + p2 exactly (round-to-nearest pieces; v_cvt_pk_bf16_f32)
__device__ __forceinline__ void split8(const float (&x)[8], b8& p0, b8& p1, b8& p2) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const __bf16 a = (__bf16)x[j];
    const float r1 = x[j] - (float)a;
    const __bf16 b = (__bf16)r1;
    const float r2 = r1 - (float)b;
    p0[j] = a;
    p1[j] = b;
    p2[j] = (__bf16)r2;
  }
}

// A 64 x 64 weight as A-operand fragments [tile][K-block s][plane][lane] of 16 bytes (K-block s of lane (c, g) holds
// the features 32 s + 16 (j >> 2) + 4 g + (j & 3), j = 0..7), in b8 elements; the planes of the six projections of one
// direction (acattn_proj_problem.split_planes: forward image, then backward image)
constexpr int SPLIT_SQ64 = 4 * 2 * 3 * 64;
constexpr int PROJ_PLANES_DIR = 6 * SPLIT_SQ64;

// acc += a . b over one K = 32 block with both operands split (a[p], b[q]: planes)
__device__ __forceinline__ f4 mfma_split(const b8 (&a)[3], const b8 (&b)[3], f4 acc) {
#define ACATTN_SPLIT_TERM(p, q) acc = mfma_bf(a[p], b[q], acc);
  ACATTN_SPLIT_TERMS(ACATTN_SPLIT_TERM)
#undef ACATTN_SPLIT_TERM
  return acc;
}

}  // namespace
