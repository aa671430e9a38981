// Shared by the two long-sequence kernel families (acattn_long_fwd.inc, acattn_long_bwd.inc): what must stay IDENTICAL in
// both -- the per-key mask table and the rule for the key tiles a query block visits (a backward that visited other tiles
// than the forward would silently drop probability mass) -- and the small row-segment helpers.
#pragma once
#include "acattn_common.h"

namespace {

__device__ __forceinline__ float ex2(float x) { return __builtin_amdgcn_exp2f(x); }
__device__ __forceinline__ float hsum(const f4 v) { return (v[0] + v[1]) + (v[2] + v[3]); }
// a wave-uniform value that only feeds vector arithmetic, or a per-lane pointer, kept in vector registers: the scalar
// register file is the tight one in these kernels
#define VREG(x) asm volatile("" : "+v"(x))

// 4 elements of an [.., L] row at key offset j0 (rows with L % 4 != 0 are only dword aligned; the last group is ragged)
__device__ __forceinline__ f4 load_seg(const float* row, int j0, int L, bool ok) {
  f4 v = {0.f, 0.f, 0.f, 0.f};
  if (ok && j0 < L) {
    if (j0 + 3 < L) {
      v = *(const f4u*)(row + j0);
    } else {
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (j0 + r < L) v[r] = row[j0 + r];
    }
  }
  return v;
}
__device__ __forceinline__ void store_seg(float* row, int j0, int L, bool ok, const f4 val) {
  if (!ok || j0 >= L) return;
  if (j0 + 3 < L) {
    *(f4u*)(row + j0) = val;
  } else {
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (j0 + r < L) row[j0 + r] = val[r];
  }
}
// keep bits (bit r set = keep) of an explicit 0/1 byte mask row (non-NULL)
__device__ __forceinline__ uint32_t load_keep(const uint8_t* row, int j0, int L, bool ok) {
  uint32_t k = 0xFu;
  if (ok) {
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (j0 + r < L && !row[j0 + r]) k &= ~(1u << r);
  }
  return k;
}

// The per-key additive mask of one sequence into LDS (s_km[0 .. LP), -inf for keys >= L) and its first / last real item
// (structured masks; L and -1 when there is none or the mask is dense).  One wave; ends with a barrier.
__device__ __forceinline__ void long_key_mask_table(const acattn_problem& P, bool structured, bool dense_ll, int L, int LP,
                                                    size_t rowbase, int lane, float* s_km, int& first_valid, int& last_valid) {
  first_valid = L;
  last_valid = -1;
  for (int j = lane; j < LP; j += 64) {
    float km = ACATTN_NEG_INF;
    if (j < L) {
      if (structured) {
        const bool v = P.key_valid[rowbase + j] != 0;
        km = v ? 0.f : ACATTN_MASK_FILL;
        if (v) {
          first_valid = min(first_valid, j);
          last_valid = max(last_valid, j);
        }
      } else {
        km = dense_ll ? 0.f : P.mask[rowbase + j];
      }
    }
    s_km[j] = km;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    first_valid = min(first_valid, __shfl_xor(first_valid, off));
    last_valid = max(last_valid, __shfl_xor(last_valid, off));
  }
  __syncthreads();
}
// Key tiles that can carry probability mass for query block qb.  A row without an allowed key (left padding) spreads over
// every key, so tiles are only skipped when no row of the block is one; dense masks are not inspected.
__device__ __forceinline__ int long_tiles_of_block(bool structured, bool causal, int nT, int qb, int first_valid, int last_valid) {
  if (structured && (causal ? first_valid <= 16 * qb : last_valid >= 0))
    return min(causal ? min(nT, qb + 1) : nT, (last_valid >> 4) + 1);
  return nT;
}

}  // namespace
