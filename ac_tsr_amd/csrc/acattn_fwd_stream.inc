// Fused calibrated attention forward, streaming form: ONE WAVE per (sequence, head, 16-row query block), no staging of
// operands in LDS, no workgroup barrier inside the passes.  Included by acattn_fwd_stream_dh{16,32,64}.hip (one
// translation unit per head size: ACATTN_STREAM_DH).
//
// Why this shape.  B * heads workgroups of the LDS-staged kernels (acattn_fwd_dma.hip) are exactly one resident
// generation on 256 CUs, so the chip runs "read everything, compute, write everything".  Here every wave is its own
// pipeline: K / Ka / V fragments go from L2 straight into the registers the MFMA reads them from (rows are shared by
// the query blocks of a head through L2, HBM sees them once), and the dispatcher places the waves one by one, heaviest
// (most key tiles under the causal mask) first.
//
// Round 3: the kernel is issue bound (DESIGN 4.1), so this version is about instruction slots.
//   * every operand is fetched with buffer loads: one per-lane byte offset per tensor, the tile / row part of the
//     address in an SGPR or the immediate field, rows past the end of the sequence answered with zeros by the
//     descriptor's range check (no min / 64-bit address arithmetic per load: 45 of 285 vector instructions per tile);
//   * V fragments are 8- or 16-byte loads (column d = VW c + e of the head sits in lane c, element e, so a lane's
//     accumulator registers are 4 VW consecutive output columns) and, for L <= 64, fetched ONCE for passes 2 and 3;
//     the gate tile of every key tile is requested before pass 2;
//   * log(|i - j| + 1) comes from a 2 L entry table in LDS (layers.py:721-723; 1 transcendental + 5 vector
//     instructions per element before), read with two ds_read2_b32 per tile whose tile offset is an immediate;
//   * the rank-1 halves of the two spatial affines (layers.py:705-708: a_i + c_j + b) and sigmoid(gate) are taken from
//     the producer of q / k / gate when it supplies them (acattn_problem.affine, .gate_is_prob; PRE = true): the
//     sigmoid of the gate is shared by the heads (layers.py:887 unsqueeze(1)) and the key halves by the query blocks,
//     so the core recomputed both 2-4 times; PRE = false keeps the in-kernel evaluation;
//   * the allowed-key bits live in the layout the validity ballot has (bit 16 t' + r of group t / 4), built with
//     two 64-bit shifts per 64 keys instead of a dozen operations per tile;
//   * p = 0.5 dropout, the only rate the reference ships, is a template flag (no run-time branches in pass 2);
//   * log2(e) is folded into the row normalisers, so the three soft-max arguments of passes 2-3 are one packed
//     multiply-add each.
//
// Lane layout and arithmetic: S^T = K.Q^T on fp32 MFMA 16x16x4, lane (c = lane & 15, g = lane >> 4) holds query row
// i0 + c and keys 16 t + 4 g + r; row reductions by permlane swaps; probabilities feed ctx^T = V^T.P^T directly.
#include <stdlib.h>
#include <string.h>

#include <type_traits>

#include "acattn_common.h"

namespace {

typedef float f2 __attribute__((ext_vector_type(2)));
typedef int i2v __attribute__((ext_vector_type(2)));
typedef int i4v __attribute__((ext_vector_type(4)));
typedef __amdgpu_buffer_rsrc_t rsrc_t;

constexpr float kLog2e = 1.44269504088896340736f;
constexpr float kLn2 = 0.69314718055994530942f;
// aux (cache policy) bits of the buffer stores on gfx950: 1 = sc0, 2 = nt (streaming), 16 = sc1.  Probe builds override
// them per tensor class (-DACATTN_M_AUX / -DACATTN_C_AUX: the M block / the two contexts).
#ifndef ACATTN_M_AUX
#define ACATTN_M_AUX 2
#endif
#ifndef ACATTN_C_AUX
#define ACATTN_C_AUX 2
#endif
constexpr int kStoreNt = ACATTN_C_AUX;

__device__ __forceinline__ float ex2(float x) { return __builtin_amdgcn_exp2f(x); }
__device__ __forceinline__ float lg2(float x) { return __builtin_amdgcn_logf(x); }
__device__ __forceinline__ float and_bits(float x, int m) { return __uint_as_float(__float_as_uint(x) & (uint32_t)m); }
// (m & a) | (~m & b): one v_bfi_b32
__device__ __forceinline__ float bit_select(int m, float a, float b) {
  return __uint_as_float((__float_as_uint(a) & (uint32_t)m) | (__float_as_uint(b) & ~(uint32_t)m));
}

// Packed fp32 (v_pk_add / mul / fma_f32: two elements per instruction slot).  The elementwise chains here run between
// transcendentals, which are scalar: left alone the DAG combiner folds "extract (binop (build a b) ..)" back into two
// scalar operations (1,805 plain against 112 packed vector instructions in the round-2 kernel).  An empty asm that
// takes and returns the REGISTER PAIR makes the pair opaque: no instruction, but the operation in front of it stays
// packed.  An f4 of this kernel is handled as its two halves (elements 0,1 | 2,3).
#ifdef ACATTN_NO_PAIR  // probe builds (tools/probe): no register-pair barriers
#define ACATTN_PAIR(x) ((void)0)
#else
#define ACATTN_PAIR(x) asm("" : "+v"(x))
#endif
struct F22 {
  f2 lo, hi;
};
__device__ __forceinline__ F22 split4(const f4 v) {
  F22 o{f2{v[0], v[1]}, f2{v[2], v[3]}};
  ACATTN_PAIR(o.lo);
  ACATTN_PAIR(o.hi);
  return o;
}
__device__ __forceinline__ f4 join4(const F22 v) { return f4{v.lo[0], v.lo[1], v.hi[0], v.hi[1]}; }
__device__ __forceinline__ F22 pin(F22 v) {
  ACATTN_PAIR(v.lo);
  ACATTN_PAIR(v.hi);
  return v;
}
template <class F>
__device__ __forceinline__ F22 map4(const F22 v, F&& f) {  // scalar function per element, result pinned as pairs
  F22 o{f2{f(v.lo[0], 0), f(v.lo[1], 1)}, f2{f(v.hi[0], 2), f(v.hi[1], 3)}};
  return pin(o);
}
__device__ __forceinline__ F22 operator+(const F22 a, const F22 b) { return pin(F22{a.lo + b.lo, a.hi + b.hi}); }
__device__ __forceinline__ F22 operator-(const F22 a, const F22 b) { return pin(F22{a.lo - b.lo, a.hi - b.hi}); }
__device__ __forceinline__ F22 operator*(const F22 a, const F22 b) { return pin(F22{a.lo * b.lo, a.hi * b.hi}); }
// a per-lane scalar as a register pair: the packed instruction then has a real pair operand (a scalar in ONE vector
// register would have to be copied in front of every use; compile-time constants travel as SGPR pairs by themselves)
__device__ __forceinline__ f2 splat2(const float x) {
  f2 v = {x, x};
  ACATTN_PAIR(v);
  return v;
}
__device__ __forceinline__ F22 operator+(const F22 a, const f2 b) { return pin(F22{a.lo + b, a.hi + b}); }
__device__ __forceinline__ F22 operator-(const F22 a, const f2 b) { return pin(F22{a.lo - b, a.hi - b}); }
__device__ __forceinline__ F22 operator*(const F22 a, const f2 b) { return pin(F22{a.lo * b, a.hi * b}); }
__device__ __forceinline__ F22 fma22(const F22 a, const f2 b, const F22 c) {
  return pin(F22{__builtin_elementwise_fma(a.lo, b, c.lo), __builtin_elementwise_fma(a.hi, b, c.hi)});
}
__device__ __forceinline__ F22 operator+(const F22 a, const float b) { return pin(F22{a.lo + b, a.hi + b}); }
__device__ __forceinline__ F22 operator-(const float a, const F22 b) { return pin(F22{a - b.lo, a - b.hi}); }
__device__ __forceinline__ F22 operator-(const F22 a, const float b) { return pin(F22{a.lo - b, a.hi - b}); }
__device__ __forceinline__ F22 operator*(const F22 a, const float b) { return pin(F22{a.lo * b, a.hi * b}); }
__device__ __forceinline__ F22 fma22(const F22 a, const F22 b, const F22 c) {
  return pin(F22{__builtin_elementwise_fma(a.lo, b.lo, c.lo), __builtin_elementwise_fma(a.hi, b.hi, c.hi)});
}
__device__ __forceinline__ F22 fma22(const F22 a, const float b, const F22 c) {
  const f2 b2 = {b, b};
  return pin(F22{__builtin_elementwise_fma(a.lo, b2, c.lo), __builtin_elementwise_fma(a.hi, b2, c.hi)});
}
__device__ __forceinline__ F22 fma22(const F22 a, const float b, const float c) {
  const f2 b2 = {b, b}, c2 = {c, c};
  return pin(F22{__builtin_elementwise_fma(a.lo, b2, c2), __builtin_elementwise_fma(a.hi, b2, c2)});
}
__device__ __forceinline__ float max4(float m, const F22 v) { return fmaxf(fmaxf(m, fmaxf(v.lo[0], v.lo[1])), fmaxf(v.hi[0], v.hi[1])); }

// A FULLY MASKED row (no allowed key: a left-padded position under the causal mask).  The reference adds -10000 to every
// score of such a row IN FP32 (abstract_recommender.py:142, layers.py:734, 918-925): the sum is rounded to the grid of
// 10000's neighbourhood, 2^-10, so the row's soft-max sees its arguments QUANTISED to about 0.001 -- probabilities that
// differ from the unquantised ones by up to 1e-3 relative (3.6e-4 on a context through P.V).  The kernels here drop the
// common shift of such a row (its keys < L all carry the "allowed" bit), so the quantisation is re-applied to the
// argument itself: exp2-domain argument -> natural domain -> (+ -10000, - -10000: exact difference of two grid points) ->
// back.  `dead_lanes` = the wave's ballot of dead rows (the other lanes keep their value bit for bit).  Only reached in waves
// that hold a dead row (wave-uniform branch at the call sites).
__device__ __forceinline__ F22 dead_row_quantise(const F22 x2, const unsigned long long dead_lanes) {
  const int dead = (dead_lanes >> threadIdx.x) & 1ull ? -1 : 0;  // from the scalar ballot: no register held outside this block
  const F22 q = ((x2 * kLn2) + ACATTN_MASK_FILL) - ACATTN_MASK_FILL;  // every step pinned: not reassociated
  const F22 r = q * kLog2e;
  return F22{f2{bit_select(dead, r.lo[0], x2.lo[0]), bit_select(dead, r.lo[1], x2.lo[1])},
             f2{bit_select(dead, r.hi[0], x2.hi[0]), bit_select(dead, r.hi[1], x2.hi[1])}};
}

// Raw buffer descriptor over `bytes` bytes at `base` (wave-uniform): loads past the end return 0, stores past the end
// are dropped.
__device__ __forceinline__ rsrc_t make_rsrc(const void* base, int bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, bytes, 0x00020000);
}
__device__ __forceinline__ float bload1(rsrc_t r, int voff, int soff) {
  return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, voff, soff, 0));
}
__device__ __forceinline__ f2 bload2(rsrc_t r, int voff, int soff) {
  return __builtin_bit_cast(f2, __builtin_amdgcn_raw_buffer_load_b64(r, voff, soff, 0));
}
__device__ __forceinline__ f4 bload4(rsrc_t r, int voff, int soff) {
  return __builtin_bit_cast(f4, __builtin_amdgcn_raw_buffer_load_b128(r, voff, soff, 0));
}
template <int W>
__device__ __forceinline__ void bloadw(rsrc_t r, int voff, int soff, float (&out)[W]) {
  if constexpr (W == 1) {
    out[0] = bload1(r, voff, soff);
  } else if constexpr (W == 2) {
    const f2 v = bload2(r, voff, soff);
    out[0] = v[0];
    out[1] = v[1];
  } else {
    static_assert(W % 4 == 0, "1, 2 or a multiple of 4 floats");
#pragma unroll
    for (int q = 0; q < W / 4; ++q) {  // (head size 128: two 16-byte loads)
      const f4 v = bload4(r, voff + 16 * q, soff);
#pragma unroll
      for (int e = 0; e < 4; ++e) out[4 * q + e] = v[e];
    }
  }
}
__device__ __forceinline__ void bstore4(rsrc_t r, int voff, int soff, const f4 v) {
  __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(i4v, v), r, voff, soff, kStoreNt);
}
__device__ __forceinline__ void bstore4m(rsrc_t r, int voff, int soff, const f4 v) {
  __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(i4v, v), r, voff, soff, ACATTN_M_AUX);
}
__device__ __forceinline__ void bstore1(rsrc_t r, int voff, int soff, const float v) {
  __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(int, v), r, voff, soff, kStoreNt);
}

// Diagnostic builds only (-DACATTN_STAMPS, tools/probe): s_memtime stamps kept in scalar registers and written once at
// the end to the buffer passed in P.noise (unused by this kernel otherwise).  -DACATTN_STAMP_WAIT drains the memory
// counters in front of every stamp, so that a stamp also says when the data requested before it had landed.
#ifdef ACATTN_STAMPS
#ifdef ACATTN_STAMP_WAIT
#define ACATTN_STAMP_DRAIN "s_waitcnt vmcnt(0) lgkmcnt(0)\n\t"
#else
#define ACATTN_STAMP_DRAIN
#endif
#define ACATTN_STAMP(k)                                                                                          \
  do {                                                                                                           \
    __builtin_amdgcn_sched_barrier(0);                                                                           \
    asm volatile(ACATTN_STAMP_DRAIN "s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(stamp_[k])::"memory");        \
    __builtin_amdgcn_sched_barrier(0);                                                                           \
  } while (0)
#else
#define ACATTN_STAMP(k)
#endif

// Timing-only builds (-DACATTN_ZERO=<bits>, tools/probe): the descriptor of a tensor class gets zero records, so the
// range check drops its loads / stores while the instruction stream stays.  bit 0 q/qa, 1 K/Ka, 2 V, 3 gate,
// 4 affine planes, 5 M stores, 6 context stores.
#ifndef ACATTN_ZERO
#define ACATTN_ZERO 0
#endif
#define ACATTN_BYTES(bit, n) (((ACATTN_ZERO) >> (bit)) & 1 ? 0 : (n))
// With the tile count a compile-time constant (below) a pass is straight-line code; left alone the scheduler then hoists
// the loads, random numbers and LDS reads of every tile to the top of the pass (111 spilled registers in the
// 4-waves-per-SIMD form).  The fence keeps one tile's working set live at a time.
#if defined(ACATTN_STRAIGHT_TILES) && !defined(ACATTN_NO_TILE_FENCE)
#define ACATTN_TILE_FENCE __builtin_amdgcn_sched_barrier(0)
#else
#define ACATTN_TILE_FENCE
#endif

// NT = key tiles a row may span (L <= 16 NT): 4 for the shipped L = 50 configurations (4 waves per SIMD), 13 for
// L <= 208 (the row's two score tile sets are 104 registers: 2 waves per SIMD).
#ifdef ACATTN_UPFRONT
constexpr bool kUpfront = true;
#else
constexpr bool kUpfront = false;
#endif
// Waves per SIMD.  The in-kernel affines (PRE = false: weights, key-half dot products) do not fit 128 registers next
// to the V fragments that stay resident; that fallback form runs three waves per SIMD rather than spill.
template <int DH, int NT, bool PRE>
constexpr int stream_waves() {
#ifdef ACATTN_WAVES
  return ACATTN_WAVES;
#endif
  return DH >= 128 ? 1 : (NT <= 4 ? (kUpfront || DH > 32 ? 2 : (PRE ? 4 : 3)) : 2);  // head size 128 [r3]: 512 registers
}

// ---------------------------------------------------------------------------------------------------------------------
// The TAIL query block.  L = 50 is three full blocks of 16 rows and a block with TWO rows, and under the causal mask that
// block visits every key tile: in the ordinary layout (16 query columns per MFMA, a tile at a time) two rows cost what
// sixteen cost -- 4 key tiles of elementwise work for 2 / 16 of a tile's lanes, 3.6-4.0 us of the 16.8-19.2 us launch
// (timing build without the block: tools/probe, ACATTN_ZERO=1024).  For a last block of at most FOUR rows the 16 MFMA
// columns are put to a different use: column n = (query n & 3, key tile n >> 2).  The B operand of step (tile t', ..)
// is the query fragment where n >> 2 == t' and ZERO elsewhere (one v_and per operand), so D[m][(q, t)] receives
// K_t[m] . Q[q] only from its own tile: one accumulator set holds the scores of ALL four key tiles, and passes 1-3 run
// ONCE over it (lane (c, g), register r  <->  query i0 + (c & 3), key 16 (c >> 2) + 4 g + r).  P.V uses the same
// block-diagonal B operand; column (q, t) then holds the context partial over tile t's keys and the four partials meet
// by two lane exchanges at the end.  MFMA count as before (the zero blocks are paid for), elementwise work a quarter.
// Same random draws per (row, key group), same arithmetic: interchangeable with the ordinary path (tests pin both to
// the general kernel).  Needs the producer extras (PRE), L <= 64, 1 <= L % 16 <= 4.
template <int DH, bool ADV, bool HALF>
__device__ __forceinline__ void stream_tail_block(const acattn_problem& P, const acattn_fwd_out& O, const int b, const int h,
                                                  const int qb, float* lt_tab, float* m_stage) {
  constexpr int NT = 4, KS = DH / 4, VW = DH / 16;
  const int L = P.L, H = P.H, nh = P.n_heads;
  const int nT = (L + 15) >> 4;
  const bool causal = P.causal != 0;
  const int lane = threadIdx.x;
  const int c = lane & 15, g = lane >> 4;
  const int qi = c & 3, tc = c >> 2;  // this lane's query row of the block and its key tile
  const size_t rowbase = (size_t)b * L;
  const int hoff = h * DH;
  const size_t bh = (size_t)b * nh + h;
  const int i0 = qb * 16, i = i0 + qi;
  const bool row_ok = i < L;
  const int j0 = 16 * tc + 4 * g;  // first of this lane's four keys

#pragma unroll
  for (int k0 = 0; k0 < 32 * NT; k0 += 64) lt_tab[k0 + lane] = lg2((float)(abs(k0 + lane - 16 * NT) + 1)) * kLn2;

  const int seq_bytes = L * H * 4;
  const int H4 = H * 4;
  const rsrc_t rK = make_rsrc(P.k + rowbase * H, ACATTN_BYTES(1, seq_bytes));
  const rsrc_t rV = make_rsrc(P.v + rowbase * H, ACATTN_BYTES(2, seq_bytes));
  const rsrc_t rKa = make_rsrc((ADV ? P.ka : P.k) + rowbase * H, ACATTN_BYTES(1, seq_bytes));
  const int koff = ((int)__umul24(c, H) + hoff + KS * g) * 4;
  const int voff = ((int)__umul24(4 * g, H) + hoff + VW * c) * 4;
  uint8_t kvb;
  {
    const rsrc_t rF = make_rsrc(P.key_valid + rowbase, L);
    kvb = __builtin_amdgcn_raw_buffer_load_b8(rF, lane, 0, 0);
  }
  float qf[KS], qaf[KS];
  {
    const rsrc_t rQ = make_rsrc(P.q + rowbase * H, ACATTN_BYTES(0, seq_bytes));
    const rsrc_t rQa = make_rsrc((ADV ? P.qa : P.q) + rowbase * H, ACATTN_BYTES(0, seq_bytes));
    const int qoff = ((int)__umul24(i, H) + hoff + KS * g) * 4;  // rows past L: out of range, zeros
#pragma unroll
    for (int s4 = 0; s4 < KS / 4; ++s4) {
      const f4 t = bload4(rQ, qoff + 16 * s4, 0);
      f4 ta = t;
      if (ADV) ta = bload4(rQa, qoff + 16 * s4, 0);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        qf[4 * s4 + e] = t[e];
        qaf[4 * s4 + e] = ta[e];
      }
    }
  }
  const int LP = 16 * nT;
  const rsrc_t rA = make_rsrc(P.affine + bh * 4 * LP, ACATTN_BYTES(4, 16 * LP));
  const float ao2 = bload1(rA, i * 4, 0), ad = bload1(rA, (LP + i) * 4, 0);
  const f4 co4 = bload4(rA, (2 * LP + j0) * 4, 0), cd4 = bload4(rA, (3 * LP + j0) * 4, 0);  // past LP: zeros
  f4 kb[KS / 4], kab[KS / 4];
#pragma unroll
  for (int s4 = 0; s4 < KS / 4; ++s4) {
    kb[s4] = bload4(rK, koff + 16 * s4, 0);
    if (ADV) kab[s4] = bload4(rKa, koff + 16 * s4, 0);
  }
  const float sc = P.scalar[0];

  const unsigned long long vk = __ballot(kvb != 0);
  const bool any_valid = vk != 0ull;
  const int first_valid = any_valid ? __ffsll((long long)vk) - 1 : L;
  const int last_valid = any_valid ? 63 - __clzll((long long)vk) : -1;
  const int nt_valid = any_valid ? (last_valid >> 4) + 1 : nT;
  const bool rows_see_a_key = causal ? first_valid <= i0 : any_valid;
  const int nt = rows_see_a_key ? min(causal ? min(nT, qb + 1) : nT, nt_valid) : nT;

  // a row's 64 keys are spread over its 16 lanes (4 key tiles x 4 lane groups): reductions over a row
  auto row_sum = [&](float x) {
    x = quad_sum(x);
    x += __shfl_xor(x, 4);
    return x + __shfl_xor(x, 8);
  };
  auto row_max = [&](float x) {
    x = quad_max(x);
    x = fmaxf(x, __shfl_xor(x, 4));
    return fmaxf(x, __shfl_xor(x, 8));
  };
  // allowed-key bits of the lane's four keys (bit r): a real item and (causal) not after the query; `ab`: after the query
  const int d0 = i - j0;
  const uint32_t vn = (uint32_t)(vk >> j0) & 0xFu;
  const uint32_t cn = d0 >= 3 ? 0xFu : (d0 < 0 ? 0u : (2u << d0) - 1u);
  uint32_t eb = causal ? (vn & cn) : vn;
  const uint32_t ab = ~cn & 0xFu;
  uint32_t seen = quad_or(eb);
  seen |= (uint32_t)__shfl_xor((int)seen, 4);
  seen |= (uint32_t)__shfl_xor((int)seen, 8);
  const bool row_dead = seen == 0u;  // fully masked row (left padding): uniform over every key < L
  const unsigned long long dead_m = __ballot(row_dead);
  const bool any_dead = dead_m != 0ull;
  if (row_dead) eb = (1u << min(max(L - j0, 0), 4)) - 1u;
  const bool order_select = !causal || any_dead;
  auto ebit = [&](int r) -> int { return sbit(eb, r); };
  int selm[NT];  // -1 where this lane's column belongs to key tile t'
#pragma unroll
  for (int t = 0; t < NT; ++t) selm[t] = tc == t ? -1 : 0;

  const float hs2 = 0.5f * (sc * sc);
  const float inv_sqrt = 1.0f / sqrtf((float)DH);
  const float scale2 = inv_sqrt * kLog2e;
  const float nc2 = -(hs2 * scale2);
  const float kNegMask2 = ACATTN_MASK_FILL * kLog2e;
  const bool has_drop = HALF || P.p_drop > 0.f;
  const float keep_scale = HALF ? 2.0f : (has_drop ? fast_rcp(1.0f - P.p_drop) : 1.0f);
  const uint32_t rng_row = (uint32_t)(bh * L + i);
  const RngKey rkey = rng_key(P.seed + (P.seed_device ? *P.seed_device : 0ull));

  __syncthreads();  // the distance table
  const float* const ltp = lt_tab + (16 * NT + i - j0);  // ltp[-r] = log(|i - (j0 + r)| + 1)

  // ---- pass 1: one accumulator set for every key tile -----------------------------------------------------------------------
  f4 aS = {0.f, 0.f, 0.f, 0.f}, aM = aS;
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    if (t < nt) {
#pragma unroll
      for (int s4 = 0; s4 < KS / 4; ++s4) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          aS = mfma16(kb[s4][e], and_bits(qf[4 * s4 + e], selm[t]), aS);
          if (ADV) aM = mfma16(kab[s4][e], and_bits(qaf[4 * s4 + e], selm[t]), aM);
        }
      }
      if (t + 1 < NT && t + 1 < nt) {
        const int ko = koff + 16 * (t + 1) * H4;
#pragma unroll
        for (int s4 = 0; s4 < KS / 4; ++s4) {
          kb[s4] = bload4(rK, ko + 16 * s4, 0);
          if (ADV) kab[s4] = bload4(rKa, ko + 16 * s4, 0);
        }
      }
    }
  }
  // V fragments of every visited tile and the gate piece of this lane's keys: in flight under the elementwise work
  float vfk[NT][4][VW];
#pragma unroll
  for (int t = 0; t < NT; ++t)
    if (t < nt) {
#pragma unroll
      for (int r = 0; r < 4; ++r) bloadw<VW>(rV, voff + (16 * t + r) * H4, 0, vfk[t][r]);
    }
  const rsrc_t rG = make_rsrc(ADV ? P.gate_logits + rowbase * L : nullptr, ADV ? ACATTN_BYTES(3, L * L * 4) : 0);
  f4 gl = {0.f, 0.f, 0.f, 0.f};
  if (ADV) gl = bload4(rG, ((int)__umul24(i, L) + j0) * 4, 0);

  const f2 ao2s = splat2(ao2), ads = splat2(ad), nc2s = splat2(nc2);
  const F22 e1 = map4(split4(co4) + ao2s, [](float x, int) { return ex2(x); });
  const F22 pr = map4(e1 + 1.0f, [](float x, int) { return fast_rcp(x); });
  F22 val = 1.0f - pr;  // layers.py:715-719
  if (order_select) val = map4(val, [&](float x, int r) { return bit_select(sbit(ab, r), r < 2 ? pr.lo[r] : pr.hi[r - 2], x); });
  const F22 lg = map4(val + ACATTN_LOG_EPS, [](float x, int) { return lg2(x); });
  F22 lt{f2{ltp[0], ltp[-1]}, f2{ltp[-2], ltp[-3]}};
  lt = pin(lt);  // log(|i - j| + 1)   layers.py:721-723
  F22 mk{f2{and_bits(kNegMask2, ~ebit(0)), and_bits(kNegMask2, ~ebit(1))}, f2{and_bits(kNegMask2, ~ebit(2)), and_bits(kNegMask2, ~ebit(3))}};
  mk = pin(mk);
  const F22 df = lt - (split4(cd4) + ads);
  F22 x = fma22(split4(aS), scale2, mk);
  x = fma22(lg, inv_sqrt, x);
  x = fma22(df * df, nc2s, x);
  if (any_dead) x = dead_row_quantise(x, dead_m);
  const float mx = row_max(max4(ACATTN_NEG_INF, x));
  F22 y = x;
  float my = 0.f;
  if (ADV) {
    y = fma22(split4(aM), scale2, mk);
    if (any_dead) y = dead_row_quantise(y, dead_m);
    my = row_max(max4(ACATTN_NEG_INF, y));
  }
  const F22 e = map4(x - splat2(mx), [](float v, int) { return ex2(v); });
  const float zx = row_sum((e.lo[0] + e.lo[1]) + (e.hi[0] + e.hi[1]));
  F22 f = e;
  float zy = 1.f;
  if (ADV) {
    f = map4(y - splat2(my), [](float v, int) { return ex2(v); });
    zy = row_sum((f.lo[0] + f.lo[1]) + (f.hi[0] + f.hi[1]));
  }
  const float rzx = fast_rcp(zx) * (ADV ? keep_scale * kLog2e : keep_scale), rzy = fast_rcp(zy) * keep_scale;

  // ---- pass 2 ------------------------------------------------------------------------------------------------------------------
  F22 n2{f2{0.f, 0.f}, f2{0.f, 0.f}};
  uint32_t ka = 0xFu, km = 0xFu;
  if (ADV || has_drop) {
    if constexpr (HALF) {
      const RngDraw rd = rng_draw_half(rkey, rng_row, (uint32_t)(4 * tc + g), kLog2e);
      n2 = pin(F22{rd.n01, rd.n23});
      ka = rd.keep_after;
      km = rd.keep_mask;
    } else {
      const RngGroup rg = rng_group(rkey, rng_row, (uint32_t)(4 * tc + g), P.p_drop);
      n2 = split4(rg.n) * kLog2e;
      if (has_drop) {
        ka = rg.keep_after;
        km = rg.keep_mask;
      }
    }
  }
  F22 p = e * splat2(rzx);  // P = dropout(softmax) (times log2(e) when ADV)   layers.py:735-736
  if (has_drop) p = map4(p, [&](float v, int r) { return keep_and(v, ka, r); });
  const int blk_rows = min(16, L - i0);
  const int n_blk = blk_rows > 0 ? blk_rows * L : 0;
  f4 ca[VW], cc[VW];
#pragma unroll
  for (int ee = 0; ee < VW; ++ee) {
    ca[ee] = f4{0.f, 0.f, 0.f, 0.f};
    cc[ee] = ca[ee];
  }
  // lane (c, g), accumulator ee, register rr  ->  partial over tile tc of ctx[i0 + qi][VW (4 g + rr) + ee]
  const int coff = ((int)__umul24(i, H) + hoff + 4 * VW * g) * 4;  // rows past L: out of range, dropped
  auto store_ctx = [&](rsrc_t rC, f4 (&acc)[VW], float s) {
#pragma unroll
    for (int ee = 0; ee < VW; ++ee)
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {  // the four key tiles' partials meet: columns c, c ^ 4, c ^ 8, c ^ 12
        float v = acc[ee][rr];
        v += __shfl_xor(v, 4);
        v += __shfl_xor(v, 8);
        acc[ee][rr] = v * s;
      }
    if (tc == 0) {
      float o[4 * VW];
#pragma unroll
      for (int rr = 0; rr < 4; ++rr)
#pragma unroll
        for (int ee = 0; ee < VW; ++ee) o[VW * rr + ee] = acc[ee][rr];
#pragma unroll
      for (int w = 0; w < VW; ++w) bstore4(rC, coff + 16 * w, 0, f4{o[4 * w], o[4 * w + 1], o[4 * w + 2], o[4 * w + 3]});
    }
  };
  float zu = 1.f, zv = 1.f, zw = 1.f;
  if (ADV) {
    F22 m = f * splat2(rzy);  // M   layers.py:670-672
    if (has_drop) m = map4(m, [&](float v, int r) { return keep_and(v, km, r); });
    {  // M into the wave's block [blk_rows][L] (zeros where the key carries no mass: skipped tiles included)
      float* mp = m_stage + qi * L + j0;
      const f4 mj = join4(m);
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (j0 + r < L) mp[r] = mj[r];
    }
    F22 au = fma22(n2, 1.0f - m, p * m);         // layers.py:918-919 (exp2 domain)
    const F22 a1 = fma22(m, -kLog2e, kLog2e);    // exp(1 - M)
    const int eb4[4] = {ebit(0), ebit(1), ebit(2), ebit(3)};
    if (any_dead) au = dead_row_quantise(au, dead_m);
    const F22 eu2 = map4(au, [&](float v, int r) { return and_bits(ex2(v), eb4[r]); });
    const F22 ex1 = map4(a1, [](float v, int) { return ex2(v); });
    zu = row_sum((eu2.lo[0] + eu2.lo[1]) + (eu2.hi[0] + eu2.hi[1]));
    F22 av = p * ex1;
    if (any_dead) av = dead_row_quantise(av, dead_m);
    const F22 ev = map4(av, [&](float v, int r) { return and_bits(ex2(v), eb4[r]); });  // layers.py:920-921
    zv = row_sum((ev.lo[0] + ev.lo[1]) + (ev.hi[0] + ev.hi[1]));
    const f4 eu = join4(eu2);
#pragma unroll
    for (int t = 0; t < NT; ++t)
      if (t < nt) {
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
          for (int ee = 0; ee < VW; ++ee) ca[ee] = mfma16(vfk[t][r][ee], and_bits(eu[r], selm[t]), ca[ee]);
      }
    // the block of M leaves as whole runs (see the ordinary path)
    const rsrc_t rM = make_rsrc(O.attack_mask + (bh * L + i0) * L, ACATTN_BYTES(5, n_blk * 4));
    if (256 * 0 < n_blk) {
      const f4 v0 = *(const f4*)(m_stage + 4 * lane);
      if (HALF && O.penalty_part) {  // (uniform) the block's sum of (1 - M)^2, as the ordinary path forms it (penalty_late)
        const f4 d = 1.0f - v0;
        float pen = 0.f;
        if (4 * lane + 4 <= n_blk) {
          pen = (d[0] * d[0] + d[1] * d[1]) + (d[2] * d[2] + d[3] * d[3]);
        } else {
#pragma unroll
          for (int r = 0; r < 4; ++r)
            if (4 * lane + r < n_blk) pen += d[r] * d[r];
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) pen += __shfl_xor(pen, off);
        if (lane == 0) O.penalty_part[bh * nT + qb] = pen;
      }
      if ((n_blk & 3) == 0) {
        bstore4(rM, 16 * lane, 0, v0);
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (4 * lane + r < n_blk) bstore1(rM, 16 * lane + 4 * r, 0, v0[r]);
      }
    }
    store_ctx(make_rsrc(O.ctx_attacked + rowbase * H, ACATTN_BYTES(6, seq_bytes)), ca, fast_rcp(zu));
    // ---- pass 3 ----------------------------------------------------------------------------------------------------------------
    const F22 gt = split4(gl);  // probabilities (PRE)
    const F22 acn = ev * splat2(fast_rcp(zv) * kLog2e);
    F22 aw = fma22(gt, p - acn, acn);  // layers.py:888, 925 (exp2 domain)
    if (any_dead) aw = dead_row_quantise(aw, dead_m);
    const F22 ew2 = map4(aw, [&](float v, int r) { return and_bits(ex2(v), eb4[r]); });
    zw = row_sum((ew2.lo[0] + ew2.lo[1]) + (ew2.hi[0] + ew2.hi[1]));
    const f4 ew = join4(ew2);
#pragma unroll
    for (int t = 0; t < NT; ++t)
      if (t < nt) {
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
          for (int ee = 0; ee < VW; ++ee) cc[ee] = mfma16(vfk[t][r][ee], and_bits(ew[r], selm[t]), cc[ee]);
      }
  } else {
    const f4 pj = join4(p);
#pragma unroll
    for (int t = 0; t < NT; ++t)
      if (t < nt) {
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
          for (int ee = 0; ee < VW; ++ee) cc[ee] = mfma16(vfk[t][r][ee], and_bits(pj[r], selm[t]), cc[ee]);
      }
  }
  store_ctx(make_rsrc(O.ctx_calibrated + rowbase * H, ACATTN_BYTES(6, seq_bytes)), cc, ADV ? fast_rcp(zw) : 1.0f);
  if (ADV && O.row_stats && g == 0 && tc == 0 && row_ok) {
    float* sp = O.row_stats + (bh * L + i) * ACATTN_NSTAT;
    const float sh = row_dead ? ACATTN_MASK_FILL : 0.f;
    store_out4(sp, f4{(mx + lg2(zx)) * kLn2 + sh, (my + lg2(zy)) * kLn2 + sh, sh + fast_log(zu), sh + fast_log(zv)});
    store_out4(sp + 4, f4{sh + fast_log(zw), 0.f, 0.f, 0.f});
  }
}

// ADV: adversarial calibrator on (contract A) / spatial calibrator only (contract A').  HALF: p_drop == 0.5.
// PRE: the producer's affine planes and gate probabilities are read instead of evaluated.
template <int DH, int NT, bool ADV, bool HALF, bool PRE>
__global__ void __launch_bounds__(64, (stream_waves<DH, NT, PRE>())) acattn_fwd_stream_kernel(const acattn_problem P, const acattn_fwd_out O) {
  constexpr int KS = DH / 4;        // floats of a row fragment per lane
  constexpr int VW = DH / 16;       // floats of a V row a lane holds = 16-row output tiles of ctx^T
  constexpr int NG = (NT + 3) / 4;  // 64-key groups
  constexpr bool KEEPV = NT <= 4;   // V fragments and gate tiles of every key tile stay in registers over passes 2-3
  // UPF: every operand of the wave is requested before its first wait (two waves per SIMD, 256 registers): the wave's
  // chain is ONE round trip, its compute, its stores -- and the launch is two generations that overlap
  constexpr bool UPF = kUpfront && NT <= 4 && PRE;
  __shared__ float lt_tab[32 * NT];  // lt_tab[16 NT + d] = log(|d| + 1)
  __shared__ __attribute__((aligned(16))) float m_stage[ADV ? 16 * 16 * NT : 4];  // the wave's block of M: [16][L]
#ifdef ACATTN_STAMPS
  unsigned long long stamp_[8] = {};
#endif
  ACATTN_STAMP(0);
  if ((ACATTN_ZERO) & 128) return;  // timing-only: launch + dispatch

  const int L = P.L, H = P.H, nh = P.n_heads;
  const int nT = (L + 15) >> 4;
  const int n_items = P.B * nh;
  const bool causal = P.causal != 0;
  // heaviest query blocks first: under the causal mask block qb visits qb + 1 key tiles
  const int rank = blockIdx.x / n_items, item = blockIdx.x - rank * n_items;
  int qb = causal ? nT - 1 - rank : rank;
#ifndef ACATTN_NO_TAIL_PATH
  // a last block of at most four rows takes the tail path below and is then lighter than the block in front of it
  if (PRE && NT == 4 && causal && nT >= 2 && (L & 15) != 0 && (L & 15) <= 4 && rank < 2) qb = nT - 2 + rank;
#endif
  if (((ACATTN_ZERO) & 1024) && qb == nT - 1 && (L & 15) != 0 && (L & 15) <= 4) return;  // timing-only: no tail block
  int b, h;
  decode_block(item, P.B, nh, b, h);
  if constexpr (PRE && NT == 4) {
#ifndef ACATTN_NO_TAIL_PATH
    if (qb == nT - 1 && (L & 15) != 0 && (L & 15) <= 4) {  // a last block of at most four rows (wave-uniform)
      stream_tail_block<DH, ADV, HALF>(P, O, b, h, qb, lt_tab, m_stage);
      return;
    }
#endif
  }
  const int lane = threadIdx.x;
  const int c = lane & 15, g = lane >> 4;
  const size_t rowbase = (size_t)b * L;
  const int hoff = h * DH;
  const size_t bh = (size_t)b * nh + h;
  const int i0 = qb * 16, i = i0 + c;
  const bool row_ok = i < L;

#pragma unroll
  for (int k0 = 0; k0 < 32 * NT; k0 += 64) {
    const int k = k0 + lane;
    if (k0 + 64 <= 32 * NT || k < 32 * NT) lt_tab[k] = lg2((float)(abs(k - 16 * NT) + 1)) * kLn2;
  }

  // ---- descriptors and per-lane byte offsets ---------------------------------------------------------------------------
  const int seq_bytes = L * H * 4;
  const int H4 = H * 4;
  const rsrc_t rK = make_rsrc(P.k + rowbase * H, ACATTN_BYTES(1, seq_bytes));
  const rsrc_t rV = make_rsrc(P.v + rowbase * H, ACATTN_BYTES(2, seq_bytes));
  const rsrc_t rKa = make_rsrc((ADV ? P.ka : P.k) + rowbase * H, ACATTN_BYTES(1, seq_bytes));
  const int koff = ((int)__umul24(c, H) + hoff + KS * g) * 4;      // row c of a key tile, this lane's slice of the head
  const int voff = ((int)__umul24(4 * g, H) + hoff + VW * c) * 4;  // row 4 g of a key tile, columns VW c.. of the head
  const int irow = (int)__umul24(i, L);

  // ---- key flags, query fragments, query halves of the affines ---------------------------------------------------------
  uint8_t kvb[NG];
  {
    const rsrc_t rF = make_rsrc(P.key_valid + rowbase, L);
#pragma unroll
    for (int q = 0; q < NG; ++q) kvb[q] = __builtin_amdgcn_raw_buffer_load_b8(rF, 64 * q + lane, 0, 0);
  }
  float qf[KS], qaf[KS];
  {
    const rsrc_t rQ = make_rsrc(P.q + rowbase * H, ACATTN_BYTES(0, seq_bytes));
    const rsrc_t rQa = make_rsrc((ADV ? P.qa : P.q) + rowbase * H, ACATTN_BYTES(0, seq_bytes));
    const int qoff = ((int)__umul24(i, H) + hoff + KS * g) * 4;  // rows past L: out of range, zeros
#pragma unroll
    for (int s4 = 0; s4 < KS / 4; ++s4) {
      const f4 t = bload4(rQ, qoff + 16 * s4, 0);
      f4 ta = t;
      if (ADV) ta = bload4(rQa, qoff + 16 * s4, 0);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        qf[4 * s4 + e] = t[e];
        qaf[4 * s4 + e] = ta[e];
      }
    }
  }
  // PRE: planes [4][16 nT] per (b, head): -log2(e) (q_i.w_o[:dh] + b_o), q_i.w_d[:dh] + b_d, -log2(e) k_j.w_o[dh:],
  // k_j.w_d[dh:]  (acattn.h: acattn_problem.affine)
  const int LP = 16 * nT;
  const rsrc_t rA = make_rsrc(PRE ? P.affine + bh * 4 * LP : P.q, PRE ? ACATTN_BYTES(4, 16 * LP) : 0);
  const int aoff = (2 * LP + 4 * g) * 4;
  float wko[PRE ? 1 : KS], wkd[PRE ? 1 : KS];  // key halves of the affine weights, this lane's slice (pass 1 only)
  float ao2, ad;
  if constexpr (PRE) {
    ao2 = bload1(rA, i * 4, 0);
    ad = bload1(rA, (LP + i) * 4, 0);
  } else {
    float ao = 0.f;
    ad = 0.f;
#pragma unroll
    for (int s4 = 0; s4 < KS / 4; ++s4) {
      const f4 a = *(const f4*)(P.w_order + KS * g + 4 * s4), d = *(const f4*)(P.w_dist + KS * g + 4 * s4);
      const f4 ak = *(const f4*)(P.w_order + DH + KS * g + 4 * s4), dk = *(const f4*)(P.w_dist + DH + KS * g + 4 * s4);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        ao += qf[4 * s4 + e] * a[e];
        ad += qf[4 * s4 + e] * d[e];
        wko[4 * s4 + e] = ak[e] * -kLog2e;  // pre-scaled: sigmoid(o) = 1 / (1 + exp2(ao2 + co2))
        wkd[4 * s4 + e] = dk[e];
      }
    }
    ao2 = -kLog2e * (quad_sum(ao) + P.b_order[0]);
    ad = quad_sum(ad) + P.b_dist[0];
  }
  const int ntc = causal ? min(nT, qb + 1) : nT;  // key tiles the causal mask leaves (known without the validity bytes)
  f4 kall[UPF ? NT : 1][KS / 4], kaall[UPF ? NT : 1][KS / 4], coA[UPF ? NT : 1], cdA[UPF ? NT : 1];
  float vfk[KEEPV ? NT : 1][4][VW];
  f4 glk[KEEPV ? NT : 1];
  const rsrc_t rG = make_rsrc(ADV ? P.gate_logits + rowbase * L : nullptr, ADV ? ACATTN_BYTES(3, L * L * 4) : 0);
  const int goff = (irow + 4 * g) * 4;
  // ONE register set for the K / Ka fragments: tile t + 1 is requested into it right behind the MFMAs that read tile t
  // and lands under the elementwise work of tile t (a second set cost 16-32 registers: spills at dh = 64).  Tile 0 is
  // requested here, before the wave waits for anything (every row sees at least one key tile).
  f4 kb[KS / 4], kab[KS / 4];
  if constexpr (!UPF) {
#pragma unroll
    for (int s4 = 0; s4 < KS / 4; ++s4) {
      kb[s4] = bload4(rK, koff + 16 * s4, 0);
      if (ADV) kab[s4] = bload4(rKa, koff + 16 * s4, 0);
    }
  }
  if constexpr (UPF) {
#pragma unroll
    for (int t = 0; t < NT; ++t)
      if (t < ntc) {
        const int ko = koff + 16 * t * H4;
#pragma unroll
        for (int s4 = 0; s4 < KS / 4; ++s4) {
          kall[t][s4] = bload4(rK, ko + 16 * s4, 0);
          if (ADV) kaall[t][s4] = bload4(rKa, ko + 16 * s4, 0);
        }
        coA[t] = bload4(rA, aoff + 64 * t, 0);
        cdA[t] = bload4(rA, aoff + 4 * LP + 64 * t, 0);
      }
#pragma unroll
    for (int t = 0; t < NT; ++t)
      if (t < ntc) {
#pragma unroll
        for (int r = 0; r < 4; ++r) bloadw<VW>(rV, voff + (16 * t + r) * H4, 0, vfk[t][r]);
        if (ADV) glk[t] = bload4(rG, goff + 64 * t, 0);
      }
  }
  // ---- [r4] the random numbers of pass 2, drawn while the wave's first loads are in flight ---------------------------
  // Every wave of the launch starts at the same moment and asks for its q / qa rows, its first K / Ka tile, the key flags
  // and the affine planes at once: ~25 MB requested in one burst, and the median wave then sits 3.5 us (7,300 cycles; the
  // 10th percentile 1.7 us, the 90th 7.7: profiles/r04_probe/probe_e_stamps_*.txt) before its first operand is there --
  // the longest phase of its life, with nothing on the SIMD able to issue.  The normals and keep bits of pass 2 depend on
  // (seed, row, key group) only, so they are drawn HERE, under that wait: ~43 vector instructions per tile (a sixth of a
  // wave's arithmetic) leave the critical path.  16 registers for the normals of four tiles + 1 for the packed keep bits,
  // live until pass 2 (pass 1 has the room: V and the gate tiles are not requested yet).  L <= 64, p_drop = 0.5 form only.
  // MEASURED [r4] (profiles/r04_probe/probe_f_*.txt, probe_g_*.txt): 15.92-15.96 against 16.03-16.07 us, inside the noise --
  // the four waves of a SIMD interleave their prologues (190 vector instructions each), so the "wait" was never idle
  // time; the draws only moved.  It costs 12 spilled registers.  Off by default; -DACATTN_EARLY_NOISE builds it.
#ifdef ACATTN_EARLY_NOISE
  constexpr bool kEarlyNoise = ADV && HALF && NT <= 4 && !UPF;
#else
  constexpr bool kEarlyNoise = false;
#endif
  F22 n2pre[kEarlyNoise ? NT : 1];
  uint32_t keep_pk = 0u;  // bits 8 t + r: keep_after, bits 8 t + 4 + r: keep_mask of key tile t
  if constexpr (kEarlyNoise) {
    const RngKey rkey0 = rng_key(P.seed + (P.seed_device ? *P.seed_device : 0ull));
    const uint32_t rng_row0 = (uint32_t)(bh * L + i);
    __builtin_amdgcn_sched_barrier(0);  // the requests above stay above
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      if (t < ntc) {
        const RngDraw rd = rng_draw_half(rkey0, rng_row0, (uint32_t)(4 * t + g), kLog2e);
        n2pre[t] = pin(F22{rd.n01, rd.n23});
        keep_pk |= (rd.keep_after | (rd.keep_mask << 4)) << (8 * t);
      }
    }
    __builtin_amdgcn_sched_barrier(0);  // ... and nothing that waits for them moves in front of the draws
  }
  const float sc = P.scalar[0];

  unsigned long long vk[NG];
  bool any_valid = false;
  int first_valid = L, last_valid = -1;
#pragma unroll
  for (int q = NG - 1; q >= 0; --q) {
    vk[q] = __ballot(kvb[q] != 0);
    if (vk[q]) {
      any_valid = true;
      first_valid = 64 * q + __ffsll((long long)vk[q]) - 1;
      if (last_valid < 0) last_valid = 64 * q + 63 - __clzll((long long)vk[q]);
    }
  }
  const int nt_valid = any_valid ? (last_valid >> 4) + 1 : nT;
  const bool rows_see_a_key = causal ? first_valid <= i0 : any_valid;
  const int nt = rows_see_a_key ? min(causal ? min(nT, qb + 1) : nT, nt_valid) : nT;

  // Allowed-key bits of this lane in the ballot's own layout: bit 16 t' + r of word pair t / 4  <=>  key 16 t + 4 g + r
  // is a real item and (causal) not after the query; the other bits of a word are never tested.  The reference adds
  // -10000 to masked scores (abstract_recommender.py:142), so a row WITHOUT an allowed key spreads over every key < L:
  // such a row gets the "key < L" bits.  `ab` marks keys after the query (layers.py:715-719 takes log(sigmoid) there,
  // log(1 - sigmoid) elsewhere).
  constexpr unsigned long long kNib = 0x000F000F000F000Full;
  auto low_bits = [](int n) -> unsigned long long {  // bits 0 .. n set (none for n < 0)
    return n < 0 ? 0ull : (n >= 63 ? ~0ull : (2ull << n) - 1ull);
  };
  uint32_t ebw[2 * NG], abw[2 * NG];
  uint32_t seen = 0u;
#pragma unroll
  for (int q = 0; q < NG; ++q) {
    const unsigned long long at_or_before = low_bits(i - 4 * g - 64 * q);
    unsigned long long e = (vk[q] >> (4 * g)) & kNib;
    if (causal) e &= at_or_before;
    ebw[2 * q] = (uint32_t)e;
    ebw[2 * q + 1] = (uint32_t)(e >> 32);
    abw[2 * q] = (uint32_t)~at_or_before;
    abw[2 * q + 1] = (uint32_t)(~at_or_before >> 32);
    seen |= ebw[2 * q] | ebw[2 * q + 1];
  }
  // fully masked row (left padding): uniform over every key < L.  A row's keys are spread over its four lanes.
  const bool row_dead = quad_or(seen) == 0u;
  const unsigned long long dead_m = __ballot(row_dead);  // see dead_row_quantise
  const bool any_dead = dead_m != 0ull;
  if (any_dead) {
#pragma unroll
    for (int q = 0; q < NG; ++q) {
      const unsigned long long in = low_bits(L - 1 - 4 * g - 64 * q) & kNib;
      if (row_dead) {
        ebw[2 * q] = (uint32_t)in;
        ebw[2 * q + 1] = (uint32_t)(in >> 32);
      }
    }
  }
  // under a causal mask the keys after the query carry probability exactly 0 unless the row is dead
  const bool order_select = !causal || any_dead;
  auto ebit = [&](int t, int r) -> int { return sbit(ebw[2 * (t >> 2) + ((t >> 1) & 1)], 16 * (t & 1) + r); };
  auto abit = [&](int t, int r) -> int { return sbit(abw[2 * (t >> 2) + ((t >> 1) & 1)], 16 * (t & 1) + r); };

  const float hs2 = 0.5f * (sc * sc);
  const float inv_sqrt = 1.0f / sqrtf((float)DH);
  const float scale2 = inv_sqrt * kLog2e;
  const float nc2 = -(hs2 * scale2);
  const float kNegMask2 = ACATTN_MASK_FILL * kLog2e;
  const bool has_drop = HALF || P.p_drop > 0.f;
  const float keep_scale = HALF ? 2.0f : (has_drop ? fast_rcp(1.0f - P.p_drop) : 1.0f);
  const uint32_t rng_row = (uint32_t)(bh * L + i);
  const RngKey rkey = rng_key(P.seed + (P.seed_device ? *P.seed_device : 0ull));

  // M leaves through LDS.  In the MFMA layout a store instruction is 64 pieces of 16 bytes spread over 16 rows of a
  // [L, L] matrix (pitch 4 L bytes): every piece a partial, misaligned line -- 8 us of the launch at B = 512, L = 50
  // with the output compiled out against 10 MB written (tools/probe, ACATTN_ZERO=32).  But the 16 rows a wave owns are
  // ONE contiguous block of 64 L bytes: the tiles are laid down in LDS as that block and leave as whole 1 KB runs.
  const int blk_rows = min(16, L - i0);
  const int n_blk = blk_rows > 0 ? blk_rows * L : 0;  // floats of this wave's block of M[b, head]
  const rsrc_t rM = make_rsrc(ADV ? O.attack_mask + (bh * L + i0) * L : nullptr, ADV ? ACATTN_BYTES(5, n_blk * 4) : 0);
  float* const mrow = m_stage + c * L + 4 * g;
  // M (or a zero tile) of key tile t into the block; columns past L would land in the next row
  auto stage_seg = [&](int t, const f4 val) {
    float* p = mrow + 16 * t;
    if (t < nT - 1) {
#pragma unroll
      for (int r = 0; r < 4; ++r) p[r] = val[r];
    } else {
      const int j0 = 16 * t + 4 * g;
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (j0 + r < L) p[r] = val[r];
    }
  };
  // (acattn_fwd_out.penalty_part: the block's sum of (1 - M)^2.  Long sequences form it from the values as they leave.
  // L <= 64 runs at its register limit there -- the sums inside store_block cost the dh = 32 kernel 8 spilled registers --
  // so it sums the block, which stays in LDS, at the very end of the wave, where nothing else is live: kPenaltyLate.
  // p_drop = 0.5 only: the general-p instantiation sits at 128 registers as well and spilled 4-8 of them wherever the
  // sums were put (inside store_block, at the end, behind a call), so its launcher leaves them to the launch behind it.)
  constexpr bool kPenalty = ADV && NT > 4;
  constexpr bool kPenaltyLate = ADV && NT <= 4 && HALF;
  const bool want_pen = kPenalty && O.penalty_part != nullptr;
  float pen_acc = 0.f;
  auto store_block = [&]() {
#pragma unroll
    for (int k = 0; k < (16 * 16 * NT + 255) / 256; ++k) {
      if (256 * k < n_blk) {
        const f4 val = *(const f4*)(m_stage + 256 * k + 4 * lane);
        if (want_pen) {
          const int o0 = 256 * k + 4 * lane;
          const f4 d = 1.0f - val;
          if (o0 + 4 <= n_blk) {
            pen_acc += (d[0] * d[0] + d[1] * d[1]) + (d[2] * d[2] + d[3] * d[3]);
          } else {
#pragma unroll
            for (int r = 0; r < 4; ++r)
              if (o0 + r < n_blk) pen_acc += d[r] * d[r];
          }
        }
        if ((n_blk & 3) == 0) {
          bstore4m(rM, 16 * lane + 1024 * k, 0, val);  // past the block: out of range, dropped
        } else {  // odd L with a short last block: the run ends inside a 16-byte piece
          const int o = 256 * k + 4 * lane;
          if (o + 4 <= n_blk) {
            bstore4m(rM, 16 * lane + 1024 * k, 0, val);
          } else {
#pragma unroll
            for (int r = 0; r < 4; ++r)
              if (o + r < n_blk) bstore1(rM, 16 * lane + 1024 * k + 4 * r, 0, val[r]);
          }
        }
      }
    }
  };

  ACATTN_STAMP(1);
  if ((ACATTN_ZERO) & 256) {  // timing-only: launch + prologue
    if (ebw[0] == 0x12345u && qf[0] == 1.25f && ao2 == ad) O.ctx_calibrated[lane] = sc;
    return;
  }
  __syncthreads();  // the distance table (one wave: a wait, no rendezvous)
  const float* const ltp = lt_tab + (13 + i0 + c - 4 * g);  // ltp[16 (NT - 1 - t) + 3 - r] = log(|i - (16 t + 4 g + r)| + 1)

  // [r4, PROBE] Everything from here on as ONE generic body: NTB > 0 = the key-tile count of the wave as a compile-time
  // constant (L <= 64: four straight-line copies, no wave-uniform branch around a tile, so the scheduler would see a pass
  // as one block and could overlap the dependent chains of neighbouring tiles); NTB = 0 = the run-time guards, which is
  // what ships (see the dispatch at the end of the kernel).
  auto rest = [&](auto ntb_c) __attribute__((always_inline)) {
  constexpr int NTB = decltype(ntb_c)::value;
  auto on = [&](int t) -> bool {
    if constexpr (NTB > 0)
      return t < NTB;
    else
      return t < nt;
  };
  // ---- pass 1: scores, spatial calibrator, first-level softmaxes ----------------------------------------------------------
  f4 tS[NT], tM[NT];
  float mx = ACATTN_NEG_INF, my = ACATTN_NEG_INF;
  // the fragments of tile t + 1 are requested before tile t is worked on (two register sets, roles fixed per tile)

  const f2 ao2s = splat2(ao2), ads = splat2(ad), nc2s = splat2(nc2);
  auto pass1 = [&](auto sel_tag) __attribute__((always_inline)) {
    constexpr bool SEL = decltype(sel_tag)::value;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      if (on(t)) {
        ACATTN_TILE_FENCE;
        f4 co4, cd4;
        if constexpr (UPF) {
          co4 = coA[t];
          cd4 = cdA[t];
        } else if constexpr (PRE) {
          co4 = bload4(rA, aoff + 64 * t, 0);
          cd4 = bload4(rA, aoff + 4 * LP + 64 * t, 0);  // LP is run time: folded into the voffset register by the compiler
        }
        f4(&k4)[KS / 4] = UPF ? kall[UPF ? t : 0] : kb;
        f4(&ka4)[KS / 4] = UPF ? kaall[UPF ? t : 0] : kab;
        f4 aS = {0.f, 0.f, 0.f, 0.f}, aM = aS;
        if constexpr (!PRE) {
          // key halves of the affines for key 16 t + c (rank-1 form of layers.py:705-708), then to the lanes of the D layout
          float co = 0.f, cd = 0.f;
#pragma unroll
          for (int s4 = 0; s4 < KS / 4; ++s4) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              co += k4[s4][e] * wko[4 * s4 + e];
              cd += k4[s4][e] * wkd[4 * s4 + e];
            }
          }
          co = quad_sum(co);
          cd = quad_sum(cd);
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int src = 4 * (4 * g + r);  // byte index of lane c' = 4 g + r (its g' = 0 copy)
            co4[r] = __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(src, __builtin_bit_cast(int, co)));
            cd4[r] = __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(src, __builtin_bit_cast(int, cd)));
          }
        }
#pragma unroll
        for (int s4 = 0; s4 < KS / 4; ++s4) {
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            aS = mfma16(k4[s4][e], qf[4 * s4 + e], aS);
            if (ADV) aM = mfma16(ka4[s4][e], qaf[4 * s4 + e], aM);
          }
        }
        if (!UPF && t + 1 < NT && on(t + 1)) {
          // (the row part of an offset goes into the VGPR offset: the descriptor's range check ignores the SGPR offset)
          const int ko = koff + 16 * (t + 1) * H4;
#pragma unroll
          for (int s4 = 0; s4 < KS / 4; ++s4) {
            kb[s4] = bload4(rK, ko + 16 * s4, 0);
            if (ADV) kab[s4] = bload4(rKa, ko + 16 * s4, 0);
          }
        }
        const F22 e1 = map4(split4(co4) + ao2s, [](float x, int) { return ex2(x); });
        const F22 pr = map4(e1 + 1.0f, [](float x, int) { return fast_rcp(x); });
        F22 val = 1.0f - pr;  // layers.py:715-719: key at or before the query -> log(1 - p)
        if constexpr (SEL) val = map4(val, [&](float x, int r) { return bit_select(abit(t, r), r < 2 ? pr.lo[r] : pr.hi[r - 2], x); });
        const F22 lg = map4(val + ACATTN_LOG_EPS, [](float x, int) { return lg2(x); });
        F22 lt{f2{ltp[16 * (NT - 1 - t) + 3], ltp[16 * (NT - 1 - t) + 2]}, f2{ltp[16 * (NT - 1 - t) + 1], ltp[16 * (NT - 1 - t)]}};
        lt = pin(lt);  // log(|i - j| + 1)   layers.py:721-723
        F22 mk{f2{and_bits(kNegMask2, ~ebit(t, 0)), and_bits(kNegMask2, ~ebit(t, 1))},
               f2{and_bits(kNegMask2, ~ebit(t, 2)), and_bits(kNegMask2, ~ebit(t, 3))}};
        mk = pin(mk);
        const F22 df = lt - (split4(cd4) + ads);  // layers.py:721-726
        F22 x = fma22(split4(aS), scale2, mk);    // (S + e_o + e_d) / sqrt(dh) + mask, exp2 domain
        x = fma22(lg, inv_sqrt, x);
        x = fma22(df * df, nc2s, x);
        if constexpr (SEL) {  // (a wave with a dead row runs the SEL form: order_select)
          if (any_dead) x = dead_row_quantise(x, dead_m);
        }
        tS[t] = join4(x);
        mx = max4(mx, x);
        if (ADV) {
          F22 y = fma22(split4(aM), scale2, mk);
          if constexpr (SEL) {
            if (any_dead) y = dead_row_quantise(y, dead_m);
          }
          tM[t] = join4(y);
          my = max4(my, y);
        }
      }
    }
  };
  if (order_select)
    pass1(std::true_type{});
  else
    pass1(std::false_type{});

  ACATTN_STAMP(2);
  if ((ACATTN_ZERO) & 512) {  // timing-only: launch + prologue + pass 1
    float acc = mx + my;
#pragma unroll
    for (int t = 0; t < NT; ++t)
      if (on(t)) acc += tS[t][0] + tS[t][1] + tS[t][2] + tS[t][3] + tM[t][0] + tM[t][1] + tM[t][2] + tM[t][3];
    if (acc == 1.2345f) O.ctx_calibrated[lane] = acc;
    return;
  }
  // V fragments: vf[.][r][e] = V[16 t + 4 g + r][VW c + e]; rows past L read as zeros (their probabilities are zero)
  if constexpr (KEEPV && !UPF) {
#pragma unroll
    for (int t = 0; t < NT; ++t)
      if (on(t)) {
        ACATTN_TILE_FENCE;
#pragma unroll
        for (int r = 0; r < 4; ++r) bloadw<VW>(rV, voff + (16 * t + r) * H4, 0, vfk[t][r]);
      }
  }

  mx = quad_max(mx);
  if (ADV) my = quad_max(my);
  const f2 mxs = splat2(mx), mys = splat2(my);
  f2 zx2 = {0.f, 0.f}, zy2 = zx2;
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    if (on(t)) {
      ACATTN_TILE_FENCE;
      const F22 e = map4(split4(tS[t]) - mxs, [](float x, int) { return ex2(x); });
      tS[t] = join4(e);
      zx2 += e.lo + e.hi;
      if (ADV) {
        const F22 f = map4(split4(tM[t]) - mys, [](float x, int) { return ex2(x); });
        tM[t] = join4(f);
        zy2 += f.lo + f.hi;
      }
    }
  }
  ACATTN_STAMP(3);
  const float zx = quad_sum(zx2[0] + zx2[1]);
  const float zy = ADV ? quad_sum(zy2[0] + zy2[1]) : 1.f;
  // dropout's 1 / (1 - p) folded in; with the adversarial calibrator P only ever enters an exp2 argument: log2(e) too
  const float rzx = fast_rcp(zx) * (ADV ? keep_scale * kLog2e : keep_scale), rzy = fast_rcp(zy) * keep_scale;

  const f2 rzxs = splat2(rzx), rzys = splat2(rzy);
  f4 ca[VW], cc[VW];
#pragma unroll
  for (int e = 0; e < VW; ++e) {
    ca[e] = f4{0.f, 0.f, 0.f, 0.f};
    cc[e] = ca[e];
  }
  f2 zu2 = {0.f, 0.f}, zv2 = zu2, zw2 = zu2;

  // gate tiles (probabilities when PRE): requested before pass 2, consumed in pass 3
  if constexpr (KEEPV && ADV && !UPF) {
#pragma unroll
    for (int t = 0; t < NT; ++t)
      if (on(t)) glk[t] = bload4(rG, goff + 64 * t, 0);
  }

  // ---- pass 1.5 [r4, PROBE BUILD ONLY: -DACATTN_EARLY_M]: M = dropout(softmax(Sa / sqrt(dh) + mask)) leaves before pass 2 ---
  // M is complete as soon as its normaliser is: 40 % of what the launch writes (10 of 23 MB at B = 512, L = 50), and with
  // the output compiled out the launch is 3.3 us (ragged) / 8 us (full length) shorter (DESIGN 4.1).  The idea: issue the
  // block before the bulk of the arithmetic (the random numbers, six of the eleven transcendentals, both P.V products)
  // instead of between passes 2 and 3.  MEASURED (profiles/r04_probe/probe_d3_*.txt): 0.3-0.7 us SLOWER at L = 50, equal
  // at L = 200, under every cache policy of the stores (default, sc0, sc1 write-through, nt, combinations; nt stays the
  // best, write-through costs 1-2 us).  When the stores are issued does not matter: what they cost is paid where the
  // dirty lines leave the XCDs' L2s, not where the wave issues them.  Kept as a probe switch.
  // Memory instructions of a wave retire in order (vmcnt): a load requested BEHIND the stores is only "there" once they
  // have been acknowledged -- with the gate tiles requested after the block the early form was 0.5 us SLOWER than round 3's.
  // So the gate tiles (pass 3) are requested first, and the form is used where every operand of passes 2-3 is already in
  // registers or in flight (KEEPV: L <= 64); the long form loads V and the gate per tile inside passes 2-3 and keeps its
  // store between them.
#ifdef ACATTN_EARLY_M
  constexpr bool kEarlyM = ADV && KEEPV && !UPF;  // probe build
#else
  constexpr bool kEarlyM = false;  // measured [r4]: round 3's order (the block stored between passes 2 and 3) is the faster one
#endif
  if constexpr (kEarlyM) {
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      if (on(t)) {
        ACATTN_TILE_FENCE;
        F22 m = split4(tM[t]) * rzys;
        if (has_drop) {
          uint32_t km;
          if constexpr (HALF)
            km = rng_keep_mask_half(rkey, rng_row, (uint32_t)(4 * t + g));
          else
            km = rng_group(rkey, rng_row, (uint32_t)(4 * t + g), P.p_drop).keep_mask;
          m = map4(m, [&](float x, int r) { return keep_and(x, km, r); });
        }
        tM[t] = join4(m);
        stage_seg(t, tM[t]);
      }
    }
    for (int t = nt; t < nT; ++t) stage_seg(t, f4{0.f, 0.f, 0.f, 0.f});  // skipped tiles
    store_block();
    if (want_pen) {
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) pen_acc += __shfl_xor(pen_acc, off);
      if (lane == 0) O.penalty_part[bh * nT + qb] = pen_acc;
    }
  }

  // ---- pass 2: dropout, M out, perturbed branch into P.V, exp of the calibrated branch --------------------------------------
  // (a wave that holds a fully masked row quantises the soft-max arguments of that row as the reference does: small
  // wave-uniform blocks, no second copy of the passes -- a copy cost the 4-waves-per-SIMD instantiation 61 spilled registers)
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    if (on(t)) {
      ACATTN_TILE_FENCE;
      float vl[4][VW];
      if constexpr (!KEEPV) {
#pragma unroll
        for (int r = 0; r < 4; ++r) bloadw<VW>(rV, voff + (16 * t + r) * H4, 0, vl[r]);  // in flight under the random numbers
      }
      const float(&vf)[4][VW] = KEEPV ? vfk[KEEPV ? t : 0] : vl;
      F22 n2{f2{0.f, 0.f}, f2{0.f, 0.f}};  // standard normals times log2(e)
      uint32_t ka = 0xFu, km = 0xFu;
      if constexpr (kEarlyNoise) {
        n2 = n2pre[kEarlyNoise ? t : 0];
        ka = keep_pk >> (8 * t);  // (keep_and tests bit r of its argument: the bits above it are ignored)
        km = keep_pk >> (8 * t + 4);
      } else if (ADV || has_drop) {
        if constexpr (HALF) {
          const RngDraw rd = rng_draw_half(rkey, rng_row, (uint32_t)(4 * t + g), kLog2e);
          n2 = pin(F22{rd.n01, rd.n23});
          ka = rd.keep_after;
          km = rd.keep_mask;
        } else {
          const RngGroup rg = rng_group(rkey, rng_row, (uint32_t)(4 * t + g), P.p_drop);
          n2 = split4(rg.n) * kLog2e;
          if (has_drop) {
            ka = rg.keep_after;
            km = rg.keep_mask;
          }
        }
      }
      F22 p = split4(tS[t]) * rzxs;  // P = dropout(softmax) (times log2(e) when ADV)   layers.py:735-736
      if (has_drop) p = map4(p, [&](float x, int r) { return keep_and(x, ka, r); });
      tS[t] = join4(p);
      f4 eu;
      if (ADV) {
        F22 m = split4(tM[t]);  // M (pass 1.5)   layers.py:670-672
        if constexpr (!kEarlyM) {
          m = m * rzys;
          if (has_drop) m = map4(m, [&](float x, int r) { return keep_and(x, km, r); });
          stage_seg(t, join4(m));
        }
        F22 au = fma22(n2, 1.0f - m, p * m);         // layers.py:918-919 (exp2 domain)
        const F22 a1 = fma22(m, -kLog2e, kLog2e);    // exp(1 - M)
        const int eb4[4] = {ebit(t, 0), ebit(t, 1), ebit(t, 2), ebit(t, 3)};
        if (any_dead) au = dead_row_quantise(au, dead_m);
        const F22 eu2 = map4(au, [&](float x, int r) { return and_bits(ex2(x), eb4[r]); });
        const F22 ex1 = map4(a1, [](float x, int) { return ex2(x); });
        zu2 += eu2.lo + eu2.hi;
        eu = join4(eu2);
        F22 av = p * ex1;
        if (any_dead) av = dead_row_quantise(av, dead_m);
        const F22 ev = map4(av, [&](float x, int r) { return and_bits(ex2(x), eb4[r]); });  // layers.py:920-921
        zv2 += ev.lo + ev.hi;
        tM[t] = join4(ev);  // M is dead from here on: keep the unnormalised A_c in its registers
      }
      const f4 pj = join4(p);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
#pragma unroll
        for (int e = 0; e < VW; ++e) {
          if (ADV)
            ca[e] = mfma16(vf[r][e], eu[r], ca[e]);
          else
            cc[e] = mfma16(vf[r][e], pj[r], cc[e]);  // spatial calibrator only: ctx = P.V
        }
      }
    }
  }

  if (ADV && !kEarlyM) {
    for (int t = nt; t < nT; ++t) stage_seg(t, f4{0.f, 0.f, 0.f, 0.f});  // skipped tiles
    store_block();  // travels under pass 3
    if (want_pen) {
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) pen_acc += __shfl_xor(pen_acc, off);
      if (lane == 0) O.penalty_part[bh * nT + qb] = pen_acc;
    }
  }
  ACATTN_STAMP(4);
  // ---- pass 3: gate combine, final softmax, calibrated branch into P.V ----------------------------------------------------
  // lane (c, g), accumulator e, register rr  ->  ctx[i0 + c][VW (4 g + rr) + e]: 4 VW consecutive columns per lane
  const rsrc_t rCc = make_rsrc(O.ctx_calibrated + rowbase * H, ACATTN_BYTES(6, seq_bytes));
  const int coff = ((int)__umul24(i, H) + hoff + 4 * VW * g) * 4;  // rows past L: out of range, dropped
  auto store_ctx = [&](rsrc_t rC, const f4 (&acc)[VW], float s) {
    float o[4 * VW];
#pragma unroll
    for (int rr = 0; rr < 4; ++rr)
#pragma unroll
      for (int e = 0; e < VW; ++e) o[VW * rr + e] = acc[e][rr] * s;
#pragma unroll
    for (int w = 0; w < VW; ++w) bstore4(rC, coff + 16 * w, 0, f4{o[4 * w], o[4 * w + 1], o[4 * w + 2], o[4 * w + 3]});
  };
  float zu = 1.f, zv = 1.f, zw = 1.f;
  if (ADV) {
    zu = quad_sum(zu2[0] + zu2[1]);
    // the perturbed branch is complete: its stores travel under pass 3
    store_ctx(make_rsrc(O.ctx_attacked + rowbase * H, ACATTN_BYTES(6, seq_bytes)), ca, fast_rcp(zu));
    zv = quad_sum(zv2[0] + zv2[1]);
    const f2 rzvs = splat2(fast_rcp(zv) * kLog2e);
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      if (on(t)) {
        ACATTN_TILE_FENCE;
        float vl[4][VW];
        f4 gl;
        if constexpr (!KEEPV) {
#pragma unroll
          for (int r = 0; r < 4; ++r) bloadw<VW>(rV, voff + (16 * t + r) * H4, 0, vl[r]);
          gl = bload4(rG, goff + 64 * t, 0);
        } else {
          gl = glk[KEEPV ? t : 0];
        }
        const float(&vf)[4][VW] = KEEPV ? vfk[KEEPV ? t : 0] : vl;
        F22 gt = split4(gl);
        if constexpr (!PRE) {
          const F22 eg = map4(gt * (-kLog2e), [](float x, int) { return ex2(x); });
          gt = map4(eg + 1.0f, [](float x, int) { return fast_rcp(x); });  // sigmoid(gate logits)   layers.py:887
        }
        const F22 acn = split4(tM[t]) * rzvs;                    // A_c log2(e)
        F22 aw = fma22(gt, split4(tS[t]) - acn, acn);           // layers.py:888, 925 (exp2 domain)
        if (any_dead) aw = dead_row_quantise(aw, dead_m);
        const F22 ew2 = map4(aw, [&](float x, int r) { return and_bits(ex2(x), ebit(t, r)); });
        zw2 += ew2.lo + ew2.hi;
        const f4 ew = join4(ew2);
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
          for (int e = 0; e < VW; ++e) cc[e] = mfma16(vf[r][e], ew[r], cc[e]);
      }
    }
    zw = quad_sum(zw2[0] + zw2[1]);
  }
  ACATTN_STAMP(5);
  store_ctx(rCc, cc, ADV ? fast_rcp(zw) : 1.0f);

  if (ADV && O.row_stats && g == 0 && row_ok) {
    // natural-log normalisers, as the backward expects them (acattn_bwd.hip): its recomputation adds the -10000
    // of a dead row to every score, so that shift goes into the stored normalisers
    float* sp = O.row_stats + (bh * L + i) * ACATTN_NSTAT;
    const float sh = row_dead ? ACATTN_MASK_FILL : 0.f;
    store_out4(sp, f4{(mx + lg2(zx)) * kLn2 + sh, (my + lg2(zy)) * kLn2 + sh, sh + fast_log(zu), sh + fast_log(zv)});
    store_out4(sp + 4, f4{sh + fast_log(zw), 0.f, 0.f, 0.f});
  }
  if constexpr (kPenaltyLate) {
    if (O.penalty_part) {  // (wave-uniform: a launch without it branches around the sums)
      __builtin_amdgcn_sched_barrier(0);  // the LDS reads stay down here (hoisted into pass 3 they are spills again)
      float pen = 0.f;
#pragma unroll
      for (int k = 0; k < (16 * 16 * NT + 255) / 256; ++k) {
        if (256 * k < n_blk) {
          const int o0 = 256 * k + 4 * lane;
          const f4 d = 1.0f - *(const f4*)(m_stage + o0);
          if (o0 + 4 <= n_blk) {
            pen += (d[0] * d[0] + d[1] * d[1]) + (d[2] * d[2] + d[3] * d[3]);
          } else {
#pragma unroll
            for (int r = 0; r < 4; ++r)
              if (o0 + r < n_blk) pen += d[r] * d[r];
          }
        }
      }
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) pen += __shfl_xor(pen, off);
      if (lane == 0) O.penalty_part[bh * nT + qb] = pen;
    }
  }
#ifdef ACATTN_STAMPS
  ACATTN_STAMP(6);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  ACATTN_STAMP(7);
  if (lane == 0 && P.noise) {
    unsigned long long* sb = (unsigned long long*)P.noise + (size_t)blockIdx.x * 16;
#pragma unroll
    for (int k = 0; k < 8; ++k) sb[k] = stamp_[k];
  }
#endif
  };
  // MEASURED [r4] (profiles/r04_probe/probe_g_*.txt): the four straight-line copies need 82-113 spilled registers at 128
  // (with or without the per-tile fence, with or without the early draws) and run 23.7-25.4 us against 16.0: the
  // run-time guards stay.  -DACATTN_STRAIGHT_TILES builds the copies.
#ifndef ACATTN_STRAIGHT_TILES
  rest(std::integral_constant<int, 0>{});
#else
  if constexpr (NT <= 4) {
    switch (nt) {
      case 1: rest(std::integral_constant<int, 1>{}); break;
      case 2: rest(std::integral_constant<int, 2>{}); break;
      case 3: rest(std::integral_constant<int, 3>{}); break;
      default: rest(std::integral_constant<int, (NT < 4 ? NT : 4)>{}); break;
    }
  } else {
    rest(std::integral_constant<int, 0>{});
  }
#endif
}

template <int DH, int NT, bool PRE>
int launch_stream_nt(const acattn_problem& p, const acattn_fwd_out& o, hipStream_t stream) {
  const int nT = (p.L + 15) / 16;
  const dim3 grid(p.B * p.n_heads * nT), block(64);
  const bool half = p.p_drop == 0.5f;
  if (p.adversarial) {
    if (half)
      hipLaunchKernelGGL((acattn_fwd_stream_kernel<DH, NT, true, true, PRE>), grid, block, 0, stream, p, o);
    else
      hipLaunchKernelGGL((acattn_fwd_stream_kernel<DH, NT, true, false, PRE>), grid, block, 0, stream, p, o);
  } else {
    if (half)
      hipLaunchKernelGGL((acattn_fwd_stream_kernel<DH, NT, false, true, PRE>), grid, block, 0, stream, p, o);
    else
      hipLaunchKernelGGL((acattn_fwd_stream_kernel<DH, NT, false, false, PRE>), grid, block, 0, stream, p, o);
  }
  return (int)hipGetLastError();
}

}  // namespace

#define ACATTN_CAT2(a, b) a##b
#define ACATTN_CAT(a, b) ACATTN_CAT2(a, b)
// pre != 0: p.affine is set (and, with the adversarial calibrator, p.gate_logits holds probabilities)
int ACATTN_CAT(acattn_launch_fwd_stream_dh, ACATTN_STREAM_DH)(const acattn_problem& p, const acattn_fwd_out& o, int pre, hipStream_t stream) {
  constexpr int DH = ACATTN_STREAM_DH;
  // both forms fill acattn_fwd_out.penalty_part themselves, the 4-tile form at p_drop = 0.5 only (see kPenaltyLate).
  // ACATTN_FWD_PENALTY=separate (measurement) keeps the 4-tile form's sums in acattn_launch_penalty_rows behind the launch.
  static const bool separate4 = getenv("ACATTN_FWD_PENALTY") && !strcmp(getenv("ACATTN_FWD_PENALTY"), "separate");
  if (p.L <= 64) {
    acattn_fwd_out o4 = o;
    if (separate4 || p.p_drop != 0.5f) o4.penalty_part = nullptr;
    if (p.adversarial && o4.penalty_part) acattn_penalty_written_set(true);
    return pre ? launch_stream_nt<DH, 4, true>(p, o4, stream) : launch_stream_nt<DH, 4, false>(p, o4, stream);
  }
  if (p.adversarial && o.penalty_part) acattn_penalty_written_set(true);
  return pre ? launch_stream_nt<DH, 13, true>(p, o, stream) : launch_stream_nt<DH, 13, false>(p, o, stream);
}
