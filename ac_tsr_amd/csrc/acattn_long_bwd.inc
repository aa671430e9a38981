// Backward of the fused calibrated attention, LONG form (any L up to acattn_max_sequence_length(), every option of the
// long forward): the two-kernel shape and the mathematics of acattn_bwd_stream.hip with its compile-time parts made
// run-time ones.  Included by acattn_long_bwd_dh{16,32,64,128}.hip (ACATTN_LONG_DH).
//
//   row kernel   one wave per (sequence, head, 16-row query block):
//                sweep 1 -> the row scalars of the chained soft-max backward, from sums that are accumulated tile by tile
//                           (below), kept in the workspace for the key kernel;
//                sweep 2 -> dS, dSa tile by tile -> dq, dqa (MFMA, registers), the gate-logit partials, the query halves
//                           of the calibrator parameter gradients;
//   key kernel   one wave per (sequence, head, 16-key tile): sweeps the query blocks that see the tile, rebuilds the same
//                tiles, turns them through an LDS scratch and accumulates dK, dKa, dV in registers (MFMA), plus the key
//                halves of the calibrator parameter gradients.
//
// Every probability tile is rebuilt from the forward's log-normalisers (row_stats) with the arithmetic of
// acattn_long_fwd.inc: the additive mask is ADDED (x + -10000 in fp32), so structured and dense masks, and the
// reference's quantisation of fully masked rows, need no case of their own; key flags are a per-key table in LDS of
// 16 * ceil(L / 16) floats (no ballot words: nothing here is sized by the ceiling); [L, L] tensors are addressed from
// 64-bit per-(sequence, head) row pointers.
//
// Row scalars (per query row; sums over keys):   da = <A_p, dA_p>   dc = <A_w, dA_w>   rf = <A_f, dw>  (combine FIXED: the
// inner soft-max A_f = softmax(P + A_c / 2))   r1 = <A_c, dA_c>   sP = <P, dP>   sM = <M, dM>.  With
//     dw = A_w (dA_w - dc),  e = dw - phi rf,  dA_c = kappa e,  dP(combine) = pi e
//     (gate g: pi = g, kappa = 1 - g, phi = 0;  annealing: g = rate;  fixed: pi = A_f, kappa = A_f / 2, phi = 1)
// every one of them is affine in the ones before it with tile-local coefficients, so ONE sweep accumulates seventeen
// sums (the streaming pair's twelve and the five that carry rf) from which all six follow.
// Reference: recbole/model/layers.py:657-742, 883-951 (what is differentiated).
#include <stdlib.h>

#include <algorithm>

#include "acattn_long_common.h"

namespace {

__device__ __forceinline__ float row16_sum(float v) {  // over the 16 lanes of a DPP row (same g, all c)
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1, 0xF, 0xF, false));
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x4E, 0xF, 0xF, false));
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x141, 0xF, 0xF, false));
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x140, 0xF, 0xF, false));
  return v;
}

// ... and the kernel arguments are fetched group by group: left alone, every scalar load of the prologue is issued at the
// top and the two argument structs (100 dwords) are live at once
#define VFENCE(x)                      \
  do {                                 \
    VREG(x);                           \
    __builtin_amdgcn_sched_barrier(0); \
  } while (0)
constexpr float kLog2e = 1.44269504088896340736f;
constexpr int NSC = 16;  // floats per row in the workspace: da, dc, r1, sP, sM, rf, (2 spare), cx, cy, cu, cv, cw, cf, (2 spare)

// Constants and options of a launch (wave-uniform).
// The yes / no options travel as bits of ONE scalar register: a wave-uniform bool that the optimiser hoists out of a loop is a
// 64-bit lane mask (two scalar registers each, and there are twenty of them); refresh() at the top of a loop body makes the
// word opaque, so every test is re-derived from it where it is used.
enum : uint32_t {
  F_STRUCTURED = 1u << 0, F_DENSE_LL = 1u << 1, F_CAUSAL = 1u << 2, F_ORDER = 1u << 3, F_DIST = 1u << 4, F_COUNTER = 1u << 5,
  F_DROP = 1u << 6, F_GA = 1u << 7, F_GC = 1u << 8, F_NOISE = 1u << 9, F_KEEPA = 1u << 10, F_KEEPM = 1u << 11, F_DM = 1u << 12,
  F_DPEN = 1u << 13, F_DG = 1u << 14, F_PRE = 1u << 15
};
struct Opt {
  int L, H, nT, LP, combine;
  uint32_t flags;
  __device__ __forceinline__ bool has(uint32_t f) const { return (flags & f) != 0; }
  __device__ __forceinline__ bool structured() const { return has(F_STRUCTURED); }
  __device__ __forceinline__ bool dense_ll() const { return has(F_DENSE_LL); }
  __device__ __forceinline__ bool causal() const { return has(F_CAUSAL); }
  __device__ __forceinline__ bool use_order() const { return has(F_ORDER); }
  __device__ __forceinline__ bool use_dist() const { return has(F_DIST); }
  __device__ __forceinline__ bool counter() const { return has(F_COUNTER); }
  __device__ __forceinline__ bool has_drop() const { return has(F_DROP); }
  __device__ __forceinline__ void refresh() {
    uint32_t v = flags;
    asm volatile("" : "+v"(v));
    flags = __builtin_amdgcn_readfirstlane(v);
  }
  int gate_is_prob;
  float inv_sqrt, sc, s2, hs2, keep_scale, p_drop, rate;
  RngKey rkey;
};
__device__ __forceinline__ Opt make_opt(const acattn_problem& P, const acattn_bwd_io& IO, int DH) {
  Opt K;
  K.L = P.L;
  K.H = P.H;
  K.nT = (P.L + 15) >> 4;
  K.LP = 16 * K.nT;
  K.combine = P.combine_option;
  const bool structured = P.mask_mode == ACATTN_MASK_STRUCTURED, counter = P.rng_mode == ACATTN_RNG_COUNTER;
  const bool drop = P.p_drop > 0.f, order = P.w_order != nullptr, dist = P.w_dist != nullptr;
  uint32_t f = 0;
  if (structured) f |= F_STRUCTURED;
  if (P.mask_mode == ACATTN_MASK_DENSE_LL) f |= F_DENSE_LL;
  if (structured && P.causal != 0) f |= F_CAUSAL;
  if (order) f |= F_ORDER;
  if (dist) f |= F_DIST;
  if (counter) f |= F_COUNTER;
  if (drop) f |= F_DROP;
  __builtin_amdgcn_sched_barrier(0);
  if (IO.d_ctx_attacked) f |= F_GA;
  if (IO.d_ctx_calibrated) f |= F_GC;
  if (!counter && P.noise) f |= F_NOISE;
  if (!counter && drop && P.keep_after) f |= F_KEEPA;
  if (!counter && drop && P.keep_mask) f |= F_KEEPM;
  __builtin_amdgcn_sched_barrier(0);
  if (IO.d_attack_mask) f |= F_DM;
  if (IO.d_penalty_part) f |= F_DPEN;
  if (P.combine_option == ACATTN_COMBINE_GATE && IO.dgate_logits) f |= F_DG;
  if (P.affine && order && dist) f |= F_PRE;
  K.flags = f;
  __builtin_amdgcn_sched_barrier(0);
  K.gate_is_prob = P.gate_is_prob;
  K.inv_sqrt = 1.0f / sqrtf((float)DH);
  K.sc = dist ? P.scalar[0] : 0.f;
  K.s2 = K.sc * K.sc;
  K.hs2 = 0.5f * K.s2;
  K.p_drop = P.p_drop;
  K.keep_scale = drop ? 1.0f / (1.0f - P.p_drop) : 1.0f;
  K.rate = P.anneal_rate;
  K.rkey = rng_key(P.seed + (P.seed_device ? *P.seed_device : 0ull));
  // The scalar register file is the tight one in these kernels (two argument structs of pointers, the loop state): wave-
  // uniform values that only feed vector arithmetic live in vector registers.
  VREG(K.inv_sqrt);
  VREG(K.sc);
  VREG(K.s2);
  VREG(K.hs2);
  VREG(K.keep_scale);
  VREG(K.rate);
  VREG(K.rkey.a);
  VREG(K.rkey.b);
  return K;
}

// the forward's mask table and tile rule (acattn_long_common.h)
__device__ __forceinline__ void key_mask_table(const acattn_problem& P, const Opt& K, size_t rowbase, int lane, float* s_km,
                                               int& first_valid, int& last_valid) {
  long_key_mask_table(P, K.structured(), K.dense_ll(), K.L, K.LP, rowbase, lane, s_km, first_valid, last_valid);
}
__device__ __forceinline__ int tiles_of_block(const Opt& K, int qb, int first_valid, int last_valid) {
  return long_tiles_of_block(K.structured(), K.causal(), K.nT, qb, first_valid, last_valid);
}

// Everything a lane knows about ITS query row (row 16 qb + c) that does not depend on the key tile.
template <int DH>
struct Row {
  static constexpr int KS = DH / 4;
  float qf[KS], qaf[KS];   // B operands of S^T = K.Q^T and Sa^T = Ka.Qa^T
  float gaf[KS], gcf[KS];  // d_ctx_attacked / d_ctx_calibrated of the row (B operands of dA^T = V.dctx^T)
  float ao2, ad;           // query halves of the order (times -log2 e) / distance affines
  float lx, ly, lu, lv, lw, lf;  // the forward's log-normalisers
  float cx, cy, cu, cv, cw, cf;  // their corrections for a fully masked row (row kernel: renormalise), 0 elsewhere; kept apart
                                 // because next to the -10000 such a normaliser carries, a correction of 1e-4 is below one ulp
  float dpen2;             // 2 * d_penalty_part of the row's query block
  int i;
  bool row_ok;
  uint32_t rng_row;
  const float *mask_row, *noise_row, *gate_row, *dm_row;
  const uint8_t *keepa_row, *keepm_row;
};

// Per-lane base pointers of one (sequence, head), formed ONCE per wave and held in vector registers: load_row runs inside
// the key kernel's loop over query blocks, and a dozen argument pointers kept in scalar registers across it do not fit.
struct Bases {
  const float *q, *qa, *ga, *gc, *wo, *wd, *stats, *mask, *noise, *gate, *dm, *dpen;
  const uint8_t *keepa, *keepm;
  const float *k, *ka, *v, *w_order, *w_dist;    // K, Ka, V of the (sequence, head); the affine weights
  float *dq, *dqa, *dk, *dka, *dv, *dg, *wpo, *wpd, *wps, *ws;  // outputs of the (sequence, head), partial rows, workspace rows
  float b_o, b_d;
};
template <int DH>
__device__ __forceinline__ Bases make_bases(const acattn_problem& P, const acattn_bwd_io& IO, const Opt& K, float* ws, size_t rowbase,
                                            size_t bh, int hoff, int g) {
  constexpr int KS = DH / 4;
  const size_t seq = rowbase * K.H + hoff + KS * g, ll = bh * K.L * (size_t)K.L, sh = rowbase * K.H + hoff;
  const int stride_w = IO.part_stride ? IO.part_stride : 2 * DH, stride_s = IO.part_stride ? IO.part_stride : 4;
  Bases A;
  A.k = P.k + sh;
  VFENCE(A.k);
  A.ka = P.ka + sh;
  VFENCE(A.ka);
  A.v = P.v + sh;
  VFENCE(A.v);
  A.w_order = P.w_order;
  VFENCE(A.w_order);
  A.w_dist = P.w_dist;
  VFENCE(A.w_dist);
  A.dq = IO.dq + sh;
  VFENCE(A.dq);
  A.dqa = IO.dqa + sh;
  VFENCE(A.dqa);
  A.dk = IO.dk + sh;
  VFENCE(A.dk);
  A.dka = IO.dka + sh;
  VFENCE(A.dka);
  A.dv = IO.dv + sh;
  VFENCE(A.dv);
  A.dg = IO.dgate_logits + ll;  // (a tensor the launch does not have is never dereferenced: every use is behind its flag)
  VFENCE(A.dg);
  A.wpo = IO.dw_order_part + bh * stride_w;
  VFENCE(A.wpo);
  A.wpd = IO.dw_dist_part + bh * stride_w;
  VFENCE(A.wpd);
  A.wps = IO.dsmall_part + bh * stride_s;
  VFENCE(A.wps);
  A.ws = ws + bh * K.L * NSC;
  VFENCE(A.ws);
  A.q = P.q + seq;
  VFENCE(A.q);
  A.qa = P.qa + seq;
  VFENCE(A.qa);
  A.ga = IO.d_ctx_attacked + seq;
  VFENCE(A.ga);
  A.gc = IO.d_ctx_calibrated + seq;
  VFENCE(A.gc);
  A.wo = P.w_order + KS * g;
  VFENCE(A.wo);
  A.wd = P.w_dist + KS * g;
  VFENCE(A.wd);
  A.stats = IO.row_stats + bh * K.L * ACATTN_NSTAT;
  VFENCE(A.stats);
  A.mask = P.mask + rowbase * K.L;
  VFENCE(A.mask);
  A.noise = P.noise + ll;
  VFENCE(A.noise);
  A.keepa = P.keep_after + ll;
  VFENCE(A.keepa);
  A.keepm = P.keep_mask + ll;
  VFENCE(A.keepm);
  A.gate = P.gate_logits + rowbase * K.L;
  VFENCE(A.gate);
  A.dm = IO.d_attack_mask + ll;
  VFENCE(A.dm);
  A.dpen = IO.d_penalty_part + bh * K.nT;
  VFENCE(A.dpen);
  A.b_o = 0.f;
  if (K.use_order()) A.b_o = P.b_order[0];
  VFENCE(A.b_o);
  A.b_d = 0.f;
  if (K.use_dist()) A.b_d = P.b_dist[0];
  VFENCE(A.b_d);
  return A;
}

// WITH_G = false (the key kernel at its register limit): the cotangent fragments are left out; load_row_cotangents then
// puts them where the query fragments were once the score products are done.
template <int DH, bool WITH_G = true>
__device__ __forceinline__ void load_row(const Bases& A, const Opt& K, size_t bh, int qb, int c, Row<DH>& R) {
  constexpr int KS = DH / 4;
  const int L = K.L, H = K.H;
  R.i = 16 * qb + c;
  R.row_ok = R.i < L;
  const int ic = R.row_ok ? R.i : 0;
  const size_t off = (size_t)ic * H;
  float ao = 0.f, adv = 0.f;
#pragma unroll
  for (int s4 = 0; s4 < KS / 4; ++s4) {
    const f4 tq = *(const f4*)(A.q + off + 4 * s4), ta = *(const f4*)(A.qa + off + 4 * s4);
    f4 ga = {0.f, 0.f, 0.f, 0.f}, gc = ga, a = ga, d = ga;
    if (WITH_G && K.has(F_GA)) ga = *(const f4*)(A.ga + off + 4 * s4);
    if (WITH_G && K.has(F_GC)) gc = *(const f4*)(A.gc + off + 4 * s4);
    if (K.use_order()) a = *(const f4*)(A.wo + 4 * s4);
    if (K.use_dist()) d = *(const f4*)(A.wd + 4 * s4);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      R.qf[4 * s4 + e] = R.row_ok ? tq[e] : 0.f;
      R.qaf[4 * s4 + e] = R.row_ok ? ta[e] : 0.f;
      if (WITH_G) {
        R.gaf[4 * s4 + e] = R.row_ok ? ga[e] : 0.f;
        R.gcf[4 * s4 + e] = R.row_ok ? gc[e] : 0.f;
      }
      ao += R.qf[4 * s4 + e] * a[e];
      adv += R.qf[4 * s4 + e] * d[e];
    }
  }
  R.ao2 = -kLog2e * (quad_sum(ao) + A.b_o);
  R.ad = quad_sum(adv) + A.b_d;
  const float* sp = A.stats + (size_t)ic * ACATTN_NSTAT;
  const f4 s0 = *(const f4*)sp, s1 = *(const f4*)(sp + 4);
  R.lx = s0[0];
  R.ly = s0[1];
  R.lu = s0[2];
  R.lv = s0[3];
  R.lw = s1[0];
  R.lf = s1[1];
  R.cx = R.cy = R.cu = R.cv = R.cw = R.cf = 0.f;
  R.rng_row = (uint32_t)(bh * L + R.i);
  const size_t prow = (size_t)ic * L;
  // (rows of tensors the launch does not have are never dereferenced: every use is behind the option's flag)
  R.mask_row = A.mask + prow;
  R.noise_row = A.noise + prow;
  R.keepa_row = A.keepa + prow;
  R.keepm_row = A.keepm + prow;
  R.gate_row = A.gate + prow;
  R.dm_row = A.dm + prow;
  R.dpen2 = 0.f;
  if (K.has(F_DPEN)) R.dpen2 = 2.0f * A.dpen[qb];
}

template <int DH>
__device__ __forceinline__ void load_row_cotangents(const Bases& A, const Opt& K, Row<DH>& R) {
  constexpr int KS = DH / 4;
  const size_t off = (size_t)(R.row_ok ? R.i : 0) * K.H;
#pragma unroll
  for (int s4 = 0; s4 < KS / 4; ++s4) {
    f4 ga = {0.f, 0.f, 0.f, 0.f}, gc = ga;
    if (K.has(F_GA)) ga = *(const f4*)(A.ga + off + 4 * s4);
    if (K.has(F_GC)) gc = *(const f4*)(A.gc + off + 4 * s4);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      R.qf[4 * s4 + e] = R.row_ok ? ga[e] : 0.f;
      R.qaf[4 * s4 + e] = R.row_ok ? gc[e] : 0.f;
    }
  }
}

// One (query block, key tile) pair: every probability tensor of the layer in the D layout of S^T = K.Q^T (lane (c, g):
// query row c, keys 16 t + 4 g + r), and what the backward needs next to them.
struct Tile {
  f4 Pt, Mt;        // softmax(x), softmax(y) before dropout
  f4 P, M;          // after dropout (M is the layer's attack mask)
  f4 Ap, Ac, Aw;    // perturbed, calibrated, combined attention
  f4 pi, kap;       // d P(combine) = pi e, d A_c = kappa e  (gate: g, 1 - g; fixed: A_f, A_f / 2)
  f4 ex1, nz;       // exp(1 - M), noise
  f4 dAp, dAw;      // cotangents of A_p and A_w (dctx . V^T)
  f4 dMout;         // cotangent of M from outside: dense d_attack_mask + the penalty's 2 d_pen (M - 1)
  f4 pr, val, df;   // spatial calibrator: sigmoid(o), its log argument, distance residual
  uint32_t ka, km;  // dropout keep bits
};

// Row fragments X[16 t + c][KS g ..] of a key tile (A operands of X . frag^T), zeros for keys >= L.
template <int DH>
__device__ __forceinline__ void row_frag(const float* X, int H, int row0, int L, int c, int g, f4 (&out)[DH / 16]) {
  const bool ok = row0 + c < L;
  const float* p = X + (size_t)(ok ? row0 + c : 0) * H + (DH / 4) * g;
#pragma unroll
  for (int s4 = 0; s4 < DH / 16; ++s4) {
    const f4 v = *(const f4*)(p + 4 * s4);
    out[s4] = ok ? v : f4{0.f, 0.f, 0.f, 0.f};
  }
}
// Column fragments X[row0 + 4 g + r][16 dt + c] (A operands of X^T . tile^T), zeros for rows >= L.
template <int DH>
__device__ __forceinline__ void col_frag(const float* X, int H, int row0, int L, int c, int g, float (&out)[4][DH / 16]) {
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = row0 + 4 * g + r;
    const float* p = X + (size_t)min(row, L - 1) * H + c;
#pragma unroll
    for (int dt = 0; dt < DH / 16; ++dt) {
      const float v = p[16 * dt];
      out[r][dt] = row < L ? v : 0.f;
    }
  }
}
// key halves of the two affines for the lane's 4 keys of a tile: the producer's planes, or from the K row fragment
template <int DH>
__device__ __forceinline__ void key_affine(const Opt& K, const float* planes, const f4 (&k4)[DH / 16], const float (&wko)[DH / 4],
                                           const float (&wkd)[DH / 4], int t, int g, f4& co4, f4& cd4) {
  co4 = cd4 = f4{0.f, 0.f, 0.f, 0.f};
  if (K.has(F_PRE)) {
    co4 = *(const f4*)(planes + 2 * K.LP + 16 * t + 4 * g);
    cd4 = *(const f4*)(planes + 3 * K.LP + 16 * t + 4 * g);
  } else if (K.use_order() || K.use_dist()) {
    float co = 0.f, cd = 0.f;
#pragma unroll
    for (int s4 = 0; s4 < DH / 16; ++s4)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        co += k4[s4][e] * wko[4 * s4 + e];
        cd += k4[s4][e] * wkd[4 * s4 + e];
      }
    co = quad_sum(co);
    cd = quad_sum(cd);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int src = 4 * (4 * g + r);
      co4[r] = __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(src, __builtin_bit_cast(int, co)));
      cd4[r] = __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(src, __builtin_bit_cast(int, cd)));
    }
  }
}
template <int DH>
__device__ __forceinline__ void key_weights(const Bases& P, const Opt& K, int g, float (&wko)[DH / 4], float (&wkd)[DH / 4]) {
#pragma unroll
  for (int s = 0; s < DH / 4; ++s) {
    wko[s] = K.use_order() ? P.w_order[DH + (DH / 4) * g + s] * -kLog2e : 0.f;
    wkd[s] = K.use_dist() ? P.w_dist[DH + (DH / 4) * g + s] : 0.f;
  }
}

// Two products of a key tile's row fragments with two query-row fragments: (S, Sa) from (K, Ka) x (q, qa), or
// (dA_p, dA_w) from (V, V) x (d ctx_attacked, d ctx_calibrated).
template <int DH>
__device__ __forceinline__ void products(const f4 (&a4)[DH / 16], const f4 (&b4)[DH / 16], const float (&x)[DH / 4],
                                         const float (&y)[DH / 4], f4& ax, f4& ay) {
  ax = ay = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int s4 = 0; s4 < DH / 16; ++s4)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      ax = mfma16(a4[s4][e], x[4 * s4 + e], ax);
      ay = mfma16(b4[s4][e], y[4 * s4 + e], ay);
    }
}

// The forward's elementwise chain behind the four products (acattn_long_fwd.inc, same expressions).
template <int DH>
__device__ __forceinline__ void tile_elementwise(const Row<DH>& R, const Opt& K, const f4 aS, const f4 aM, const f4 aP, const f4 aW,
                                                 const f4 co4, const f4 cd4, const float* s_km, const int t, const int g, Tile& T) {
  T.dAp = aP;
  T.dAw = aW;
  const int L = K.L, i = R.i, j0 = 16 * t + 4 * g;
  const f4 km4 = *(const f4*)(s_km + j0);
  f4 md = {0.f, 0.f, 0.f, 0.f}, mk;
  if (K.dense_ll()) md = load_seg(R.mask_row, j0, L, R.row_ok);
  T.nz = f4{0.f, 0.f, 0.f, 0.f};
  T.ka = T.km = 0xFu;
  if (K.counter()) {
    const RngGroup rg = rng_group(K.rkey, R.rng_row, (uint32_t)(4 * t + g), K.p_drop);
    T.nz = rg.n;
    if (K.has_drop()) {
      T.ka = rg.keep_after;
      T.km = rg.keep_mask;
    }
  } else {
    if (K.has(F_NOISE)) T.nz = load_seg(R.noise_row, j0, L, R.row_ok);
    if (K.has(F_KEEPA)) T.ka = load_keep(R.keepa_row, j0, L, R.row_ok);
    if (K.has(F_KEEPM)) T.km = load_keep(R.keepm_row, j0, L, R.row_ok);
  }
  f4 gt = {0.f, 0.f, 0.f, 0.f};
  if (K.combine == ACATTN_COMBINE_GATE) gt = gate_value(load_seg(R.gate_row, j0, L, R.row_ok), K.gate_is_prob);
  f4 dmx = {0.f, 0.f, 0.f, 0.f};
  if (K.has(F_DM)) dmx = load_seg(R.dm_row, j0, L, R.row_ok);
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int j = j0 + r;
    float m = km4[r];
    if (K.causal() && j > i) m = fminf(m, ACATTN_MASK_FILL);
    if (K.dense_ll() && j < L) m = md[r];
    mk[r] = m;
    float s = aS[r];
    T.pr[r] = 0.f;
    T.val[r] = 1.0f;
    T.df[r] = 0.f;
    if (K.use_order()) {  // layers.py:715-719
      const float pr = fast_rcp(1.0f + ex2(R.ao2 + co4[r]));
      const float val = (j > i) ? pr : 1.0f - pr;
      T.pr[r] = pr;
      T.val[r] = val;
      s += fast_log(val + ACATTN_LOG_EPS);
    }
    if (K.use_dist()) {  // layers.py:721-727
      const float df = fast_log((float)(abs(i - j) + 1)) - (R.ad + cd4[r]);
      T.df[r] = df;
      s -= (df * df) * K.hs2;
    }
    const float x = s * K.inv_sqrt + m, y = aM[r] * K.inv_sqrt + m;
    // rows past L: every probability exactly 0 (keys past L: exp(-inf) = 0)
    T.Pt[r] = R.row_ok ? fast_exp((x - R.lx) - R.cx) : 0.f;
    T.Mt[r] = R.row_ok ? fast_exp((y - R.ly) - R.cy) : 0.f;
    T.P[r] = ((T.ka >> r) & 1u) ? T.Pt[r] * K.keep_scale : 0.f;
    T.M[r] = ((T.km >> r) & 1u) ? T.Mt[r] * K.keep_scale : 0.f;
    const float p = T.P[r], mm = T.M[r];
    T.ex1[r] = fast_exp(1.0f - mm);
    T.Ap[r] = R.row_ok ? fast_exp((((p * mm + T.nz[r] * (1.0f - mm)) + m) - R.lu) - R.cu) : 0.f;  // layers.py:918-919
    T.Ac[r] = R.row_ok ? fast_exp(((p * T.ex1[r] + m) - R.lv) - R.cv) : 0.f;                      // layers.py:920-921
    float ag;
    if (K.combine == ACATTN_COMBINE_FIXED) {  // layers.py:885: no mask inside
      ag = (j < L && R.row_ok) ? fast_exp(((p + 0.5f * T.Ac[r]) - R.lf) - R.cf) : 0.f;
      T.pi[r] = ag;
      T.kap[r] = 0.5f * ag;
    } else {
      const float gg = K.combine == ACATTN_COMBINE_GATE ? gt[r] : K.rate;
      ag = gg * p + (1.0f - gg) * T.Ac[r];
      T.pi[r] = gg;
      T.kap[r] = 1.0f - gg;
    }
    T.Aw[r] = R.row_ok ? fast_exp(((ag + m) - R.lw) - R.cw) : 0.f;  // layers.py:925
    T.dMout[r] = dmx[r] + (mm - 1.0f) * R.dpen2;
  }
}

template <int DH>
__device__ __forceinline__ void tile_forward(const Row<DH>& R, const Opt& K, const f4 (&k4)[DH / 16], const f4 (&ka4)[DH / 16],
                                             const f4 (&v4)[DH / 16], const f4 co4, const f4 cd4, const float* s_km, const int t,
                                             const int g, Tile& T) {
  f4 aS, aM, aP, aW;
  products<DH>(k4, ka4, R.qf, R.qaf, aS, aM);
  products<DH>(v4, v4, R.gaf, R.gcf, aP, aW);
  tile_elementwise<DH>(R, K, aS, aM, aP, aW, co4, cd4, s_km, t, g, T);
}

// Backward part once the row scalars are known: dS, dSa (raw scores), the gate-logit gradient, d o and d d of the two
// spatial affines, and the scalar's partial.
__device__ __forceinline__ void tile_backward(const Tile& T, const Opt& K, const float da, const float dc, const float rf,
                                              const float r1, const float sP, const float sM, const int i, const int j0, f4& dS,
                                              f4& dSa, f4& dgl, f4& d_o, f4& d_d, float& dsc) {
  const float phi_rf = K.combine == ACATTN_COMBINE_FIXED ? rf : 0.f;
  const f4 du = T.Ap * (T.dAp - da);
  const f4 dw = T.Aw * (T.dAw - dc);  // = d A_g
  const f4 e = dw - phi_rf;
  dgl = dw * (T.P - T.Ac) * (T.pi * (1.0f - T.pi));  // (read for combine GATE only: pi = g)
  const f4 dv = T.Ac * (T.kap * e - r1);
  f4 dP = T.pi * e + dv * T.ex1 + du * T.M;
  f4 dM = T.dMout - dv * (T.P * T.ex1) + du * (T.P - T.nz);
#pragma unroll
  for (int r = 0; r < 4; ++r) {  // through the dropouts: kept entries are scaled, dropped ones carry nothing
    dP[r] = ((T.ka >> r) & 1u) ? dP[r] * K.keep_scale : 0.f;
    dM[r] = ((T.km >> r) & 1u) ? dM[r] * K.keep_scale : 0.f;
  }
  dS = (T.Pt * (dP - sP)) * K.inv_sqrt;
  dSa = (T.Mt * (dM - sM)) * K.inv_sqrt;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const float sgn = (j0 + r > i) ? 1.0f : -1.0f;  // d val / d sigmoid: +1 for keys after the query, -1 otherwise
    d_o[r] = K.use_order() ? dS[r] * (sgn * T.pr[r] * (1.0f - T.pr[r])) * fast_rcp(T.val[r] + ACATTN_LOG_EPS) : 0.f;
  }
  d_d = dS * (T.df * K.s2);
  dsc = hsum(dS * (T.df * T.df)) * (-K.sc);
}

// ---------------------------------------------------------------------------------------------------------------------
// row kernel
// ---------------------------------------------------------------------------------------------------------------------
template <int DH>
__global__ void __launch_bounds__(64, 1) acattn_long_bwd_row_kernel(const acattn_problem P, const acattn_bwd_io IO, float* __restrict__ ws) {
  constexpr int KS = DH / 4, DT = DH / 16;
  extern __shared__ __attribute__((aligned(16))) float s_km[];  // [16 nT]
  Opt K = make_opt(P, IO, DH);
  const int L = K.L, H = K.H, nh = P.n_heads, nT = K.nT;
  const int n_items = P.B * nh;
  const int rank = blockIdx.x / n_items, item = blockIdx.x - rank * n_items;
  const int qb = K.causal() ? nT - 1 - rank : rank;  // heaviest query blocks first
  int b, h;
  decode_block(item, P.B, nh, b, h);
  const int lane = threadIdx.x, c = lane & 15, g = lane >> 4;
  const size_t rowbase = (size_t)b * L, bh = (size_t)b * nh + h;
  const int hoff = h * DH;

  int first_valid, last_valid;
  key_mask_table(P, K, rowbase, lane, s_km, first_valid, last_valid);
  const int nt = tiles_of_block(K, qb, first_valid, last_valid);
  const Bases A = make_bases<DH>(P, IO, K, ws, rowbase, bh, hoff, g);
  Row<DH> R;
  load_row<DH>(A, K, bh, qb, c, R);
  const size_t prow = (size_t)(R.row_ok ? R.i : 0) * L;
  const float* planes = K.has(F_PRE) ? P.affine + bh * 4 * K.LP : nullptr;
  VREG(planes);
  float wko[KS], wkd[KS];
  key_weights<DH>(A, K, g, wko, wkd);

  auto build = [&](int t, Tile& T) {
    f4 k4[DT], ka4[DT], v4[DT], co4, cd4;
    row_frag<DH>(A.k, H, 16 * t, L, c, g, k4);
    row_frag<DH>(A.ka, H, 16 * t, L, c, g, ka4);
    row_frag<DH>(A.v, H, 16 * t, L, c, g, v4);
    key_affine<DH>(K, planes, k4, wko, wkd, t, g, co4, cd4);
    tile_forward<DH>(R, K, k4, ka4, v4, co4, cd4, s_km, t, g, T);
  };

  const bool fixed = K.combine == ACATTN_COMBINE_FIXED;
  // ---- fully masked rows (left padding).  Their normalisers carry the -10000 of the mask fill: the forward's fp32
  // "maximum + log(sum)" is rounded to 2^-10 there, every rebuilt probability row of such a row would sum to 1 +- 5e-4, and
  // the row's whole gradient contribution would be scaled by that -- harmless for a tensor, not for the calibrator's bias
  // gradients, which are sums over rows that cancel to 1e-2 of their terms.  A block that holds such a row re-sums its
  // probability rows level by level (each level needs the corrected one before it) and keeps log(sum) as a correction next
  // to the normaliser; the corrections travel to the key kernel in the workspace row.  Other blocks: two sweeps as before.
  if (__ballot(R.row_ok && R.lx < 0.5f * ACATTN_MASK_FILL) != 0ull) {
    const int levels = fixed ? 4 : 3;
#pragma unroll 1
    for (int lev = 0; lev < levels; ++lev) {
      const bool inner = fixed && lev == 2;  // the un-masked soft-max of combine FIXED sits between levels 2 and 3
      float s0 = 0.f, s1 = 0.f;
#pragma unroll 1
      for (int t = 0; t < nt; ++t) {
        K.refresh();
        Tile T;
        build(t, T);
        s0 += hsum(lev == 0 ? T.Pt : (lev == 1 ? T.Ap : (inner ? T.pi : T.Aw)));
        s1 += hsum(lev == 0 ? T.Mt : T.Ac);
      }
      s0 = quad_sum(s0);
      s1 = quad_sum(s1);
      const float d0 = (R.row_ok && s0 > 0.f) ? fast_log(s0) : 0.f, d1 = (R.row_ok && s1 > 0.f) ? fast_log(s1) : 0.f;
      if (lev == 0) {
        R.cx += d0;
        R.cy += d1;
      } else if (lev == 1) {
        R.cu += d0;
        R.cv += d1;
      } else if (inner) {
        R.cf += d0;
      } else {
        R.cw += d0;
      }
    }
  }

  // ---- sweep 1: the seventeen row sums ------------------------------------------------------------------------------------
  float s_da = 0.f, s_dc = 0.f, s_rfa = 0.f, s_rfb = 0.f, s_r1a = 0.f, s_r1b = 0.f, s_r1f = 0.f;
  float cP0 = 0.f, cPa = 0.f, cPc = 0.f, cPf = 0.f, cPr = 0.f, cM0 = 0.f, cMa = 0.f, cMc = 0.f, cMf = 0.f, cMr = 0.f;
#pragma unroll 1
  for (int t = 0; t < nt; ++t) {
    K.refresh();
    Tile T;
    build(t, T);
    const f4 apd = T.Ap * T.dAp, alpha = T.Aw * T.dAw, beta = T.Aw;
    const f4 gam = T.Ac * T.kap, PE = T.P * T.ex1, pn = T.P - T.nz;
    s_da += hsum(apd);
    s_dc += hsum(alpha);
    s_r1a += hsum(gam * alpha);
    s_r1b += hsum(gam * beta);
    cP0 += hsum(T.P * (apd * T.M + T.pi * alpha + T.ex1 * (gam * alpha)));
    cPa += hsum(T.P * (T.Ap * T.M));
    cPc += hsum(T.P * (T.pi * beta + T.ex1 * (gam * beta)));
    cPr += hsum(PE * T.Ac);
    cM0 += hsum(T.M * (apd * pn - PE * (gam * alpha) + T.dMout));
    cMa += hsum(T.M * (T.Ap * pn));
    cMc += hsum(T.M * (PE * (gam * beta)));
    cMr += hsum(T.M * (PE * T.Ac));
    if (fixed) {  // (pi = A_f, phi = 1)
      s_rfa += hsum(T.pi * alpha);
      s_rfb += hsum(T.pi * beta);
      s_r1f += hsum(gam);
      cPf += hsum(T.P * (T.pi + T.ex1 * gam));
      cMf += hsum(T.M * (PE * gam));
    }
  }
  const float da = quad_sum(s_da), dc = quad_sum(s_dc);
  const float rf = quad_sum(s_rfa) - dc * quad_sum(s_rfb);
  const float r1 = quad_sum(s_r1a) - dc * quad_sum(s_r1b) - rf * quad_sum(s_r1f);
  const float sP = quad_sum(cP0) - da * quad_sum(cPa) - dc * quad_sum(cPc) - rf * quad_sum(cPf) - r1 * quad_sum(cPr);
  const float sM = quad_sum(cM0) - da * quad_sum(cMa) + dc * quad_sum(cMc) + rf * quad_sum(cMf) + r1 * quad_sum(cMr);
  if (R.row_ok && g == 0) {
    float* wrow = A.ws + (size_t)R.i * NSC;
    *(f4*)wrow = f4{da, dc, r1, sP};
    *(f4*)(wrow + 4) = f4{sM, rf, 0.f, 0.f};
    *(f4*)(wrow + 8) = f4{R.cx, R.cy, R.cu, R.cv};
    *(f4*)(wrow + 12) = f4{R.cw, R.cf, 0.f, 0.f};
  }

  // ---- sweep 2: dS, dSa -> dq, dqa; gate partials; query halves of the parameter gradients -------------------------------
  f4 oq[DT], oqa[DT];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) {
    oq[dt] = f4{0.f, 0.f, 0.f, 0.f};
    oqa[dt] = oq[dt];
  }
  float* const dg_row = A.dg + prow;  // (used behind F_DG only)
  float da_o = 0.f, da_d = 0.f, dsc_acc = 0.f;
#pragma unroll 1
  for (int t = 0; t < nt; ++t) {
    K.refresh();
    Tile T;
    build(t, T);
    const int j0 = 16 * t + 4 * g;
    f4 dS, dSa, dgl, d_o, d_d;
    float dsc;
    tile_backward(T, K, da, dc, rf, r1, sP, sM, R.i, j0, dS, dSa, dgl, d_o, d_d, dsc);
    if (K.has(F_DG)) store_seg(dg_row, j0, L, R.row_ok, dgl);
    da_o += hsum(d_o);
    da_d += hsum(d_d);
    dsc_acc += dsc;
    float kc[4][DT], kac[4][DT];
    __builtin_amdgcn_sched_barrier(0);  // (the column fragments are not requested while the tile's working set is live)
    col_frag<DH>(A.k, H, 16 * t, L, c, g, kc);
    col_frag<DH>(A.ka, H, 16 * t, L, c, g, kac);
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) {
        oq[dt] = mfma16(kc[r][dt], dS[r], oq[dt]);
        oqa[dt] = mfma16(kac[r][dt], dSa[r], oqa[dt]);
      }
  }
  if (K.has(F_DG))
    for (int t = nt; t < nT; ++t) store_seg(dg_row, 16 * t + 4 * g, L, R.row_ok, f4{0.f, 0.f, 0.f, 0.f});
  da_o = quad_sum(da_o);
  da_d = quad_sum(da_d);
  dsc_acc = quad_sum(dsc_acc);
  if (R.row_ok) {
    const size_t off = (size_t)R.i * H + 4 * g;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) {
      // rank-1 terms of dq: query halves of the affine weights in the lane's output-column order
      f4 o = oq[dt];
      if (K.use_order()) o += da_o * *(const f4*)(A.w_order + 16 * dt + 4 * g);
      if (K.use_dist()) o += da_d * *(const f4*)(A.w_dist + 16 * dt + 4 * g);
      *(f4*)(A.dq + off + 16 * dt) = o;
      *(f4*)(A.dqa + off + 16 * dt) = oqa[dt];
    }
  }
  // query halves of dw_order / dw_dist, db_order, db_dist, d scalar: summed over the block's 16 rows, then added to the
  // (sequence, head) partial row (zeroed by the launcher)
  const float ro = R.row_ok ? 1.0f : 0.0f;
#pragma unroll
  for (int s = 0; s < KS; ++s) {
    const float vo = row16_sum(da_o * R.qf[s] * ro), vd = row16_sum(da_d * R.qf[s] * ro);
    if (c == 0) {
      atomicAdd(A.wpo + KS * g + s, vo);
      atomicAdd(A.wpd + KS * g + s, vd);
    }
  }
  const float so = row16_sum(da_o * ro), sd = row16_sum(da_d * ro), ss = row16_sum(dsc_acc * ro);
  if (lane == 0) {
    atomicAdd(A.wps + 0, so);
    atomicAdd(A.wps + 1, sd);
    atomicAdd(A.wps + 2, ss);
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// key kernel
// ---------------------------------------------------------------------------------------------------------------------
template <int DH>
__global__ void __launch_bounds__(64, 1) acattn_long_bwd_key_kernel(const acattn_problem P, const acattn_bwd_io IO, const float* __restrict__ ws) {
  constexpr int KS = DH / 4, DT = DH / 16;
  constexpr int TS = 20;  // row stride of a transposed 16 x 16 tile in LDS (16-byte aligned rows, conflict-free reads)
  __shared__ __attribute__((aligned(16))) float tr[4][16 * TS + 32];
  extern __shared__ __attribute__((aligned(16))) float s_km[];  // [16 nT]
  Opt K = make_opt(P, IO, DH);
  const int L = K.L, H = K.H, nh = P.n_heads, nT = K.nT;
  const int n_items = P.B * nh;
  const int t = blockIdx.x / n_items, item = blockIdx.x - t * n_items;  // causal: key tile 0 is seen by every block, heaviest first
  int b, h;
  decode_block(item, P.B, nh, b, h);
  const int lane = threadIdx.x, c = lane & 15, g = lane >> 4;
  const size_t rowbase = (size_t)b * L, bh = (size_t)b * nh + h;
  const int hoff = h * DH;

  int first_valid, last_valid;
  key_mask_table(P, K, rowbase, lane, s_km, first_valid, last_valid);
  // this wave's 16 keys: row fragments of K, Ka, V (fixed), key halves of the affines
  const Bases A = make_bases<DH>(P, IO, K, const_cast<float*>(ws), rowbase, bh, hoff, g);
  f4 k4[DT], ka4[DT], v4[DT], co4, cd4;
  row_frag<DH>(A.k, H, 16 * t, L, c, g, k4);
  row_frag<DH>(A.ka, H, 16 * t, L, c, g, ka4);
  row_frag<DH>(A.v, H, 16 * t, L, c, g, v4);
  {
    const float* planes = K.has(F_PRE) ? P.affine + bh * 4 * K.LP : nullptr;
    float wko[KS], wkd[KS];
    key_weights<DH>(A, K, g, wko, wkd);
    key_affine<DH>(K, planes, k4, wko, wkd, t, g, co4, cd4);
  }
  f4 aK[DT], aKa[DT], aV[DT];  // dK^T, dKa^T, dV^T: lane (c, g) holds key 16 t + c, columns 16 dt + 4 g ..
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) {
    aK[dt] = f4{0.f, 0.f, 0.f, 0.f};
    aKa[dt] = aK[dt];
    aV[dt] = aK[dt];
  }
  f4 dco = {0.f, 0.f, 0.f, 0.f}, dcd = dco;  // d (key half of the affines) of keys 16 t + 4 g + r, summed over queries at the end

#pragma unroll 1
  for (int qb = 0; qb < nT; ++qb) {
    K.refresh();
    if (t >= tiles_of_block(K, qb, first_valid, last_valid)) continue;  // the row kernel skipped this pair too: no mass
    const int i0 = 16 * qb;
    Row<DH> R;
    load_row<DH, false>(A, K, bh, qb, c, R);
    f4 aS, aM, aP, aW;
    products<DH>(k4, ka4, R.qf, R.qaf, aS, aM);
    __builtin_amdgcn_sched_barrier(0);
    load_row_cotangents<DH>(A, K, R);  // (into the registers of the query fragments)
    products<DH>(v4, v4, R.qf, R.qaf, aP, aW);
    __builtin_amdgcn_sched_barrier(0);
    const float* wrow = A.ws + (size_t)(R.row_ok ? R.i : 0) * NSC;
    const f4 w0 = *(const f4*)wrow, w1 = *(const f4*)(wrow + 4), w2 = *(const f4*)(wrow + 8), w3 = *(const f4*)(wrow + 12);
    R.cx = w2[0];  // (fully masked rows: the row kernel's corrections of the normalisers; 0 elsewhere)
    R.cy = w2[1];
    R.cu = w2[2];
    R.cv = w2[3];
    R.cw = w3[0];
    R.cf = w3[1];
    const int j0 = 16 * t + 4 * g;
    Tile T;
    tile_elementwise<DH>(R, K, aS, aM, aP, aW, co4, cd4, s_km, t, g, T);
    f4 dS, dSa, dgl, d_o, d_d;
    float dsc;
    tile_backward(T, K, w0[0], w0[1], w1[1], w0[2], w0[3], w1[0], R.i, j0, dS, dSa, dgl, d_o, d_d, dsc);
    dco += d_o;
    dcd += d_d;
    // turn the four [query c][key 4 g + r] tiles so that the query index becomes the MFMA reduction index
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    *(f4*)(&tr[0][c * TS + 4 * g]) = dS;
    *(f4*)(&tr[1][c * TS + 4 * g]) = dSa;
    *(f4*)(&tr[2][c * TS + 4 * g]) = T.Ap;
    *(f4*)(&tr[3][c * TS + 4 * g]) = T.Aw;
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    // one operand at a time (the column fragments of all four at once do not fit next to the accumulators at head size 128)
    auto accumulate = [&](const float* X, const int which, f4 (&acc)[DT]) {
      __builtin_amdgcn_sched_barrier(0);
      float xc[4][DT];
      col_frag<DH>(X, H, i0, L, c, g, xc);
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const float bt = tr[which][(4 * g + s) * TS + c];
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) acc[dt] = mfma16(xc[s][dt], bt, acc[dt]);
      }
    };
    accumulate(A.q - KS * g, 0, aK);
    accumulate(A.qa - KS * g, 1, aKa);
    if (K.has(F_GA)) accumulate(A.ga - KS * g, 2, aV);
    if (K.has(F_GC)) accumulate(A.gc - KS * g, 3, aV);
    __builtin_amdgcn_sched_barrier(0);
  }

  // ---- results: dk (+ rank-1 key-half terms), dka, dv; key halves of the parameter gradients --------------------------------
  // d co_j, d cd_j: sum over the query lanes; then every lane needs the value of ITS output key 16 t + c
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const float so = row16_sum(dco[r]), sd = row16_sum(dcd[r]);
    if (c == 0) {
      tr[0][4 * g + r] = so;
      tr[1][4 * g + r] = sd;
    }
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  const float dco_c = tr[0][c], dcd_c = tr[1][c];
  const int key = 16 * t + c;
  if (key < L) {
    const size_t o = (size_t)key * H + 4 * g;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) {
      f4 ok = aK[dt];
      if (K.use_order()) ok += dco_c * *(const f4*)(A.w_order + DH + 16 * dt + 4 * g);
      if (K.use_dist()) ok += dcd_c * *(const f4*)(A.w_dist + DH + 16 * dt + 4 * g);
      *(f4*)(A.dk + o + 16 * dt) = ok;
      *(f4*)(A.dka + o + 16 * dt) = aKa[dt];
      *(f4*)(A.dv + o + 16 * dt) = aV[dt];
    }
  }
  // dw_order[dh:] += sum_j d co_j K_j (natural units: the key half carries -log2 e inside the sigmoid argument only)
#pragma unroll
  for (int s4 = 0; s4 < KS / 4; ++s4)
#pragma unroll
    for (int e = 0; e < 4; ++e) {  // (k4 is zero for keys >= L)
      const float vo = row16_sum(dco_c * k4[s4][e]), vd = row16_sum(dcd_c * k4[s4][e]);
      if (c == 0) {
        atomicAdd(A.wpo + DH + KS * g + 4 * s4 + e, vo);
        atomicAdd(A.wpd + DH + KS * g + 4 * s4 + e, vd);
      }
    }
}

template <int DH>
int launch_long_bwd(const acattn_problem& p, const acattn_bwd_io& io, hipStream_t stream) {
  const int nT = (p.L + 15) / 16;
  const size_t rows = (size_t)p.B * p.n_heads;
  {  // the parameter partial rows are accumulated with atomics: start from zero (acattn_launch_zero: see acattn_util.hip)
    int rc = 0;
    auto zero = [&](float* ptr, size_t n) { if (!rc) rc = acattn_launch_zero(ptr, n, stream); };
    if (io.part_stride) {
      zero(std::min(io.dw_order_part, std::min(io.dw_dist_part, io.dsmall_part)), rows * io.part_stride);
    } else {
      zero(io.dw_order_part, rows * 2 * DH);
      zero(io.dw_dist_part, rows * 2 * DH);
      zero(io.dsmall_part, rows * 4);
    }
    if (rc) return rc;
  }
  const dim3 grid(p.B * p.n_heads * nT), block(64);
  const size_t lds = (size_t)16 * nT * sizeof(float);
  float* ws = (float*)io.workspace;
  hipLaunchKernelGGL((acattn_long_bwd_row_kernel<DH>), grid, block, lds, stream, p, io, ws);
  hipLaunchKernelGGL((acattn_long_bwd_key_kernel<DH>), grid, block, lds, stream, p, io, (const float*)ws);
  return (int)hipGetLastError();
}

}  // namespace

#define ACATTN_CAT2(a, b) a##b
#define ACATTN_CAT(a, b) ACATTN_CAT2(a, b)
int ACATTN_CAT(acattn_launch_long_bwd_dh, ACATTN_LONG_DH)(const acattn_problem& p, const acattn_bwd_io& io, hipStream_t stream) {
  return launch_long_bwd<ACATTN_LONG_DH>(p, io, stream);
}
