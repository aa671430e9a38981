// Backward of the SPATIAL-ONLY calibrated attention (acattn_problem.adversarial == 0):
//     z = q k^T + e_order + e_distance     x = z / sqrt(dh) + mask     Pt = softmax(x)     P = keep . Pt / (1 - p)
//     ctx = P . V                                                   recbole/model/layers.py:695-740, 677-680
// in the row-kernel / key-kernel form of acattn_bwd_stream.hip with ONE soft-max instead of four.
//
// The spatial-only forward saves nothing but its context, so everything is rebuilt from q, k, v, the calibrator
// parameters, the mask and the dropout key:
//
//   row kernel   one wave per (sequence, head, 16-row query block):
//                sweep 1 -> the row's log-normaliser and  D = <Pt, dPt>  by an online soft-max over the key tiles
//                           (running maximum, rescaled sums), written to the workspace for the key kernel.  The
//                           normaliser travels as (maximum, log of the shifted sum): a fully masked row's maximum is
//                           near -10000, where ONE float holds the sum's logarithm to 2^-10 only;
//                sweep 2 -> dz tile by tile -> dq (MFMA, registers), the query halves of the calibrator gradients;
//   key kernel   one wave per (sequence, head, 16-key tile): sweeps the query blocks that see the tile, rebuilds the same
//                tiles from the row scalars in the workspace, turns dz and P through a 2.5 KB LDS scratch and accumulates dK, dV (MFMA),
//                plus the key halves of the calibrator gradients.
//
// Lane layout of a tile as everywhere here: lane (c, g) holds query row i0 + c and keys 16 t + 4 g + r of S^T = K.Q^T.
// The additive mask is added LITERALLY in fp32 in the natural domain, as the general forward kernel and the reference do
// (layers.py:734): a fully masked row (left padding under the causal mask) then sees its arguments quantised to 2^-10
// exactly as the forward's rows are without a special case.  Every mask mode, either spatial term,
// counter and explicit dropout.  dq, dk, dv are written once each by the wave that owns them: no float atomics, two
// launches give the same bits.  The per-(sequence, head) parameter partial rows are accumulated with atomics like the
// streaming backward's (zeroed by the launcher).
#include <stdlib.h>

#include <algorithm>

#include "acattn_common.h"

namespace {

constexpr float kLog2e = 1.44269504088896340736f;
constexpr float kLn2 = 0.69314718055994530942f;
constexpr int NSC = 4;  // floats per query row in the workspace: row maximum, log of the shifted sum, D, (spare)

// GEN = false: the training form fixed at compile time -- structured mask, counter RNG, both spatial terms (every shipped
// configuration); GEN = true: the same code with the flags read at run time (dense masks, explicit keep bits, one term).
#define SP_UO (GEN ? K.use_order : true)
#define SP_UD (GEN ? K.use_dist : true)
#define SP_CTR (GEN ? K.counter : true)
#define SP_MODE (GEN ? P.mask_mode : (int)ACATTN_MASK_STRUCTURED)

__device__ __forceinline__ float hsum(const f4 v) { return (v[0] + v[1]) + (v[2] + v[3]); }
__device__ __forceinline__ float row16_sum(float v) {  // over the 16 lanes of a DPP row (same g, all c)
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1, 0xF, 0xF, false));
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x4E, 0xF, 0xF, false));
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x141, 0xF, 0xF, false));
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x140, 0xF, 0xF, false));
  return v;
}

// A sequence's key flags under the structured mask (up to 208 keys: four 64-bit ballots); dense masks: nothing known.
struct KeyFlags {
  unsigned long long vk[4];
  int first_valid, nt_valid;
  bool any_valid;
};
template <bool GEN>
__device__ __forceinline__ KeyFlags load_key_flags(const acattn_problem& P, size_t rowbase, int L, int nT, int lane) {
  KeyFlags F;
  F.any_valid = false;
  F.first_valid = L;
  F.nt_valid = nT;
#pragma unroll
  for (int q = 0; q < 4; ++q) F.vk[q] = 0ull;
  if (SP_MODE != ACATTN_MASK_STRUCTURED) return F;
  int last_valid = -1;
#pragma unroll
  for (int q = 3; q >= 0; --q) {
    const uint8_t b = (64 * q + lane < L) ? P.key_valid[rowbase + 64 * q + lane] : (uint8_t)0;
    F.vk[q] = __ballot(b != 0);
    if (F.vk[q]) {
      F.any_valid = true;
      F.first_valid = 64 * q + __ffsll((long long)F.vk[q]) - 1;
      if (last_valid < 0) last_valid = 64 * q + 63 - __clzll((long long)F.vk[q]);
    }
  }
  F.nt_valid = F.any_valid ? (last_valid >> 4) + 1 : nT;
  return F;
}
// Key tiles a query block has to visit: tiles behind the causal diagonal or past the last real item carry exactly zero
// probability (exp(-10000 + ..) == 0 in fp32) PROVIDED every row of the block sees an allowed key; a block with a fully
// masked row, and every block of a dense mask, visits all of them.  The forward's rule (acattn_fwd_general.inc).
template <bool GEN>
__device__ __forceinline__ int tiles_of_block(const acattn_problem& P, const KeyFlags& F, int qb, int nT) {
  if (SP_MODE != ACATTN_MASK_STRUCTURED) return nT;
  const bool rows_see_a_key = P.causal ? F.first_valid <= 16 * qb : F.any_valid;
  return rows_see_a_key ? min(P.causal ? min(nT, qb + 1) : nT, F.nt_valid) : nT;
}

__device__ __forceinline__ bool block_has_cotangent(const acattn_spatial_bwd_io& IO, int b, int qb) {
  if (!IO.read_rows) return true;
  // (a position outside [0, L) matches no block: its row is treated as carrying no cotangent)
  for (int r = 0; r < IO.n_read_rows; ++r)
    if ((int)(IO.read_rows[(size_t)b * IO.n_read_rows + r] >> 4) == qb) return true;
  return false;
}
// the same for all query blocks of a sequence at once: bit qb set = the block may carry a cotangent
__device__ __forceinline__ uint32_t blocks_with_cotangent(const acattn_spatial_bwd_io& IO, int b) {
  if (!IO.read_rows) return 0xFFFFFFFFu;
  uint32_t m = 0u;
  for (int r = 0; r < IO.n_read_rows; ++r) {
    const long long pos = IO.read_rows[(size_t)b * IO.n_read_rows + r];
    if (pos >= 0 && pos < 16 * 32) m |= 1u << (int)(pos >> 4);
  }
  return m;
}

struct Consts {
  float inv_sqrt, sc, s2, keep_scale, p_drop, b_o, b_d;
  bool has_drop, counter, use_order, use_dist;
  RngKey rkey;
};
__device__ __forceinline__ Consts make_consts(const acattn_problem& P, int DH) {
  Consts K;
  K.use_order = P.w_order != nullptr;
  K.use_dist = P.w_dist != nullptr;
  K.sc = K.use_dist ? P.scalar[0] : 0.f;
  K.b_o = K.use_order ? P.b_order[0] : 0.f;
  K.b_d = K.use_dist ? P.b_dist[0] : 0.f;
  K.s2 = K.sc * K.sc;
  K.inv_sqrt = 1.0f / sqrtf((float)DH);
  K.p_drop = P.p_drop;
  K.has_drop = P.p_drop > 0.f;
  K.keep_scale = K.has_drop ? 1.0f / (1.0f - P.p_drop) : 1.0f;
  K.counter = P.rng_mode == ACATTN_RNG_COUNTER;
  K.rkey = rng_key(P.seed + (P.seed_device ? *P.seed_device : 0ull));
  return K;
}

// What a lane knows about ITS query row (row 16 qb + c) that does not depend on the key tile.
template <int DH>
struct Row {
  float qf[DH / 4];  // B operand of S^T = K.Q^T
  float gf[DH / 4];  // d_ctx of the row: B operand of dP^T = V.dctx^T
  float ao, ad;      // query halves of the two affines (bias included)
  int i, il;         // the row, and the row clamped into [0, L) for addresses
  bool row_ok;
};
template <int DH, bool GEN>
__device__ __forceinline__ void load_row(const acattn_problem& P, const acattn_spatial_bwd_io& IO, const Consts& K, size_t rowbase,
                                         int hoff, int qb, int c, int g, Row<DH>& R) {
  constexpr int KS = DH / 4;
  R.i = 16 * qb + c;
  R.row_ok = R.i < P.L;
  R.il = min(R.i, P.L - 1);
  const size_t off = (rowbase + R.il) * P.H + hoff + KS * g;
  float ao = 0.f, ad = 0.f;
#pragma unroll
  for (int s4 = 0; s4 < KS / 4; ++s4) {
    const f4 tq = *(const f4*)(P.q + off + 4 * s4), tg = *(const f4*)(IO.d_ctx + off + 4 * s4);
    f4 a = {0.f, 0.f, 0.f, 0.f}, d = a;
    if (SP_UO) a = *(const f4*)(P.w_order + KS * g + 4 * s4);
    if (SP_UD) d = *(const f4*)(P.w_dist + KS * g + 4 * s4);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      R.qf[4 * s4 + e] = R.row_ok ? tq[e] : 0.f;
      R.gf[4 * s4 + e] = R.row_ok ? tg[e] : 0.f;
      ao += R.qf[4 * s4 + e] * a[e];
      ad += R.qf[4 * s4 + e] * d[e];
    }
  }
  R.ao = quad_sum(ao) + K.b_o;
  R.ad = quad_sum(ad) + K.b_d;
}

// Key-tile operands in the two shapes the MFMAs want them:
//   row fragment  X[16 t + c][KS g ..]            (A operand of  X . frag^T : scores, dP)
//   col fragment  X[16 t + 4 g + r][16 dt + c]    (A operand of  X^T . tile^T : dq, and with query rows: dk, dv)
// Rows past L are clamped for the address; a row fragment's clamped rows only feed keys whose probability is forced to
// zero, a column fragment's are zeroed.
template <int DH>
__device__ __forceinline__ void row_frag(const float* X, size_t rowbase, int H, int hoff, int row0, int L, int c, int g,
                                         f4 (&out)[DH / 16]) {
  const float* p = X + (rowbase + min(row0 + c, L - 1)) * H + hoff + (DH / 4) * g;
#pragma unroll
  for (int s4 = 0; s4 < DH / 16; ++s4) out[s4] = *(const f4*)(p + 4 * s4);
}
template <int DH>
__device__ __forceinline__ void col_frag(const float* X, size_t rowbase, int H, int hoff, int row0, int L, int c, int g,
                                         float (&out)[4][DH / 16]) {
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = row0 + 4 * g + r;
    const float* p = X + (rowbase + min(row, L - 1)) * H + hoff + c;
#pragma unroll
    for (int dt = 0; dt < DH / 16; ++dt) out[r][dt] = row < L ? p[16 * dt] : 0.f;
  }
}
// key halves of the two affines for the lane's 4 keys of a tile, from the K row fragment (lane c holds key 16 t + c)
template <int DH, bool GEN>
__device__ __forceinline__ void key_affine(const Consts& K, const f4 (&k4)[DH / 16], const float (&wko)[DH / 4],
                                           const float (&wkd)[DH / 4], int g, f4& co4, f4& cd4) {
  co4 = f4{0.f, 0.f, 0.f, 0.f};
  cd4 = co4;
  if (!SP_UO && !SP_UD) return;
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
template <int DH, bool GEN>
__device__ __forceinline__ void key_weights(const acattn_problem& P, const Consts& K, int g, float (&wko)[DH / 4],
                                            float (&wkd)[DH / 4]) {
  constexpr int KS = DH / 4;
#pragma unroll
  for (int s4 = 0; s4 < KS / 4; ++s4) {
    f4 a = {0.f, 0.f, 0.f, 0.f}, d = a;
    if (SP_UO) a = *(const f4*)(P.w_order + DH + KS * g + 4 * s4);
    if (SP_UD) d = *(const f4*)(P.w_dist + DH + KS * g + 4 * s4);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      wko[4 * s4 + e] = a[e];
      wkd[4 * s4 + e] = d[e];
    }
  }
}

// One (query block, key tile) pair: soft-max arguments, the cotangent of the kept probabilities, and what the spatial
// calibrator's derivative needs.
struct Tile {
  f4 x;          // z / sqrt(dh) + mask                          layers.py:732-734
  f4 dPk;        // keep / (1 - p) . (dctx . V^T)                cotangent of Pt
  f4 pr, val;    // sigmoid(o) and the argument of its log       layers.py:715-719
  f4 df;         // log(|i - j| + 1) - d                         layers.py:721-727
  uint32_t inb;  // bit r: key 16 t + 4 g + r exists (< L)
  uint32_t keep; // bit r: the dropout keeps the entry
};

// Per-(sequence, head) addresses of the per-element inputs (wave-uniform), so that a tile indexes them with the row and
// the key alone.
struct Seq {
  const float* mask;     // dense modes: the sequence's mask rows; row stride `mstride` (0 for the [B,1,1,L] form)
  const uint8_t* keep;   // explicit dropout: keep_after of this (sequence, head)
  int mstride;
  uint32_t rng_row0;     // counter dropout: row id of query row 0
};
template <bool GEN>
__device__ __forceinline__ Seq make_seq(const acattn_problem& P, size_t rowbase, size_t bh) {
  Seq S;
  S.mask = nullptr;
  S.keep = nullptr;
  S.mstride = 0;
  S.rng_row0 = (uint32_t)(bh * P.L);
  if constexpr (GEN) {
    if (P.mask_mode == ACATTN_MASK_DENSE_L) S.mask = P.mask + rowbase;
    if (P.mask_mode == ACATTN_MASK_DENSE_LL) {
      S.mask = P.mask + rowbase * P.L;
      S.mstride = P.L;
    }
    if (P.rng_mode != ACATTN_RNG_COUNTER && P.p_drop > 0.f) S.keep = P.keep_after + bh * P.L * (size_t)P.L;
  }
  return S;
}

template <int DH, bool GEN>
__device__ __forceinline__ void tile_forward(const acattn_problem& P, const Consts& K, const KeyFlags& F, const Row<DH>& R,
                                             const Seq& S, const f4 (&k4)[DH / 16], const f4 (&v4)[DH / 16],
                                             const f4 co4, const f4 cd4, int t, int g, Tile& T) {
  constexpr int KS = DH / 4;
  const int L = P.L;
  f4 aS = {0.f, 0.f, 0.f, 0.f}, aW = aS;
#pragma unroll
  for (int s4 = 0; s4 < KS / 4; ++s4) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      aS = mfma16(k4[s4][e], R.qf[4 * s4 + e], aS);
      aW = mfma16(v4[s4][e], R.gf[4 * s4 + e], aW);
    }
  }
  const int j0 = 16 * t + 4 * g;
  T.inb = 0u;
  uint32_t keep = 0xFu;
  if (K.has_drop && SP_CTR) keep = rng_group(K.rkey, S.rng_row0 + (uint32_t)R.i, (uint32_t)(4 * t + g), K.p_drop).keep_after;
  // structured: the 4 keys' validity (selects, not an indexed array: the ballots stay in scalar registers)
  const unsigned long long vkt = t < 4 ? F.vk[0] : t < 8 ? F.vk[1] : t < 12 ? F.vk[2] : F.vk[3];
  const uint32_t vn = (uint32_t)(vkt >> (16 * (t & 3) + 4 * g)) & 0xFu;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int j = j0 + r;
    const bool in = j < L;
    if (in) T.inb |= 1u << r;
    float s = aS[r];
    T.pr[r] = 0.f;
    T.val[r] = 1.f;
    T.df[r] = 0.f;
    if (SP_UO) {  // layers.py:715-719
      const float pr = fast_sigmoid(R.ao + co4[r]);
      const float val = (j > R.i) ? pr : 1.0f - pr;
      T.pr[r] = pr;
      T.val[r] = val;
      s += fast_log(val + ACATTN_LOG_EPS);
    }
    if (SP_UD) {  // layers.py:721-727
      const float lt = __builtin_amdgcn_logf((float)(abs(R.i - j) + 1)) * kLn2;
      const float df = lt - (R.ad + cd4[r]);
      T.df[r] = df;
      s += -0.5f * ((df * df) * K.s2);
    }
    float m = 0.f;
    if (SP_MODE == ACATTN_MASK_STRUCTURED) {
      m = ((vn >> r) & 1u) ? 0.f : ACATTN_MASK_FILL;
      if (P.causal && j > R.i) m = ACATTN_MASK_FILL;
    } else {  // (a key past L reads the last one's value: its probability is forced to zero below)
      m = S.mask[R.il * S.mstride + min(j, L - 1)];
    }
    T.x[r] = s * K.inv_sqrt + m;
    if (GEN && S.keep) keep &= ~((S.keep[R.il * L + min(j, L - 1)] ? 0u : 1u) << r);
  }
  T.keep = keep;
#pragma unroll
  for (int r = 0; r < 4; ++r) T.dPk[r] = ((keep >> r) & 1u) ? aW[r] * K.keep_scale : 0.f;
}

// Pt from the row's normaliser (maximum mx, log of the shifted sum lz), dz from D = <Pt, dPt>, and the spatial
// calibrator's cotangents.
template <bool GEN>
__device__ __forceinline__ void tile_backward(const Tile& T, const Consts& K, float mx, float lz, float D, int i, int j0, f4& Pt, f4& dz,
                                              f4& d_o, f4& d_d, float& dsc) {
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    Pt[r] = ((T.inb >> r) & 1u) ? fast_exp((T.x[r] - mx) - lz) : 0.f;
    dz[r] = (Pt[r] * (T.dPk[r] - D)) * K.inv_sqrt;
    const float sgn = (j0 + r > i) ? 1.0f : -1.0f;  // d val / d sigmoid
    d_o[r] = SP_UO ? dz[r] * (sgn * T.pr[r] * (1.0f - T.pr[r])) * fast_rcp(T.val[r] + ACATTN_LOG_EPS) : 0.f;
  }
  d_d = dz * (T.df * K.s2);
  dsc = hsum(dz * (T.df * T.df)) * (-K.sc);
}

// ---------------------------------------------------------------------------------------------------------------------
// row kernel
// ---------------------------------------------------------------------------------------------------------------------
template <int DH, bool GEN>
__global__ void __launch_bounds__(64) acattn_spatial_bwd_row_kernel(const acattn_problem P, const acattn_spatial_bwd_io IO,
                                                                    float* __restrict__ ws) {
  constexpr int KS = DH / 4, DT = DH / 16;
  const int L = P.L, H = P.H, nh = P.n_heads;
  const int nT = (L + 15) >> 4;
  const int n_items = P.B * nh;
  const bool causal = SP_MODE == ACATTN_MASK_STRUCTURED && P.causal != 0;
  const int rank = blockIdx.x / n_items, item = blockIdx.x - rank * n_items;
  const int qb = causal ? nT - 1 - rank : rank;  // heaviest query blocks first
  int b, h;
  decode_block(item, P.B, nh, b, h);
  const int lane = threadIdx.x, c = lane & 15, g = lane >> 4;
  const size_t rowbase = (size_t)b * L, bh = (size_t)b * nh + h;
  const int hoff = h * DH;
  const int i = 16 * qb + c;
  const bool row_ok = i < L;

  // a query block none of whose rows carries a cotangent contributes nothing anywhere
  if (!block_has_cotangent(IO, b, qb)) {
    if (row_ok) {
      const size_t off = (rowbase + i) * H + hoff + 4 * g;
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) *(f4*)(IO.dq + off + 16 * dt) = f4{0.f, 0.f, 0.f, 0.f};
    }
    return;
  }

  const Consts K = make_consts(P, DH);
  const Seq S = make_seq<GEN>(P, rowbase, bh);
  const KeyFlags F = load_key_flags<GEN>(P, rowbase, L, nT, lane);
  Row<DH> R;
  load_row<DH, GEN>(P, IO, K, rowbase, hoff, qb, c, g, R);
  const int nt = tiles_of_block<GEN>(P, F, qb, nT);
  float wko[KS], wkd[KS];
  key_weights<DH, GEN>(P, K, g, wko, wkd);

  auto build = [&](int t, Tile& T) {
    f4 k4[DT], v4[DT];
    row_frag<DH>(P.k, rowbase, H, hoff, 16 * t, L, c, g, k4);
    row_frag<DH>(P.v, rowbase, H, hoff, 16 * t, L, c, g, v4);
    f4 co4, cd4;
    key_affine<DH, GEN>(K, k4, wko, wkd, g, co4, cd4);
    tile_forward<DH, GEN>(P, K, F, R, S, k4, v4, co4, cd4, t, g, T);
  };

  // ---- sweep 1: online soft-max -> log-normaliser and D = <Pt, dPt> ---------------------------------------------------
  float m_l = ACATTN_NEG_INF, z_l = 0.f, d_l = 0.f;  // this lane's keys only; the quad is joined after the sweep
  for (int t = 0; t < nt; ++t) {
    Tile T;
    build(t, T);
    float tm = ACATTN_NEG_INF;
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if ((T.inb >> r) & 1u) tm = fmaxf(tm, T.x[r]);
    const float m_new = fmaxf(m_l, tm);
    const float mu = m_new == ACATTN_NEG_INF ? 0.f : m_new;
    const float f = fast_exp(m_l - mu);  // exp(-inf) = 0 while the lane has seen no key
    z_l *= f;
    d_l *= f;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float e = ((T.inb >> r) & 1u) ? fast_exp(T.x[r] - mu) : 0.f;
      z_l += e;
      d_l += e * T.dPk[r];
    }
    m_l = m_new;
  }
  const float mx = quad_max(m_l);  // finite: key 0 of the row exists
  const float fl = fast_exp(m_l - mx);
  const float zx = quad_sum(z_l * fl);
  const float lz = fast_log(zx);
  const float D = quad_sum(d_l * fl) * fast_rcp(zx);
  if (row_ok && g == 0) {
    float* wrow = ws + (bh * L + i) * NSC;
    *(f4*)wrow = f4{mx, lz, D, 0.f};
  }

  // ---- sweep 2: dz -> dq; query halves of the parameter gradients ------------------------------------------------------
  f4 oq[DT];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) oq[dt] = f4{0.f, 0.f, 0.f, 0.f};
  float da_o = 0.f, da_d = 0.f, dsc_acc = 0.f;
  for (int t = 0; t < nt; ++t) {
    Tile T;
    build(t, T);
    f4 Pt, dz, d_o, d_d;
    float dsc;
    tile_backward<GEN>(T, K, mx, lz, D, R.i, 16 * t + 4 * g, Pt, dz, d_o, d_d, dsc);
    da_o += hsum(d_o);
    da_d += hsum(d_d);
    dsc_acc += dsc;
    float kc[4][DT];
    col_frag<DH>(P.k, rowbase, H, hoff, 16 * t, L, c, g, kc);
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) oq[dt] = mfma16(kc[r][dt], dz[r], oq[dt]);
  }
  da_o = quad_sum(da_o);
  da_d = quad_sum(da_d);
  dsc_acc = quad_sum(dsc_acc);
  if (row_ok) {
    const size_t off = (rowbase + i) * H + hoff + 4 * g;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) {
      // rank-1 terms of dq: query halves of the affine weights in the lane's output-column order
      f4 o = oq[dt];
      if (SP_UO) o += da_o * *(const f4*)(P.w_order + 16 * dt + 4 * g);
      if (SP_UD) o += da_d * *(const f4*)(P.w_dist + 16 * dt + 4 * g);
      *(f4*)(IO.dq + off + 16 * dt) = o;
    }
  }
  // query halves of dw_order / dw_dist, db_order, db_dist, d scalar: summed over the block's 16 rows, then added to the
  // (sequence, head) partial row (zeroed by the launcher)
  const int stride_w = IO.part_stride ? IO.part_stride : 2 * DH, stride_s = IO.part_stride ? IO.part_stride : 4;
  const float ro = row_ok ? 1.0f : 0.0f;
#pragma unroll
  for (int s = 0; s < KS; ++s) {
    const float vo = row16_sum(da_o * R.qf[s] * ro), vd = row16_sum(da_d * R.qf[s] * ro);
    if (c == 0) {
      if (SP_UO) atomicAdd(IO.dw_order_part + bh * stride_w + KS * g + s, vo);
      if (SP_UD) atomicAdd(IO.dw_dist_part + bh * stride_w + KS * g + s, vd);
    }
  }
  const float so = row16_sum(da_o * ro), sd = row16_sum(da_d * ro), ss = row16_sum(dsc_acc * ro);
  if (lane == 0) {
    if (SP_UO) atomicAdd(IO.dsmall_part + bh * stride_s + 0, so);
    if (SP_UD) {
      atomicAdd(IO.dsmall_part + bh * stride_s + 1, sd);
      atomicAdd(IO.dsmall_part + bh * stride_s + 2, ss);
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// key kernel
// ---------------------------------------------------------------------------------------------------------------------
template <int DH, bool GEN>
__global__ void __launch_bounds__(64) acattn_spatial_bwd_key_kernel(const acattn_problem P, const acattn_spatial_bwd_io IO,
                                                                    const float* __restrict__ ws) {
  constexpr int KS = DH / 4, DT = DH / 16;
  constexpr int TS = 20;  // row stride of a transposed 16 x 16 tile in LDS (16-byte aligned rows, conflict-free reads)
  __shared__ __attribute__((aligned(16))) float tr[2][16 * TS];
  const int L = P.L, H = P.H, nh = P.n_heads;
  const int nT = (L + 15) >> 4;
  const int n_items = P.B * nh;
  const bool causal = SP_MODE == ACATTN_MASK_STRUCTURED && P.causal != 0;
  const int rank = blockIdx.x / n_items, item = blockIdx.x - rank * n_items;
  const int t = rank;  // under the causal mask key tile 0 is seen by every query block: heaviest first
  int b, h;
  decode_block(item, P.B, nh, b, h);
  const int lane = threadIdx.x, c = lane & 15, g = lane >> 4;
  const size_t rowbase = (size_t)b * L, bh = (size_t)b * nh + h;
  const int hoff = h * DH;

  const Consts K = make_consts(P, DH);
  const Seq S = make_seq<GEN>(P, rowbase, bh);
  const KeyFlags F = load_key_flags<GEN>(P, rowbase, L, nT, lane);
  // this wave's 16 keys: row fragments of K, V (fixed), key halves of the affines
  f4 k4[DT], v4[DT];
  row_frag<DH>(P.k, rowbase, H, hoff, 16 * t, L, c, g, k4);
  row_frag<DH>(P.v, rowbase, H, hoff, 16 * t, L, c, g, v4);
  f4 co4, cd4;
  {
    float wko[KS], wkd[KS];
    key_weights<DH, GEN>(P, K, g, wko, wkd);
    key_affine<DH, GEN>(K, k4, wko, wkd, g, co4, cd4);
  }

  f4 aK[DT], aV[DT];  // dK^T, dV^T: lane (c, g) holds key 16 t + c, columns 16 dt + 4 g ..
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) {
    aK[dt] = f4{0.f, 0.f, 0.f, 0.f};
    aV[dt] = aK[dt];
  }
  f4 dco = {0.f, 0.f, 0.f, 0.f}, dcd = dco;  // d (key half of the affines) of keys 16 t + 4 g + r, summed over queries at the end

  // the query blocks that visit this tile in the row kernel (every other pair carries no probability mass: under the
  // causal mask the blocks in front of the tile, unless they hold a fully masked row, which spreads over every key) and
  // may carry a cotangent
  uint32_t visit = 0u;
  for (int qb = 0; qb < nT; ++qb)
    if (t < tiles_of_block<GEN>(P, F, qb, nT)) visit |= 1u << qb;
  visit &= blocks_with_cotangent(IO, b);
  while (visit) {
    const int qb = __ffs((int)visit) - 1;
    visit &= visit - 1u;
    Row<DH> R;
    load_row<DH, GEN>(P, IO, K, rowbase, hoff, qb, c, g, R);
    const float* wrow = ws + (bh * L + R.il) * NSC;
    // (a row past L reads the last row's scalars for a finite tile; with D = 0 and a zero cotangent its dz is exactly 0)
    const f4 w4 = *(const f4*)wrow;
    const float mx = w4[0], lz = w4[1], D = R.row_ok ? w4[2] : 0.f;
    float qc[4][DT], gc[4][DT];  // requested in front of the tile's arithmetic: one round trip per pair
    col_frag<DH>(P.q, rowbase, H, hoff, 16 * qb, L, c, g, qc);
    col_frag<DH>(IO.d_ctx, rowbase, H, hoff, 16 * qb, L, c, g, gc);
    Tile T;
    tile_forward<DH, GEN>(P, K, F, R, S, k4, v4, co4, cd4, t, g, T);
    f4 Pt, dz, d_o, d_d;
    float dsc;
    tile_backward<GEN>(T, K, mx, lz, D, R.i, 16 * t + 4 * g, Pt, dz, d_o, d_d, dsc);
    dco += d_o;
    dcd += d_d;
    f4 Pk;
#pragma unroll
    for (int r = 0; r < 4; ++r) Pk[r] = ((T.keep >> r) & 1u) ? Pt[r] * K.keep_scale : 0.f;
    // turn the two [query c][key 4 g + r] tiles so that the query index becomes the MFMA reduction index
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    *(f4*)(&tr[0][c * TS + 4 * g]) = dz;
    *(f4*)(&tr[1][c * TS + 4 * g]) = Pk;
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const float b_z = tr[0][(4 * g + s) * TS + c], b_p = tr[1][(4 * g + s) * TS + c];
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) {
        aK[dt] = mfma16(qc[s][dt], b_z, aK[dt]);
        aV[dt] = mfma16(gc[s][dt], b_p, aV[dt]);
      }
    }
  }

  // ---- results: dk (+ rank-1 key-half terms), dv; key halves of the parameter gradients ---------------------------------
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
    const size_t o = (rowbase + key) * H + hoff + 4 * g;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) {
      f4 ok = aK[dt];
      if (SP_UO) ok += dco_c * *(const f4*)(P.w_order + DH + 16 * dt + 4 * g);
      if (SP_UD) ok += dcd_c * *(const f4*)(P.w_dist + DH + 16 * dt + 4 * g);
      *(f4*)(IO.dk + o + 16 * dt) = ok;
      *(f4*)(IO.dv + o + 16 * dt) = aV[dt];
    }
  }
  // dw_order[dh:] += sum_j d co_j K_j, the same for the distance affine
  const int stride_w = IO.part_stride ? IO.part_stride : 2 * DH;
  const float okk = key < L ? 1.0f : 0.0f;
#pragma unroll
  for (int s4 = 0; s4 < KS / 4; ++s4)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float vo = row16_sum(dco_c * k4[s4][e] * okk), vd = row16_sum(dcd_c * k4[s4][e] * okk);
      if (c == 0) {
        if (SP_UO) atomicAdd(IO.dw_order_part + bh * stride_w + DH + KS * g + 4 * s4 + e, vo);
        if (SP_UD) atomicAdd(IO.dw_dist_part + bh * stride_w + DH + KS * g + 4 * s4 + e, vd);
      }
    }
}

template <int DH>
int launch_spatial_bwd(const acattn_problem& p, const acattn_spatial_bwd_io& io, hipStream_t stream) {
  const int nT = (p.L + 15) / 16;
  const size_t rows = (size_t)p.B * p.n_heads;
  // the parameter partial rows are accumulated with atomics: start from zero (this also writes the columns of a
  // disabled term and the spare one).  A failed fill must not be followed by atomics into whatever the buffer held.
  int rc = 0;
  auto zero = [&](float* ptr, size_t n) {
    if (!rc) rc = acattn_launch_zero(ptr, n, stream);
  };
  if (io.part_stride) {
    zero(std::min(io.dw_order_part, std::min(io.dw_dist_part, io.dsmall_part)), rows * io.part_stride);
  } else {
    zero(io.dw_order_part, rows * 2 * DH);
    zero(io.dw_dist_part, rows * 2 * DH);
    zero(io.dsmall_part, rows * 4);
  }
  if (rc) return rc;
  const dim3 grid(p.B * p.n_heads * nT), block(64);
  float* ws = (float*)io.workspace;
  if (p.mask_mode == ACATTN_MASK_STRUCTURED && p.rng_mode == ACATTN_RNG_COUNTER && p.w_order && p.w_dist) {
    hipLaunchKernelGGL((acattn_spatial_bwd_row_kernel<DH, false>), grid, block, 0, stream, p, io, ws);
    hipLaunchKernelGGL((acattn_spatial_bwd_key_kernel<DH, false>), grid, block, 0, stream, p, io, (const float*)ws);
  } else {
    hipLaunchKernelGGL((acattn_spatial_bwd_row_kernel<DH, true>), grid, block, 0, stream, p, io, ws);
    hipLaunchKernelGGL((acattn_spatial_bwd_key_kernel<DH, true>), grid, block, 0, stream, p, io, (const float*)ws);
  }
  return (int)hipGetLastError();
}

}  // namespace

int64_t acattn_spatial_bwd_ws_bytes(const acattn_problem& p) { return (int64_t)p.B * p.n_heads * p.L * NSC * sizeof(float); }

int acattn_launch_spatial_bwd(const acattn_problem& p, const acattn_spatial_bwd_io& io, hipStream_t stream) {
  switch (p.H / p.n_heads) {
    case 16: return launch_spatial_bwd<16>(p, io, stream);
    case 32: return launch_spatial_bwd<32>(p, io, stream);
    case 64: return launch_spatial_bwd<64>(p, io, stream);
    case 128: return launch_spatial_bwd<128>(p, io, stream);
  }
  acattn_set_error("unsupported head size: dh must be 16, 32, 64 or 128");
  return -1;
}
