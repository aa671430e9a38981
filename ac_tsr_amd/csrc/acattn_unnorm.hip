// The UN-NORMALISED attention core of ACSSEPT (L <= 64): recbole/model/transformer_layers.py:873-1006, the encoder
// acssept.py:17 builds.  It shares every parameter with the encoder of recbole/model/layers.py but has none of that one's
// three re-normalisations (layers.py:919, 921, 925): the raw mixtures go straight into the value product.  Per head:
//     C  = q.K^T + e_order + e_distance                   transformer_layers.py:823-857
//     P  = dropout(softmax(C / sqrt(dh) + mask))          keep_after   :859-867
//     M  = dropout(softmax(qa.Ka^T / sqrt(dh) + mask))    keep_mask    :785-802   (the returned attack mask)
//     A_att = P M + N (1 - M),  N ~ randn                 :921-922     no soft-max
//     A_w   = P (g + (1 - g) exp(1 - M))                  :924, :901-902   no soft-max; g = sigmoid(gate(query))[b, i, j]
//     ctx_attacked = A_att.V,  ctx_calibrated = A_w.V     :805
// A new kernel pair behind its own entry points (acattn_unnorm_attention_fwd / _bwd): no kernel of the normalised core and
// neither of its dispatchers is involved.
//
// What having no re-normalisation means here:
//   - where M = 0 (future keys under the causal mask, padded keys) A_att = N: ctx_attacked sums over ALL L keys, the rows of
//     V at padded and future positions included (a NaN there reaches ctx_attacked, as in the reference).  No key tile is
//     skipped anywhere in this file: every block visits all ceil(L/16) tiles;
//   - nothing hides the tile padding columns L .. 16 ceil(L/16) - 1: P and M are exact zeros there (mask -inf), the noise is
//     forced to zero, and the staged rows of K, Ka and V past L are zeros;
//   - a query row without an allowed key (a left-padded sequence under the causal mask) has -10000 added to every score in
//     the reference; the common shift is dropped and the soft-max runs over all L keys (the float64 value of such a row;
//     the reference's fp32 rounding of `score - 10000` is not reproduced).
//
// Frame (acattn_row64.h, shared with acattn_timeaware.hip): one workgroup per (sequence, head), one wave per 16-row query
// block, K, Ka, V and the key halves of the spatial affines staged once in LDS, fp32 MFMA 16x16x4, exponentials in the exp2 domain, the block body compiled per tile count.
// Backward: phase A, a wave works its query block down to dS, dSa (dq, dqa and the gate gradient leave here) and parks
// dS, dSa, A_att, A_w as [query][key] matrices in LDS; one barrier; phase B, wave w owns key tile w and sums the query
// blocks' contributions to dk, dka, dv in ascending block order on the MFMA.  No atomic, no exchange whose order depends
// on timing: two launches give the same bits.
#include "acattn_row64.h"

#define ACATTN_L64_WHAT "un-normalised attention"
#include "acattn_l64_checks.inc"

namespace {

// blockDim.x == 4 * LP: thread idx + it * blockDim covers the LP x DH/4 16-byte pieces of a matrix in DH / 16 rounds
template <int DH>
__device__ __forceinline__ void stage(const acattn_problem& P, const Staged<DH>& S, size_t rowbase, int hoff, int L, int LP) {
  constexpr int VS = DH + 4, C4 = DH / 4;
  const f4 w_ko = *(const f4*)(P.w_order + DH + 4 * (threadIdx.x % C4));
  const f4 w_kd = *(const f4*)(P.w_dist + DH + 4 * (threadIdx.x % C4));
#pragma unroll
  for (int it = 0; it < DH / 16; ++it) {
    const int idx = threadIdx.x + it * blockDim.x;
    const int row = idx / C4, c4 = idx - row * C4;
    f4 kv = {0.f, 0.f, 0.f, 0.f}, kav = kv, vv = kv;
    if (row < L) {
      const size_t o = (rowbase + row) * P.H + hoff + 4 * c4;
      kv = *(const f4*)(P.k + o);
      kav = *(const f4*)(P.ka + o);
      vv = *(const f4*)(P.v + o);
    }
    *(f4*)(S.Ks + row * VS + 4 * c4) = kv;
    *(f4*)(S.Kas + row * VS + 4 * c4) = kav;
    *(f4*)(S.Vs + row * VS + 4 * c4) = vv;
    float co = kv.x * w_ko.x + kv.y * w_ko.y + kv.z * w_ko.z + kv.w * w_ko.w;
    float cd = kv.x * w_kd.x + kv.y * w_kd.y + kv.z * w_kd.z + kv.w * w_kd.w;
#pragma unroll
    for (int off = 1; off < C4; off <<= 1) {
      co += __shfl_xor(co, off);
      cd += __shfl_xor(cd, off);
    }
    if (c4 == 0) {
      S.s_co[row] = -kLog2e * co;
      S.s_cd[row] = cd;
    }
  }
  if ((int)threadIdx.x < LP) {
    const int j = threadIdx.x;
    S.s_lt[j] = logf((float)(j + 1));
    S.s_ok[j] = (j < L && P.key_valid[rowbase + j]) ? 1.0f : 0.0f;
  }
}

// RowCore plus what this file alone does with a row
template <int DH>
struct Row : RowCore<DH> {
  using Core = RowCore<DH>;
  using Core::Core;
  using Core::KS, Core::VS, Core::P, Core::c, Core::g, Core::i, Core::row_ok, Core::rowbase, Core::hoff;

  // x = C / sqrt(dh) + mask and y = qa.Ka^T / sqrt(dh) + mask, both in exp2 units
  template <int NTB>
  __device__ __forceinline__ void scores(f4 (&x)[NTB], f4 (&y)[NTB]) const {
    this->template scores_dense<NTB>(x, y);
    this->template scores_finish<NTB>(x, y);
  }
  // w[query c][key] = sum over the head's columns of X[key][.] d[query c][.]  (d: a [B,L,H] tensor, NULL = zeros)
  template <int NTB>
  __device__ __forceinline__ void keys_times(const float* X, const float* d, f4 (&w)[NTB]) const {
#pragma unroll
    for (int t = 0; t < NTB; ++t) w[t] = f4{0.f, 0.f, 0.f, 0.f};
    if (!d) return;
    const size_t off = (rowbase + (row_ok ? i : 0)) * P.H + hoff + KS * g;
#pragma unroll
    for (int s4 = 0; s4 < KS / 4; ++s4) {
      f4 d4 = {0.f, 0.f, 0.f, 0.f};
      if (row_ok) d4 = *(const f4*)(d + off + 4 * s4);
#pragma unroll
      for (int t = 0; t < NTB; ++t) {
        const f4 x4 = *(const f4*)(X + (16 * t + c) * VS + KS * g + 4 * s4);
#pragma unroll
        for (int e = 0; e < 4; ++e) w[t] = mfma16(x4[e], d4[e], w[t]);
      }
    }
  }
};

// ------------------------------------------------------------------------------------------------------------------------
// forward
// ------------------------------------------------------------------------------------------------------------------------
template <int DH, int NTB>
__device__ __forceinline__ void fwd_block(const acattn_problem& P, const acattn_fwd_out& O, const Row<DH>& R) {
  f4 x[NTB], y[NTB];
  R.template scores<NTB>(x, y);
  // the two row soft-maxes of this core
  float mx = ACATTN_NEG_INF, my = ACATTN_NEG_INF;
#pragma unroll
  for (int t = 0; t < NTB; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      mx = fmaxf(mx, x[t][r]);
      my = fmaxf(my, y[t][r]);
    }
  mx = quad_max(mx);
  my = quad_max(my);
  float sx = 0.f, sy = 0.f;
#pragma unroll
  for (int t = 0; t < NTB; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      sx += ex2(x[t][r] - mx);
      sy += ex2(y[t][r] - my);
    }
  const float lse_x2 = mx + __builtin_amdgcn_logf(quad_sum(sx)), lse_y2 = my + __builtin_amdgcn_logf(quad_sum(sy));
  if (O.row_stats && R.row_ok && R.g == 0) {
    float* sp = O.row_stats + (R.bh * R.L + R.i) * ACATTN_NSTAT;
    *(f4*)sp = f4{lse_x2, lse_y2, 0.f, 0.f};
    *(f4*)(sp + 4) = f4{0.f, 0.f, 0.f, 0.f};
  }
  const float* gate = R.gate_row();
  f4 a_att[NTB], a_w[NTB];
#pragma unroll
  for (int t = 0; t < NTB; ++t) {
    f4 n;
    uint32_t ka, km;
    R.draws(t, n, ka, km);
    f4 p, m, e;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      p[r] = ex2(x[t][r] - lse_x2);
      m[r] = ex2(y[t][r] - lse_y2);
    }
    p = R.live(p * keep_scale4(ka, R.keep_scale));
    m = R.live(m * keep_scale4(km, R.keep_scale));
    R.store_seg(O.attack_mask, t, m);
#pragma unroll
    for (int r = 0; r < 4; ++r) e[r] = ex2((1.0f - m[r]) * kLog2e);
    const f4 gt = gate_value(R.load_row(gate, t), P.gate_is_prob);
    a_att[t] = R.live(p * m + n * (1.0f - m));
    a_w[t] = p * (gt + (1.0f - gt) * e);
  }
  f4 o[DH / 16];
  const size_t off = (R.rowbase + R.i) * P.H + R.hoff + 4 * R.g;
  R.template times_keys<NTB>(R.S.Vs, a_att, o);
  if (R.row_ok) {
#pragma unroll
    for (int dt = 0; dt < DH / 16; ++dt) *(f4*)(O.ctx_attacked + off + 16 * dt) = o[dt];
  }
  R.template times_keys<NTB>(R.S.Vs, a_w, o);
  if (R.row_ok) {
#pragma unroll
    for (int dt = 0; dt < DH / 16; ++dt) *(f4*)(O.ctx_calibrated + off + 16 * dt) = o[dt];
  }
}

template <int DH>
__global__ void __launch_bounds__(256) acattn_unnorm_fwd_kernel(const acattn_problem P, const acattn_fwd_out O) {
  const int L = P.L, nT = (L + 15) >> 4, LP = 16 * nT;
  int b, h;
  decode_block(blockIdx.x, P.B, P.n_heads, b, h);
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const Staged<DH> S(smem, LP);
  stage<DH>(P, S, (size_t)b * L, h * DH, L, LP);
  __syncthreads();
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const Row<DH> R(P, S, b, h, wave, threadIdx.x & 63);
  switch (nT) {
    case 1: fwd_block<DH, 1>(P, O, R); break;
    case 2: fwd_block<DH, 2>(P, O, R); break;
    case 3: fwd_block<DH, 3>(P, O, R); break;
    default: fwd_block<DH, 4>(P, O, R); break;
  }
}

// ------------------------------------------------------------------------------------------------------------------------
// backward
// ------------------------------------------------------------------------------------------------------------------------
// LDS behind the staged operands: four [LP][LP + 4] matrices (dS, dSa, A_att, A_w), per-wave column sums of the two affine
// cotangents, their totals, and three per-row sums
struct BwdShared {
  float *mat, *colp, *col, *rows;
  int LS, LP;
  __device__ __forceinline__ BwdShared(float* base, int LP_) {
    LP = LP_;
    LS = LP + 4;
    mat = base;
    colp = mat + 4 * LP * LS;
    col = colp + 4 * 2 * LP;
    rows = col + 2 * LP;
  }
  static constexpr int floats(int LP) { return 4 * LP * (LP + 4) + 8 * LP + 2 * LP + 3 * LP; }
};

template <int DH, int NTB>
__device__ __forceinline__ void bwd_block(const acattn_problem& P, const acattn_bwd_io& IO, const Row<DH>& R, const BwdShared& W) {
  constexpr int DT = DH / 16;
  const int c = R.c, g = R.g, qb = R.qb;
  f4 x[NTB], y[NTB];
  R.template scores<NTB>(x, y);
  float lse_x2 = 0.f, lse_y2 = 0.f;
  if (R.row_ok) {
    const float* sp = IO.row_stats + (R.bh * R.L + R.i) * ACATTN_NSTAT;
    lse_x2 = sp[0];
    lse_y2 = sp[1];
  }
  f4 dAa[NTB], dAw[NTB];
  R.template keys_times<NTB>(R.S.Vs, IO.d_ctx_attacked, dAa);
  R.template keys_times<NTB>(R.S.Vs, IO.d_ctx_calibrated, dAw);
  const float* gate = R.gate_row();
  const float dpen2 = IO.d_penalty_part ? 2.0f * IO.d_penalty_part[R.bh * ((R.L + 15) >> 4) + qb] : 0.f;
  const float inv_sqrt = 1.0f / sqrtf((float)DH);
  uint32_t keepA = 0, keepM = 0;
  float r1 = 0.f, r2 = 0.f;
  // x becomes Pt, then dS; y becomes Mt, then dSa; dAa becomes d Pt, dAw becomes d Mt
#pragma unroll
  for (int t = 0; t < NTB; ++t) {
    f4 n;
    uint32_t ka, km;
    R.draws(t, n, ka, km);
    keepA |= ka << (4 * t);
    keepM |= km << (4 * t);
    f4 pt, mt, e;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      pt[r] = ex2(x[t][r] - lse_x2);
      mt[r] = ex2(y[t][r] - lse_y2);
    }
    pt = R.live(pt);
    mt = R.live(mt);
    const f4 ksa = keep_scale4(ka, R.keep_scale), ksm = keep_scale4(km, R.keep_scale);
    const f4 p = pt * ksa, m = mt * ksm;
#pragma unroll
    for (int r = 0; r < 4; ++r) e[r] = ex2((1.0f - m[r]) * kLog2e);
    const f4 gt = gate_value(R.load_row(gate, t), P.gate_is_prob);
    const f4 mix = gt + (1.0f - gt) * e;
    // the two mixtures, for dv
    *(f4*)(W.mat + (2 * W.LP + 16 * qb + c) * W.LS + 16 * t + 4 * g) = R.live(p * m + n * (1.0f - m));
    *(f4*)(W.mat + (3 * W.LP + 16 * qb + c) * W.LS + 16 * t + 4 * g) = p * mix;
    const f4 dp = dAa[t] * m + dAw[t] * mix;
    f4 dm = dAa[t] * (p - n) - dAw[t] * p * (1.0f - gt) * e + R.load_seg(IO.d_attack_mask, t);
    if (IO.d_penalty_part) dm += (m - 1.0f) * dpen2;  // d sum (1 - M)^2 = 2 (M - 1)
    if (IO.dgate_logits) R.store_seg(IO.dgate_logits, t, dAw[t] * p * (1.0f - e) * gt * (1.0f - gt));
    dAa[t] = R.live(dp * ksa);
    dAw[t] = R.live(dm * ksm);
    r1 += hsum(pt * dAa[t]);
    r2 += hsum(mt * dAw[t]);
    x[t] = pt;
    y[t] = mt;
  }
  r1 = quad_sum(r1);
  r2 = quad_sum(r2);
  float go_r = 0.f, gd_r = 0.f, dsc_r = 0.f;
  const float sc2 = R.sc * R.sc;
#pragma unroll
  for (int t = 0; t < NTB; ++t) {
    x[t] = (x[t] * (dAa[t] - r1)) * inv_sqrt;  // dS = d C
    y[t] = (y[t] * (dAw[t] - r2)) * inv_sqrt;  // dSa
    *(f4*)(W.mat + (0 * W.LP + 16 * qb + c) * W.LS + 16 * t + 4 * g) = x[t];
    *(f4*)(W.mat + (1 * W.LP + 16 * qb + c) * W.LS + 16 * t + 4 * g) = y[t];
    // the spatial calibrator: cotangents of the two affines' values
    f4 pr, val, df, go, gd;
    R.spatial(t, pr, val, df);
    const int d0 = R.i - (16 * t + 4 * g);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float slope = pr[r] * (1.0f - pr[r]) / (val[r] + ACATTN_LOG_EPS);
      go[r] = x[t][r] * (d0 - r < 0 ? slope : -slope);
      gd[r] = x[t][r] * df[r] * sc2;
      dsc_r -= x[t][r] * df[r] * df[r] * R.sc;
    }
    go_r += hsum(go);
    gd_r += hsum(gd);
    // this block's column sums (over its 16 rows) of both, keys 16 t + 4 g + r
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      go[r] = rows16_sum(go[r]);
      gd[r] = rows16_sum(gd[r]);
    }
    if (c == 0) {
      *(f4*)(W.colp + (2 * qb + 0) * W.LP + 16 * t + 4 * g) = go;
      *(f4*)(W.colp + (2 * qb + 1) * W.LP + 16 * t + 4 * g) = gd;
    }
  }
  go_r = quad_sum(go_r);
  gd_r = quad_sum(gd_r);
  dsc_r = quad_sum(dsc_r);
  if (g == 0) {
    W.rows[0 * W.LP + 16 * qb + c] = go_r;
    W.rows[1 * W.LP + 16 * qb + c] = gd_r;
    W.rows[2 * W.LP + 16 * qb + c] = dsc_r;
  }
  // dq = dS.K + the query halves of the affines; dqa = dSa.Ka
  f4 o[DT];
  const size_t off = (R.rowbase + R.i) * P.H + R.hoff + 4 * g;
  R.template times_keys<NTB>(R.S.Ks, x, o);
  if (R.row_ok) {
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) {
      const f4 wo = *(const f4*)(P.w_order + 16 * dt + 4 * g), wd = *(const f4*)(P.w_dist + 16 * dt + 4 * g);
      *(f4*)(IO.dq + off + 16 * dt) = o[dt] + wo * go_r + wd * gd_r;
    }
  }
  R.template times_keys<NTB>(R.S.Kas, y, o);
  if (R.row_ok) {
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) *(f4*)(IO.dqa + off + 16 * dt) = o[dt];
  }
}

template <int DH>
__global__ void __launch_bounds__(256) acattn_unnorm_bwd_kernel(const acattn_problem P, const acattn_bwd_io IO) {
  constexpr int DT = DH / 16, VS = DH + 4;
  const int L = P.L, H = P.H, nT = (L + 15) >> 4, LP = 16 * nT;
  int b, h;
  decode_block(blockIdx.x, P.B, P.n_heads, b, h);
  const size_t rowbase = (size_t)b * L, bh = (size_t)b * P.n_heads + h;
  const int hoff = h * DH;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const Staged<DH> S(smem, LP);
  const BwdShared W(smem + Staged<DH>::floats(LP), LP);
  stage<DH>(P, S, rowbase, hoff, L, LP);
  __syncthreads();
  const int lane = threadIdx.x & 63, c = lane & 15, g = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  {
    const Row<DH> R(P, S, b, h, wave, lane);
    switch (nT) {
      case 1: bwd_block<DH, 1>(P, IO, R, W); break;
      case 2: bwd_block<DH, 2>(P, IO, R, W); break;
      case 3: bwd_block<DH, 3>(P, IO, R, W); break;
      default: bwd_block<DH, 4>(P, IO, R, W); break;
    }
  }
  __syncthreads();
  // column totals of the two affine cotangents: the blocks' parts in ascending block order
  if ((int)threadIdx.x < 2 * LP) {
    const int which = threadIdx.x / LP, j = threadIdx.x - which * LP;
    float tot = 0.f;
    for (int q = 0; q < nT; ++q) tot += W.colp[(2 * q + which) * LP + j];
    W.col[which * LP + j] = tot;
  }
  __syncthreads();

  // ---- phase B: wave w owns key tile w ------------------------------------------------------------------------------------
  // out[key 16 w + c][16 dt + 4 g + r] = sum over the query rows of mat[row][key] src[row][.], blocks in ascending order
  const int key = 16 * wave + c;
  auto key_side = [&](const float* mat, const float* src, f4 (&o)[DT]) {
    if (!src) return;
    for (int q = 0; q < nT; ++q) {
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const int row = 16 * q + 4 * g + s;
        const float w = mat[row * W.LS + key];
        const float* p = src + (rowbase + (row < L ? row : 0)) * H + hoff + c;
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) o[dt] = mfma16(row < L ? p[16 * dt] : 0.f, w, o[dt]);
      }
    }
  };
  const size_t koff = (rowbase + key) * H + hoff + 4 * g;
  f4 o[DT];
  auto zero = [&]() {
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) o[dt] = f4{0.f, 0.f, 0.f, 0.f};
  };
  zero();
  key_side(W.mat + 0 * LP * W.LS, P.q, o);
  if (key < L) {
    const float go_c = W.col[key], gd_c = W.col[LP + key];
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) {
      const f4 wo = *(const f4*)(P.w_order + DH + 16 * dt + 4 * g), wd = *(const f4*)(P.w_dist + DH + 16 * dt + 4 * g);
      *(f4*)(IO.dk + koff + 16 * dt) = o[dt] + wo * go_c + wd * gd_c;
    }
  }
  zero();
  key_side(W.mat + 1 * LP * W.LS, P.qa, o);
  if (key < L) {
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) *(f4*)(IO.dka + koff + 16 * dt) = o[dt];
  }
  zero();
  key_side(W.mat + 2 * LP * W.LS, IO.d_ctx_attacked, o);
  key_side(W.mat + 3 * LP * W.LS, IO.d_ctx_calibrated, o);
  if (key < L) {
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) *(f4*)(IO.dv + koff + 16 * dt) = o[dt];
  }

  // ---- the calibrator's parameters: this (sequence, head)'s partial sums, rows and keys in ascending order -------------------
  const int wstride = IO.part_stride ? IO.part_stride : 2 * DH, sstride = IO.part_stride ? IO.part_stride : 4;
  if ((int)threadIdx.x < DH) {
    const int d = threadIdx.x;
    float wo_q = 0.f, wd_q = 0.f, wo_k = 0.f, wd_k = 0.f;
    for (int r = 0; r < L; ++r) {
      const float qv = P.q[(rowbase + r) * H + hoff + d], kv = S.Ks[r * VS + d];
      wo_q += W.rows[r] * qv;
      wd_q += W.rows[LP + r] * qv;
      wo_k += W.col[r] * kv;
      wd_k += W.col[LP + r] * kv;
    }
    IO.dw_order_part[bh * wstride + d] = wo_q;
    IO.dw_order_part[bh * wstride + DH + d] = wo_k;
    IO.dw_dist_part[bh * wstride + d] = wd_q;
    IO.dw_dist_part[bh * wstride + DH + d] = wd_k;
  }
  if (threadIdx.x == 63) {
    float dbo = 0.f, dbd = 0.f, dsc = 0.f;
    for (int r = 0; r < L; ++r) {
      dbo += W.rows[r];
      dbd += W.rows[LP + r];
      dsc += W.rows[2 * LP + r];
    }
    float* sp = IO.dsmall_part + bh * sstride;
    sp[0] = dbo;
    sp[1] = dbd;
    sp[2] = dsc;
    sp[3] = 0.f;
  }
}

// The configuration this pair covers (include/acattn.h): the limit a problem breaks, or NULL.
const char* unnorm_limit(const acattn_problem& p) {
  const char* w = l64_config(p);
  return w ? w : l64_sizes(p);
}

}  // namespace

int acattn_unnorm_supported(const acattn_problem& p) { return unnorm_limit(p) ? 0 : 1; }

int acattn_launch_unnorm_fwd(const acattn_problem& p, const acattn_fwd_out& o, hipStream_t stream) {
  const char* why = unnorm_limit(p);
  if (!why) why = l64_pointers(p);
  if (!why) why = l64_fwd_out(o);
  if (why) {
    acattn_set_error(why);
    return -1;
  }
  const int nT = (p.L + 15) / 16, LP = 16 * nT, grid = p.B * p.n_heads;
  switch (p.H / p.n_heads) {
    case 16: return launch(acattn_unnorm_fwd_kernel<16>, sizeof(float) * Staged<16>::floats(LP), grid, 64 * nT, stream, p, o);
    case 32: return launch(acattn_unnorm_fwd_kernel<32>, sizeof(float) * Staged<32>::floats(LP), grid, 64 * nT, stream, p, o);
    default: return launch(acattn_unnorm_fwd_kernel<64>, sizeof(float) * Staged<64>::floats(LP), grid, 64 * nT, stream, p, o);
  }
}

int acattn_launch_unnorm_bwd(const acattn_problem& p, const acattn_bwd_io& io, hipStream_t stream) {
  const char* why = unnorm_limit(p);
  if (!why) why = l64_pointers(p);
  if (!why) why = l64_bwd_io(p, io);
  if (why) {
    acattn_set_error(why);
    return -1;
  }
  const int nT = (p.L + 15) / 16, LP = 16 * nT, grid = p.B * p.n_heads;
  const size_t extra = sizeof(float) * BwdShared::floats(LP);
  switch (p.H / p.n_heads) {
    case 16: return launch(acattn_unnorm_bwd_kernel<16>, sizeof(float) * Staged<16>::floats(LP) + extra, grid, 64 * nT, stream, p, io);
    case 32: return launch(acattn_unnorm_bwd_kernel<32>, sizeof(float) * Staged<32>::floats(LP) + extra, grid, 64 * nT, stream, p, io);
    default: return launch(acattn_unnorm_bwd_kernel<64>, sizeof(float) * Staged<64>::floats(LP) + extra, grid, 64 * nT, stream, p, io);
  }
}
