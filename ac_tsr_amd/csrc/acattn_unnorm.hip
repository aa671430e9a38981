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
// Frame: one workgroup per (sequence, head), one wave per 16-row query block, K, Ka, V and the key halves of the spatial
// affines staged once in LDS, fp32 MFMA 16x16x4, exponentials in the exp2 domain, the block body compiled per tile count.
// Backward: phase A, a wave works its query block down to dS, dSa (dq, dqa and the gate gradient leave here) and parks
// dS, dSa, A_att, A_w as [query][key] matrices in LDS; one barrier; phase B, wave w owns key tile w and sums the query
// blocks' contributions to dk, dka, dv in ascending block order on the MFMA.  No atomic, no exchange whose order depends
// on timing: two launches give the same bits.
#include <type_traits>

#include "acattn_common.h"

namespace {

constexpr float kLog2e = 1.44269504088896340736f;
constexpr float kLn2 = 0.69314718055994530942f;

__device__ __forceinline__ float ex2(float x) { return __builtin_amdgcn_exp2f(x); }
__device__ __forceinline__ float hsum(const f4 v) { return (v[0] + v[1]) + (v[2] + v[3]); }

// What a workgroup stages once: K, Ka, V rows of its head ([LP][DH + 4], rows past L zeros) and per key the halves of the
// two spatial affines, log(distance + 1) and the key's validity.
template <int DH>
struct Staged {
  static constexpr int VS = DH + 4;
  float *Ks, *Kas, *Vs, *s_co, *s_cd, *s_lt, *s_ok;
  __device__ __forceinline__ Staged(float* base, int LP) {
    Ks = base;
    Kas = Ks + LP * VS;
    Vs = Kas + LP * VS;
    s_co = Vs + LP * VS;
    s_cd = s_co + LP;
    s_lt = s_cd + LP;
    s_ok = s_lt + LP;
  }
  static constexpr int floats(int LP) { return 3 * LP * VS + 4 * LP; }
};

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

// One lane's view of its query row: lane = 16 g + c holds, of query row i = 16 qb + c, the keys 16 t + 4 g + r of tile t.
template <int DH>
struct Row {
  static constexpr int KS = DH / 4, VS = DH + 4;
  const acattn_problem& P;
  const Staged<DH>& S;
  int L, c, g, qb, i;
  bool row_ok, dead, causal, has_drop;
  size_t rowbase, bh, prow;
  int hoff;
  float ao2, ad, sc, scale2, keep_scale;
  RngKey rkey;
  float qf[KS], qaf[KS];

  __device__ __forceinline__ Row(const acattn_problem& P_, const Staged<DH>& S_, int b, int h, int qb_, int lane)
      : P(P_), S(S_) {
    L = P.L;
    c = lane & 15;
    g = lane >> 4;
    qb = qb_;
    i = 16 * qb + c;
    row_ok = i < L;
    causal = P.causal != 0;
    rowbase = (size_t)b * L;
    hoff = h * DH;
    bh = (size_t)b * P.n_heads + h;
    prow = (bh * L + (row_ok ? i : 0)) * (size_t)L;
    has_drop = P.p_drop > 0.f;
    keep_scale = has_drop ? 1.0f / (1.0f - P.p_drop) : 1.0f;
    scale2 = kLog2e / sqrtf((float)DH);
    // a row none of whose keys is allowed: the mask's common shift is dropped, the soft-max runs over all L keys
    const unsigned long long valid = __ballot(lane < L && S.s_ok[lane < L ? lane : 0] != 0.f);
    const unsigned long long upto = (causal && i < 63) ? ((2ull << i) - 1ull) : ~0ull;
    dead = !row_ok || (valid & upto) == 0ull;
    const size_t off = (rowbase + (row_ok ? i : 0)) * P.H + hoff + KS * g;
    float ao = 0.f, adq = 0.f;
#pragma unroll
    for (int s4 = 0; s4 < KS / 4; ++s4) {
      f4 tq = {0.f, 0.f, 0.f, 0.f}, ta = tq;
      if (row_ok) {
        tq = *(const f4*)(P.q + off + 4 * s4);
        ta = *(const f4*)(P.qa + off + 4 * s4);
      }
      const f4 a = *(const f4*)(P.w_order + KS * g + 4 * s4), d = *(const f4*)(P.w_dist + KS * g + 4 * s4);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        qf[4 * s4 + e] = tq[e];
        qaf[4 * s4 + e] = ta[e];
        ao += tq[e] * a[e];
        adq += tq[e] * d[e];
      }
    }
    ao2 = -kLog2e * (quad_sum(ao) + P.b_order[0]);
    ad = quad_sum(adq) + P.b_dist[0];
    sc = P.scalar[0];
    rkey = rng_key(P.seed + (P.seed_device ? *P.seed_device : 0ull));
  }

  // additive mask of tile t in exp2 units: 0 allowed, -10000 log2(e) masked, -inf in the tile padding
  __device__ __forceinline__ f4 mask4(int t) const {
    const f4 ok4 = *(const f4*)(S.s_ok + 16 * t + 4 * g);
    f4 m;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int j = 16 * t + 4 * g + r;
      const bool allowed = dead || (ok4[r] != 0.f && (!causal || j <= i));
      m[r] = j >= L ? ACATTN_NEG_INF : (allowed ? 0.f : ACATTN_MASK_FILL * kLog2e);
    }
    return m;
  }
  // pr = sigmoid(order affine), val = the probability the order term takes the log of (pr for a key after the query,
  // 1 - pr otherwise; transformer_layers.py:833-845), df = log(|i - j| + 1) - distance affine (:847-855)
  __device__ __forceinline__ void spatial(int t, f4& pr, f4& val, f4& df) const {
    const f4 ea = *(const f4*)(S.s_co + 16 * t + 4 * g) + ao2;
    const f4 cd4 = *(const f4*)(S.s_cd + 16 * t + 4 * g);
    const int d0 = i - (16 * t + 4 * g);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      pr[r] = fast_rcp(1.0f + ex2(ea[r]));
      val[r] = (d0 - r < 0) ? pr[r] : 1.0f - pr[r];
      const int dist = d0 - r < 0 ? r - d0 : d0 - r;
      df[r] = S.s_lt[dist] - (cd4[r] + ad);  // (dist < LP: both indices are)
    }
  }
  // 4 keys of this row from the row's L floats (NULL = zeros); zeros past L and for rows past L
  __device__ __forceinline__ f4 load_row(const float* rowp, int t) const {
    const int j0 = 16 * t + 4 * g;
    f4 v = {0.f, 0.f, 0.f, 0.f};
    if (rowp && row_ok && j0 < L) {
      const float* p = rowp + j0;
      if (j0 + 3 < L) {
        v = *(const f4u*)p;
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (j0 + r < L) v[r] = p[r];
      }
    }
    return v;
  }
  // the same from a [B,nh,L,L] tensor
  __device__ __forceinline__ f4 load_seg(const float* t4, int t) const { return load_row(t4 ? t4 + prow : nullptr, t); }
  __device__ __forceinline__ const float* gate_row() const { return P.gate_logits + (rowbase + (row_ok ? i : 0)) * L; }
  __device__ __forceinline__ void store_seg(float* t4, int t, const f4 v) const {
    const int j0 = 16 * t + 4 * g;
    if (row_ok && j0 < L) {
      float* p = t4 + prow + j0;
      if (j0 + 3 < L) {
        *(f4u*)p = v;
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (j0 + r < L) p[r] = v[r];
      }
    }
  }
  __device__ __forceinline__ uint32_t load_bits(const uint8_t* k4, int t) const {
    uint32_t bits = 0xFu;
    if (k4 && row_ok) {
      bits = 0;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int j = 16 * t + 4 * g + r;
        bits |= ((j < L ? k4[prow + j] : (uint8_t)1) ? 1u : 0u) << r;
      }
    }
    return bits;
  }
  // the draws of tile t: four normals (zero past L) and the keep bits of P's and M's dropout
  __device__ __forceinline__ void draws(int t, f4& n, uint32_t& ka, uint32_t& km) const {
    ka = km = 0xFu;
    if (P.rng_mode == ACATTN_RNG_COUNTER) {
      const RngGroup rg = rng_group(rkey, (uint32_t)(bh * L + i), (uint32_t)(4 * t + g), P.p_drop);
      n = rg.n;
      if (has_drop) {
        ka = rg.keep_after;
        km = rg.keep_mask;
      }
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (16 * t + 4 * g + r >= L) n[r] = 0.f;
    } else {
      n = load_seg(P.noise, t);
      if (has_drop) {
        ka = load_bits(P.keep_after, t);
        km = load_bits(P.keep_mask, t);
      }
    }
  }
  // x = C / sqrt(dh) + mask and y = qa.Ka^T / sqrt(dh) + mask, both in exp2 units
  template <int NTB>
  __device__ __forceinline__ void scores(f4 (&x)[NTB], f4 (&y)[NTB]) const {
    const float nhs2 = -0.5f * (sc * sc);
#pragma unroll
    for (int t = 0; t < NTB; ++t) {
      f4 pr, val, df, lg;
      spatial(t, pr, val, df);
#pragma unroll
      for (int r = 0; r < 4; ++r) lg[r] = __builtin_amdgcn_logf(val[r] + ACATTN_LOG_EPS);
      x[t] = lg * kLn2 + (df * df) * nhs2;
      y[t] = f4{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int s4 = 0; s4 < KS / 4; ++s4) {
#pragma unroll
      for (int t = 0; t < NTB; ++t) {
        const f4 k4 = *(const f4*)(S.Ks + (16 * t + c) * VS + KS * g + 4 * s4);
        const f4 a4 = *(const f4*)(S.Kas + (16 * t + c) * VS + KS * g + 4 * s4);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          x[t] = mfma16(k4[e], qf[4 * s4 + e], x[t]);
          y[t] = mfma16(a4[e], qaf[4 * s4 + e], y[t]);
        }
      }
    }
#pragma unroll
    for (int t = 0; t < NTB; ++t) {
      const f4 mk = mask4(t);
      x[t] = x[t] * scale2 + mk;
      y[t] = y[t] * scale2 + mk;
    }
  }
  // out[query c][16 dt + 4 g + r] = sum over the keys of w[query c][key] X[key][.], X one of the staged matrices
  template <int NTB>
  __device__ __forceinline__ void times_keys(const float* X, const f4 (&w)[NTB], f4 (&o)[DH / 16]) const {
#pragma unroll
    for (int dt = 0; dt < DH / 16; ++dt) o[dt] = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < NTB; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float* xp = X + (16 * t + 4 * g + r) * VS + c;
#pragma unroll
        for (int dt = 0; dt < DH / 16; ++dt) o[dt] = mfma16(xp[16 * dt], w[t][r], o[dt]);
      }
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
  __device__ __forceinline__ f4 live(const f4 v) const { return row_ok ? v : f4{0.f, 0.f, 0.f, 0.f}; }
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

// sum over the 16 query rows of a block (lanes of equal g), for every lane
__device__ __forceinline__ float rows16_sum(float v) {
  v += __shfl_xor(v, 1);
  v += __shfl_xor(v, 2);
  v += __shfl_xor(v, 4);
  v += __shfl_xor(v, 8);
  return v;
}

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

// The configuration this pair covers (include/acattn.h); `why` receives the limit a problem breaks.
bool unnorm_supported(const acattn_problem& p, const char** why) {
  const char* w = nullptr;
  if (p.B < 1 || p.L < 1 || p.H < 1 || p.n_heads < 1 || p.H % p.n_heads != 0) w = "un-normalised attention: B, L, H, n_heads must be positive and H a multiple of n_heads";
  else if (p.L > 64) w = "un-normalised attention: sequence length L must be <= 64";
  else if (p.H / p.n_heads != 16 && p.H / p.n_heads != 32 && p.H / p.n_heads != 64) w = "un-normalised attention: head size must be 16, 32 or 64";
  else if (!p.adversarial) w = "un-normalised attention: needs the adversarial calibrator (adversarial = 1)";
  else if (p.combine_option != ACATTN_COMBINE_GATE) w = "un-normalised attention: combine_option must be gate (fixed / annealing are not built)";
  else if (!p.two_level) w = "un-normalised attention: two_level must be 1 (the one-level form is not built)";
  else if (p.mask_mode != ACATTN_MASK_STRUCTURED) w = "un-normalised attention: the mask must be structured (key_valid + causal); dense masks are not built";
  else if (p.rng_mode != ACATTN_RNG_EXPLICIT && p.rng_mode != ACATTN_RNG_COUNTER) w = "un-normalised attention: unknown rng_mode";
  else if (!(p.p_drop >= 0.f && p.p_drop < 1.f)) w = "un-normalised attention: p_drop must lie in [0, 1)";
  else if ((int64_t)p.B * p.n_heads * p.L * p.L >= (1LL << 31) || (int64_t)p.B * p.L * p.H >= (1LL << 31)) w = "un-normalised attention: tensors of 2^31 elements or more";
  if (why) *why = w;
  return w == nullptr;
}

const char* unnorm_pointers(const acattn_problem& p) {
  if (!p.q || !p.k || !p.v || !p.qa || !p.ka) return "un-normalised attention: q, k, v, qa, ka must be non-NULL";
  if (!p.gate_logits) return "un-normalised attention: combine_option gate needs gate_logits";
  if (!p.key_valid) return "un-normalised attention: structured mask needs key_valid";
  if (!p.w_order || !p.b_order || !p.w_dist || !p.b_dist || !p.scalar) return "un-normalised attention: both spatial terms must be present (order and distance affines, scalar)";
  if (p.rng_mode == ACATTN_RNG_EXPLICIT) {
    if (!p.noise) return "un-normalised attention: explicit rng mode needs noise";
    if (p.p_drop > 0.f && (!p.keep_after || !p.keep_mask)) return "un-normalised attention: explicit dropout needs keep_after and keep_mask";
  }
  return nullptr;
}

template <class K, class IO>
int launch(K kern, size_t lds, int grid, int threads, hipStream_t stream, const acattn_problem& p, const IO& io) {
  if (lds > 64 * 1024) {
    const hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return (int)e;
  }
  hipLaunchKernelGGL(kern, dim3(grid), dim3(threads), lds, stream, p, io);
  return (int)hipGetLastError();
}

}  // namespace

int acattn_unnorm_supported(const acattn_problem& p) { return unnorm_supported(p, nullptr) ? 1 : 0; }

int acattn_launch_unnorm_fwd(const acattn_problem& p, const acattn_fwd_out& o, hipStream_t stream) {
  const char* why = nullptr;
  if (!unnorm_supported(p, &why) || (why = unnorm_pointers(p))) {
    acattn_set_error(why);
    return -1;
  }
  if (!o.ctx_attacked || !o.ctx_calibrated || !o.attack_mask) {
    acattn_set_error("un-normalised attention forward: ctx_attacked, ctx_calibrated and attack_mask must be non-NULL");
    return -1;
  }
  if (o.after_spatial || o.before_spatial || o.perturbed_attention || o.calibrated_attention) {
    acattn_set_error("un-normalised attention forward: the probability dumps are not built");
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
  const char* why = nullptr;
  if (!unnorm_supported(p, &why) || (why = unnorm_pointers(p))) {
    acattn_set_error(why);
    return -1;
  }
  if (!io.row_stats || !io.attack_mask) why = "un-normalised attention backward: needs the forward's attack_mask and row_stats";
  else if (!io.dq || !io.dk || !io.dv || !io.dqa || !io.dka) why = "un-normalised attention backward: dq, dk, dv, dqa, dka must be non-NULL";
  else if (!io.dgate_logits) why = "un-normalised attention backward: gate combine needs dgate_logits";
  else if (!io.dw_order_part || !io.dw_dist_part || !io.dsmall_part) why = "un-normalised attention backward: parameter partial buffers must be non-NULL";
  else if (io.part_stride != 0 && io.part_stride < 2 * (p.H / p.n_heads)) why = "un-normalised attention backward: part_stride is smaller than a partial row";
  else if (io.dgate_summed) why = "un-normalised attention backward: dgate_summed is not built (per-head partials only)";
  else if (io.dqa2 || io.dka2 || io.d_ctx_calibrated2 || io.d_penalty_part2) why = "un-normalised attention backward: the second cotangent set is not built";
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
