// The row frame of the two L <= 64 attention cores without re-normalisation: acattn_unnorm.hip (ACSSEPT) and
// acattn_timeaware.hip (ACTiSASRec).  One workgroup per (sequence, head), one wave per 16-row query block, the key side
// staged once in LDS, fp32 MFMA 16x16x4, exponentials in the exp2 domain.  Here: the staged layout, one lane's view of its
// query row (which rows are dead, the mask, the spatial prior, the replay of noise and keep bits, the dense scores, the
// products against the staged matrices) and the launch helper.  Each file derives its Row<DH> from RowCore<DH> and keeps
// its own stage(), block bodies and kernels.
#pragma once
#include "acattn_common.h"

namespace {

constexpr float kLog2e = 1.44269504088896340736f;
constexpr float kLn2 = 0.69314718055994530942f;

__device__ __forceinline__ float ex2(float x) { return __builtin_amdgcn_exp2f(x); }
__device__ __forceinline__ float hsum(const f4 v) { return (v[0] + v[1]) + (v[2] + v[3]); }

// sum over the 16 query rows of a block (lanes of equal g), for every lane
__device__ __forceinline__ float rows16_sum(float v) {
  v += __shfl_xor(v, 1);
  v += __shfl_xor(v, 2);
  v += __shfl_xor(v, 4);
  v += __shfl_xor(v, 8);
  return v;
}

// What a workgroup stages once: K, Ka, V rows of its head ([LP][DH + 4], rows past L zeros; the time-interval core stages
// K + pk and V + pv) and per key the halves of the two spatial affines (from the plain k), log(distance + 1) and the key's
// validity.
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

// One lane's view of its query row: lane = 16 g + c holds, of query row i = 16 qb + c, the keys 16 t + 4 g + r of tile t.
// Of the row's dh-vectors (q, qa) it holds the columns KS g .. KS g + KS - 1.
template <int DH>
struct RowCore {
  static constexpr int KS = DH / 4, VS = DH + 4;
  const acattn_problem& P;
  const Staged<DH>& S;
  int L, c, g, qb, i;
  bool row_ok, dead, causal, has_drop;
  size_t rowbase, bh, prow;
  size_t ll_row;  // the row's offset in a [B,L,L] tensor (a row past L: row 0's); set on request only, see the constructor
  int hoff;
  float ao2, ad, sc, scale2, keep_scale;
  RngKey rkey;
  float qf[KS], qaf[KS];

  // `with_ll_row`: also set ll_row.  It is formed here, right behind prow, because that is where the time-interval kernels
  // have always formed it: behind this constructor the same product gives them other machine code, and the un-normalised
  // kernels, which form it where gate_row() is used, keep theirs by not asking.
  __device__ __forceinline__ RowCore(const acattn_problem& P_, const Staged<DH>& S_, int b, int h, int qb_, int lane,
                                     bool with_ll_row = false)
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
    if (with_ll_row) ll_row = (rowbase + (row_ok ? i : 0)) * (size_t)L;
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
  // 1 - pr otherwise), df = log(|i - j| + 1) - distance affine.  transformer_layers.py:833-845 and :847-855 in the
  // un-normalised layer, :1152-1156 and :1158-1164 in the time-interval layer
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
  // The scores in two halves; a derived Row's scores() runs them back to back or adds its own terms to x in between.
  // First x = e_order + e_distance + q.K^T and y = qa.Ka^T, unscaled ...
  template <int NTB>
  __device__ __forceinline__ void scores_dense(f4 (&x)[NTB], f4 (&y)[NTB]) const {
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
  }
  // ... then x / sqrt(dh) + mask and y / sqrt(dh) + mask, both in exp2 units
  template <int NTB>
  __device__ __forceinline__ void scores_finish(f4 (&x)[NTB], f4 (&y)[NTB]) const {
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
  __device__ __forceinline__ f4 live(const f4 v) const { return row_ok ? v : f4{0.f, 0.f, 0.f, 0.f}; }
};

template <class K, class... A>
int launch(K kern, size_t lds, int grid, int threads, hipStream_t stream, const A&... args) {
  if (lds > 64 * 1024) {
    const hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return (int)e;
  }
  hipLaunchKernelGGL(kern, dim3(grid), dim3(threads), lds, stream, args...);
  return (int)hipGetLastError();
}

}  // namespace
