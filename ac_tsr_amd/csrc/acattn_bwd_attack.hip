// Attention backward, attack side alone (L <= 64): dqa and dka from a cotangent of the attack mask, nothing else.
//
// The attacked-loss walk asks the last layer for exactly this (the mask-only launch of the split, acattn_bwd.hip): no
// context cotangent anywhere, so of the whole chain only the soft-max of the mask scores is left,
//     Sa = qa.Ka^T / sqrt(dh),  Mt = exp2(y - lse_y),  dM = keep . (d_attack_mask + 2 d_pen (Mt keep - 1)),
//     r2 = sum_j Mt dM,  dSa = Mt (dM - r2) / sqrt(dh),  dqa = dSa.Ka,  dka = dSa^T.qa.
// acattn_bwd_fast_kernel evaluates it on its MASK_ONLY path, behind a prologue built for the full backward (K and V staged,
// three accumulators zeroed, the key-side calibrator terms, 55 KB of LDS, two workgroups per CU).  Here the workgroup
// shares Ka, the key mask and the key-side slots only.
//
// One workgroup per (sequence, head), wave = 16-row query block, the tile count per block by acattn_bwd_fast.hip's rule.
// Key side without an atomic and without an exchange between the waves' tile sets: every wave turns its dSa tiles through
// a wave-private 16 x 16 LDS scratch, forms ITS partial dka tiles on the MFMA and parks them in per-(block, tile) slots;
// one barrier; the slots of a key tile are summed in ascending block order and stored.  The same bits on every launch.
// The slots are sized for the regular case (under the causal mask block qb reaches qb + 1 tiles: 10 slots at four blocks).
// A left-padded sequence has blocks none of whose rows sees a key and which spread over every tile; when the tiles of a
// workgroup do not fit, its waves take turns, in the same ascending order, at one accumulator kept in the slot area.
//
// CTX: the same frame for an attack-only launch that also carries a cotangent of the CALIBRATED context (layer 0 of the
// attacked-loss walk: dense d_ctx_calibrated from the layer tail, no d_ctx_attacked).  The calibrated branch is
// acattn_bwd_fast.hip's body on its `!IO.d_ctx_attacked` path reduced to what reaches dM:
//     Pt (scores q.K^T, spatial calibrator, lse_x), the keep bits, dAw = V.dctx_c, Ac, the gate, Aw,
//     dc = sum Aw dAw, dac = (1 - gt) Aw (dAw - dc), r1 = sum Ac dac, dM = -Ac (dac - r1) (p ex1)
// and from there the chain above.  No dP, no gate gradient, no dv, no calibrator gradients, no LDS atomic.  K and V are
// staged next to Ka; both are dead once every wave has formed Pt and dAw, so behind one more barrier the slots take their
// place (38 KB instead of 57 KB at head size 32, L = 50).
#include <stdlib.h>

#include <type_traits>

#include "acattn_common.h"

namespace {

constexpr float kLog2e = 1.44269504088896340736f;
constexpr float kLn2 = 0.69314718055994530942f;

__device__ __forceinline__ float ex2(float x) { return __builtin_amdgcn_exp2f(x); }
__device__ __forceinline__ float hsum(const f4 v) { return (v[0] + v[1]) + (v[2] + v[3]); }

constexpr int TS = 20;  // row stride of a turned 16 x 16 tile (16-byte rows, conflict-free column reads)

// The value behind an empty asm: what is computed from it is computed again, not kept in registers from an earlier use
__device__ __forceinline__ int again(int x) {
  asm volatile("" : "+v"(x));
  return x;
}

// keep_after and keep_mask of rng_group for the same arguments, without the normals
__device__ __forceinline__ void rng_keep_pair(const RngKey key, uint32_t row_id, uint32_t grp, float p_drop, uint32_t& keep_after,
                                              uint32_t& keep_mask) {
  if (p_drop == 0.5f) {  // wave-uniform
    uint32_t x = (row_id * 64u + grp) ^ key.a;
    x *= 0x7feb352dU;
    x ^= x >> 15;
    x *= 0x846ca68bU;
    x ^= x >> 16;
    x += key.b;
    const uint32_t w2 = rng_word(x, 0xB5297A4Du, 0x85EBCA77u);
    keep_after = (w2 >> 4) & 0xFu;
    keep_mask = (w2 >> 12) & 0xFu;
  } else {
    const RngGroup rg = rng_group(key, row_id, grp, p_drop);
    keep_after = rg.keep_after;
    keep_mask = rg.keep_mask;
  }
}

template <int DH, bool CTX>
__global__ void __launch_bounds__(256, CTX ? 3 : 4) acattn_bwd_attack_kernel(const acattn_problem P, const acattn_bwd_io IO, float* gate_zero,
                                                                    const int n_slots) {
  constexpr int KS = DH / 4;
  constexpr int DT = DH / 16;
  constexpr int VS = DH + 4;
  constexpr int SLOT = 16 * VS;  // one parked 16-key tile of dka

  const int L = P.L, H = P.H, nh = P.n_heads;
  const int nT = (L + 15) >> 4;
  const int LP = nT * 16;
  int b, h;
  decode_block(blockIdx.x, P.B, nh, b, h);
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int c = lane & 15, g = lane >> 4;
  const size_t rowbase = (size_t)b * L;
  const int hoff = h * DH;
  const size_t bh = (size_t)b * nh + h;

  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* Kas = smem;               // [LP][VS]
  float* s_km = Kas + LP * VS;     // [LP] exp2-domain key mask
  float* scr_all = s_km + LP;      // [nT][16 * TS] the waves' turning scratch
  float* slots = scr_all + nT * 16 * TS;  // [n_slots][SLOT]; n_slots >= nT
  float* scr = scr_all + wave * 16 * TS;
  // CTX: the key-side calibrator terms, then K and V in the place the slots take once both are dead
  float* s_co = slots;         // [LP] -log2e * (k_j . w_order[dh:])
  float* s_cd = s_co + LP;     // [LP] k_j . w_dist[dh:]
  float* s_lt = s_cd + LP;     // [LP] log(j + 1)
  float* Ks = s_lt + LP;       // [LP][VS]
  float* Vs = Ks + LP * VS;    // [LP][VS]
  if constexpr (CTX) slots = Ks;

  // ---- this block's rows of qa: as the B operand of the scores, and column-wise as the A operand of dka ----------------
  const int qb = wave, i0 = qb * 16, i = i0 + c;
  const bool row_ok = i < L;
  float qaf[KS];
  [[maybe_unused]] float qf[KS];
  {
    const size_t off = (rowbase + (row_ok ? i : 0)) * H + hoff + KS * g;
#pragma unroll
    for (int s4 = 0; s4 < KS / 4; ++s4) {
      f4 ta = {0.f, 0.f, 0.f, 0.f};
      if (row_ok) ta = *(const f4*)(P.qa + off + 4 * s4);
#pragma unroll
      for (int e = 0; e < 4; ++e) qaf[4 * s4 + e] = ta[e];
      if constexpr (CTX) {
        f4 tq = {0.f, 0.f, 0.f, 0.f};
        if (row_ok) tq = *(const f4*)(P.q + off + 4 * s4);
#pragma unroll
        for (int e = 0; e < 4; ++e) qf[4 * s4 + e] = tq[e];
      }
    }
  }
  const float lse_y2 = row_ok ? IO.row_stats[(bh * L + i) * ACATTN_NSTAT + 1] * kLog2e : 0.f;
  [[maybe_unused]] float lse_x2 = 0.f, lse_v2 = 0.f, lse_w2 = 0.f;
  if constexpr (CTX) {
    if (row_ok) {
      const float* sp = IO.row_stats + (bh * L + i) * ACATTN_NSTAT;
      lse_x2 = sp[0] * kLog2e;
      lse_v2 = sp[3] * kLog2e;
      lse_w2 = sp[4] * kLog2e;
    }
  }
  float qac[4][DT];
  auto load_qac = [&](int c, int g) {
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int row = i0 + 4 * g + s;
      const float* p = P.qa + (rowbase + min(row, L - 1)) * H + hoff + c;
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) qac[s][dt] = row < L ? p[16 * dt] : 0.f;
    }
  };
  if constexpr (!CTX) load_qac(c, g);  // CTX: asked for behind the calibrated branch, whose registers it would take

  // ---- stage Ka and the key mask ------------------------------------------------------------------------------------------
  constexpr int KV_IT = DH / 16;
  f4 r_ka[KV_IT];
#pragma unroll
  for (int it = 0; it < KV_IT; ++it) {
    const int idx = threadIdx.x + it * blockDim.x;
    const int row = idx / (DH / 4), c4 = idx - row * (DH / 4);
    r_ka[it] = f4{0.f, 0.f, 0.f, 0.f};
    if (row < L) r_ka[it] = *(const f4*)(P.ka + (rowbase + row) * H + hoff + 4 * c4);
  }
  const uint8_t r_valid = (threadIdx.x < L) ? P.key_valid[rowbase + threadIdx.x] : (uint8_t)0;
  if constexpr (CTX) {  // K, V and the key-side calibrator terms, as acattn_bwd_fast.hip stages them
    const f4 w_ko = *(const f4*)(P.w_order + DH + 4 * (threadIdx.x % (DH / 4)));
    const f4 w_kd = *(const f4*)(P.w_dist + DH + 4 * (threadIdx.x % (DH / 4)));
#pragma unroll
    for (int it = 0; it < KV_IT; ++it) {
      const int idx = threadIdx.x + it * blockDim.x;
      const int row = idx / (DH / 4), c4 = idx - row * (DH / 4);
      f4 kv = {0.f, 0.f, 0.f, 0.f}, vv = kv;
      if (row < L) {
        const size_t o = (rowbase + row) * H + hoff + 4 * c4;
        kv = *(const f4*)(P.k + o);
        vv = *(const f4*)(P.v + o);
      }
      *(f4*)(Ks + row * VS + 4 * c4) = kv;
      *(f4*)(Vs + row * VS + 4 * c4) = vv;
      float co = kv.x * w_ko.x + kv.y * w_ko.y + kv.z * w_ko.z + kv.w * w_ko.w;
      float cd = kv.x * w_kd.x + kv.y * w_kd.y + kv.z * w_kd.z + kv.w * w_kd.w;
#pragma unroll
      for (int off = 1; off < DH / 4; off <<= 1) {
        co += __shfl_xor(co, off);
        cd += __shfl_xor(cd, off);
      }
      if (c4 == 0) {
        s_co[row] = -kLog2e * co;
        s_cd[row] = cd;
      }
    }
    if (threadIdx.x < LP) s_lt[threadIdx.x] = logf((float)(threadIdx.x + 1));
  }
  [[maybe_unused]] float ao = 0.f, ad = 0.f, sc = 0.f;
  if constexpr (CTX) {
#pragma unroll
    for (int s4 = 0; s4 < KS / 4; ++s4) {
      const f4 a = *(const f4*)(P.w_order + KS * g + 4 * s4), d = *(const f4*)(P.w_dist + KS * g + 4 * s4);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        ao += qf[4 * s4 + e] * a[e];
        ad += qf[4 * s4 + e] * d[e];
      }
    }
    ao = quad_sum(ao) + P.b_order[0];
    ad = quad_sum(ad) + P.b_dist[0];
    sc = P.scalar[0];
  }
  // the split's gate gradient is a zeroed [B,L,L] the one-row launch adds its read row to: head 0's workgroup writes the zeros
  if (gate_zero && h == 0) {
    float* zp = gate_zero + rowbase * L;
    const int n = L * L;
    for (int j = 4 * threadIdx.x; j < n; j += 4 * blockDim.x) {
      if (j + 3 < n) {
        *(f4u*)(zp + j) = f4{0.f, 0.f, 0.f, 0.f};
      } else {
        for (int r = 0; j + r < n; ++r) zp[j + r] = 0.f;
      }
    }
  }
#pragma unroll
  for (int it = 0; it < KV_IT; ++it) {
    const int idx = threadIdx.x + it * blockDim.x;
    const int row = idx / (DH / 4), c4 = idx - row * (DH / 4);
    *(f4*)(Kas + row * VS + 4 * c4) = r_ka[it];
  }
  if (threadIdx.x < LP) {
    const int j = threadIdx.x;
    float km = ACATTN_NEG_INF;
    if (j < L) km = r_valid ? 0.f : ACATTN_MASK_FILL * kLog2e;
    s_km[j] = km;
  }
  const uint64_t seed_eff = P.seed + (P.seed_device ? *P.seed_device : 0ull);
  const RngKey rkey = rng_key(seed_eff);
  __syncthreads();

  // ---- key tiles per block: acattn_bwd_fast.hip's rule, for every block of the workgroup (all wave-uniform) -----------------
  const unsigned long long valid_keys = __ballot(lane < L && s_km[lane] == 0.f);
  const int first_valid = valid_keys ? __ffsll((long long)valid_keys) - 1 : L;
  const bool causal = P.causal != 0;
  const int nt_valid = valid_keys ? ((63 - __clzll((long long)valid_keys)) >> 4) + 1 : nT;
  auto tiles_of_block = [&](int q) {
    const bool rows_see_a_key = causal ? first_valid <= 16 * q : valid_keys != 0;
    return rows_see_a_key ? min(causal ? min(nT, q + 1) : nT, nt_valid) : nT;
  };
  int nts[4], base[4], total = 0;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    nts[q] = q < nT ? tiles_of_block(q) : 0;
    base[q] = total;
    total += nts[q];
  }
  const int nt = tiles_of_block(qb);
  const int my_base = qb == 0 ? base[0] : qb == 1 ? base[1] : qb == 2 ? base[2] : base[3];
  const bool in_turns = total > n_slots;  // (uniform over the workgroup) the tiles do not fit the slots: see the top

  const float inv_sqrt = 1.0f / sqrtf((float)DH);
  const float scale2 = inv_sqrt * kLog2e;
  const bool has_drop = P.p_drop > 0.f;
  const float keep_scale = has_drop ? 1.0f / (1.0f - P.p_drop) : 1.0f;
  const uint32_t prow = ((uint32_t)bh * L + (row_ok ? i : 0)) * (uint32_t)L;
  const float dpen2 = IO.d_penalty_part ? 2.0f * IO.d_penalty_part[(size_t)bh * nT + qb] : 0.f;  // (uniform per wave)
  const uint32_t rng_row = (uint32_t)(bh * L + i);
  const float okf = row_ok ? 1.0f : 0.0f;

  auto mask4 = [&](int t) -> f4 {
    const f4 km4 = *(const f4*)(s_km + 16 * t + 4 * g);
    if (causal && (16 * t + 15 > i0)) {
      const int dq = (c - 4 * g) + 16 * (qb - t);  // key after query  <=>  dq < r  (see acattn_fwd_dma.hip)
      f4 m;
#pragma unroll
      for (int r = 0; r < 4; ++r) m[r] = (dq < r) ? fminf(km4[r], ACATTN_MASK_FILL * kLog2e) : km4[r];
      return m;
    }
    return km4;
  };
  // sigmoid(order affine), its log-argument and the distance residual of tile t (acattn_bwd_fast.hip's spatial())
  [[maybe_unused]] const float ao2 = -kLog2e * ao;
  [[maybe_unused]] const float nhs2 = -0.5f * (sc * sc);
  [[maybe_unused]] auto spatial = [&](int t, f4& val, f4& df) {
    const f4 ea = *(const f4*)(s_co + 16 * t + 4 * g) + ao2;
    const f4 cd4 = *(const f4*)(s_cd + 16 * t + 4 * g);
    const int d0 = i - (16 * t + 4 * g);
    f4 lt4;
#pragma unroll
    for (int r = 0; r < 4; ++r) {  // (no branch on the tile's place against the diagonal: see mask4_flat)
      const float pr = fast_rcp(1.0f + ex2(ea[r]));
      val[r] = (d0 - r < 0) ? pr : 1.0f - pr;
      lt4[r] = s_lt[d0 - r < 0 ? r - d0 : d0 - r];
    }
    df = lt4 - (cd4 + ad);
  };
  // CTX: mask4 without its branch (a tile wholly below the diagonal has dq >= 4 > r: the select keeps km4 there), so that a
  // tile's chain stays one straight line; `fresh`: read again, the four tiles' masks are not worth 16 registers from
  // phase 0 to phase 2
  [[maybe_unused]] auto mask4_flat = [&](int t, bool fresh) -> f4 {
    const int g_ = fresh ? again(g) : g;
    const f4 km4 = *(const f4*)(s_km + 16 * t + 4 * g_);
    const int dq = causal ? (c - 4 * g_) + 16 * (qb - t) : 4;
    f4 m;
#pragma unroll
    for (int r = 0; r < 4; ++r) m[r] = (dq < r) ? fminf(km4[r], ACATTN_MASK_FILL * kLog2e) : km4[r];
    return m;
  };
  auto load_seg = [&](const float* rowp, int t) -> f4 {  // 4 keys of this row from a [B,nh,L,L] row
    const int j0 = 16 * t + 4 * g;
    f4 v = {0.f, 0.f, 0.f, 0.f};
    if (row_ok && j0 < L) {
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
  };

  const int c0 = c, g0 = g;
  auto body = [&](auto ntb_c) {
    constexpr int NTB = decltype(ntb_c)::value;
    // CTX: nothing of a body is evaluated in front of the switch for all four of them (the calibrator's terms were)
    if constexpr (CTX) asm volatile("; %0 key tiles" ::"n"(NTB) : "memory");

    // ---- Mt from the saved log-normaliser -----------------------------------------------------------------------------------
    f4 tM[NTB], dMa[NTB];
    [[maybe_unused]] f4 tS[CTX ? NTB : 1];  // CTX: Pt
#pragma unroll
    for (int t = 0; t < NTB; ++t) tM[t] = f4{0.f, 0.f, 0.f, 0.f};
    if constexpr (CTX) {
      // Pt's scores start from the spatial calibrator's terms in the scores' own unit (x = scale2 (q.k + log(val) ln 2 -
      // s^2 df^2 / 2) + mask, acattn_bwd_fast.hip's phase 0 with the sum in another order): the MFMA adds q.k on top,
      // and of the calibrator nothing but these four registers per tile is alive behind this loop
#pragma unroll
      for (int t = 0; t < NTB; ++t) {
        f4 val, df, lg;
        spatial(t, val, df);
#pragma unroll
        for (int r = 0; r < 4; ++r) lg[r] = __builtin_amdgcn_logf(val[r] + ACATTN_LOG_EPS);
        tS[t] = lg * kLn2 + (df * df) * nhs2;
      }
#pragma unroll
      for (int s4 = 0; s4 < KS / 4; ++s4) {
#pragma unroll
        for (int t = 0; t < NTB; ++t) {
          const f4 x4 = *(const f4*)(Ks + (16 * t + c) * VS + KS * g + 4 * s4);
#pragma unroll
          for (int e = 0; e < 4; ++e) tS[t] = mfma16(x4[e], qf[4 * s4 + e], tS[t]);
        }
      }
    }
#pragma unroll
    for (int s4 = 0; s4 < KS / 4; ++s4) {
#pragma unroll
      for (int t = 0; t < NTB; ++t) {
        const f4 x4 = *(const f4*)(Kas + (16 * t + c) * VS + KS * g + 4 * s4);
#pragma unroll
        for (int e = 0; e < 4; ++e) tM[t] = mfma16(x4[e], qaf[4 * s4 + e], tM[t]);
      }
    }
#pragma unroll
    for (int t = 0; t < NTB; ++t) {
      f4 mk4;
      if constexpr (CTX) mk4 = mask4_flat(t, false); else mk4 = mask4(t);
      const f4 y = tM[t] * scale2 + mk4;
#pragma unroll
      for (int r = 0; r < 4; ++r) tM[t][r] = ex2(y[r] - lse_y2) * okf;
      if constexpr (CTX) {
        const f4 x = tS[t] * scale2 + mk4;
#pragma unroll
        for (int r = 0; r < 4; ++r) tS[t][r] = ex2(x[r] - lse_x2) * okf;
      }
    }

    // ---- CTX: the calibrated branch, from the context cotangent down to dM --------------------------------------------------
    [[maybe_unused]] uint32_t keepM = 0;  // dropout keep bits of the mask, 4 per tile
    if constexpr (CTX) {
      f4 dAw[NTB], Ac[NTB], Aw[NTB];
      uint32_t keepA = 0;
#pragma unroll
      for (int t = 0; t < NTB; ++t) dAw[t] = f4{0.f, 0.f, 0.f, 0.f};
      // dAw = V.dctx_c
      {
        const size_t off = (rowbase + (row_ok ? i : 0)) * H + hoff + KS * g;
#pragma unroll
        for (int s4 = 0; s4 < KS / 4; ++s4) {
          f4 gc = {0.f, 0.f, 0.f, 0.f};
          if (row_ok) gc = *(const f4*)(IO.d_ctx_calibrated + off + 4 * s4);
#pragma unroll
          for (int t = 0; t < NTB; ++t) {
            const f4 x4 = *(const f4*)(Vs + (16 * t + c) * VS + KS * g + 4 * s4);
#pragma unroll
            for (int e = 0; e < 4; ++e) dAw[t] = mfma16(x4[e], gc[e], dAw[t]);
          }
        }
      }
#pragma unroll
      for (int t = 0; t < NTB; ++t) {
        uint32_t ka = 0xFu, km = 0xFu;
        if (has_drop) rng_keep_pair(rkey, rng_row, (uint32_t)(4 * t + g), P.p_drop, ka, km);
        keepA |= ka << (4 * t);
        keepM |= km << (4 * t);
      }
      // Ac, Aw; tS becomes p ex1, Aw becomes (1 - gt) Aw once dc has its term
      const float* grow = P.gate_logits + (rowbase + (row_ok ? i : 0)) * L;
      float dc = 0.f;
#pragma unroll
      for (int t = 0; t < NTB; ++t) {
        const uint32_t ka = (keepA >> (4 * t)) & 0xFu, km = (keepM >> (4 * t)) & 0xFu;
        const f4 p = tS[t] * keep_scale4(ka, keep_scale), m = tM[t] * keep_scale4(km, keep_scale);
        const f4 mk4 = mask4_flat(t, true);
        const f4 a1 = m * (-kLog2e) + kLog2e;
        f4 ex1;
#pragma unroll
        for (int r = 0; r < 4; ++r) ex1[r] = ex2(a1[r]);
        const f4 pe = p * ex1;
        const f4 v2 = pe * kLog2e + (mk4 - lse_v2);
        const f4 gt = gate_value(load_seg(grow, t), P.gate_is_prob);
#pragma unroll
        for (int r = 0; r < 4; ++r) Ac[t][r] = ex2(v2[r]) * okf;
        const f4 w2 = (gt * (p - Ac[t]) + Ac[t]) * kLog2e + (mk4 - lse_w2);
#pragma unroll
        for (int r = 0; r < 4; ++r) Aw[t][r] = ex2(w2[r]) * okf;
        dc += hsum(Aw[t] * dAw[t]);
        Aw[t] *= 1.0f - gt;
        tS[t] = pe;
      }
      dc = quad_sum(dc);
      float r1 = 0.f;
#pragma unroll
      for (int t = 0; t < NTB; ++t) {
        dAw[t] = Aw[t] * (dAw[t] - dc);  // d A_c
        r1 += hsum(Ac[t] * dAw[t]);
      }
      r1 = quad_sum(r1);
#pragma unroll
      for (int t = 0; t < NTB; ++t) dMa[t] = -(Ac[t] * (dAw[t] - r1)) * tS[t];
    }

    // ---- the mask cotangent through dropout and the soft-max -> dSa -----------------------------------------------------------
    float r2 = 0.f;
#pragma unroll
    for (int t = 0; t < NTB; ++t) {
      uint32_t keep = 0xFu;
      if constexpr (CTX) {
        keep = ((uint32_t)again((int)keepM) >> (4 * t)) & 0xFu;
      } else if (has_drop) {
        keep = P.p_drop == 0.5f ? rng_keep_mask_half(rkey, rng_row, (uint32_t)(4 * t + g))
                                : rng_group(rkey, rng_row, (uint32_t)(4 * t + g), P.p_drop).keep_mask;
      }
      const f4 sm = keep_scale4(keep, keep_scale);
      if constexpr (!CTX) dMa[t] = f4{0.f, 0.f, 0.f, 0.f};
      if (IO.d_attack_mask) {
        const f4 dm = load_seg(IO.d_attack_mask + prow, t);
        if constexpr (CTX) dMa[t] += dm; else dMa[t] = dm;
      }
      // the mask penalty's cotangent from the rebuilt tile (acattn_bwd_io.d_penalty_part): d M = 2 d_pen (M - 1), M = Mt . keep
      if (IO.d_penalty_part) dMa[t] += (tM[t] * sm - 1.0f) * dpen2;
      dMa[t] *= sm;
      r2 += hsum(tM[t] * dMa[t]);
    }
    r2 = quad_sum(r2);
#pragma unroll
    for (int t = 0; t < NTB; ++t) dMa[t] = (tM[t] * (dMa[t] - r2)) * inv_sqrt;  // dSa

    // CTX: the lane's place taken from the lane number again, so that the addresses of this phase are formed here and
    // not held in registers through the calibrated branch
    int c = c0, g = g0;
    if constexpr (CTX) {
      const int l = again(lane);
      c = l & 15;
      g = l >> 4;
    }
    const int i = i0 + c;
    if constexpr (CTX) load_qac(c, g);  // (L2 hits; in flight under dqa's MFMAs and the barrier)

    // ---- dqa = dSa.Ka -----------------------------------------------------------------------------------------------------------
    {
      f4 oqa[DT];
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) oqa[dt] = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int t = 0; t < NTB; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float* kap = Kas + (16 * t + 4 * g + r) * VS + c;
#pragma unroll
          for (int dt = 0; dt < DT; ++dt) oqa[dt] = mfma16(kap[16 * dt], dMa[t][r], oqa[dt]);
        }
      if (row_ok) {
        const uint32_t off = ((uint32_t)rowbase + i) * H + hoff + 4 * g;
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) *(f4*)(IO.dqa + off + 16 * dt) = oqa[dt];
      }
    }

    // ---- key side: this block's part of dka, tile by tile ----------------------------------------------------------------------
    // the [query c][key 4 g + r] tile is turned so that the query index becomes the MFMA reduction index; lane (c, g) then
    // holds dka_part[key 16 t + c][16 dt + 4 g + r]
    auto key_side = [&](auto sink) {
#pragma unroll
      for (int t = 0; t < NTB; ++t) {
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the reads of the tile before
        *(f4*)(scr + c * TS + 4 * g) = dMa[t];
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        f4 o[DT];
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) o[dt] = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          const float b_sa = scr[(4 * g + s) * TS + c];
#pragma unroll
          for (int dt = 0; dt < DT; ++dt) o[dt] = mfma16(qac[s][dt], b_sa, o[dt]);
        }
        sink(t, o);
      }
    };
    if constexpr (CTX) __syncthreads();  // every wave has formed Pt and dAw: K and V make room for the slots
    if (!in_turns) {
      key_side([&](int t, const f4 (&o)[DT]) {
        float* sl = slots + (my_base + t) * SLOT + c * VS + 4 * g;
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) *(f4*)(sl + 16 * dt) = o[dt];
      });
      __syncthreads();
    } else {
      // one accumulator [LP][VS] in the slot area (slot t = key tile t); wave w zeroes tile w, then block 0, 1, ... add
      for (int j = lane; j < SLOT; j += 64) slots[wave * SLOT + j] = 0.f;
      __syncthreads();
      for (int q = 0; q < nT; ++q) {
        if (q == qb)
          key_side([&](int t, const f4 (&o)[DT]) {
            float* sl = slots + t * SLOT + c * VS + 4 * g;
#pragma unroll
            for (int dt = 0; dt < DT; ++dt) *(f4*)(sl + 16 * dt) += o[dt];
          });
        __syncthreads();
      }
    }
  };
  switch (nt) {
    case 1: body(std::integral_constant<int, 1>{}); break;
    case 2: body(std::integral_constant<int, 2>{}); break;
    case 3: body(std::integral_constant<int, 3>{}); break;
    default: body(std::integral_constant<int, 4>{}); break;
  }

  // ---- dka: the parts of a key tile in ascending block order --------------------------------------------------------------------
  for (int idx = threadIdx.x; idx < L * (DH / 4); idx += blockDim.x) {
    const int row = idx / (DH / 4), c4 = idx - row * (DH / 4);
    const int t = row >> 4, in = (row & 15) * VS + 4 * c4;
    f4 sum = {0.f, 0.f, 0.f, 0.f};
    if (in_turns) {
      sum = *(const f4*)(slots + t * SLOT + in);
    } else {
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (nts[q] > t) sum += *(const f4*)(slots + (base[q] + t) * SLOT + in);
    }
    *(f4*)(IO.dka + (rowbase + row) * H + hoff + 4 * c4) = sum;
  }
}

template <int DH, bool CTX>
int launch_attack(const acattn_problem& p, const acattn_bwd_io& io, float* gate_zero, hipStream_t stream) {
  const int nT = (p.L + 15) / 16, LP = nT * 16;
  const int n_slots = p.causal ? nT * (nT + 1) / 2 : nT * nT;
  int tail = n_slots * 16 * (DH + 4);  // the slots; CTX: the calibrator terms, then the slots in K's and V's place
  if (CTX) tail = 3 * LP + (tail > 2 * LP * (DH + 4) ? tail : 2 * LP * (DH + 4));
  const size_t lds = (size_t)(LP * (DH + 4) + LP + nT * 16 * TS + tail) * sizeof(float);
  auto kern = acattn_bwd_attack_kernel<DH, CTX>;
  if (lds > 64 * 1024) {
    const hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return (int)e;
  }
  hipLaunchKernelGGL(kern, dim3(p.B * p.n_heads), dim3(64 * nT), lds, stream, p, io, gate_zero, n_slots);
  return (int)hipGetLastError();
}

}  // namespace

// Returns -100 outside its domain: acattn_launch_bwd_fast's, an attack-only launch (dqa, dka alone) without a cotangent of
// the attacked context, read rows or block bitmap, carrying a mask cotangent (d_attack_mask / d_penalty_part), a cotangent
// of the calibrated context (the CTX form; ACATTN_BWD_ATTACK_CTX=0 in the environment leaves it to the row-resident
// kernel, for A/B runs), or both.  `gate_zero`: a [B,L,L] buffer head 0's workgroups fill with zeros (the split's
// head-summed gate gradient, acattn_bwd.hip), or NULL; mask-only form only.
int acattn_launch_bwd_attack(const acattn_problem& p, const acattn_bwd_io& io, hipStream_t stream, float* gate_zero) {
  static const bool ctx_on = getenv("ACATTN_BWD_ATTACK_CTX") ? atoi(getenv("ACATTN_BWD_ATTACK_CTX")) != 0 : true;
  const bool ctx = io.d_ctx_calibrated != nullptr;
  const bool ok = p.L >= 1 && p.L <= 64 && (int64_t)p.B * p.n_heads * p.L * p.L < (1LL << 30) && (int64_t)p.B * p.L * p.H < (1LL << 30) &&
                  p.mask_mode == ACATTN_MASK_STRUCTURED && p.rng_mode == ACATTN_RNG_COUNTER && p.w_order && p.w_dist &&
                  p.adversarial && p.combine_option == ACATTN_COMBINE_GATE && p.two_level && io.attack_only &&
                  (io.d_attack_mask || io.d_penalty_part || ctx) && !io.d_ctx_attacked && (!ctx || (ctx_on && !gate_zero)) &&
                  !(io.read_rows && io.n_read_rows > 0) && !io.active_qblocks && !io.dqa2 && !io.dka2 && io.dqa && io.dka &&
                  io.row_stats;
  if (!ok) return -100;
  if (ctx) {
    if (!(p.q && p.k && p.v && p.gate_logits && p.b_order && p.b_dist && p.scalar)) return -100;
    switch (p.H / p.n_heads) {
      case 16: return launch_attack<16, true>(p, io, nullptr, stream);
      case 32: return launch_attack<32, true>(p, io, nullptr, stream);
      case 64: return launch_attack<64, true>(p, io, nullptr, stream);
    }
    return -100;
  }
  switch (p.H / p.n_heads) {
    case 16: return launch_attack<16, false>(p, io, gate_zero, stream);
    case 32: return launch_attack<32, false>(p, io, gate_zero, stream);
    case 64: return launch_attack<64, false>(p, io, gate_zero, stream);
  }
  return -100;
}
