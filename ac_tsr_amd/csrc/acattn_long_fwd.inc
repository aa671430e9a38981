// Fused calibrated attention forward, LONG form: one wave per (sequence, head, 16-row query block), key tiles visited in
// a run-time loop, nothing of size L in registers.  Included by acattn_long_fwd_dh{16,32,64,128}.hip (ACATTN_LONG_DH).
//
// The streaming kernel (acattn_fwd_stream.inc) and the general kernel (acattn_fwd_general.inc) keep a query block's
// whole score row in registers (13 key tiles: L <= 208).  Here the row exists one 16-key tile at a time and every level
// of the soft-max chain (layers.py:695-740, 657-674, 917-927) that needs a finished row sum gets a sweep of its own;
// each sweep recomputes K.Q^T and Ka.Qa^T of the tile on the fp32 MFMA:
//
//   sweep 1   online max / sum of the two level-1 rows  ->  lx, ly (log-normalisers of P and M) and the row's mask shift
//   sweep 2   P, M from lx, ly; M is written; level 2: A_p with an online max and sum exp(.) V accumulated un-normalised
//             (flash style: the noise term n (1 - M) scaled by the dropout is not bounded well enough for a fixed shift),
//             the sum of A_c's exponentials
//   sweep 3   P, M, A_c again; level 3: sum exp(combine + mask) and sum exp(.) V for the calibrated context
//   (combine FIXED only: a sweep between 2 and 3 for the un-masked inner soft-max softmax(P + A_c / 2), layers.py:885)
//
// Same lane layout as every kernel here: S^T = K.Q^T, lane (c = lane & 15, g = lane >> 4) holds query row i0 + c and
// keys 16 t + 4 g + r; probabilities are the B operand of ctx^T = V^T.P^T.  Operands come through buffer descriptors
// over ONE sequence (rows past its end read as zeros); [L, L] tensors are addressed from a 64-bit per-(sequence, head)
// row pointer, so no 32-bit offset grows with B * heads * L^2.  The additive mask is applied as the reference applies
// it (x + -10000 in fp32), which gives fully masked rows the reference's quantised arguments (DESIGN 4.1b) by itself.
// Every option of acattn_problem is read at run time; two_level == 0 and the probability dumps are refused by the
// launcher.  row_stats: the natural-log normalisers of the five soft-maxes (mask shift included), as the other forward
// kernels write them.
#include <stdlib.h>

#include "acattn_long_common.h"

namespace {

typedef __amdgpu_buffer_rsrc_t rsrc_t;

constexpr float kLog2e = 1.44269504088896340736f;
constexpr float kLn2 = 0.69314718055994530942f;

__device__ __forceinline__ float max4(const f4 v) { return fmaxf(fmaxf(v[0], v[1]), fmaxf(v[2], v[3])); }
// a running maximum that is still -inf (nothing seen) must not enter exp(m - m)
__device__ __forceinline__ float finite_or_zero(float m) { return m == ACATTN_NEG_INF ? 0.f : m; }

// Raw buffer descriptor over `bytes` bytes at `base` (wave-uniform): loads past the end return 0.
__device__ __forceinline__ rsrc_t make_rsrc(const void* base, int bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, bytes, 0x00020000);
}
__device__ __forceinline__ f4 bload4(rsrc_t r, int voff) {
  return __builtin_bit_cast(f4, __builtin_amdgcn_raw_buffer_load_b128(r, voff, 0, 0));
}

template <int DH, bool ADV>
__global__ void __launch_bounds__(64, DH >= 128 ? 1 : 2) acattn_long_fwd_kernel(const acattn_problem P, const acattn_fwd_out O) {
  constexpr int KS = DH / 4;   // floats of a row fragment per lane == k-steps of the score products
  constexpr int DT = DH / 16;  // 16-wide column tiles of the context
  extern __shared__ __attribute__((aligned(16))) float s_km[];  // [16 nT] per-key additive mask, -inf for keys >= L

  const int L = P.L, H = P.H, nh = P.n_heads;
  const int nT = (L + 15) >> 4, LP = 16 * nT;
  const int n_items = P.B * nh;
  const bool structured = P.mask_mode == ACATTN_MASK_STRUCTURED;
  const bool dense_ll = P.mask_mode == ACATTN_MASK_DENSE_LL;
  const bool causal = structured && P.causal != 0;
  // heaviest query blocks first: under the causal mask block qb visits qb + 1 key tiles
  const int rank = blockIdx.x / n_items, item = blockIdx.x - rank * n_items;
  const int qb = causal ? nT - 1 - rank : rank;
  int b, h;
  decode_block(item, P.B, nh, b, h);
  const int lane = threadIdx.x, c = lane & 15, g = lane >> 4;
  const size_t rowbase = (size_t)b * L, bh = (size_t)b * nh + h;
  const int hoff = h * DH;
  const int i0 = 16 * qb, i = i0 + c;
  const bool row_ok = i < L;
  const bool use_order = P.w_order != nullptr, use_dist = P.w_dist != nullptr;
  const bool pre = P.affine != nullptr && use_order && use_dist;  // the producer's affine planes (acattn_problem.affine)
  const int combine_option = P.combine_option;

  // ---- per-key additive mask, first / last real item, key tiles that can carry mass (acattn_long_common.h) ----------------
  int first_valid, last_valid;
  long_key_mask_table(P, structured, dense_ll, L, LP, rowbase, lane, s_km, first_valid, last_valid);
  const int nt = long_tiles_of_block(structured, causal, nT, qb, first_valid, last_valid);

  // ---- descriptors, query fragments, query halves of the affines ---------------------------------------------------------
  const int seq_bytes = L * H * 4, H4 = H * 4;
  const rsrc_t rK = make_rsrc(P.k + rowbase * H, seq_bytes);
  const rsrc_t rKa = make_rsrc((ADV ? P.ka : P.k) + rowbase * H, seq_bytes);
  const float* const planes = pre ? P.affine + bh * 4 * LP + 4 * g : nullptr;  // (per lane: a vector register pair)
  const int koff = (c * H + hoff + KS * g) * 4;    // row c of a key tile, this lane's slice of the head
  const float* const vcol = P.v + rowbase * H + hoff + c;  // column c of the head (per lane), rows by key index
  float qf[KS], qaf[KS];
  {
    const rsrc_t rQ = make_rsrc(P.q + rowbase * H, seq_bytes);
    const rsrc_t rQa = make_rsrc((ADV ? P.qa : P.q) + rowbase * H, seq_bytes);
    const int qoff = (i * H + hoff + KS * g) * 4;  // rows past L: out of range, zeros
#pragma unroll
    for (int s4 = 0; s4 < KS / 4; ++s4) {
      const f4 tq = bload4(rQ, qoff + 16 * s4);
      f4 ta = tq;
      if (ADV) ta = bload4(rQa, qoff + 16 * s4);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        qf[4 * s4 + e] = tq[e];
        qaf[4 * s4 + e] = ta[e];
      }
    }
  }
  // sigmoid(o) = 1 / (1 + exp2(ao2 + co2)): both halves of the order affine carry -log2(e), as the planes do
  float wko[KS], wkd[KS];
  float ao2 = 0.f, ad = 0.f;
  if (pre) {
    const float* pq = P.affine + bh * 4 * LP + min(i, LP - 1);
    ao2 = pq[0];
    ad = pq[LP];
#pragma unroll
    for (int s = 0; s < KS; ++s) wko[s] = wkd[s] = 0.f;
  } else {
    float ao = 0.f;
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      ao += qf[s] * (use_order ? P.w_order[KS * g + s] : 0.f);
      ad += qf[s] * (use_dist ? P.w_dist[KS * g + s] : 0.f);
      wko[s] = use_order ? P.w_order[DH + KS * g + s] * -kLog2e : 0.f;
      wkd[s] = use_dist ? P.w_dist[DH + KS * g + s] : 0.f;
    }
    ao2 = -kLog2e * (quad_sum(ao) + (use_order ? P.b_order[0] : 0.f));
    ad = quad_sum(ad) + (use_dist ? P.b_dist[0] : 0.f);
  }
  const float sc = use_dist ? P.scalar[0] : 0.f;
  float hs2 = 0.5f * (sc * sc);
  float inv_sqrt = 1.0f / sqrtf((float)DH);
  const bool has_drop = P.p_drop > 0.f;
  float keep_scale = has_drop ? 1.0f / (1.0f - P.p_drop) : 1.0f;
  const bool counter = P.rng_mode == ACATTN_RNG_COUNTER;
  RngKey rkey = rng_key(P.seed + (P.seed_device ? *P.seed_device : 0ull));
  const uint32_t rng_row = (uint32_t)(bh * L + i);
  // row pointers into the [B, nh, L, L] / [B, L, L] tensors (64-bit; rows past L are never dereferenced)
  const size_t prow = (bh * L + (row_ok ? i : 0)) * (size_t)L;
  const float* mask_row = dense_ll ? P.mask + (rowbase + (row_ok ? i : 0)) * L : nullptr;
  const float* noise_row = (ADV && !counter && P.noise) ? P.noise + prow : nullptr;
  const uint8_t* keepa_row = (has_drop && !counter && P.keep_after) ? P.keep_after + prow : nullptr;
  const uint8_t* keepm_row = (ADV && has_drop && !counter && P.keep_mask) ? P.keep_mask + prow : nullptr;
  // output rows of this lane, formed once (the four pointers of acattn_fwd_out would otherwise sit in scalar registers
  // from the first instruction to the last store)
  float* out_cal = O.ctx_calibrated + (rowbase + (row_ok ? i : 0)) * H + hoff + 4 * g;
  float* out_att = ADV ? O.ctx_attacked + (rowbase + (row_ok ? i : 0)) * H + hoff + 4 * g : nullptr;
  float* m_row = ADV ? O.attack_mask + prow : nullptr;
  float* stat_row = O.row_stats ? O.row_stats + (bh * L + (row_ok ? i : 0)) * ACATTN_NSTAT : nullptr;
  VREG(out_cal);
  VREG(out_att);
  VREG(m_row);
  VREG(stat_row);
  // The scalar register file is the tight one here (four buffer descriptors, the kernel arguments, the loop state): wave-
  // uniform values that only feed vector arithmetic live in vector registers, of which there are plenty.
  VREG(inv_sqrt);
  VREG(hs2);
  VREG(keep_scale);
  VREG(rkey.a);
  VREG(rkey.b);

  // ---- one key tile: the two level-1 arguments x (after_spatial) and y (attack mask) and the additive mask ---------------
  auto tile_scores = [&](const int t, f4& x, f4& y, f4& mk) {
    const int ko = koff + 16 * t * H4;
    f4 k4[KS / 4], ka4[KS / 4];
#pragma unroll
    for (int s4 = 0; s4 < KS / 4; ++s4) {
      k4[s4] = bload4(rK, ko + 16 * s4);  // keys past L: zeros
      if (ADV) ka4[s4] = bload4(rKa, ko + 16 * s4);
    }
    const int j0 = 16 * t + 4 * g;
    f4 co4 = {0.f, 0.f, 0.f, 0.f}, cd4 = co4;
    if (pre) {
      co4 = *(const f4*)(planes + 2 * LP + 16 * t);  // (the planes are padded to whole tiles)
      cd4 = *(const f4*)(planes + 3 * LP + 16 * t);
    }
    f4 aS = {0.f, 0.f, 0.f, 0.f}, aM = aS;
#pragma unroll
    for (int s4 = 0; s4 < KS / 4; ++s4)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        aS = mfma16(k4[s4][e], qf[4 * s4 + e], aS);
        if (ADV) aM = mfma16(ka4[s4][e], qaf[4 * s4 + e], aM);
      }
    if (!pre && (use_order || use_dist)) {
      // key halves of the affines: lane c holds key 16 t + c; the sum over the head meets in the four lanes of the key,
      // and every lane then fetches the values of ITS four keys 4 g + r
      float co = 0.f, cd = 0.f;
#pragma unroll
      for (int s4 = 0; s4 < KS / 4; ++s4)
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
    const f4 km4 = *(const f4*)(s_km + j0);
    f4 md = {0.f, 0.f, 0.f, 0.f};
    if (dense_ll) md = load_seg(mask_row, j0, L, row_ok);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int j = j0 + r;
      float m = km4[r];
      if (causal && j > i) m = fminf(m, ACATTN_MASK_FILL);
      if (dense_ll && j < L) m = md[r];
      float s = aS[r];
      if (use_order) {  // layers.py:715-719
        const float pr = fast_rcp(1.0f + ex2(ao2 + co4[r]));
        const float val = (j > i) ? pr : 1.0f - pr;
        s += fast_log(val + ACATTN_LOG_EPS);
      }
      if (use_dist) {  // layers.py:721-727
        const float df = fast_log((float)(abs(i - j) + 1)) - (ad + cd4[r]);
        s -= (df * df) * hs2;
      }
      x[r] = s * inv_sqrt + m;  // layers.py:732-734
      y[r] = aM[r] * inv_sqrt + m;
      mk[r] = m;
    }
  };
  // the tile's randomness: noise and the keep bits of the two dropouts
  auto tile_draws = [&](const int t, f4& nz, uint32_t& ka, uint32_t& km) {
    nz = f4{0.f, 0.f, 0.f, 0.f};
    ka = km = 0xFu;
    if (!(ADV || has_drop)) return;
    const int j0 = 16 * t + 4 * g;
    if (counter) {
      const RngGroup rg = rng_group(rkey, rng_row, (uint32_t)(4 * t + g), P.p_drop);
      nz = rg.n;
      if (has_drop) {
        ka = rg.keep_after;
        km = rg.keep_mask;
      }
    } else {
      if (noise_row) nz = load_seg(noise_row, j0, L, row_ok);
      if (keepa_row) ka = load_keep(keepa_row, j0, L, row_ok);
      if (keepm_row) km = load_keep(keepm_row, j0, L, row_ok);
    }
  };
  // P = dropout(softmax(x)), M = dropout(softmax(y)) of the tile from the finished normalisers   layers.py:735-736, 670-672
  // (ma, rza: the row's maximum and keep_scale / sum, kept apart: folded into one log-normaliser a fully masked row's
  // -10000 would round the pair to 1e-3)
  auto dropped = [&](const f4 a, const float ma, const float rza, const uint32_t keep) {
    f4 o;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float e = fast_exp(a[r] - ma) * rza;  // keys past L: exp(-inf) = 0
      o[r] = ((keep >> r) & 1u) ? e : 0.f;
    }
    return o;
  };
  // acc += V_tile^T . e^T : lane (c, g), register rr of acc[dt]  =  ctx[query c][16 dt + 4 g + rr]
  auto add_context = [&](const int t, const f4 e, f4 (&acc)[DT]) {
    float vf[4][DT];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = 16 * t + 4 * g + r;
      const float* vp = vcol + min(row, L - 1) * H;
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) {
        const float v = vp[16 * dt];
        vf[r][dt] = row < L ? v : 0.f;  // keys past L: zeros
      }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) acc[dt] = mfma16(vf[r][dt], e[r], acc[dt]);
  };

  // ---- sweep 1: online max and sum of the two level-1 rows ----------------------------------------------------------------
  float mxl = ACATTN_NEG_INF, zxl = 0.f, myl = ACATTN_NEG_INF, zyl = 0.f, shl = ACATTN_NEG_INF;
#pragma unroll 1
  for (int t = 0; t < nt; ++t) {
    f4 x, y, mk;
    tile_scores(t, x, y, mk);
    shl = fmaxf(shl, max4(mk));
    {
      const float mn = fmaxf(mxl, max4(x)), ms = finite_or_zero(mn);
      float z = 0.f;
#pragma unroll
      for (int r = 0; r < 4; ++r) z += fast_exp(x[r] - ms);
      zxl = zxl * fast_exp(mxl - ms) + z;
      mxl = mn;
    }
    if (ADV) {
      const float mn = fmaxf(myl, max4(y)), ms = finite_or_zero(mn);
      float z = 0.f;
#pragma unroll
      for (int r = 0; r < 4; ++r) z += fast_exp(y[r] - ms);
      zyl = zyl * fast_exp(myl - ms) + z;
      myl = mn;
    }
  }
  const float mx = finite_or_zero(quad_max(mxl));
  const float zx = quad_sum(zxl * fast_exp(mxl - mx));
  const float lx = mx + fast_log(zx), rzx = fast_rcp(zx) * keep_scale;
  float my = 0.f, ly = 0.f, rzy = 1.0f;
  if (ADV) {
    my = finite_or_zero(quad_max(myl));
    const float zy = quad_sum(zyl * fast_exp(myl - my));
    ly = my + fast_log(zy);
    rzy = fast_rcp(zy) * keep_scale;
  }
  const float row_shift = finite_or_zero(quad_max(shl));  // 0 when the row has an unmasked key, else -10000

  float stat[ACATTN_NSTAT];
#pragma unroll
  for (int s = 0; s < ACATTN_NSTAT; ++s) stat[s] = 0.f;
  stat[0] = lx;
  f4 cc[DT];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) cc[dt] = f4{0.f, 0.f, 0.f, 0.f};

  if constexpr (!ADV) {
    // ---- spatial calibrator only: ctx = after_spatial . V ----------------------------------------------------------------
#pragma unroll 1
    for (int t = 0; t < nt; ++t) {
      f4 x, y, mk, nz;
      uint32_t ka, km;
      tile_scores(t, x, y, mk);
      tile_draws(t, nz, ka, km);
      add_context(t, dropped(x, mx, rzx, ka), cc);
    }
  } else {
    stat[1] = ly;
    // ---- sweep 2: M out; perturbed attention softmax(P M + n (1 - M) + mask) with its context; sum of A_c ----------------
    f4 ca[DT];
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) ca[dt] = f4{0.f, 0.f, 0.f, 0.f};
    float mu = ACATTN_NEG_INF, zul = 0.f, zvl = 0.f;
#pragma unroll 1
    for (int t = 0; t < nt; ++t) {
      f4 x, y, mk, nz;
      uint32_t ka, km;
      tile_scores(t, x, y, mk);
      tile_draws(t, nz, ka, km);
      const f4 p = dropped(x, mx, rzx, ka), m = dropped(y, my, rzy, km);
      store_seg(m_row, 16 * t + 4 * g, L, row_ok, m);
      const f4 u = (p * m + nz * (1.0f - m)) + mk;  // layers.py:918-919
      const float mn = fmaxf(mu, quad_max(max4(u))), ms = finite_or_zero(mn);
      const float alpha = fast_exp(mu - ms);  // the row's earlier tiles were taken relative to the old maximum
      mu = mn;
      f4 eu, ev;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        eu[r] = fast_exp(u[r] - ms);
        // layers.py:920-921; arguments lie in [0, e * keep_scale] + mask: shifted by the row's mask maximum
        ev[r] = fast_exp((p[r] * fast_exp(1.0f - m[r]) + mk[r]) - row_shift);
      }
      zul = zul * alpha + hsum(eu);
      zvl += hsum(ev);
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) ca[dt] *= alpha;
      add_context(t, eu, ca);
    }
    for (int t = nt; t < nT; ++t) store_seg(m_row, 16 * t + 4 * g, L, row_ok, f4{0.f, 0.f, 0.f, 0.f});
    const float zu = quad_sum(zul), zv = quad_sum(zvl);
    stat[2] = finite_or_zero(mu) + fast_log(zu);
    stat[3] = row_shift + fast_log(zv);
    const float rzu = fast_rcp(zu), rzv = fast_rcp(zv);
    if (row_ok) {
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) *(f4*)(out_att + 16 * dt) = ca[dt] * rzu;
    }

    // P and the calibrated attention A_c of a tile, rebuilt (sweeps F and 3)
    auto tile_pac = [&](const int t, f4& p, f4& ac, f4& mk) {
      f4 x, y, nz;
      uint32_t ka, km;
      tile_scores(t, x, y, mk);
      tile_draws(t, nz, ka, km);
      p = dropped(x, mx, rzx, ka);
      const f4 m = dropped(y, my, rzy, km);
#pragma unroll
      for (int r = 0; r < 4; ++r) ac[r] = fast_exp((p[r] * fast_exp(1.0f - m[r]) + mk[r]) - row_shift) * rzv;
    };
    // ---- combine FIXED: the inner softmax(P + A_c / 2) carries NO mask (layers.py:885): every key < L takes part, the
    // skipped tiles (P = A_c = 0) with exp(0) each -------------------------------------------------------------------------
    float rzf = 1.0f;
    if (combine_option == ACATTN_COMBINE_FIXED) {
      float zfl = 0.f;
#pragma unroll 1
      for (int t = 0; t < nt; ++t) {
        f4 p, ac, mk;
        tile_pac(t, p, ac, mk);
#pragma unroll
        for (int r = 0; r < 4; ++r) zfl += (16 * t + 4 * g + r < L) ? fast_exp(p[r] + 0.5f * ac[r]) : 0.f;
      }
      const float zf = quad_sum(zfl) + (float)(L - min(L, 16 * nt));
      stat[5] = fast_log(zf);
      rzf = fast_rcp(zf);
    }
    // ---- sweep 3: combine (layers.py:883-896), final soft-max (:925) and the calibrated context ---------------------------
    const float* gate_row = combine_option == ACATTN_COMBINE_GATE ? P.gate_logits + (rowbase + (row_ok ? i : 0)) * L : nullptr;
    float rate = P.anneal_rate;
    VREG(rate);
    float zwl = 0.f;
#pragma unroll 1
    for (int t = 0; t < nt; ++t) {
      f4 p, ac, mk, cb;
      tile_pac(t, p, ac, mk);
      if (combine_option == ACATTN_COMBINE_FIXED) {
#pragma unroll
        for (int r = 0; r < 4; ++r) cb[r] = fast_exp(p[r] + 0.5f * ac[r]) * rzf;
      } else if (combine_option == ACATTN_COMBINE_GATE) {
        const f4 gt = gate_value(load_seg(gate_row, 16 * t + 4 * g, L, row_ok), P.gate_is_prob);
        cb = gt * p + (1.0f - gt) * ac;
      } else {
        cb = rate * p + (1.0f - rate) * ac;
      }
      f4 ew;
#pragma unroll
      for (int r = 0; r < 4; ++r) ew[r] = fast_exp((cb[r] + mk[r]) - row_shift);
      zwl += hsum(ew);
      add_context(t, ew, cc);
    }
    const float zw = quad_sum(zwl);
    stat[4] = row_shift + fast_log(zw);
    const float rzw = fast_rcp(zw);
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) cc[dt] *= rzw;
  }

  // ---- contexts (head-merged [B, L, H]) and the row statistics ---------------------------------------------------------------
  if (row_ok) {
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) *(f4*)(out_cal + 16 * dt) = cc[dt];
    if (stat_row && g == 0) {
      float* sp = stat_row;
      *(f4*)sp = f4{stat[0], stat[1], stat[2], stat[3]};
      *(f4*)(sp + 4) = f4{stat[4], stat[5], stat[6], stat[7]};
    }
  }
}

template <int DH>
int launch_long(const acattn_problem& p, const acattn_fwd_out& o, hipStream_t stream) {
  const int nT = (p.L + 15) / 16;
  const dim3 grid(p.B * p.n_heads * nT), block(64);
  const size_t lds = (size_t)16 * nT * sizeof(float);
  if (p.adversarial)
    hipLaunchKernelGGL((acattn_long_fwd_kernel<DH, true>), grid, block, lds, stream, p, o);
  else
    hipLaunchKernelGGL((acattn_long_fwd_kernel<DH, false>), grid, block, lds, stream, p, o);
  return (int)hipGetLastError();
}

}  // namespace

#define ACATTN_CAT2(a, b) a##b
#define ACATTN_CAT(a, b) ACATTN_CAT2(a, b)
int ACATTN_CAT(acattn_launch_long_fwd_dh, ACATTN_LONG_DH)(const acattn_problem& p, const acattn_fwd_out& o, hipStream_t stream) {
  return launch_long<ACATTN_LONG_DH>(p, o, stream);
}
