// The six projections in front of the attention core as ONE launch, forward and backward (input gradients), gfx950:
//
//     mq, mk, mv = query(x), key(x), value(x)                               recbole/model/layers.py:687-689
//     qa, ka     = attack_query_transform(mq), attack_key_transform(mk)     layers.py:658-659
//     gate       = gate(mq)                                                 layers.py:887 (combine_option 'gate')
//
// As library GEMMs these are six launches of 8-9 us forward and six more per backward walk, each re-reading x / mq /
// mk from HBM.  Here one wave owns 16 (or 32) rows: x is read once, mq and mk never leave the registers between the
// product that makes them and the products that consume them.  Same register-chain scheme as acattn_tail.hip: every
// product is computed transposed (out^T = W . in^T, exact-fp32 16x16x4 MFMA) so an accumulator is directly the B
// operand of the next product; the weight fragment of an output tile is one 16-byte load per lane, the next
// product's fragments are requested before the current product's MFMAs.
//
// Backward: dmq_t = dmq + dqa . Waq + dgate . Wg,  dmk_t = dmk + dka . Wak,  dx = dmq_t . Wq + dmk_t . Wk + dmv . Wv
// with the transposed weights gathered as dwords from the row-major parameters.  dmq_t / dmk_t are written because
// they are the cotangent operands of the query / key weight gradients (acattn_linear_wgrad_grouped).
//
// At hidden 64 these kernels are the exact-fp32 form (acattn_linear_products(0)); by default the same chains run on
// split bf16 products (proj_split_fwd_kernel / proj_split_bwd_kernel below).
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <type_traits>

#include "acattn_common.h"
#include "acattn_split.h"
#include "acattn_wstage.h"

namespace {

template <int NB>
struct Rows {
  int row[NB];
  bool ok[NB];
};

template <int NB>
__device__ __forceinline__ Rows<NB> wave_rows(int R) {
  Rows<NB> w;
  const int c = threadIdx.x & 15;
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) {
    const int r = (blockIdx.x * NB + nb) * 16 + c;
    w.ok[nb] = r < R;
    w.row[nb] = r < R ? r : R - 1;
  }
  return w;
}

// A fragments of out^T = W . in^T for all output tiles: lane (c, g) holds W[16nt + c][16t + 4g .. +3]
template <int DT>
__device__ __forceinline__ void load_weight(const float* w, int H, int n_out, int c, int g, f4 (&frag)[DT][DT]) {
#pragma unroll
  for (int nt = 0; nt < DT; ++nt) {
    const int o = min(16 * nt + c, n_out - 1);
#pragma unroll
    for (int t = 0; t < DT; ++t) frag[nt][t] = *(const f4*)(w + (size_t)o * H + 16 * t + 4 * g);
  }
}

// A fragments of in_grad^T = W^T . out_grad^T for a square [H, H] weight: lane (c, g) holds W[16t + 4g + r][16nt + c],
// r = 0..3 (dword gathers, unconditional: a range check per element becomes a branch per load)
template <int DT>
__device__ __forceinline__ void load_weight_t(const float* w, int c, int g, f4 (&frag)[DT][DT]) {
  constexpr int H = 16 * DT;
  // contraction group t = DT - 1 is requested last: the product that starts with it has waited for the whole set
#pragma unroll
  for (int t = 0; t < DT; ++t)
#pragma unroll
    for (int nt = 0; nt < DT; ++nt)
#pragma unroll
      for (int r = 0; r < 4; ++r) frag[nt][t][r] = w[(16 * t + 4 * g + r) * H + 16 * nt + c];
}

// contraction groups [T0, T1) of the product (all of it by default)
template <int DT, int NB, int T0 = 0, int T1 = DT>
__device__ __forceinline__ void product(const f4 (&w)[DT][DT], const f4 (&in)[NB][DT], f4 (&acc)[NB][DT]) {
#pragma unroll
  for (int t = T0; t < T1; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int nt = 0; nt < DT; ++nt)
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) acc[nb][nt] = mfma16(w[nt][t][r], in[nb][t][r], acc[nb][nt]);
}

template <int DT, int NB>
__device__ __forceinline__ void init_bias(const float* bias, int n_out, int g, f4 (&acc)[NB][DT]) {
#pragma unroll
  for (int nt = 0; nt < DT; ++nt) {
    f4 b;
#pragma unroll
    for (int r = 0; r < 4; ++r) b[r] = bias[min(16 * nt + 4 * g + r, n_out - 1)];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) acc[nb][nt] = b;
  }
}

template <int DT, int NB>
__device__ __forceinline__ void store_rows(float* out, const Rows<NB>& W, int g, const f4 (&v)[NB][DT]) {
  constexpr int H = 16 * DT;
#pragma unroll
  for (int nb = 0; nb < NB; ++nb)
    if (W.ok[nb])
#pragma unroll
      for (int t = 0; t < DT; ++t) *(f4*)(out + (size_t)W.row[nb] * H + 16 * t + 4 * g) = v[nb][t];
}

template <int DT, int NB>
__device__ __forceinline__ void load_rows(const float* in, const Rows<NB>& W, int g, f4 (&v)[NB][DT]) {
  constexpr int H = 16 * DT;
#pragma unroll
  for (int nb = 0; nb < NB; ++nb)
#pragma unroll
    for (int t = 0; t < DT; ++t) v[nb][t] = *(const f4*)(in + (size_t)W.row[nb] * H + 16 * t + 4 * g);
}

// bias of a full-width product in accumulator layout: lane (c, g) holds b[16nt + 4g .. +3]
template <int DT>
__device__ __forceinline__ void load_bias(const float* bias, int g, f4 (&b)[DT]) {
#pragma unroll
  for (int nt = 0; nt < DT; ++nt) b[nt] = *(const f4*)(bias + 16 * nt + 4 * g);
}

template <int DT, int NB>
__device__ __forceinline__ void set_rows(const f4 (&b)[DT], f4 (&acc)[NB][DT]) {
#pragma unroll
  for (int nb = 0; nb < NB; ++nb)
#pragma unroll
    for (int nt = 0; nt < DT; ++nt) acc[nb][nt] = b[nt];
}


// Rank-1 halves of the spatial calibrator's affines (layers.py:705-708) for the rows of this wave, from the projected
// rows still in the accumulators (v[nb][nt][r] = value[row c][feature 16 nt + 4 g + r]):
//     plane P0     [i] = -log2(e) (v_i . w_order[woff : woff + dh] + bias_o)
//     plane P0 + 1 [i] =           v_i . w_dist [woff : woff + dh] + bias_d
// into affine[b, head, plane, i] (acattn_problem.affine).  Query halves: woff = 0, biases, P0 = 0; key halves: woff =
// dh, no bias, P0 = 2.
template <int DT, int NB>
__device__ __forceinline__ void write_affine(const f4 (&v)[NB][DT], const Rows<NB>& W, const acattn_proj_problem& P, float* affine,
                                             int woff, float bias_o, float bias_d, int P0, int c, int g) {
  constexpr float kL2e = 1.44269504088896340736f;
  const int nh = P.n_heads, dh = (16 * DT) / nh, tph = dh >> 4;  // 16-feature tiles per head
  const int LP = ((P.L + 15) >> 4) << 4;
  // the two vectors' tiles: all requested up front where the registers allow it (hidden <= 128), else tile by tile
  constexpr int PRE = DT <= 8 ? DT : 1;
  f4 wo_[PRE], wd_[PRE];
  if constexpr (DT <= 8) {
#pragma unroll
    for (int nt = 0; nt < DT; ++nt) {
      const int f0 = woff + (16 * nt) % dh + 4 * g;
      wo_[nt] = *(const f4*)(P.w_order + f0);
      wd_[nt] = *(const f4*)(P.w_dist + f0);
    }
  }
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) {
    const int row = W.row[nb], b = row / P.L, i = row - b * P.L;
    float so = 0.f, sd = 0.f;
#pragma unroll
    for (int nt = 0; nt < DT; ++nt) {
      f4 wo, wd;
      if constexpr (DT <= 8) {
        wo = wo_[nt];
        wd = wd_[nt];
      } else {
        const int f0 = woff + (16 * nt) % dh + 4 * g;
        wo = *(const f4*)(P.w_order + f0);
        wd = *(const f4*)(P.w_dist + f0);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        so = fmaf(v[nb][nt][r], wo[r], so);
        sd = fmaf(v[nb][nt][r], wd[r], sd);
      }
      if ((nt + 1) % tph == 0) {  // head complete (wave-uniform)
        const float o = quad_sum(so), d = quad_sum(sd);
        if (g == 0 && W.ok[nb]) {
          float* pl = affine + ((size_t)(b * nh + nt / tph) * 4 + P0) * LP + i;
          pl[0] = -kL2e * (o + bias_o);
          pl[LP] = d + bias_d;
        }
        so = 0.f;
        sd = 0.f;
      }
    }
  }
}

template <int H, int NB>
__global__ void __launch_bounds__(64) proj_fwd_kernel(const acattn_proj_problem P, const acattn_proj_out O) {
  constexpr int DT = H / 16;
  const int c = threadIdx.x & 15, g = threadIdx.x >> 4;
  const Rows<NB> W = wave_rows<NB>(P.rows);
  f4 xb[NB][DT];
  f4 wa[DT][DT], wb[DT][DT];  // two fragment sets: a product's weights are requested two products ahead
  f4 ba[DT], bb[DT];          // ... and its bias with them
  f4 m[NB][DT], acc[NB][DT];

  load_rows<DT, NB>(P.x, W, g, xb);
  load_weight<DT>(P.wq, H, H, c, g, wa);
  load_bias<DT>(P.bq, g, ba);
  PIN_ORDER();
  load_weight<DT>(P.waq, H, H, c, g, wb);
  load_bias<DT>(P.baq, g, bb);
  PIN_ORDER();
  set_rows<DT, NB>(ba, m);
  product<DT, NB>(wa, xb, m);  // mq
  store_rows<DT, NB>(O.mq, W, g, m);
  if (O.affine) write_affine<DT, NB>(m, W, P, O.affine, 0, P.b_order[0], P.b_dist[0], 0, c, g);
  load_weight<DT>(P.wk, H, H, c, g, wa);
  load_bias<DT>(P.bk, g, ba);
  PIN_ORDER();
  set_rows<DT, NB>(bb, acc);
  product<DT, NB>(wb, m, acc);  // qa = attack_query_transform(mq)
  store_rows<DT, NB>(O.qa, W, g, acc);
  if (P.wg) {
    // gate logits [rows, G], G = seq_length (50 ... 200): one 16-wide output tile at a time, weight rows requested
    // two tiles ahead
    const int GT = (P.G + 15) >> 4;
    f4 gw[3][DT], gb[3];
    auto load_tile = [&](int nt, f4 (&w)[DT], f4& b) {
      nt = min(nt, GT - 1);
      const int o = min(16 * nt + c, P.G - 1);
#pragma unroll
      for (int t = 0; t < DT; ++t) w[t] = *(const f4*)(P.wg + (size_t)o * H + 16 * t + 4 * g);
#pragma unroll
      for (int r = 0; r < 4; ++r) b[r] = P.bg[min(16 * nt + 4 * g + r, P.G - 1)];
    };
    // tile nt from buffer `cur`, tile nt + 2 requested into the buffer tile nt - 1 has left (the three buffers change
    // roles from step to step: a register copy would have to wait for the load it copies)
    auto gate_step = [&](int nt, const f4 (&cw)[DT], const f4& cb, f4 (&fw)[DT], f4& fb) {
      load_tile(nt + 2, fw, fb);
      PIN_ORDER();
      f4 ga[NB][2];
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) {
        ga[nb][0] = cb;
        ga[nb][1] = f4{0.f, 0.f, 0.f, 0.f};
      }
#pragma unroll
      for (int t = 0; t < DT; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
          for (int nb = 0; nb < NB; ++nb) ga[nb][r & 1] = mfma16(cw[t][r], m[nb][t][r], ga[nb][r & 1]);
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) {
        f4 v = ga[nb][0] + ga[nb][1];
        if (O.gate_prob) v = gate_value(v, 0);  // sigmoid once per (b, i, j): the heads share it (layers.py:887)
        // the lane's four logits are consecutive in the row: one (dword-aligned) 16-byte store, not four scattered ones
        const int j0 = 16 * nt + 4 * g;
        float* dst = O.gate + (size_t)W.row[nb] * P.G + j0;
        if (W.ok[nb] && j0 + 3 < P.G) {
          *(f4u*)dst = v;
        } else if (W.ok[nb]) {
#pragma unroll
          for (int r = 0; r < 4; ++r)
            if (j0 + r < P.G) dst[r] = v[r];
        }
      }
      PIN_ORDER();
    };
    load_tile(0, gw[0], gb[0]);
    load_tile(1, gw[1], gb[1]);
    // straight-line code for the 16 possible tiles (G <= 256): around a back edge the wait-count insertion drains every
    // request at the loop header
    static_for<16>([&](auto k) {
      constexpr int K = decltype(k)::value;
      if (K < GT) gate_step(K, gw[K % 3], gb[K % 3], gw[(K + 2) % 3], gb[(K + 2) % 3]);
    });
  }
  load_weight<DT>(P.wak, H, H, c, g, wb);
  load_bias<DT>(P.bak, g, bb);
  PIN_ORDER();
  set_rows<DT, NB>(ba, m);
  product<DT, NB>(wa, xb, m);  // mk
  store_rows<DT, NB>(O.mk, W, g, m);
  if (O.affine) write_affine<DT, NB>(m, W, P, O.affine, H / P.n_heads, 0.f, 0.f, 2, c, g);
  load_weight<DT>(P.wv, H, H, c, g, wa);
  load_bias<DT>(P.bv, g, ba);
  PIN_ORDER();
  set_rows<DT, NB>(bb, acc);
  product<DT, NB>(wb, m, acc);  // ka = attack_key_transform(mk)
  store_rows<DT, NB>(O.ka, W, g, acc);
  set_rows<DT, NB>(ba, acc);
  product<DT, NB>(wa, xb, acc);  // mv
  store_rows<DT, NB>(O.mv, W, g, acc);
}

// MODE fixes which cotangents exist at compile time (a run-time test around a request makes the wait-count insertion
// assume the shorter path and drain every load in flight): 1 = all of them (the calibrated-loss walk), 2 = dqa and dka
// only (the attacked-loss walk: everything but the attack transforms is frozen), 0 = whatever IO says.
template <int H, int NB, int MODE>
__global__ void __launch_bounds__(64) proj_bwd_kernel(const acattn_proj_problem P, const acattn_proj_bwd_io IO) {
  constexpr int DT = H / 16;
  const bool h_dmq = MODE == 1 || (MODE == 0 && IO.dmq), h_dmk = MODE == 1 || (MODE == 0 && IO.dmk);
  const bool h_dmv = MODE == 1 || (MODE == 0 && IO.dmv);
  const bool h_dqa = MODE != 0 || IO.dqa, h_dka = MODE != 0 || IO.dka, h_dx = MODE != 0 || IO.dx;
  const bool h_qt = MODE != 0 || IO.dmq_total, h_kt = MODE != 0 || IO.dmk_total;
  const int c = threadIdx.x & 15, g = threadIdx.x >> 4;
  const Rows<NB> W = wave_rows<NB>(P.rows);
  // Two fragment sets.  A product's transposed weights are 64 dword gathers and s_waitcnt counts at most 63 requests,
  // so the next product's requests go out AFTER the current product's first MFMAs (whose wait then has nothing newer
  // behind it) and have the rest of that product to arrive.
  // Order of the products: Waq^T (A), gate tiles, Wq^T (B), Wak^T (A), Wk^T (B), Wv^T (A).
  f4 wa[DT][DT], wb[DT][DT];
  f4 in[NB][DT], dq[NB][DT], dk[NB][DT], dx[NB][DT];
  auto zero = [&](f4 (&v)[NB][DT]) {
#pragma unroll
    for (int nb = 0; nb < NB; ++nb)
#pragma unroll
      for (int t = 0; t < DT; ++t) v[nb][t] = f4{0.f, 0.f, 0.f, 0.f};
  };
  if (IO.dx_init && h_dx) load_rows<DT, NB>(IO.dx_init, W, g, dx); else zero(dx);  // the residual path's share of dx
  const bool gate = MODE != 2 && IO.dgate && P.wg;
  const int GT = gate ? (P.G + 15) >> 4 : 0;
  f4 gw[2][DT];   // gate tile: A[k = 16nt + c][j = 16 kt + 4g + r] = Wg[j][k]
  f4 gd[2][NB];   //            B[j][row] = dgate[row][j]
  auto load_tile = [&](int kt, f4 (&w)[DT], f4 (&d)[NB]) {
    kt = min(kt, GT - 1);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int j = 16 * kt + 4 * g + r;
      const float live = j < P.G ? 1.f : 0.f;  // the clamped element is loaded and multiplied away
      const int jc = min(j, P.G - 1);
#pragma unroll
      for (int nt = 0; nt < DT; ++nt) w[nt][r] = P.wg[(size_t)jc * H + 16 * nt + c] * live;
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) d[nb][r] = IO.dgate[(size_t)W.row[nb] * P.G + jc];
    }
  };

  // ---- d mq (total) = dmq + dqa . Waq + dgate . Wg;  dx += d mq . Wq ------------------------------------------------
  if (h_dmq) load_rows<DT, NB>(IO.dmq, W, g, dq); else zero(dq);
  if (h_dqa) {
    load_rows<DT, NB>(IO.dqa, W, g, in);
    load_weight_t<DT>(P.waq, c, g, wa);
  }
  PIN_ORDER();
  if (h_dqa) product<DT, NB, DT - 1, DT>(wa, in, dq);
  PIN_ORDER();
  if (h_dx) load_weight_t<DT>(P.wq, c, g, wb);
  if (gate) load_tile(0, gw[0], gd[0]);
  PIN_ORDER();
  if (h_dqa) product<DT, NB, 0, DT - 1>(wa, in, dq);
  if (gate) {
    // d mq += dgate . Wg: the contraction runs over the G gate outputs, 16 at a time, the next tile requested ahead
    auto gate_step = [&](int kt, const f4 (&cw)[DT], const f4 (&cd)[NB], f4 (&fw)[DT], f4 (&fd)[NB]) {
      load_tile(kt + 1, fw, fd);
      PIN_ORDER();
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int nt = 0; nt < DT; ++nt)
#pragma unroll
          for (int nb = 0; nb < NB; ++nb) dq[nb][nt] = mfma16(cw[nt][r], cd[nb][r], dq[nb][nt]);
      PIN_ORDER();
    };
    static_for<16>([&](auto k) {
      constexpr int K = decltype(k)::value;
      if (K < GT) gate_step(K, gw[K % 2], gd[K % 2], gw[(K + 1) % 2], gd[(K + 1) % 2]);
    });
  }
  if (h_qt) store_rows<DT, NB>(IO.dmq_total, W, g, dq);
  PIN_ORDER();
  if (h_dx) product<DT, NB, DT - 1, DT>(wb, dq, dx);
  PIN_ORDER();

  // ---- d mk (total) = dmk + dka . Wak;  dx += d mk . Wk + d mv . Wv ---------------------------------------------------
  if (h_dmk) load_rows<DT, NB>(IO.dmk, W, g, dk); else zero(dk);
  if (h_dka) {
    load_rows<DT, NB>(IO.dka, W, g, in);
    load_weight_t<DT>(P.wak, c, g, wa);
  }
  PIN_ORDER();
  if (h_dx) product<DT, NB, 0, DT - 1>(wb, dq, dx);
  PIN_ORDER();
  if (h_dka) product<DT, NB, DT - 1, DT>(wa, in, dk);
  PIN_ORDER();
  if (h_dx) load_weight_t<DT>(P.wk, c, g, wb);
  PIN_ORDER();
  if (h_dka) product<DT, NB, 0, DT - 1>(wa, in, dk);
  if (h_kt) store_rows<DT, NB>(IO.dmk_total, W, g, dk);
  if (h_dx) {
    PIN_ORDER();
    product<DT, NB, DT - 1, DT>(wb, dk, dx);
    PIN_ORDER();
    if (h_dmv) {
      load_rows<DT, NB>(IO.dmv, W, g, in);
      load_weight_t<DT>(P.wv, c, g, wa);
    }
    PIN_ORDER();
    product<DT, NB, 0, DT - 1>(wb, dk, dx);
    if (h_dmv) product<DT, NB>(wa, in, dx);
    store_rows<DT, NB>(IO.dx, W, g, dx);
  }
}

// =====================================================================================================================
// Hidden sizes 128 and 256 (BASELINE configs[3], [4]) [round 3].  The H = 64 kernels above hold a product's whole weight
// matrix as MFMA fragments (two sets of H^2 / 64 registers); at H = 128 that is 512 registers.  Here the weights STREAM:
// one 16-row output tile of W at a time (H / 16 float4 per lane), the next tile requested while the current one is on
// the matrix cores, two waves per SIMD covering what is left of the latency.  What stays in registers is what the chain
// needs: the input rows x, and mq / mk between the product that makes them and the products that consume them.  The
// backward uses the same streamed product on TRANSPOSED copies of the weights (a 0.5 MB workspace filled by
// transpose_weights_kernel in front of it: the dword gathers of the H = 64 backward would be 256 per product here).
// ---------------------------------------------------------------------------------------------------------------------
// timing-only probe builds (tools/probe/build_proj_variant.sh; results are WRONG with any of them):
//   ACATTN_PROJ_W0       every tile reads weight tile 0 (what the weight stream itself costs)
//   ACATTN_PROJ_NOSTORE  no output stores                (what the output traffic costs)
//   ACATTN_PROJ_NB1      one row block per wave at hidden 128
__device__ __forceinline__ void load_wchunk(const float* w, int ld, int n_out, int nt, int kc, int c, int g, f4 (&frag)[KT]) {
#ifdef ACATTN_PROJ_W0
  nt = 0;
#endif
#ifdef ACATTN_PROJ_COALESCED  // timing only: what a pre-swizzled weight layout (one contiguous KB per wave load) would cost
  const int ntc = min(nt, (n_out >> 4) - 1), lane = 16 * g + c, dt = ld / 16;
#pragma unroll
  for (int t = 0; t < KT; ++t) frag[t] = *(const f4*)(w + ((size_t)(ntc * dt + KT * kc + t) * 64 + lane) * 4);
  return;
#endif
  const int o = min(16 * nt + c, n_out - 1);
#pragma unroll
  for (int t = 0; t < KT; ++t) frag[t] = *(const f4*)(w + (size_t)o * ld + 16 * (KT * kc + t) + 4 * g);
}

template <int DT, int NB>
__device__ __forceinline__ void chunk_product(const f4 (&w)[KT], int kc, const f4 (&in)[NB][DT], f4 (&acc)[NB]) {
  static_for<DT / KT>([&](auto q) {  // kc is a run-time value in product_emit; the register index must not be
    constexpr int KC = decltype(q)::value;
    if (kc != KC) return;
#pragma unroll
    for (int t = 0; t < KT; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) acc[nb] = mfma16(w[t][r], in[nb][KT * KC + t][r], acc[nb]);
  });
}

// acc[nb][nt] (+)= W[16 nt ..][:] . in^T for nt = 0 .. DT - 1, kept in registers; the steps (tile, chunk) are unrolled
// (register arrays want compile-time indices), the weights one step ahead in two rotating buffers.  INIT: start from
// the bias instead of from what acc holds.
template <int DT, int NB, bool INIT>
__device__ __forceinline__ void product_keep(const float* w, const float* bias, int c, int g, const f4 (&in)[NB][DT],
                                             f4 (&acc)[NB][DT]) {
  constexpr int H = 16 * DT, KC = DT / KT;
  f4 wbuf[2][KT], bb[2];
  if constexpr (INIT) bb[0] = bias_tile(bias, H, 0, g);
  load_wchunk(w, H, H, 0, 0, c, g, wbuf[0]);
  static_for<DT * KC>([&](auto k) {
    constexpr int S = decltype(k)::value, NT = S / KC, C0 = S % KC;
    if constexpr (S + 1 < DT * KC) {
      if constexpr (INIT && (S + 1) % KC == 0) bb[((S + 1) / KC) & 1] = bias_tile(bias, H, (S + 1) / KC, g);
      load_wchunk(w, H, H, (S + 1) / KC, (S + 1) % KC, c, g, wbuf[(S + 1) & 1]);
    }
    PIN_ORDER();
    f4 a[NB];
    if constexpr (INIT && C0 == 0) {
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) a[nb] = bb[NT & 1];
    } else {
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) a[nb] = acc[nb][NT];
    }
    chunk_product<DT, NB>(wbuf[S & 1], C0, in, a);
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) acc[nb][NT] = a[nb];
  });
}

// the same for ceil(n_out / 16) output tiles that are only EMITTED (stored), tile index at run time; two steps per trip
// (two tiles at H = 128, the two chunks of one tile at H = 256)
template <int DT, int NB, class Emit>
__device__ __forceinline__ void product_emit(const float* w, int ld, const float* bias, int n_out, int c, int g,
                                             const f4 (&in)[NB][DT], Emit&& emit) {
  constexpr int KC = DT / KT;
  static_assert(KC == 1 || KC == 2, "hidden 128 or 256");
  const int n_tiles = (n_out + 15) >> 4;
  f4 wa[KT], wb[KT];
  f4 ba = bias_tile(bias, n_out, 0, g), bn;
  load_wchunk(w, ld, n_out, 0, 0, c, g, wa);
  if constexpr (KC == 1) {
    for (int nt = 0; nt < n_tiles; nt += 2) {
      bn = bias_tile(bias, n_out, min(nt + 1, n_tiles - 1), g);
      load_wchunk(w, ld, n_out, min(nt + 1, n_tiles - 1), 0, c, g, wb);
      PIN_ORDER();
      {
        f4 a[NB];
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) a[nb] = ba;
        chunk_product<DT, NB>(wa, 0, in, a);
        emit(nt, a);
      }
      ba = bias_tile(bias, n_out, min(nt + 2, n_tiles - 1), g);
      load_wchunk(w, ld, n_out, min(nt + 2, n_tiles - 1), 0, c, g, wa);
      PIN_ORDER();
      if (nt + 1 < n_tiles) {
        f4 a[NB];
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) a[nb] = bn;
        chunk_product<DT, NB>(wb, 0, in, a);
        emit(nt + 1, a);
      }
    }
  } else {
    for (int nt = 0; nt < n_tiles; ++nt) {
      load_wchunk(w, ld, n_out, nt, 1, c, g, wb);
      PIN_ORDER();
      f4 a[NB];
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) a[nb] = ba;
      chunk_product<DT, NB>(wa, 0, in, a);
      ba = bias_tile(bias, n_out, min(nt + 1, n_tiles - 1), g);
      load_wchunk(w, ld, n_out, min(nt + 1, n_tiles - 1), 0, c, g, wa);
      PIN_ORDER();
      chunk_product<DT, NB>(wb, 1, in, a);
      emit(nt, a);
    }
  }
}

#ifndef ACATTN_PROJ_WAVES
#define ACATTN_PROJ_WAVES 2
#endif
template <int H, int NB>
__global__ void __launch_bounds__(64, ACATTN_PROJ_WAVES) proj_wide_fwd_kernel(const acattn_proj_problem P, const acattn_proj_out O) {
  constexpr int DT = H / 16;
  const int c = threadIdx.x & 15, g = threadIdx.x >> 4;
  const Rows<NB> W = wave_rows<NB>(P.rows);
  f4 xb[NB][DT], m[NB][DT];
  load_rows<DT, NB>(P.x, W, g, xb);
  auto store_tile = [&](float* out, int ld, int n_out, int nt, const f4 (&a)[NB]) {
    const int j0 = 16 * nt + 4 * g;
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
      if (!W.ok[nb]) continue;
#ifdef ACATTN_PROJ_NOSTORE
      if (a[nb][0] != 12345.678f) continue;
#endif
      float* dst = out + (size_t)W.row[nb] * ld + j0;
      if (j0 + 3 < n_out) {
#ifdef ACATTN_PROJ_NT
        __builtin_nontemporal_store(a[nb], (f4u*)dst);
#else
        *(f4u*)dst = a[nb];
#endif
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (j0 + r < n_out) dst[r] = a[nb][r];
      }
    }
  };
  product_keep<DT, NB, true>(P.wq, P.bq, c, g, xb, m);  // mq
#ifdef ACATTN_PROJ_NOSTORE
  if (m[0][0][0] == 12345.678f)
#endif
  store_rows<DT, NB>(O.mq, W, g, m);
  if (O.affine) write_affine<DT, NB>(m, W, P, O.affine, 0, P.b_order[0], P.b_dist[0], 0, c, g);
  product_emit<DT, NB>(P.waq, H, P.baq, H, c, g, m, [&](int nt, const f4 (&a)[NB]) { store_tile(O.qa, H, H, nt, a); });
  if (P.wg) {
    product_emit<DT, NB>(P.wg, H, P.bg, P.G, c, g, m, [&](int nt, const f4 (&a)[NB]) {
      f4 v[NB];
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) v[nb] = O.gate_prob ? gate_value(a[nb], 0) : a[nb];  // sigmoid once for all heads
      store_tile(O.gate, P.G, P.G, nt, v);
    });
  }
  product_keep<DT, NB, true>(P.wk, P.bk, c, g, xb, m);  // mk
#ifdef ACATTN_PROJ_NOSTORE
  if (m[0][0][0] == 12345.678f)
#endif
  store_rows<DT, NB>(O.mk, W, g, m);
  if (O.affine) write_affine<DT, NB>(m, W, P, O.affine, H / P.n_heads, 0.f, 0.f, 2, c, g);
  product_emit<DT, NB>(P.wak, H, P.bak, H, c, g, m, [&](int nt, const f4 (&a)[NB]) { store_tile(O.ka, H, H, nt, a); });
  product_emit<DT, NB>(P.wv, H, P.bv, H, c, g, xb, [&](int nt, const f4 (&a)[NB]) { store_tile(O.mv, H, H, nt, a); });
}

// ---------------------------------------------------------------------------------------------------------------------
// The same products with the weights staged through LDS, once per WORKGROUP [round 3, second form].  Measured on the
// per-wave stream above (tools/gpu_pmc_proj.sh, probe builds): the matrix pipe is busy 39 % of the time, and neither the
// weight addresses (always tile 0: same time), nor their coalescing, nor the L2 matter -- a CU's vector memory path
// delivers ~10 B/clk (MI355X_MICROARCH.md, per-instruction constants) and eight waves each fetching 1 KB per 4 NB MFMAs
// ask for 16.  Here the four waves of a workgroup fetch each weight chunk ONCE (2 float4 per lane instead of 8), park it
// in LDS in fragment order (conflict-free ds_write_b128 / ds_read_b128, LDS delivers 128+ B/clk) and all read it from
// there: a quarter of the vector-memory traffic, one workgroup barrier per 32 NB MFMAs.
// ---------------------------------------------------------------------------------------------------------------------
// acc[nb][nt] (+)= W . in^T, kept in registers (see product_keep); `next` asks for the first chunk of whatever follows
template <int DT, int NB, bool INIT, class Next>
__device__ __forceinline__ void staged_keep(WeightStage& st, const float* w, const float* bias, const f4 (&in)[NB][DT],
                                            f4 (&acc)[NB][DT], Next&& next) {
  constexpr int H = 16 * DT, KC = DT / KT;
  static_for<DT * KC>([&](auto k) {
    constexpr int S = decltype(k)::value, NT = S / KC, C0 = S % KC;
    f4 frag[KT], b;
    st.fetch(frag, b);
    if constexpr (S + 1 < DT * KC)
      st.request(w, H, INIT ? bias : nullptr, H, (S + 1) / KC, (S + 1) % KC);
    else
      next();
    PIN_ORDER();
    f4 a[NB];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) a[nb] = (INIT && C0 == 0) ? b : acc[nb][NT];
    chunk_product<DT, NB>(frag, C0, in, a);
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) acc[nb][NT] = a[nb];
    PIN_ORDER();
    st.commit();
  });
}

// the same for ceil(n_out / 16) tiles that are only emitted (see product_emit)
template <int DT, int NB, class Emit, class Next>
__device__ __forceinline__ void staged_emit(WeightStage& st, const float* w, int ld, const float* bias, int n_out,
                                            const f4 (&in)[NB][DT], Emit&& emit, Next&& next) {
  constexpr int KC = DT / KT;
  const int n_tiles = (n_out + 15) >> 4;
  for (int nt = 0; nt < n_tiles; ++nt) {
    f4 a[NB];
#pragma unroll
    for (int kc = 0; kc < KC; ++kc) {
      f4 frag[KT], b;
      st.fetch(frag, b);
      if (kc + 1 < KC)
        st.request(w, ld, bias, n_out, nt, kc + 1);
      else if (nt + 1 < n_tiles)
        st.request(w, ld, bias, n_out, nt + 1, 0);
      else
        next();
      PIN_ORDER();
      if (kc == 0) {
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) a[nb] = b;
      }
      chunk_product<DT, NB>(frag, kc, in, a);
      PIN_ORDER();
      st.commit();
    }
    emit(nt, a);
  }
}

template <int NB>
__device__ __forceinline__ Rows<NB> wg_rows(int R, int wave) {
  Rows<NB> w;
  const int c = threadIdx.x & 15;
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) {
    const int r = ((blockIdx.x * NWV + wave) * NB + nb) * 16 + c;
    w.ok[nb] = r < R;
    w.row[nb] = r < R ? r : R - 1;
  }
  return w;
}

template <int H, int NB>
__global__ void __launch_bounds__(64 * NWV, ACATTN_PROJ_WAVES) proj_staged_fwd_kernel(const acattn_proj_problem P, const acattn_proj_out O) {
  constexpr int DT = H / 16;
  __shared__ f4 stage_lds[2 * STAGE_F4];
  WeightStage st;
  st.lds = stage_lds;
  st.par = 0;
  st.lane = threadIdx.x & 63;
  st.wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  st.c = threadIdx.x & 15;
  st.g = (threadIdx.x >> 4) & 3;
  const int c = st.c, g = st.g;
  const Rows<NB> W = wg_rows<NB>(P.rows, st.wave);  // (a wave past the last row keeps walking: the barriers need it)
  st.request(P.wq, H, P.bq, H, 0, 0);
  f4 xb[NB][DT], m[NB][DT];
  load_rows<DT, NB>(P.x, W, g, xb);
  st.par = 1;  // the first commit fills buffer 0 ...
  st.commit();  // ... and flips back to it
  auto store_tile = [&](float* out, int ld, int n_out, int nt, const f4 (&a)[NB]) {
    const int j0 = 16 * nt + 4 * g;
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
      if (!W.ok[nb]) continue;
#ifdef ACATTN_PROJ_NOSTORE
      if (a[nb][0] != 12345.678f) continue;
#endif
      float* dst = out + (size_t)W.row[nb] * ld + j0;
      if (j0 + 3 < n_out) {
        *(f4u*)dst = a[nb];
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (j0 + r < n_out) dst[r] = a[nb][r];
      }
    }
  };
  auto masked_store_rows = [&](float* out, const f4 (&v)[NB][DT]) {
#pragma unroll
    for (int nb = 0; nb < NB; ++nb)
#ifdef ACATTN_PROJ_NOSTORE
      if (W.ok[nb] && v[nb][0][0] == 12345.678f)
#else
      if (W.ok[nb])
#endif
#pragma unroll
        for (int t = 0; t < DT; ++t) *(f4*)(out + (size_t)W.row[nb] * H + 16 * t + 4 * g) = v[nb][t];
  };
  staged_keep<DT, NB, true>(st, P.wq, P.bq, xb, m, [&] { st.request(P.waq, H, P.baq, H, 0, 0); });  // mq
  masked_store_rows(O.mq, m);
  if (O.affine) write_affine<DT, NB>(m, W, P, O.affine, 0, P.b_order[0], P.b_dist[0], 0, c, g);
  staged_emit<DT, NB>(st, P.waq, H, P.baq, H, m, [&](int nt, const f4 (&a)[NB]) { store_tile(O.qa, H, H, nt, a); },
                      [&] { if (P.wg) st.request(P.wg, H, P.bg, P.G, 0, 0); else st.request(P.wk, H, P.bk, H, 0, 0); });
  if (P.wg) {
    staged_emit<DT, NB>(st, P.wg, H, P.bg, P.G, m, [&](int nt, const f4 (&a)[NB]) {
      f4 v[NB];
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) v[nb] = O.gate_prob ? gate_value(a[nb], 0) : a[nb];  // sigmoid once for all heads
      store_tile(O.gate, P.G, P.G, nt, v);
    }, [&] { st.request(P.wk, H, P.bk, H, 0, 0); });
  }
  staged_keep<DT, NB, true>(st, P.wk, P.bk, xb, m, [&] { st.request(P.wak, H, P.bak, H, 0, 0); });  // mk
  masked_store_rows(O.mk, m);
  if (O.affine) write_affine<DT, NB>(m, W, P, O.affine, H / P.n_heads, 0.f, 0.f, 2, c, g);
  staged_emit<DT, NB>(st, P.wak, H, P.bak, H, m, [&](int nt, const f4 (&a)[NB]) { store_tile(O.ka, H, H, nt, a); },
                      [&] { st.request(P.wv, H, P.bv, H, 0, 0); });
  staged_emit<DT, NB>(st, P.wv, H, P.bv, H, xb, [&](int nt, const f4 (&a)[NB]) { store_tile(O.mv, H, H, nt, a); },
                      [&] { st.has_bias = false; });
}

// transposed copies of the layer's weights for the backward: wt[m] = W_m^T as [n_in][ldt], ldt = n_out rounded up to 16
// (pad columns zero), matrices in the order Wq, Wk, Wv, Waq, Wak ([H, H] each) and Wg ([G, H]) behind them
struct TransposeJob {
  const float* src[6];
  int n_out[6];
};
__global__ void __launch_bounds__(256) transpose_weights_kernel(const TransposeJob J, int H, float* ws) {
  __shared__ float tile[16][17];
  const int mtx = blockIdx.z;
  const float* src = J.src[mtx];
  if (!src) return;
  const int n_out = J.n_out[mtx], ldt = (n_out + 15) & ~15;
  size_t off = 0;
  for (int k = 0; k < mtx; ++k) off += (size_t)H * ((J.n_out[k] + 15) & ~15);
  float* dst = ws + off;
  const int o0 = blockIdx.x * 16, i0 = blockIdx.y * 16;
  if (o0 >= ldt) return;
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  tile[ty][tx] = (o0 + ty < n_out) ? src[(size_t)(o0 + ty) * H + i0 + tx] : 0.f;
  __syncthreads();
  dst[(size_t)(i0 + ty) * ldt + o0 + tx] = tile[tx][ty];
}

// dx etc. as in proj_bwd_kernel; wt = the transposed weights above.  Three row-fragment sets fit beside the weight
// buffers, so the totals are written first and read back (by the lanes that wrote them) as the sources of dx:
// dmq_total and dmk_total are required outputs here whenever dx is asked for.
template <int H, int NB, int MODE>
__global__ void __launch_bounds__(64, 2) proj_wide_bwd_kernel(const acattn_proj_problem P, const acattn_proj_bwd_io IO,
                                                              const float* __restrict__ wt) {
  constexpr int DT = H / 16;
  const bool h_dmq = MODE == 1 || (MODE == 0 && IO.dmq), h_dmk = MODE == 1 || (MODE == 0 && IO.dmk);
  const bool h_dmv = MODE == 1 || (MODE == 0 && IO.dmv);
  const bool h_dqa = MODE != 0 || IO.dqa, h_dka = MODE != 0 || IO.dka, h_dx = MODE != 0 || IO.dx;
  const bool h_qt = MODE != 0 || IO.dmq_total, h_kt = MODE != 0 || IO.dmk_total;
  const int c = threadIdx.x & 15, g = threadIdx.x >> 4;
  const Rows<NB> W = wave_rows<NB>(P.rows);
  const size_t HH = (size_t)H * H;
  const float *wqT = wt, *wkT = wt + HH, *wvT = wt + 2 * HH, *waqT = wt + 3 * HH, *wakT = wt + 4 * HH, *wgT = wt + 5 * HH;
  const int ldg = (P.G + 15) & ~15;
  f4 in[NB][DT], tot[NB][DT];
  auto zero = [&](f4 (&v)[NB][DT]) {
#pragma unroll
    for (int nb = 0; nb < NB; ++nb)
#pragma unroll
      for (int t = 0; t < DT; ++t) v[nb][t] = f4{0.f, 0.f, 0.f, 0.f};
  };
  // ---- d mq (total) = dmq + dqa . Waq + dgate . Wg ------------------------------------------------------------------
  if (h_dmq) load_rows<DT, NB>(IO.dmq, W, g, tot); else zero(tot);
  if (h_dqa) {
    load_rows<DT, NB>(IO.dqa, W, g, in);
    product_keep<DT, NB, false>(waqT, nullptr, c, g, in, tot);
  }
  if (MODE != 2 && IO.dgate && P.wg) {
    // the contraction runs over the G gate outputs, 16 at a time: B = dgate[row][16 kt + 4 g ..], A = WgT[16 nt + c][16 kt + 4 g ..]
    const int GT = ldg >> 4;
    for (int kt = 0; kt < GT; ++kt) {
      f4 d[NB];
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) {
        const int j0 = 16 * kt + 4 * g;
        const float* src = IO.dgate + (size_t)W.row[nb] * P.G + j0;
        f4 v = {0.f, 0.f, 0.f, 0.f};
        if (j0 + 3 < P.G) {
          v = *(const f4u*)src;
        } else {
#pragma unroll
          for (int r = 0; r < 4; ++r)
            if (j0 + r < P.G) v[r] = src[r];
        }
        d[nb] = v;
      }
      f4 wg4[DT];
#pragma unroll
      for (int nt = 0; nt < DT; ++nt) wg4[nt] = *(const f4*)(wgT + (size_t)(16 * nt + c) * ldg + 16 * kt + 4 * g);
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int nt = 0; nt < DT; ++nt)
#pragma unroll
          for (int nb = 0; nb < NB; ++nb) tot[nb][nt] = mfma16(wg4[nt][r], d[nb][r], tot[nb][nt]);
    }
  }
  if (h_qt) store_rows<DT, NB>(IO.dmq_total, W, g, tot);
  // ---- d mk (total) = dmk + dka . Wak ---------------------------------------------------------------------------------
  if (h_dmk) load_rows<DT, NB>(IO.dmk, W, g, tot); else zero(tot);
  if (h_dka) {
    load_rows<DT, NB>(IO.dka, W, g, in);
    product_keep<DT, NB, false>(wakT, nullptr, c, g, in, tot);
  }
  if (h_kt) store_rows<DT, NB>(IO.dmk_total, W, g, tot);
  // ---- dx = dx_init + d mk . Wk + d mq . Wq + d mv . Wv  (tot still holds d mk; d mq comes back from dmq_total) ----------
  if (h_dx) {
    f4 (&dx)[NB][DT] = in;
    if (IO.dx_init) load_rows<DT, NB>(IO.dx_init, W, g, dx); else zero(dx);
    product_keep<DT, NB, false>(wkT, nullptr, c, g, tot, dx);
    load_rows<DT, NB>(IO.dmq_total, W, g, tot);
    product_keep<DT, NB, false>(wqT, nullptr, c, g, tot, dx);
    if (h_dmv) {
      load_rows<DT, NB>(IO.dmv, W, g, tot);
      product_keep<DT, NB, false>(wvT, nullptr, c, g, tot, dx);
    }
    store_rows<DT, NB>(IO.dx, W, g, dx);
  }
}

// the backward of proj_wide_bwd_kernel with the (transposed) weights staged through LDS once per workgroup
template <int H, int NB, int MODE>
__global__ void __launch_bounds__(64 * NWV, 2) proj_staged_bwd_kernel(const acattn_proj_problem P, const acattn_proj_bwd_io IO,
                                                                      const float* __restrict__ wt) {
  constexpr int DT = H / 16;
  static_assert(DT == KT || MODE >= 0, "");
  const bool h_dmq = MODE == 1 || (MODE == 0 && IO.dmq), h_dmk = MODE == 1 || (MODE == 0 && IO.dmk);
  const bool h_dmv = MODE == 1 || (MODE == 0 && IO.dmv);
  const bool h_dqa = MODE != 0 || IO.dqa, h_dka = MODE != 0 || IO.dka, h_dx = MODE != 0 || IO.dx;
  const bool h_qt = MODE != 0 || IO.dmq_total, h_kt = MODE != 0 || IO.dmk_total;
  const bool h_gate = MODE != 2 && IO.dgate && P.wg;
  __shared__ f4 stage_lds[2 * STAGE_F4];
  WeightStage st;
  st.lds = stage_lds;
  st.lane = threadIdx.x & 63;
  st.wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  st.c = threadIdx.x & 15;
  st.g = (threadIdx.x >> 4) & 3;
  const int c = st.c, g = st.g;
  const Rows<NB> W = wg_rows<NB>(P.rows, st.wave);
  const size_t HH = (size_t)H * H;
  const float *wqT = wt, *wkT = wt + HH, *wvT = wt + 2 * HH, *waqT = wt + 3 * HH, *wakT = wt + 4 * HH, *wgT = wt + 5 * HH;
  const int ldg = (P.G + 15) & ~15, GT = ldg >> 4;
  // the chain of products (all flags are uniform over the launch): each asks for the first chunk of the next one
  auto first = [&](const float* wT) { st.request(wT, H, nullptr, H, 0, 0); };
  auto after_k_total = [&] { if (h_dx) first(wkT); else st.has_bias = false; };
  auto after_q_total = [&] { if (h_dka) first(wakT); else after_k_total(); };
  auto after_qa = [&] { if (h_gate) st.request_cols(wgT, ldg, 0); else after_q_total(); };
  if (h_dqa) first(waqT); else after_qa();
  st.par = 1;
  f4 in[NB][DT], tot[NB][DT];
  auto zero = [&](f4 (&v)[NB][DT]) {
#pragma unroll
    for (int nb = 0; nb < NB; ++nb)
#pragma unroll
      for (int t = 0; t < DT; ++t) v[nb][t] = f4{0.f, 0.f, 0.f, 0.f};
  };
  auto masked_store_rows = [&](float* out, const f4 (&v)[NB][DT]) {
#pragma unroll
    for (int nb = 0; nb < NB; ++nb)
      if (W.ok[nb])
#pragma unroll
        for (int t = 0; t < DT; ++t) *(f4*)(out + (size_t)W.row[nb] * H + 16 * t + 4 * g) = v[nb][t];
  };
  // ---- d mq (total) = dmq + dqa . Waq + dgate . Wg ------------------------------------------------------------------
  if (h_dmq) load_rows<DT, NB>(IO.dmq, W, g, tot); else zero(tot);
  if (h_dqa) load_rows<DT, NB>(IO.dqa, W, g, in);
  st.commit();
  if (h_dqa) staged_keep<DT, NB, false>(st, waqT, nullptr, in, tot, after_qa);
  if (h_gate) {
    // the contraction runs over the G gate outputs, 16 at a time: one staged chunk = the DT row tiles of WgT for that block
    static_assert(DT == KT || DT == 2 * KT, "");
    for (int kt = 0; kt < GT; ++kt) {
      f4 d[NB];
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) {
        const int j0 = 16 * kt + 4 * g;
        const float* src = IO.dgate + (size_t)W.row[nb] * P.G + j0;
        f4 v = {0.f, 0.f, 0.f, 0.f};
        if (j0 + 3 < P.G) {
          v = *(const f4u*)src;
        } else {
#pragma unroll
          for (int r = 0; r < 4; ++r)
            if (j0 + r < P.G) v[r] = src[r];
        }
        d[nb] = v;
      }
#pragma unroll
      for (int half = 0; half < DT / KT; ++half) {  // hidden 256: the 16 row tiles of a column block are two chunks
        f4 frag[KT], b;
        st.fetch(frag, b);
        if (half + 1 < DT / KT)
          st.request_cols(wgT + (size_t)(16 * KT) * ldg * (half + 1), ldg, kt);
        else if (kt + 1 < GT)
          st.request_cols(wgT, ldg, kt + 1);
        else
          after_q_total();
        PIN_ORDER();
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
          for (int nt = 0; nt < KT; ++nt)
#pragma unroll
            for (int nb = 0; nb < NB; ++nb) {
              // (compile-time index: the half loop is unrolled)
              if (half == 0) tot[nb][nt] = mfma16(frag[nt][r], d[nb][r], tot[nb][nt]);
              else tot[nb][DT - KT + nt] = mfma16(frag[nt][r], d[nb][r], tot[nb][DT - KT + nt]);
            }
        PIN_ORDER();
        st.commit();
      }
    }
  }
  if (h_qt) masked_store_rows(IO.dmq_total, tot);
  // ---- d mk (total) = dmk + dka . Wak ---------------------------------------------------------------------------------
  if (h_dmk) load_rows<DT, NB>(IO.dmk, W, g, tot); else zero(tot);
  if (h_dka) {
    load_rows<DT, NB>(IO.dka, W, g, in);
    staged_keep<DT, NB, false>(st, wakT, nullptr, in, tot, after_k_total);
  }
  if (h_kt) masked_store_rows(IO.dmk_total, tot);
  // ---- dx = dx_init + d mk . Wk + d mq . Wq + d mv . Wv  (tot still holds d mk; d mq comes back from dmq_total) ----------
  if (h_dx) {
    f4 (&dx)[NB][DT] = in;
    if (IO.dx_init) load_rows<DT, NB>(IO.dx_init, W, g, dx); else zero(dx);
    staged_keep<DT, NB, false>(st, wkT, nullptr, tot, dx, [&] { first(wqT); });
    load_rows<DT, NB>(IO.dmq_total, W, g, tot);
    staged_keep<DT, NB, false>(st, wqT, nullptr, tot, dx, [&] { if (h_dmv) first(wvT); else st.has_bias = false; });
    if (h_dmv) {
      load_rows<DT, NB>(IO.dmv, W, g, tot);
      staged_keep<DT, NB, false>(st, wvT, nullptr, tot, dx, [&] { st.has_bias = false; });
    }
    masked_store_rows(IO.dx, dx);
  }
}

// =====================================================================================================================
// Hidden 64 on split bf16 products.  The same chains as proj_fwd_kernel / proj_bwd_kernel, every
// product on v_mfma_f32_16x16x32_bf16 with both operands split exactly into three bf16 planes (acattn_split.h): 2 x 6
// MFMAs of 16 cycles per 16 x 16 output tile instead of 16 fp32 MFMAs of 32.
//   Layouts (lane = 16 g + c).  A[m = c][k = 8g + j], B[k = 8g + j][n = c], D[m = 4g + r][n = c].  The contraction of
//   K-block s runs over the features k(s, g, j) = 32 s + 16 (j >> 2) + 4 g + (j & 3): the B operand of a lane is then
//   registers 0..3 of accumulator tiles 2s and 2s + 1 of the product that made it (row c, features 16 t + 4 g + r), so
//   an output feeds the next product with no shuffle, and a row read from memory in that layout is two 16-byte loads.
//   The weights are split ONCE per workgroup: wave w splits output tile w of each matrix into the workgroup's LDS as
//   [matrix][tile][s][plane][lane] fragments, every wave reads all of them back with ds_read_b128 (conflict-free).  The
//   six matrices take 144 KB, so the gate (one matrix of the six) must have G <= 64 outputs; wider gates stay on
//   proj_fwd_kernel / proj_bwd_kernel.
//   With acattn_proj_problem.split_planes the same fragments, split once per encoder forward by split_many_kernel
//   (acattn_tail.hip), are read from global memory instead (proj_planes_fwd_kernel / proj_planes_bwd_kernel, below the
//   LDS kernels): no LDS image, no barrier, one wave per workgroup; DESIGN.md 4.6.
// ---------------------------------------------------------------------------------------------------------------------
constexpr int SPW = 4;                                       // waves per workgroup (one per output tile)
constexpr int SPLIT_MAT = SPLIT_SQ64;                        // b8 per matrix: [tile][s][plane][lane]
constexpr int SPLIT_LDS = 6 * SPLIT_MAT * (int)sizeof(b8);  // bytes
static_assert(6 * SPLIT_MAT == PROJ_PLANES_DIR, "the planes image of one direction is the LDS image");

__device__ __forceinline__ int kperm(int s, int g, int j) { return 32 * s + 16 * (j >> 2) + 4 * g + (j & 3); }

// the raw values of output tile `nt`, K-block s, of one matrix.  T = false: A[m][k] = W[m][k] (outputs m, rows past
// n_out read as row n_out - 1 and never stored); T = true: A[m][k] = W[k][m] (the input gradient), k >= n_out zero.
template <bool T>
__device__ __forceinline__ void split_raw(const float* w, int n_out, int nt, int c, int g, float (&v)[2][8]) {
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    if constexpr (!T) {
      const float* row = w + (size_t)min(16 * nt + c, n_out - 1) * 64 + 32 * s + 4 * g;
      const f4 lo = *(const f4*)row, hi = *(const f4*)(row + 16);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        v[s][r] = lo[r];
        v[s][4 + r] = hi[r];
      }
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int k = kperm(s, g, j);
        const float t = w[(size_t)min(k, n_out - 1) * 64 + 16 * nt + c];
        v[s][j] = k < n_out ? t : 0.f;
      }
    }
  }
}

__device__ __forceinline__ void split_store(const float (&v)[2][8], b8* mat, int nt, int lane) {
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    b8 p[3];
    split8(v[s], p[0], p[1], p[2]);
#pragma unroll
    for (int q = 0; q < 3; ++q) mat[((nt * 2 + s) * 3 + q) * 64 + lane] = p[q];
  }
}

// B operand planes of rows held in accumulator layout (v[nb][t][r] = row c, feature 16 t + 4 g + r)
template <int NB>
__device__ __forceinline__ void split_rows(const f4 (&v)[NB][4], b8 (&b)[NB][2][3]) {
#pragma unroll
  for (int nb = 0; nb < NB; ++nb)
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      float x[8];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        x[r] = v[nb][2 * s][r];
        x[4 + r] = v[nb][2 * s + 1][r];
      }
      split8(x, b[nb][s][0], b[nb][s][1], b[nb][s][2]);
    }
}

// acc[nb][nt] += A(mat)[tile nt] . B[nb] for the tiles nt < NT
template <int NB, int NT = 4>
__device__ __forceinline__ void split_product(const b8* mat, int lane, const b8 (&b)[NB][2][3], f4 (&acc)[NB][4]) {
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    b8 a[2][3];
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int q = 0; q < 3; ++q) a[s][q] = mat[((nt * 2 + s) * 3 + q) * 64 + lane];
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) acc[nb][nt] = mfma_split(a[s], b[nb][s], acc[nb][nt]);
  }
}

template <int NB>
__device__ __forceinline__ Rows<NB> split_rows_of(int R, int wave) {
  Rows<NB> w;
  const int c = threadIdx.x & 15;
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) {
    const int r = ((blockIdx.x * SPW + wave) * NB + nb) * 16 + c;
    w.ok[nb] = r < R;
    w.row[nb] = r < R ? r : R - 1;
  }
  return w;
}

// LDS matrices of the forward: Wq, Waq, Wg, Wk, Wak, Wv
template <int NB>
__global__ void __launch_bounds__(64 * SPW) proj_split_fwd_kernel(const acattn_proj_problem P, const acattn_proj_out O) {
  extern __shared__ b8 wsp[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 15, g = lane >> 4;
  const Rows<NB> W = split_rows_of<NB>(P.rows, wave);
  const bool gate = P.wg != nullptr;
  {
    const float* src[6] = {P.wq, P.waq, gate ? P.wg : P.wq, P.wk, P.wak, P.wv};
    float v[6][2][8];
#pragma unroll
    for (int m = 0; m < 6; ++m) split_raw<false>(src[m], m == 2 && gate ? P.G : 64, wave, c, g, v[m]);
#pragma unroll
    for (int m = 0; m < 6; ++m)
      if (m != 2 || gate) split_store(v[m], wsp + m * SPLIT_MAT, wave, lane);
  }
  f4 xb[NB][4], m[NB][4], acc[NB][4];
  b8 xs[NB][2][3], ms[NB][2][3];
  f4 bias[4];
  load_rows<4, NB>(P.x, W, g, xb);
  load_bias<4>(P.bq, g, bias);
  __syncthreads();
  split_rows<NB>(xb, xs);
  set_rows<4, NB>(bias, m);
  split_product<NB>(wsp, lane, xs, m);  // mq
  store_rows<4, NB>(O.mq, W, g, m);
  if (O.affine) write_affine<4, NB>(m, W, P, O.affine, 0, P.b_order[0], P.b_dist[0], 0, c, g);
  split_rows<NB>(m, ms);
  load_bias<4>(P.baq, g, bias);
  set_rows<4, NB>(bias, acc);
  split_product<NB>(wsp + SPLIT_MAT, lane, ms, acc);  // qa
  store_rows<4, NB>(O.qa, W, g, acc);
  if (gate) {
    const int GT = (P.G + 15) >> 4;  // 1 .. 4
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
      f4 b;
#pragma unroll
      for (int r = 0; r < 4; ++r) b[r] = P.bg[min(16 * nt + 4 * g + r, P.G - 1)];
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) acc[nb][nt] = b;
    }
    split_product<NB>(wsp + 2 * SPLIT_MAT, lane, ms, acc);  // gate logits (tiles past G are computed and dropped)
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
      if (nt >= GT) break;
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) {
        f4 v = acc[nb][nt];
        if (O.gate_prob) v = gate_value(v, 0);  // sigmoid once per (b, i, j): the heads share it (layers.py:887)
        const int j0 = 16 * nt + 4 * g;
        float* dst = O.gate + (size_t)W.row[nb] * P.G + j0;
        if (W.ok[nb] && j0 + 3 < P.G) {
          *(f4u*)dst = v;
        } else if (W.ok[nb]) {
#pragma unroll
          for (int r = 0; r < 4; ++r)
            if (j0 + r < P.G) dst[r] = v[r];
        }
      }
    }
  }
  load_bias<4>(P.bk, g, bias);
  set_rows<4, NB>(bias, m);
  split_product<NB>(wsp + 3 * SPLIT_MAT, lane, xs, m);  // mk
  store_rows<4, NB>(O.mk, W, g, m);
  if (O.affine) write_affine<4, NB>(m, W, P, O.affine, 64 / P.n_heads, 0.f, 0.f, 2, c, g);
  split_rows<NB>(m, ms);
  load_bias<4>(P.bak, g, bias);
  set_rows<4, NB>(bias, acc);
  split_product<NB>(wsp + 4 * SPLIT_MAT, lane, ms, acc);  // ka
  store_rows<4, NB>(O.ka, W, g, acc);
  load_bias<4>(P.bv, g, bias);
  set_rows<4, NB>(bias, acc);
  split_product<NB>(wsp + 5 * SPLIT_MAT, lane, xs, acc);  // mv
  store_rows<4, NB>(O.mv, W, g, acc);
}

// The three projections of a layer WITHOUT the adversarial calibrator (mq, mk, mv; acattn_projections_qkv_fwd): the
// chains of proj_split_fwd_kernel that end in an attack transform or the gate left out.  LDS matrices: Wq, Wk, Wv.
constexpr int SPLIT_QKV_LDS = 3 * SPLIT_MAT * (int)sizeof(b8);
template <int NB>
__global__ void __launch_bounds__(64 * SPW) proj_split_qkv_fwd_kernel(const acattn_proj_problem P, const acattn_proj_out O) {
  extern __shared__ b8 wsp[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 15, g = lane >> 4;
  const Rows<NB> W = split_rows_of<NB>(P.rows, wave);
  {
    const float* src[3] = {P.wq, P.wk, P.wv};
    float v[3][2][8];
#pragma unroll
    for (int m = 0; m < 3; ++m) split_raw<false>(src[m], 64, wave, c, g, v[m]);
#pragma unroll
    for (int m = 0; m < 3; ++m) split_store(v[m], wsp + m * SPLIT_MAT, wave, lane);
  }
  f4 xb[NB][4], acc[NB][4];
  b8 xs[NB][2][3];
  f4 bias[4];
  load_rows<4, NB>(P.x, W, g, xb);
  load_bias<4>(P.bq, g, bias);
  __syncthreads();
  split_rows<NB>(xb, xs);
  set_rows<4, NB>(bias, acc);
  split_product<NB>(wsp, lane, xs, acc);  // mq
  store_rows<4, NB>(O.mq, W, g, acc);
  if (O.affine) write_affine<4, NB>(acc, W, P, O.affine, 0, P.b_order[0], P.b_dist[0], 0, c, g);
  load_bias<4>(P.bk, g, bias);
  set_rows<4, NB>(bias, acc);
  split_product<NB>(wsp + SPLIT_MAT, lane, xs, acc);  // mk
  store_rows<4, NB>(O.mk, W, g, acc);
  if (O.affine) write_affine<4, NB>(acc, W, P, O.affine, 64 / P.n_heads, 0.f, 0.f, 2, c, g);
  load_bias<4>(P.bv, g, bias);
  set_rows<4, NB>(bias, acc);
  split_product<NB>(wsp + 2 * SPLIT_MAT, lane, xs, acc);  // mv
  store_rows<4, NB>(O.mv, W, g, acc);
}

// LDS matrices of the backward (transposed): Waq, Wg, Wq, Wak, Wk, Wv.  MODE as in proj_bwd_kernel.
template <int NB, int MODE>
__global__ void __launch_bounds__(64 * SPW) proj_split_bwd_kernel(const acattn_proj_problem P, const acattn_proj_bwd_io IO) {
  extern __shared__ b8 wsp[];
  const bool h_dmq = MODE == 1 || (MODE == 0 && IO.dmq), h_dmk = MODE == 1 || (MODE == 0 && IO.dmk);
  const bool h_dmv = MODE == 1 || (MODE == 0 && IO.dmv);
  const bool h_dqa = MODE != 0 || IO.dqa, h_dka = MODE != 0 || IO.dka, h_dx = MODE != 0 || IO.dx;
  const bool h_qt = MODE != 0 || IO.dmq_total, h_kt = MODE != 0 || IO.dmk_total;
  const bool gate = MODE != 2 && IO.dgate && P.wg;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 15, g = lane >> 4;
  const Rows<NB> W = split_rows_of<NB>(P.rows, wave);
  {
    const float* src[6] = {P.waq, gate ? P.wg : P.waq, P.wq, P.wak, P.wk, P.wv};
    const bool need[6] = {h_dqa, gate, h_dx, h_dka, h_dx, h_dx && h_dmv};
    float v[6][2][8];
#pragma unroll
    for (int m = 0; m < 6; ++m)
      if (need[m]) split_raw<true>(src[m], m == 1 ? P.G : 64, wave, c, g, v[m]);
#pragma unroll
    for (int m = 0; m < 6; ++m)
      if (need[m]) split_store(v[m], wsp + m * SPLIT_MAT, wave, lane);
  }
  auto zero = [&](f4 (&v)[NB][4]) {
#pragma unroll
    for (int nb = 0; nb < NB; ++nb)
#pragma unroll
      for (int t = 0; t < 4; ++t) v[nb][t] = f4{0.f, 0.f, 0.f, 0.f};
  };
  f4 in[NB][4], dq[NB][4], dk[NB][4], dx[NB][4];
  b8 bs[NB][2][3];
  if (IO.dx_init && h_dx) load_rows<4, NB>(IO.dx_init, W, g, dx); else zero(dx);  // the residual path's share of dx
  if (h_dmq) load_rows<4, NB>(IO.dmq, W, g, dq); else zero(dq);
  if (h_dqa) load_rows<4, NB>(IO.dqa, W, g, in);
  __syncthreads();

  // ---- d mq (total) = dmq + dqa . Waq + dgate . Wg;  dx += d mq . Wq ------------------------------------------------
  if (h_dqa) {
    split_rows<NB>(in, bs);
    split_product<NB>(wsp, lane, bs, dq);
  }
  if (gate) {
    // B[k][row c] = dgate[row][k], k = kperm(s, g, j) < G (G <= 64; rows of G floats: dword reads)
#pragma unroll
    for (int nb = 0; nb < NB; ++nb)
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        float x[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int k = kperm(s, g, j);
          const float t = IO.dgate[(size_t)W.row[nb] * P.G + min(k, P.G - 1)];
          x[j] = k < P.G ? t : 0.f;
        }
        split8(x, bs[nb][s][0], bs[nb][s][1], bs[nb][s][2]);
      }
    split_product<NB>(wsp + SPLIT_MAT, lane, bs, dq);
  }
  if (h_qt) store_rows<4, NB>(IO.dmq_total, W, g, dq);
  if (h_dx) {
    split_rows<NB>(dq, bs);
    split_product<NB>(wsp + 2 * SPLIT_MAT, lane, bs, dx);
  }

  // ---- d mk (total) = dmk + dka . Wak;  dx += d mk . Wk + d mv . Wv ---------------------------------------------------
  if (h_dmk) load_rows<4, NB>(IO.dmk, W, g, dk); else zero(dk);
  if (h_dka) {
    load_rows<4, NB>(IO.dka, W, g, in);
    split_rows<NB>(in, bs);
    split_product<NB>(wsp + 3 * SPLIT_MAT, lane, bs, dk);
  }
  if (h_kt) store_rows<4, NB>(IO.dmk_total, W, g, dk);
  if (h_dx) {
    split_rows<NB>(dk, bs);
    split_product<NB>(wsp + 4 * SPLIT_MAT, lane, bs, dx);
    if (h_dmv) {
      load_rows<4, NB>(IO.dmv, W, g, in);
      split_rows<NB>(in, bs);
      split_product<NB>(wsp + 5 * SPLIT_MAT, lane, bs, dx);
    }
    store_rows<4, NB>(IO.dx, W, g, dx);
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// The split chains on the planes of acattn_proj_problem.split_planes: the fragments above, written once per
// encoder forward by split_many_kernel (acattn_tail.hip), read from global memory.  No LDS image, no split of the weights,
// no barrier; one wave per workgroup.  Same products in the same MFMA order per accumulator as the LDS kernels: every
// tensor written is bitwise theirs.  (The LDS kernels keep their own text: routed through these chains their register
// allocation changed -- proj_split_bwd_kernel<2, 0> 192 + 36 -> 220 + 68 -- and NULL planes must select them as they were.)
// `product(next, ..)`: the product with the matrix in the ring; `next` names the matrix of the product that follows it in
// the chain (-1: none), `begin(m)` the first one.
// ---------------------------------------------------------------------------------------------------------------------
// The planes in global memory (L2): one matrix (24 fragments) is in registers or on its way.  Every tile's six fragments
// are requested for the NEXT product as soon as this product's MFMAs of that tile are issued, so a request has three
// tiles of matrix work and the split of the next operand to arrive.  Same MFMA order per accumulator as split_product.
struct PlaneWeights {
  const b8* img;
  int lane;
  b8 ring[4][2][3];
  __device__ __forceinline__ void fetch(int m, int nt) {
    const b8* mat = img + (size_t)m * SPLIT_MAT + lane;
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int q = 0; q < 3; ++q) ring[nt][s][q] = mat[((nt * 2 + s) * 3 + q) * 64];
  }
  __device__ __forceinline__ void begin(int m) {
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) fetch(m, nt);
  }
  template <int NB>
  __device__ __forceinline__ void product(int next, const b8 (&b)[NB][2][3], f4 (&acc)[NB][4]) {
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
      PIN_ORDER();
#pragma unroll
      for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) acc[nb][nt] = mfma_split(ring[nt][s], b[nb][s], acc[nb][nt]);
      if (next >= 0) fetch(next, nt);  // (the scheduler would sink the requests to their use: pinned behind the tile)
      PIN_ORDER();
    }
  }
};

// The same interface on an LDS image of the planes (proj_fill_bwd_kernel): a fragment is read where it is used.
struct LdsImage {
  const b8* img;
  int lane, cur;
  __device__ __forceinline__ void begin(int m) {
    cur = m;
    __syncthreads();  // the image is complete
  }
  template <int NB>
  __device__ __forceinline__ void product(int next, const b8 (&b)[NB][2][3], f4 (&acc)[NB][4]) {
    split_product<NB>(img + cur * SPLIT_MAT, lane, b, acc);
    cur = next;
  }
};

// proj_split_fwd_kernel's chain; matrices of the forward image: Wq, Waq, Wg, Wk, Wak, Wv (product k of the chain uses matrix k)
template <int NB>
__device__ __forceinline__ void split_fwd_chain(const acattn_proj_problem& P, const acattn_proj_out& O, const Rows<NB>& W,
                                                PlaneWeights& ws, int c, int g) {
  const bool gate = P.wg != nullptr;
  f4 xb[NB][4], m[NB][4], acc[NB][4];
  b8 xs[NB][2][3], ms[NB][2][3];
  f4 bias[4];
  load_rows<4, NB>(P.x, W, g, xb);
  load_bias<4>(P.bq, g, bias);
  ws.begin(0);  // (behind the rows: their split is the first thing to wait)
  split_rows<NB>(xb, xs);
  set_rows<4, NB>(bias, m);
  ws.product<NB>(1, xs, m);  // mq
  store_rows<4, NB>(O.mq, W, g, m);
  if (O.affine) write_affine<4, NB>(m, W, P, O.affine, 0, P.b_order[0], P.b_dist[0], 0, c, g);
  split_rows<NB>(m, ms);
  load_bias<4>(P.baq, g, bias);
  set_rows<4, NB>(bias, acc);
  ws.product<NB>(gate ? 2 : 3, ms, acc);  // qa
  store_rows<4, NB>(O.qa, W, g, acc);
  if (gate) {
    const int GT = (P.G + 15) >> 4;  // 1 .. 4
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
      f4 b;
#pragma unroll
      for (int r = 0; r < 4; ++r) b[r] = P.bg[min(16 * nt + 4 * g + r, P.G - 1)];
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) acc[nb][nt] = b;
    }
    ws.product<NB>(3, ms, acc);  // gate logits (tiles past G are computed and dropped)
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
      if (nt >= GT) break;
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) {
        f4 v = acc[nb][nt];
        if (O.gate_prob) v = gate_value(v, 0);  // sigmoid once per (b, i, j): the heads share it (layers.py:887)
        const int j0 = 16 * nt + 4 * g;
        float* dst = O.gate + (size_t)W.row[nb] * P.G + j0;
        if (W.ok[nb] && j0 + 3 < P.G) {
          *(f4u*)dst = v;
        } else if (W.ok[nb]) {
#pragma unroll
          for (int r = 0; r < 4; ++r)
            if (j0 + r < P.G) dst[r] = v[r];
        }
      }
    }
  }
  load_bias<4>(P.bk, g, bias);
  set_rows<4, NB>(bias, m);
  ws.product<NB>(4, xs, m);  // mk
  store_rows<4, NB>(O.mk, W, g, m);
  if (O.affine) write_affine<4, NB>(m, W, P, O.affine, 64 / P.n_heads, 0.f, 0.f, 2, c, g);
  split_rows<NB>(m, ms);
  load_bias<4>(P.bak, g, bias);
  set_rows<4, NB>(bias, acc);
  ws.product<NB>(5, ms, acc);  // ka
  store_rows<4, NB>(O.ka, W, g, acc);
  load_bias<4>(P.bv, g, bias);
  set_rows<4, NB>(bias, acc);
  ws.product<NB>(-1, xs, acc);  // mv
  store_rows<4, NB>(O.mv, W, g, acc);
}

// The same chain on the planes of acattn_proj_problem.split_planes: one wave per workgroup, nothing shared.  Two waves fit
// a SIMD (198 registers at NB = 1, 256 at NB = 2).
template <int NB>
__global__ void __launch_bounds__(64, 2) proj_planes_fwd_kernel(const acattn_proj_problem P, const acattn_proj_out O) {
  const int lane = threadIdx.x, c = lane & 15, g = lane >> 4;
  const Rows<NB> W = wave_rows<NB>(P.rows);
  PlaneWeights ws;
  ws.img = (const b8*)P.split_planes;
  ws.lane = lane;
  split_fwd_chain<NB>(P, O, W, ws, c, g);
}

// proj_split_bwd_kernel's chain; matrices of the backward image (transposed): Waq, Wg, Wq, Wak, Wk, Wv.  MODE as in
// proj_bwd_kernel.
template <int MODE>
struct SplitBwdFlags {
  bool h_dmq, h_dmk, h_dmv, h_dqa, h_dka, h_dx, h_qt, h_kt, gate;
  __device__ __forceinline__ SplitBwdFlags(const acattn_proj_problem& P, const acattn_proj_bwd_io& IO)
      : h_dmq(MODE == 1 || (MODE == 0 && IO.dmq)), h_dmk(MODE == 1 || (MODE == 0 && IO.dmk)),
        h_dmv(MODE == 1 || (MODE == 0 && IO.dmv)), h_dqa(MODE != 0 || IO.dqa), h_dka(MODE != 0 || IO.dka),
        h_dx(MODE != 0 || IO.dx), h_qt(MODE != 0 || IO.dmq_total), h_kt(MODE != 0 || IO.dmk_total),
        gate(MODE != 2 && IO.dgate && P.wg) {}
  // the first matrix behind `m` that a product of this launch uses, -1 = none (m = -1: the first of all)
  __device__ __forceinline__ int next(int m) const {
    const bool need[6] = {h_dqa, gate, h_dx, h_dka, h_dx, h_dx && h_dmv};
    int n = -1;
#pragma unroll
    for (int j = 5; j >= 0; --j)
      if (j > m && need[j]) n = j;
    return n;
  }
};

template <int NB, int MODE, class WS>
__device__ __forceinline__ void split_bwd_chain(const acattn_proj_problem& P, const acattn_proj_bwd_io& IO, const Rows<NB>& W,
                                                const SplitBwdFlags<MODE>& F, WS& ws, int g) {
  const bool h_dmq = F.h_dmq, h_dmk = F.h_dmk, h_dmv = F.h_dmv, h_dqa = F.h_dqa, h_dka = F.h_dka, h_dx = F.h_dx;
  const bool h_qt = F.h_qt, h_kt = F.h_kt, gate = F.gate;
  auto zero = [&](f4 (&v)[NB][4]) {
#pragma unroll
    for (int nb = 0; nb < NB; ++nb)
#pragma unroll
      for (int t = 0; t < 4; ++t) v[nb][t] = f4{0.f, 0.f, 0.f, 0.f};
  };
  f4 in[NB][4], dq[NB][4], dk[NB][4], dx[NB][4];
  b8 bs[NB][2][3];
  if (IO.dx_init && h_dx) load_rows<4, NB>(IO.dx_init, W, g, dx); else zero(dx);  // the residual path's share of dx
  if (h_dmq) load_rows<4, NB>(IO.dmq, W, g, dq); else zero(dq);
  if (h_dqa) load_rows<4, NB>(IO.dqa, W, g, in);
  const int first = F.next(-1);
  if (first >= 0) ws.begin(first);  // (behind the rows: their split is the first thing to wait)

  // ---- d mq (total) = dmq + dqa . Waq + dgate . Wg;  dx += d mq . Wq ------------------------------------------------
  if (h_dqa) {
    split_rows<NB>(in, bs);
    ws.template product<NB>(F.next(0), bs, dq);
  }
  if (gate) {
    // B[k][row c] = dgate[row][k], k = kperm(s, g, j) < G (G <= 64; rows of G floats: dword reads)
#pragma unroll
    for (int nb = 0; nb < NB; ++nb)
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        float x[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int k = kperm(s, g, j);
          const float t = IO.dgate[(size_t)W.row[nb] * P.G + min(k, P.G - 1)];
          x[j] = k < P.G ? t : 0.f;
        }
        split8(x, bs[nb][s][0], bs[nb][s][1], bs[nb][s][2]);
      }
    ws.template product<NB>(F.next(1), bs, dq);
  }
  if (h_qt) store_rows<4, NB>(IO.dmq_total, W, g, dq);
  if (h_dx) {
    split_rows<NB>(dq, bs);
    ws.template product<NB>(F.next(2), bs, dx);
  }

  // ---- d mk (total) = dmk + dka . Wak;  dx += d mk . Wk + d mv . Wv ---------------------------------------------------
  if (h_dmk) load_rows<4, NB>(IO.dmk, W, g, dk); else zero(dk);
  if (h_dka) {
    load_rows<4, NB>(IO.dka, W, g, in);
    split_rows<NB>(in, bs);
    ws.template product<NB>(F.next(3), bs, dk);
  }
  if (h_kt) store_rows<4, NB>(IO.dmk_total, W, g, dk);
  if (h_dx) {
    split_rows<NB>(dk, bs);
    ws.template product<NB>(F.next(4), bs, dx);
    if (h_dmv) {
      load_rows<4, NB>(IO.dmv, W, g, in);
      split_rows<NB>(in, bs);
      ws.template product<NB>(-1, bs, dx);
    }
    store_rows<4, NB>(IO.dx, W, g, dx);
  }
}

// The same chain on the backward image of acattn_proj_problem.split_planes (see proj_planes_fwd_kernel).  Four row sets,
// the split operand and the ring: 202 registers at NB = 1 (two waves per SIMD), 308 + 68 at NB = 2 (one).
template <int NB, int MODE>
__global__ void __launch_bounds__(64, NB == 1 ? 2 : 1) proj_planes_bwd_kernel(const acattn_proj_problem P, const acattn_proj_bwd_io IO) {
  const SplitBwdFlags<MODE> F(P, IO);
  const int lane = threadIdx.x, g = lane >> 4;
  const Rows<NB> W = wave_rows<NB>(P.rows);
  PlaneWeights ws;
  ws.img = (const b8*)P.split_planes + PROJ_PLANES_DIR;
  ws.lane = lane;
  split_bwd_chain<NB, MODE>(P, IO, W, F, ws, g);
}

// The fallback form of the backward: the workgroups of proj_split_bwd_kernel, their LDS image filled from the planes with
// straight 16-byte copies (no gathers, no split8), then the chain on the image.
template <int NB, int MODE>
__global__ void __launch_bounds__(64 * SPW) proj_fill_bwd_kernel(const acattn_proj_problem P, const acattn_proj_bwd_io IO) {
  extern __shared__ b8 wsp[];
  const SplitBwdFlags<MODE> F(P, IO);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4;
  const Rows<NB> W = split_rows_of<NB>(P.rows, wave);
  const b8* src = (const b8*)P.split_planes + PROJ_PLANES_DIR;
  const bool need[6] = {F.h_dqa, F.gate, F.h_dx, F.h_dka, F.h_dx, F.h_dx && F.h_dmv};
#pragma unroll
  for (int m = 0; m < 6; ++m)
    if (need[m]) {
#pragma unroll
      for (int i = 0; i < SPLIT_MAT / (64 * SPW); ++i)
        wsp[m * SPLIT_MAT + i * 64 * SPW + threadIdx.x] = src[m * SPLIT_MAT + i * 64 * SPW + threadIdx.x];
    }
  LdsImage ws{wsp, lane, 0};
  split_bwd_chain<NB, MODE>(P, IO, W, F, ws, g);
}

int rows_per_wave(int rows) {
  static const int forced = getenv("ACATTN_PROJ_ROWS_PER_WAVE") ? atoi(getenv("ACATTN_PROJ_ROWS_PER_WAVE")) : 0;  // measurements
  if (forced == 16 || forced == 32) return forced;
  // 32 rows per wave once that still gives most SIMDs a wave: each weight fragment then feeds two row blocks.  Inside
  // the training step (B = 512, L = 50: 25,600 rows, 800 waves) 1.540 against 1.581 ms per step with 16 rows per wave.
  return rows >= 16384 ? 32 : 16;
}

}  // namespace

bool acattn_proj_supported(int H, int G) { return (H == 64 || H == 128 || H == 256) && G >= 0 && G <= 256; }

int64_t acattn_proj_bwd_ws_bytes(const acattn_proj_problem& p) {
  if (p.H == 64) return 0;
  return ((int64_t)5 * p.H * p.H + (int64_t)p.H * ((p.G + 15) & ~15)) * (int64_t)sizeof(float);
}

namespace {
template <int H>
int launch_wide_fwd(const acattn_proj_problem& p, const acattn_proj_out& o, hipStream_t stream) {
#ifdef ACATTN_PROJ_NB1
  constexpr int NB = 1;
#else
  constexpr int NB = H == 128 ? 2 : 1;
#endif
  static const bool per_wave = getenv("ACATTN_PROJ_PER_WAVE") != nullptr;  // measurement: the per-wave weight stream
  if (!per_wave) {
    const int blocks = (p.rows + 16 * NB * NWV - 1) / (16 * NB * NWV);
    hipLaunchKernelGGL((proj_staged_fwd_kernel<H, NB>), dim3(blocks), dim3(64 * NWV), 0, stream, p, o);
    return (int)hipGetLastError();
  }
  const int blocks = (p.rows + 16 * NB - 1) / (16 * NB);
  hipLaunchKernelGGL((proj_wide_fwd_kernel<H, NB>), dim3(blocks), dim3(64), 0, stream, p, o);
  return (int)hipGetLastError();
}
template <int H>
int launch_wide_bwd(const acattn_proj_problem& p, const acattn_proj_bwd_io& io, hipStream_t stream) {
  constexpr int NB = H == 128 ? 2 : 1;
  if (!io.workspace) {
    acattn_set_error("projections backward at hidden 128 / 256 needs acattn_proj_bwd_io.workspace");
    return -1;
  }
  if (io.dx && !io.dmq_total) {
    acattn_set_error("projections backward at hidden 128 / 256: dx needs dmq_total (it is read back as a source of dx)");
    return -1;
  }
  float* wt = (float*)io.workspace;
  TransposeJob J;
  const float* src[6] = {p.wq, p.wk, p.wv, p.waq, p.wak, p.wg};
  for (int k = 0; k < 6; ++k) {
    J.src[k] = src[k];
    J.n_out[k] = k < 5 ? p.H : p.G;
  }
  const int max_out = std::max(p.H, (p.G + 15) & ~15);
  hipLaunchKernelGGL(transpose_weights_kernel, dim3(max_out / 16, p.H / 16, p.wg ? 6 : 5), dim3(256), 0, stream, J, p.H, wt);
  const bool outs = io.dx && io.dmq_total && io.dmk_total, attack = io.dqa && io.dka;
  const bool all_in = attack && io.dmq && io.dmk && io.dmv && (io.dgate || !p.wg);
  const bool attack_only = attack && !io.dmq && !io.dmk && !io.dmv && !io.dgate;
  const int mode = !outs ? 0 : all_in ? 1 : attack_only ? 2 : 0;
  static const bool per_wave = getenv("ACATTN_PROJ_PER_WAVE") != nullptr;  // measurement: the per-wave weight stream
  if (!per_wave) {
    const int wgs = (p.rows + 16 * NB * NWV - 1) / (16 * NB * NWV);
    if (mode == 1)
      hipLaunchKernelGGL((proj_staged_bwd_kernel<H, NB, 1>), dim3(wgs), dim3(64 * NWV), 0, stream, p, io, (const float*)wt);
    else if (mode == 2)
      hipLaunchKernelGGL((proj_staged_bwd_kernel<H, NB, 2>), dim3(wgs), dim3(64 * NWV), 0, stream, p, io, (const float*)wt);
    else
      hipLaunchKernelGGL((proj_staged_bwd_kernel<H, NB, 0>), dim3(wgs), dim3(64 * NWV), 0, stream, p, io, (const float*)wt);
    return (int)hipGetLastError();
  }
  const int blocks = (p.rows + 16 * NB - 1) / (16 * NB);
  if (mode == 1)
    hipLaunchKernelGGL((proj_wide_bwd_kernel<H, NB, 1>), dim3(blocks), dim3(64), 0, stream, p, io, (const float*)wt);
  else if (mode == 2)
    hipLaunchKernelGGL((proj_wide_bwd_kernel<H, NB, 2>), dim3(blocks), dim3(64), 0, stream, p, io, (const float*)wt);
  else
    hipLaunchKernelGGL((proj_wide_bwd_kernel<H, NB, 0>), dim3(blocks), dim3(64), 0, stream, p, io, (const float*)wt);
  return (int)hipGetLastError();
}
}  // namespace

namespace {
// g_linear_products: 0 = exact fp32 MFMA everywhere (acattn_linear_products, or ACATTN_LINEAR_PRODUCTS=fp32), 1 = the
// hidden-64 projections on split bf16 products (gates up to 64 outputs; the default)
int g_linear_products = -1;
int linear_products() {
  if (g_linear_products < 0) {
    const char* e = getenv("ACATTN_LINEAR_PRODUCTS");
    g_linear_products = e && !strcmp(e, "fp32") ? 0 : 1;
  }
  return g_linear_products;
}
bool use_split(const acattn_proj_problem& p) { return p.H == 64 && (!p.wg || p.G <= 64) && linear_products() == 1; }
int64_t proj_split_bytes(int H, int G) {
  if (H != 64 || G < 0 || G > 64 || linear_products() != 1) return 0;
  return (int64_t)2 * PROJ_PLANES_DIR * (int64_t)sizeof(b8);
}

// the dynamic LDS of a split kernel is above the 64 KB default: raised once per kernel
template <class K>
bool allow_split_lds(K kern) {
  return hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, SPLIT_LDS) == hipSuccess;
}

template <int NB>
int launch_split_fwd(const acattn_proj_problem& p, const acattn_proj_out& o, hipStream_t stream) {
  static const bool lds_ok = allow_split_lds(proj_split_fwd_kernel<NB>);
  if (!lds_ok) return (int)hipErrorInvalidValue;
  const int wgs = (p.rows + 16 * NB * SPW - 1) / (16 * NB * SPW);
  hipLaunchKernelGGL((proj_split_fwd_kernel<NB>), dim3(wgs), dim3(64 * SPW), SPLIT_LDS, stream, p, o);
  return (int)hipGetLastError();
}

template <int NB, int MODE>
int launch_split_bwd(const acattn_proj_problem& p, const acattn_proj_bwd_io& io, hipStream_t stream) {
  static const bool lds_ok = allow_split_lds(proj_split_bwd_kernel<NB, MODE>);
  if (!lds_ok) return (int)hipErrorInvalidValue;
  const int wgs = (p.rows + 16 * NB * SPW - 1) / (16 * NB * SPW);
  hipLaunchKernelGGL((proj_split_bwd_kernel<NB, MODE>), dim3(wgs), dim3(64 * SPW), SPLIT_LDS, stream, p, io);
  return (int)hipGetLastError();
}

// rows per wave of the planes kernels (16 * NB).  Measured per direction at 25,600 rows: forward 19.0 us
// with 32 against 19.3 with 16, backward 18.35 against 19.1 -- twice the waves do not pay for twice the fragment traffic;
// below 16,384 rows one row block, as the LDS kernels.  ACATTN_PROJ_PLANES_ROWS_FWD / _BWD = 16 | 32: measurements.
int planes_rows_per_wave(int rows, bool bwd) {
  static const int forced[2] = {getenv("ACATTN_PROJ_PLANES_ROWS_FWD") ? atoi(getenv("ACATTN_PROJ_PLANES_ROWS_FWD")) : 0,
                                getenv("ACATTN_PROJ_PLANES_ROWS_BWD") ? atoi(getenv("ACATTN_PROJ_PLANES_ROWS_BWD")) : 0};
  if (forced[bwd] == 16 || forced[bwd] == 32) return forced[bwd];
  return rows >= 16384 ? 32 : 16;
}

template <int NB>
int launch_planes_fwd(const acattn_proj_problem& p, const acattn_proj_out& o, hipStream_t stream) {
  const int blocks = (p.rows + 16 * NB - 1) / (16 * NB);
  hipLaunchKernelGGL((proj_planes_fwd_kernel<NB>), dim3(blocks), dim3(64), 0, stream, p, o);
  return (int)hipGetLastError();
}

template <int NB, int MODE>
int launch_planes_bwd(const acattn_proj_problem& p, const acattn_proj_bwd_io& io, hipStream_t stream) {
  const int blocks = (p.rows + 16 * NB - 1) / (16 * NB);
  hipLaunchKernelGGL((proj_planes_bwd_kernel<NB, MODE>), dim3(blocks), dim3(64), 0, stream, p, io);
  return (int)hipGetLastError();
}

template <int NB, int MODE>
int launch_fill_bwd(const acattn_proj_problem& p, const acattn_proj_bwd_io& io, hipStream_t stream) {
  static const bool lds_ok = allow_split_lds(proj_fill_bwd_kernel<NB, MODE>);
  if (!lds_ok) return (int)hipErrorInvalidValue;
  const int wgs = (p.rows + 16 * NB * SPW - 1) / (16 * NB * SPW);
  hipLaunchKernelGGL((proj_fill_bwd_kernel<NB, MODE>), dim3(wgs), dim3(64 * SPW), SPLIT_LDS, stream, p, io);
  return (int)hipGetLastError();
}

// which backward reads the planes: 0 the direct-from-L2 kernel, 1 the LDS image filled from them, 2 none (the LDS kernel that
// splits for itself).  ACATTN_PROJ_PLANES_BWD = direct | fill | lds: measurements.
int planes_bwd_form() {
  static const char* e = getenv("ACATTN_PROJ_PLANES_BWD");
  static const int form = !e ? 0 : !strcmp(e, "fill") ? 1 : !strcmp(e, "lds") ? 2 : 0;
  return form;
}
}  // namespace

int64_t acattn_proj_split_bytes(int H, int G) { return proj_split_bytes(H, G); }

int acattn_linear_products_choice(int mode) {
  const int old = linear_products();
  if (mode >= 0 && mode <= 1) g_linear_products = mode;
  return old;
}

int acattn_launch_proj_fwd(const acattn_proj_problem& p, const acattn_proj_out& o, hipStream_t stream) {
  if (p.H == 128) return launch_wide_fwd<128>(p, o, stream);
  if (p.H == 256) return launch_wide_fwd<256>(p, o, stream);
  const int rpw = rows_per_wave(p.rows), blocks = (p.rows + rpw - 1) / rpw;
  // (planes given where the split kernels do not run -- the product mode changed since they were made: they are not read)
  if (p.split_planes && use_split(p))
    return planes_rows_per_wave(p.rows, false) == 32 ? launch_planes_fwd<2>(p, o, stream) : launch_planes_fwd<1>(p, o, stream);
  if (use_split(p)) return rpw == 32 ? launch_split_fwd<2>(p, o, stream) : launch_split_fwd<1>(p, o, stream);
  if (rpw == 32)
    hipLaunchKernelGGL((proj_fwd_kernel<64, 2>), dim3(blocks), dim3(64), 0, stream, p, o);
  else
    hipLaunchKernelGGL((proj_fwd_kernel<64, 1>), dim3(blocks), dim3(64), 0, stream, p, o);
  return (int)hipGetLastError();
}

// mq, mk, mv alone: served at hidden 64 on the split products (the form the training step runs); every other width or
// mode is three plain linear layers for the caller.
bool acattn_proj_qkv_supported(int H) { return H == 64 && linear_products() == 1; }

namespace {
template <int NB>
int launch_split_qkv_fwd(const acattn_proj_problem& p, const acattn_proj_out& o, hipStream_t stream) {
  static const bool lds_ok = hipFuncSetAttribute((const void*)proj_split_qkv_fwd_kernel<NB>,
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, SPLIT_QKV_LDS) == hipSuccess;
  if (!lds_ok) return (int)hipErrorInvalidValue;
  const int wgs = (p.rows + 16 * NB * SPW - 1) / (16 * NB * SPW);
  hipLaunchKernelGGL((proj_split_qkv_fwd_kernel<NB>), dim3(wgs), dim3(64 * SPW), SPLIT_QKV_LDS, stream, p, o);
  return (int)hipGetLastError();
}
}  // namespace

int acattn_launch_proj_qkv_fwd(const acattn_proj_problem& p, const acattn_proj_out& o, hipStream_t stream) {
  if (!acattn_proj_qkv_supported(p.H)) {
    acattn_set_error("projections (q, k, v only): hidden_size must be 64 with the split products on");
    return -1;
  }
  return rows_per_wave(p.rows) == 32 ? launch_split_qkv_fwd<2>(p, o, stream) : launch_split_qkv_fwd<1>(p, o, stream);
}

int acattn_launch_proj_bwd(const acattn_proj_problem& p, const acattn_proj_bwd_io& io, hipStream_t stream) {
  if (p.H == 128) return launch_wide_bwd<128>(p, io, stream);
  if (p.H == 256) return launch_wide_bwd<256>(p, io, stream);
  const int rpw = rows_per_wave(p.rows), blocks = (p.rows + rpw - 1) / rpw;
  const bool outs = io.dx && io.dmq_total && io.dmk_total, attack = io.dqa && io.dka;
  const bool all_in = attack && io.dmq && io.dmk && io.dmv && (io.dgate || !p.wg);
  const bool attack_only = attack && !io.dmq && !io.dmk && !io.dmv && !io.dgate;
  const int mode = !outs ? 0 : all_in ? 1 : attack_only ? 2 : 0;
  if (p.split_planes && use_split(p) && planes_bwd_form() == 1) {
    if (rpw == 32) {
      if (mode == 1) return launch_fill_bwd<2, 1>(p, io, stream);
      if (mode == 2) return launch_fill_bwd<2, 2>(p, io, stream);
      return launch_fill_bwd<2, 0>(p, io, stream);
    }
    if (mode == 1) return launch_fill_bwd<1, 1>(p, io, stream);
    if (mode == 2) return launch_fill_bwd<1, 2>(p, io, stream);
    return launch_fill_bwd<1, 0>(p, io, stream);
  }
  if (p.split_planes && use_split(p) && planes_bwd_form() == 0) {
    if (planes_rows_per_wave(p.rows, true) == 32) {
      if (mode == 1) return launch_planes_bwd<2, 1>(p, io, stream);
      if (mode == 2) return launch_planes_bwd<2, 2>(p, io, stream);
      return launch_planes_bwd<2, 0>(p, io, stream);
    }
    if (mode == 1) return launch_planes_bwd<1, 1>(p, io, stream);
    if (mode == 2) return launch_planes_bwd<1, 2>(p, io, stream);
    return launch_planes_bwd<1, 0>(p, io, stream);
  }
  if (use_split(p)) {
    if (rpw == 32) {
      if (mode == 1) return launch_split_bwd<2, 1>(p, io, stream);
      if (mode == 2) return launch_split_bwd<2, 2>(p, io, stream);
      return launch_split_bwd<2, 0>(p, io, stream);
    }
    if (mode == 1) return launch_split_bwd<1, 1>(p, io, stream);
    if (mode == 2) return launch_split_bwd<1, 2>(p, io, stream);
    return launch_split_bwd<1, 0>(p, io, stream);
  }
#define LAUNCH(NB, MODE) hipLaunchKernelGGL((proj_bwd_kernel<64, NB, MODE>), dim3(blocks), dim3(64), 0, stream, p, io)
  if (rpw == 32) {
    if (mode == 1) LAUNCH(2, 1); else if (mode == 2) LAUNCH(2, 2); else LAUNCH(2, 0);
  } else {
    if (mode == 1) LAUNCH(1, 1); else if (mode == 2) LAUNCH(1, 2); else LAUNCH(1, 0);
  }
#undef LAUNCH
  return (int)hipGetLastError();
}
