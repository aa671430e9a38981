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
#include <stdlib.h>

#include <type_traits>

#include "acattn_common.h"

namespace {

constexpr float kLog2e = 1.44269504088896340736f;

__device__ __forceinline__ float ex2(float x) { return __builtin_amdgcn_exp2f(x); }
__device__ __forceinline__ float hsum(const f4 v) { return (v[0] + v[1]) + (v[2] + v[3]); }

constexpr int TS = 20;  // row stride of a turned 16 x 16 tile (16-byte rows, conflict-free column reads)

template <int DH>
__global__ void __launch_bounds__(256, 4) acattn_bwd_attack_kernel(const acattn_problem P, const acattn_bwd_io IO, float* gate_zero,
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

  // ---- this block's rows of qa: as the B operand of the scores, and column-wise as the A operand of dka ----------------
  const int qb = wave, i0 = qb * 16, i = i0 + c;
  const bool row_ok = i < L;
  float qaf[KS];
  {
    const size_t off = (rowbase + (row_ok ? i : 0)) * H + hoff + KS * g;
#pragma unroll
    for (int s4 = 0; s4 < KS / 4; ++s4) {
      f4 ta = {0.f, 0.f, 0.f, 0.f};
      if (row_ok) ta = *(const f4*)(P.qa + off + 4 * s4);
#pragma unroll
      for (int e = 0; e < 4; ++e) qaf[4 * s4 + e] = ta[e];
    }
  }
  const float lse_y2 = row_ok ? IO.row_stats[(bh * L + i) * ACATTN_NSTAT + 1] * kLog2e : 0.f;
  float qac[4][DT];
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const int row = i0 + 4 * g + s;
    const float* p = P.qa + (rowbase + min(row, L - 1)) * H + hoff + c;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) qac[s][dt] = row < L ? p[16 * dt] : 0.f;
  }

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

  auto body = [&](auto ntb_c) {
    constexpr int NTB = decltype(ntb_c)::value;

    // ---- Mt from the saved log-normaliser -----------------------------------------------------------------------------------
    f4 tM[NTB], dMa[NTB];
#pragma unroll
    for (int t = 0; t < NTB; ++t) tM[t] = f4{0.f, 0.f, 0.f, 0.f};
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
      const f4 y = tM[t] * scale2 + mask4(t);
#pragma unroll
      for (int r = 0; r < 4; ++r) tM[t][r] = ex2(y[r] - lse_y2) * okf;
    }

    // ---- the mask cotangent through dropout and the soft-max -> dSa -----------------------------------------------------------
    float r2 = 0.f;
#pragma unroll
    for (int t = 0; t < NTB; ++t) {
      uint32_t keep = 0xFu;
      if (has_drop)
        keep = P.p_drop == 0.5f ? rng_keep_mask_half(rkey, rng_row, (uint32_t)(4 * t + g))
                                : rng_group(rkey, rng_row, (uint32_t)(4 * t + g), P.p_drop).keep_mask;
      const f4 sm = keep_scale4(keep, keep_scale);
      dMa[t] = f4{0.f, 0.f, 0.f, 0.f};
      if (IO.d_attack_mask) dMa[t] = load_seg(IO.d_attack_mask + prow, t);
      // the mask penalty's cotangent from the rebuilt tile (acattn_bwd_io.d_penalty_part): d M = 2 d_pen (M - 1), M = Mt . keep
      if (IO.d_penalty_part) dMa[t] += (tM[t] * sm - 1.0f) * dpen2;
      dMa[t] *= sm;
      r2 += hsum(tM[t] * dMa[t]);
    }
    r2 = quad_sum(r2);
#pragma unroll
    for (int t = 0; t < NTB; ++t) dMa[t] = (tM[t] * (dMa[t] - r2)) * inv_sqrt;  // dSa

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

template <int DH>
int launch_attack(const acattn_problem& p, const acattn_bwd_io& io, float* gate_zero, hipStream_t stream) {
  const int nT = (p.L + 15) / 16, LP = nT * 16;
  const int n_slots = p.causal ? nT * (nT + 1) / 2 : nT * nT;
  const size_t lds = (size_t)(LP * (DH + 4) + LP + nT * 16 * TS + n_slots * 16 * (DH + 4)) * sizeof(float);
  auto kern = acattn_bwd_attack_kernel<DH>;
  if (lds > 64 * 1024) {
    const hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return (int)e;
  }
  hipLaunchKernelGGL(kern, dim3(p.B * p.n_heads), dim3(64 * nT), lds, stream, p, io, gate_zero, n_slots);
  return (int)hipGetLastError();
}

}  // namespace

// Returns -100 outside its domain: acattn_launch_bwd_fast's, an attack-only launch (dqa, dka alone) with a mask cotangent
// and no context cotangent, read rows or block bitmap.  `gate_zero`: a [B,L,L] buffer head 0's workgroups fill with zeros
// (the split's head-summed gate gradient, acattn_bwd.hip), or NULL.
int acattn_launch_bwd_attack(const acattn_problem& p, const acattn_bwd_io& io, hipStream_t stream, float* gate_zero) {
  const bool ok = p.L >= 1 && p.L <= 64 && (int64_t)p.B * p.n_heads * p.L * p.L < (1LL << 30) && (int64_t)p.B * p.L * p.H < (1LL << 30) &&
                  p.mask_mode == ACATTN_MASK_STRUCTURED && p.rng_mode == ACATTN_RNG_COUNTER && p.w_order && p.w_dist &&
                  p.adversarial && p.combine_option == ACATTN_COMBINE_GATE && p.two_level && io.attack_only &&
                  (io.d_attack_mask || io.d_penalty_part) && !io.d_ctx_attacked && !io.d_ctx_calibrated &&
                  !(io.read_rows && io.n_read_rows > 0) && !io.active_qblocks && !io.dqa2 && !io.dka2 && io.dqa && io.dka &&
                  io.row_stats;
  if (!ok) return -100;
  switch (p.H / p.n_heads) {
    case 16: return launch_attack<16>(p, io, gate_zero, stream);
    case 32: return launch_attack<32>(p, io, gate_zero, stream);
    case 64: return launch_attack<64>(p, io, gate_zero, stream);
  }
  return -100;
}
