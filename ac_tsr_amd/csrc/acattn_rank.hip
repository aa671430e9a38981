// Full-sort evaluation without the [B, N] scores, for gfx950 (MI355X): the rank of each row's target among the admissible
// items of the catalogue.
//
// Replaces, for leave-one-out evaluation (one positive per row), what the reference does per evaluation batch:
//     scores = full_sort_predict(...)            [B, N]  written once            recbole/trainer/trainer.py:926-941
//     scores[:, 0] = -inf; scores[history] = -inf        read and written again  trainer.py:942-944
//     topk_idx = topk(scores, K); gather(pos_matrix, topk_idx)                    recbole/evaluator/collector.py:141-153
// Hit / Recall / MRR / NDCG / Precision of a row with one positive are functions of ONE integer, the target's rank
//     rank[b] = 1 + #{ j admissible, j != target_b : s_bj ahead of s_b,target }
// and a rank is a count: no soft-max, no selection network, no [B, K] merge, no float atomics.
//
// The sweep has the shape of ce_fwd_kernel (acattn_ce.hip): items stationary (a wave keeps 16 * NTILES table rows as MFMA A
// fragments for the whole launch), the batch swept in 16-row blocks with the next block's rows in flight under the current
// block's products, scores^T = E . out^T on exact-fp32 MFMA 16x16x4.  The batch row sits on the lane, so the target's score of
// a row is one register per block and the comparison is register-local.
//
// ONE ARITHMETIC FOR EVERY SCORE.  A score is the accumulator chain  acc = mfma16(e[s], h[s], acc), s = 0 .. CH/4 - 1, with
// lane (c, g) supplying columns (CH/4) g + s of its table row and its batch row -- in a main tile, in the ragged last tile and
// in rank_pair_score_kernel (which keeps the diagonal of the same 16x16 product).  An element of the product depends on its
// own row and column only, so a (row, item) pair has the same bits wherever it is formed.  The tie rule rests on this: an item
// is ahead iff !(s_j <= s_t), so the target itself (s_j == s_t bit for bit) and every item whose table row equals the
// target's are never counted, and no test against target[row] is needed inside the sweep.  A NaN item score counts as ahead
// (torch.topk orders NaN first); a NaN target score makes every comparison true and the fold writes rank 0, "invalid".
// This file is built WITHOUT -fno-honor-nans: the rule above needs honest comparisons.
#include <stdlib.h>

#include "acattn_common.h"

namespace {

constexpr int RK_NW = 4;  // waves per workgroup

__device__ __forceinline__ int quad_sum_i(int x) {
  auto r = __builtin_amdgcn_permlane16_swap((uint32_t)x, (uint32_t)x, false, false);
  const uint32_t y = r[0] + r[1];
  auto s = __builtin_amdgcn_permlane32_swap(y, y, false, false);
  return (int)(s[0] + s[1]);
}

// lane (c, g)'s fragment of a [.., CH] row: columns (CH/4) g .. (CH/4) g + CH/4 - 1; zeros for row == nullptr
template <int CH>
__device__ __forceinline__ void load_frag(const float* __restrict__ row, const int g, float (&dst)[CH / 4]) {
  constexpr int KS = CH / 4;
#pragma unroll
  for (int s4 = 0; s4 < KS / 4; ++s4) {
    f4 v = {0.f, 0.f, 0.f, 0.f};
    if (row) v = *(const f4*)(row + KS * g + 4 * s4);
#pragma unroll
    for (int e = 0; e < 4; ++e) dst[4 * s4 + e] = v[e];
  }
}

// ---------------------------------------------------------------------------------------------------------
// (a) scores of a list of (row, item) pairs: one wave per 16 pairs, the diagonal of E_gathered . out_gathered^T
// ---------------------------------------------------------------------------------------------------------
// pair_row == nullptr: the B target pairs (b, target[b]); st_out[b] = the score, NaN for a target outside
// [first_item, N) (clamped for the address, never read out of bounds).
// pair_row != nullptr: history exclusion.  A pair whose item was counted as ahead by the sweep takes 1 off rank[row]
// (integer atomic: the result does not depend on the order).  Ignored: rows outside [0, B), items outside [first_item, N),
// the target itself, rows whose rank is the invalid marker (NaN target score).
template <int CH>
__global__ void __launch_bounds__(64 * RK_NW) rank_pair_score_kernel(const acattn_ce_problem P, const int first_item,
                                                                     const int64_t* __restrict__ pair_row,
                                                                     const int64_t* __restrict__ pair_item, const int64_t n_pairs,
                                                                     float* __restrict__ st_out, const float* __restrict__ st_in,
                                                                     int* __restrict__ rank) {
  constexpr int KS = CH / 4;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int c = lane & 15, g = lane >> 4;
  const bool excl = pair_row != nullptr;
  const int64_t n = excl ? n_pairs : (int64_t)P.B;
  const int64_t p0 = ((int64_t)blockIdx.x * RK_NW + wave) * 16;
  if (p0 >= n) return;  // (uniform per wave)
  const int64_t p = p0 + c;
  long long row = 0, item = 0;
  bool ok = false;
  if (p < n) {
    if (excl) {
      row = pair_row[p];
      item = pair_item[p];
      ok = row >= 0 && row < P.B && item >= first_item && item < P.N;
      if (ok) ok = item != P.target[row];
    } else {
      row = p;
      item = P.target[p];
      ok = item >= first_item && item < P.N;
    }
  }
  float ef[KS], hf[KS];
  load_frag<CH>(ok ? P.table + (size_t)item * CH : nullptr, g, ef);
  load_frag<CH>(ok ? P.out + (size_t)row * CH : nullptr, g, hf);
  f4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int s = 0; s < KS; ++s) acc = mfma16(ef[s], hf[s], acc);
  // D[i][j] = item_i . row_j sits in register i & 3 of lane (j, i >> 2): the diagonal element of pair c in lane (c, c >> 2)
  if (g == (c >> 2) && p < n) {
    const int r = c & 3;
    const float s = r == 0 ? acc[0] : r == 1 ? acc[1] : r == 2 ? acc[2] : acc[3];
    if (!excl) {
      st_out[p] = ok ? s : __builtin_nanf("");
    } else if (ok) {
      const float t = st_in[row];
      if (t == t && !(s <= t)) atomicSub(rank + row, 1);
    }
  }
}

// ---------------------------------------------------------------------------------------------------------
// (b) the sweep: part[wave][row] = # items of the wave's 16 * NTILES that are ahead of the row's target
// ---------------------------------------------------------------------------------------------------------
template <int CH, int NTILES>
__global__ void __launch_bounds__(64 * RK_NW) rank_sweep_kernel(const acattn_ce_problem P, const int first_item,
                                                                const float* __restrict__ st, int* __restrict__ part) {
  constexpr int KS = CH / 4, ITEMS = 16 * NTILES;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int c = lane & 15, g = lane >> 4;
  const int wid = blockIdx.x * RK_NW + wave;
  const int item0 = wid * ITEMS;
  const int B = P.B, N = P.N;

  float ef[NTILES][KS];  // A operand: table rows of this wave, lane (c, g) holds row 16t+c, columns KS*g ..
#pragma unroll
  for (int t = 0; t < NTILES; ++t) {
    const int item = item0 + 16 * t + c;
    load_frag<CH>(item < N ? P.table + (size_t)item * CH : nullptr, g, ef[t]);
  }
  const int nrb = (B + 15) >> 4;
  // the admissible range [first_item, N) is tested only in the waves that straddle one of its ends (uniform per wave)
  const bool edge = item0 < first_item || item0 + ITEMS > N;
  float hf[KS];
  float s_t;
  auto load_rows = [&](int rb, float (&dst)[KS], float& s_dst) {
    const int row = 16 * rb + c;
    load_frag<CH>(row < B ? P.out + (size_t)row * CH : nullptr, g, dst);
    s_dst = row < B ? st[row] : 0.f;
  };
  load_rows(0, hf, s_t);
  for (int rb = 0; rb < nrb; ++rb) {
    float hn[KS];
    float s_n = 0.f;
    if (rb + 1 < nrb) load_rows(rb + 1, hn, s_n);  // next block's rows are in flight under this block's MFMAs
    f4 acc[NTILES];
#pragma unroll
    for (int t = 0; t < NTILES; ++t) acc[t] = f4{0.f, 0.f, 0.f, 0.f};
    // k-step outer, tiles inner (independent accumulators back to back); per tile ONE chain in ascending k
#pragma unroll
    for (int s = 0; s < KS; ++s)
#pragma unroll
      for (int t = 0; t < NTILES; ++t) acc[t] = mfma16(ef[t][s], hf[s], acc[t]);
    if (edge) {
#pragma unroll
      for (int t = 0; t < NTILES; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int item = item0 + 16 * t + 4 * g + r;
          if (item < first_item || item >= N) acc[t][r] = ACATTN_NEG_INF;  // never ahead of a non-NaN target score
        }
    }
    int cnt = 0;
#pragma unroll
    for (int t = 0; t < NTILES; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) cnt += (acc[t][r] <= s_t) ? 0 : 1;  // NaN item score: ahead
    cnt = quad_sum_i(cnt);
    const int row = 16 * rb + c;
    if (g == 0 && row < B) part[(size_t)wid * B + row] = cnt;
    if (rb + 1 < nrb) {
#pragma unroll
      for (int s = 0; s < KS; ++s) hf[s] = hn[s];
      s_t = s_n;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------
// (c) rank[b] = 1 + sum_w part[w][b], 0 for a NaN target score; target_score[b]
// ---------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) rank_fold_kernel(const int* __restrict__ part, const int n_waves, const float* __restrict__ st,
                                                        const int B, int* __restrict__ rank, float* __restrict__ target_score) {
  const int rl = threadIdx.x & 63, q = threadIdx.x >> 6;
  const int row = blockIdx.x * 64 + rl;
  int a[4] = {0, 0, 0, 0};
  if (row < B) {
    const int* ps = part + row;
    int w = q;
    for (; w + 12 < n_waves; w += 16) {
#pragma unroll
      for (int u = 0; u < 4; ++u) a[u] += ps[(size_t)(w + 4 * u) * B];
    }
    for (; w < n_waves; w += 4) a[0] += ps[(size_t)w * B];
  }
  __shared__ int red[4][64];
  red[q][rl] = (a[0] + a[1]) + (a[2] + a[3]);
  __syncthreads();
  if (q == 0 && row < B) {
    const int total = (red[0][rl] + red[1][rl]) + (red[2][rl] + red[3][rl]);
    const float s = st[row];
    rank[row] = (s == s) ? 1 + total : 0;
    target_score[row] = s;
  }
}

int num_cus() {
  static int n = 0;
  if (!n) {
    int dev = 0;
    hipDeviceProp_t prop;
    if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess) n = prop.multiProcessorCount;
    if (n <= 0) n = 256;
  }
  return n;
}

// 16-item tiles per wave, as ce_fwd_kernel's launcher picks them: the smallest count of {1, 2, 4, 6, 7} (hidden 64),
// {1, 2, 3} (128), {1} (256) whose single round of (#CUs) workgroups covers N items; the largest beyond.
int pick_tiles(int H, int N) {
  const int64_t per_tile = (int64_t)num_cus() * RK_NW * 16;
  const int64_t need = (N + per_tile - 1) / per_tile;
  if (H == 64) return need <= 1 ? 1 : need <= 2 ? 2 : need <= 4 ? 4 : need <= 6 ? 6 : 7;
  if (H == 128) return need <= 1 ? 1 : need <= 2 ? 2 : 3;
  return 1;
}

inline int64_t align256(int64_t x) { return (x + 255) / 256 * 256; }

int n_workgroups(int N, int tiles) { return (int)(((int64_t)N + RK_NW * 16 * tiles - 1) / (RK_NW * 16 * tiles)); }

template <int CH, int NTILES>
int launch_t(const acattn_ce_problem& p, int first_item, void* ws, int* rank, float* target_score, hipStream_t stream) {
  const int n_wg = n_workgroups(p.N, NTILES);
  float* st = (float*)ws;
  int* part = (int*)((char*)ws + align256((int64_t)p.B * (int64_t)sizeof(float)));
  hipLaunchKernelGGL((rank_pair_score_kernel<CH>), dim3((p.B + 16 * RK_NW - 1) / (16 * RK_NW)), dim3(64 * RK_NW), 0, stream, p,
                     first_item, (const int64_t*)nullptr, (const int64_t*)nullptr, (int64_t)0, st, (const float*)nullptr,
                     (int*)nullptr);
  hipLaunchKernelGGL((rank_sweep_kernel<CH, NTILES>), dim3(n_wg), dim3(64 * RK_NW), 0, stream, p, first_item, (const float*)st, part);
  hipLaunchKernelGGL(rank_fold_kernel, dim3((p.B + 63) / 64), dim3(256), 0, stream, (const int*)part, n_wg * RK_NW,
                     (const float*)st, p.B, rank, target_score);
  return (int)hipGetLastError();
}

template <int CH>
int launch_exclude_t(const acattn_ce_problem& p, int first_item, const int64_t* pair_row, const int64_t* pair_item, int64_t n_pairs,
                     const float* target_score, int* rank, hipStream_t stream) {
  const int64_t n_blocks = (n_pairs + 16 * RK_NW - 1) / (16 * RK_NW);
  hipLaunchKernelGGL((rank_pair_score_kernel<CH>), dim3((unsigned)n_blocks), dim3(64 * RK_NW), 0, stream, p, first_item, pair_row,
                     pair_item, n_pairs, (float*)nullptr, target_score, rank);
  return (int)hipGetLastError();
}

}  // namespace

int64_t acattn_rank_ws_bytes(const acattn_ce_problem& p) {
  const int tiles = pick_tiles(p.H, p.N);
  return align256((int64_t)p.B * (int64_t)sizeof(float)) +
         (int64_t)n_workgroups(p.N, tiles) * RK_NW * p.B * (int64_t)sizeof(int);
}

int acattn_launch_rank(const acattn_ce_problem& p, int first_item, void* ws, int* rank, float* target_score, hipStream_t stream) {
  const int tiles = pick_tiles(p.H, p.N);
  switch (p.H) {
    case 64:
      switch (tiles) {
        case 1: return launch_t<64, 1>(p, first_item, ws, rank, target_score, stream);
        case 2: return launch_t<64, 2>(p, first_item, ws, rank, target_score, stream);
        case 4: return launch_t<64, 4>(p, first_item, ws, rank, target_score, stream);
        case 6: return launch_t<64, 6>(p, first_item, ws, rank, target_score, stream);
        default: return launch_t<64, 7>(p, first_item, ws, rank, target_score, stream);
      }
    case 128:
      switch (tiles) {
        case 1: return launch_t<128, 1>(p, first_item, ws, rank, target_score, stream);
        case 2: return launch_t<128, 2>(p, first_item, ws, rank, target_score, stream);
        default: return launch_t<128, 3>(p, first_item, ws, rank, target_score, stream);
      }
    case 256: return launch_t<256, 1>(p, first_item, ws, rank, target_score, stream);
  }
  return -1;
}

int acattn_launch_rank_exclude(const acattn_ce_problem& p, int first_item, const int64_t* pair_row, const int64_t* pair_item,
                               int64_t n_pairs, const float* target_score, int* rank, hipStream_t stream) {
  switch (p.H) {
    case 64: return launch_exclude_t<64>(p, first_item, pair_row, pair_item, n_pairs, target_score, rank, stream);
    case 128: return launch_exclude_t<128>(p, first_item, pair_row, pair_item, n_pairs, target_score, rank, stream);
    case 256: return launch_exclude_t<256>(p, first_item, pair_row, pair_item, n_pairs, target_score, rank, stream);
  }
  return -1;
}
