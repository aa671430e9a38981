// y = dropout(LayerNorm(cat(item_embedding[idx], user_embedding[user]) + position_embedding)) and its backward, gfx950: one
// launch forward, one (+ a small row sum for the user table) backward.
//
// The front end of ACSSEPT (recbole/model/sequential_recommender/acssept.py:120-131): torch runs two gathers, an expand, a
// cat, an add, LayerNorm and dropout as separate HBM round trips.  Here, as in acattn_embed.hip:
//   forward  : a row (H/4 adjacent lanes, 16 bytes each) is gathered straight from the two tables -- lanes left of the seam
//              (column Di) read the item row, lanes right of it the sequence's user row; Di and H - Di are multiples of 4, so
//              no lane straddles the seam -- normalised and written once; (mean, 1/std) are kept for the backward;
//   backward : workgroup (l, chunk) walks the sequences of its chunk at ONE position l (the position-embedding gradient
//              accumulates in registers); the row is re-gathered, the LayerNorm backward is formed in registers and each
//              item lane scatters its four columns with float atomics into the item-table gradient.  Rows of the two
//              padding indices are skipped, as nn.Embedding does.  A user row collects the L positions of each of its
//              sequences.  Scattered per (b, l) like the item half that is L atomics per address, issued at the same moment
//              by the L workgroups that walk the same sequences (3.0 x the item-only backward at B = 512, L = 50, 64 + 64:
//              profiles/ssept_front_end.txt).  So, given a [rows, H - Di] workspace, the user lanes store their columns
//              there instead and a second, small kernel sums each sequence over its L positions and adds ONE atomic per
//              (sequence, column); users need not be distinct either way.
#include <algorithm>

#include "acattn_common.h"
#include "acattn_rowops.h"

namespace {

__device__ __forceinline__ int64_t clamp_id(int64_t id, int64_t n) {
  return id < 0 ? 0 : (id >= n ? n - 1 : id);  // an out-of-range id must not become an out-of-bounds read
}

// the 16 bytes lane c4 of a row reads: item columns left of the seam, user columns right of it
template <int H>
__device__ __forceinline__ const float* lane_source(const acattn_embed_user_problem& P, int64_t id, int64_t uid, int c4) {
  const int col = 4 * c4;
  return col < P.Di ? P.table + id * P.Di + col : P.user_table + uid * (H - P.Di) + (col - P.Di);
}

template <int H>
__global__ void __launch_bounds__(256) embed_user_ln_fwd_kernel(const acattn_embed_user_problem P, float* __restrict__ y,
                                                                float* __restrict__ stats) {
  constexpr int LPR = H / 4;
  constexpr int RPB = 256 / LPR;
  const int c4 = threadIdx.x % LPR, rsub = threadIdx.x / LPR;
  const uint64_t seed = P.seed + (P.seed_device ? *P.seed_device : 0ull);
  const f4 gm = *(const f4*)(P.gamma + 4 * c4), bt = *(const f4*)(P.beta + 4 * c4);
  for (int row = blockIdx.x * RPB + rsub; row < P.rows; row += gridDim.x * RPB) {
    const int64_t raw = P.idx[row];
    const int64_t id = clamp_id(raw, P.n_table_rows);
    const int64_t uid = clamp_id(P.user[row / P.L], P.n_user_rows);
    f4 s = *(const f4*)lane_source<H>(P, id, uid, c4);
    if (P.pos) s += *(const f4*)(P.pos + (size_t)(row % P.L) * H + 4 * c4);
    const float mean = row_sum<LPR>((s[0] + s[1]) + (s[2] + s[3])) * (1.0f / H);
    const f4 d = s - mean;
    const float var = row_sum<LPR>((d[0] * d[0] + d[1] * d[1]) + (d[2] * d[2] + d[3] * d[3])) * (1.0f / H);
    const float rstd = __builtin_amdgcn_rsqf(var + P.eps);
    const f4 keep = row_keep_scale(P.p_drop, P.keep, seed, row, c4, H);
    *(f4*)(y + (size_t)row * H + 4 * c4) = ((d * rstd) * gm + bt) * keep;
    if (c4 == 0) {
      *(float2*)(stats + 2 * (size_t)row) = float2{mean, rstd};
      if (P.nonzero_out) P.nonzero_out[row] = raw != 0;
    }
  }
}

template <int H>
__global__ void __launch_bounds__(256) embed_user_ln_bwd_kernel(const acattn_embed_user_problem P, const float* __restrict__ dy,
                                                                const float* __restrict__ stats, const int64_t item_padding_idx,
                                                                const int64_t user_padding_idx, float* __restrict__ d_item,
                                                                float* __restrict__ d_user, float* __restrict__ user_rows,
                                                                float* __restrict__ d_pos_part, float* __restrict__ dgb_part) {
  constexpr int LPR = H / 4;
  constexpr int RPB = 256 / LPR;
  const int c4 = threadIdx.x % LPR, rsub = threadIdx.x / LPR;
  const int l = blockIdx.x, bc = blockIdx.y, BC = gridDim.y;
  const int B = P.rows / P.L;
  const int per = (B + BC - 1) / BC;
  const int b_end = min(B, (bc + 1) * per);
  const uint64_t seed = P.seed + (P.seed_device ? *P.seed_device : 0ull);
  const f4 gm = *(const f4*)(P.gamma + 4 * c4);
  f4 pos = {0.f, 0.f, 0.f, 0.f};
  if (P.pos) pos = *(const f4*)(P.pos + (size_t)l * H + 4 * c4);
  f4 acc_g = {0.f, 0.f, 0.f, 0.f}, acc_b = acc_g, acc_p = acc_g;
  const bool item_lane = 4 * c4 < P.Di;
  for (int b = bc * per + rsub; b < b_end; b += RPB) {
    const int row = b * P.L + l;
    const int64_t id = clamp_id(P.idx[row], P.n_table_rows);
    const int64_t uid = clamp_id(P.user[b], P.n_user_rows);
    const size_t o = (size_t)row * H + 4 * c4;
    const f4 s = *(const f4*)lane_source<H>(P, id, uid, c4) + pos;
    const float2 st = *(const float2*)(stats + 2 * (size_t)row);
    const f4 xh = (s - st.x) * st.y;
    const f4 g = *(const f4*)(dy + o) * row_keep_scale(P.p_drop, P.keep, seed, row, c4, H);  // dropout sits AFTER the norm
    acc_g += g * xh;
    acc_b += g;
    const f4 gg = g * gm;
    const float m1 = row_sum<LPR>((gg[0] + gg[1]) + (gg[2] + gg[3])) * (1.0f / H);
    const float m2 = row_sum<LPR>((gg[0] * xh[0] + gg[1] * xh[1]) + (gg[2] * xh[2] + gg[3] * xh[3])) * (1.0f / H);
    const f4 dx = (gg - m1 - xh * m2) * st.y;
    acc_p += dx;
    float* t = nullptr;
    if (item_lane) {
      if (d_item && id != item_padding_idx) t = d_item + id * P.Di + 4 * c4;
    } else if (user_rows) {  // summed over the sequence's positions by embed_user_sum_kernel
      *(f4*)(user_rows + (size_t)row * (H - P.Di) + (4 * c4 - P.Di)) = dx;
    } else {
      if (d_user && uid != user_padding_idx) t = d_user + uid * (H - P.Di) + (4 * c4 - P.Di);
    }
    if (t) {
#pragma unroll
      for (int e = 0; e < 4; ++e) unsafeAtomicAdd(t + e, dx[e]);
    }
  }
  // fold the RPB row slots of the workgroup through LDS
  __shared__ float red[3 * 256 * 4];
  *(f4*)(red + 4 * threadIdx.x) = acc_g;
  *(f4*)(red + 1024 + 4 * threadIdx.x) = acc_b;
  *(f4*)(red + 2048 + 4 * threadIdx.x) = acc_p;
  __syncthreads();
  if (rsub == 0) {
    f4 sg = {0.f, 0.f, 0.f, 0.f}, sb = sg, sp = sg;
#pragma unroll
    for (int k = 0; k < RPB; ++k) {
      sg += *(const f4*)(red + 4 * (k * LPR + c4));
      sb += *(const f4*)(red + 1024 + 4 * (k * LPR + c4));
      sp += *(const f4*)(red + 2048 + 4 * (k * LPR + c4));
    }
    const size_t wg = (size_t)bc * P.L + l;
    if (dgb_part) {
      *(f4*)(dgb_part + wg * 2 * H + 4 * c4) = sg;
      *(f4*)(dgb_part + wg * 2 * H + H + 4 * c4) = sb;
    }
    if (d_pos_part) *(f4*)(d_pos_part + wg * H + 4 * c4) = sp;  // [BC, L, H]
  }
}

// d_user[user[b], col] += sum_l user_rows[b, l, col]: thread (b, col), consecutive threads read consecutive columns
__global__ void __launch_bounds__(256) embed_user_sum_kernel(const float* __restrict__ user_rows, const int64_t* __restrict__ user,
                                                             int B, int L, int Du, int64_t n_user_rows,
                                                             int64_t user_padding_idx, float* __restrict__ d_user) {
  const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (gid >= (int64_t)B * Du) return;
  const int b = (int)(gid / Du), col = (int)(gid % Du);
  const int64_t uid = clamp_id(user[b], n_user_rows);
  if (uid == user_padding_idx) return;
  const float* src = user_rows + (size_t)b * L * Du + col;
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
  int l = 0;
  for (; l + 4 <= L; l += 4) {
    s0 += src[(size_t)l * Du];
    s1 += src[(size_t)(l + 1) * Du];
    s2 += src[(size_t)(l + 2) * Du];
    s3 += src[(size_t)(l + 3) * Du];
  }
  for (; l < L; ++l) s0 += src[(size_t)l * Du];
  unsafeAtomicAdd(d_user + uid * Du + col, (s0 + s1) + (s2 + s3));
}

template <int H>
int launch_fwd(const acattn_embed_user_problem& p, float* y, float* stats, hipStream_t stream) {
  constexpr int RPB = 256 / (H / 4);
  const int grid = (int)std::min<int64_t>(((int64_t)p.rows + RPB - 1) / RPB, 2048);
  hipLaunchKernelGGL((embed_user_ln_fwd_kernel<H>), dim3(grid), dim3(256), 0, stream, p, y, stats);
  return (int)hipGetLastError();
}

template <int H>
int launch_bwd(const acattn_embed_user_problem& p, const float* dy, const float* stats, int64_t item_padding_idx,
               int64_t user_padding_idx, float* d_item, float* d_user, float* user_rows, float* d_pos_part, float* dgb_part,
               hipStream_t stream) {
  if (!d_user) user_rows = nullptr;
  hipLaunchKernelGGL((embed_user_ln_bwd_kernel<H>), dim3(p.L, ACATTN_EMBED_BWD_CHUNKS), dim3(256), 0, stream, p, dy, stats,
                     item_padding_idx, user_padding_idx, d_item, d_user, user_rows, d_pos_part, dgb_part);
  if (const int rc = (int)hipGetLastError()) return rc;
  if (user_rows) {
    const int B = p.rows / p.L, Du = H - p.Di;
    const int grid = (int)(((int64_t)B * Du + 255) / 256);
    hipLaunchKernelGGL(embed_user_sum_kernel, dim3(grid), dim3(256), 0, stream, user_rows, p.user, B, p.L, Du, p.n_user_rows,
                       user_padding_idx, d_user);
  }
  return (int)hipGetLastError();
}

}  // namespace

int acattn_launch_embed_user_fwd(const acattn_embed_user_problem& p, float* y, float* stats, hipStream_t stream) {
  switch (p.H) {
    case 64: return launch_fwd<64>(p, y, stats, stream);
    case 128: return launch_fwd<128>(p, y, stats, stream);
    case 256: return launch_fwd<256>(p, y, stats, stream);
  }
  return -1;
}

int acattn_launch_embed_user_bwd(const acattn_embed_user_problem& p, const float* dy, const float* stats,
                                 int64_t item_padding_idx, int64_t user_padding_idx, float* d_item, float* d_user,
                                 float* user_rows, float* d_pos_part, float* dgb_part, hipStream_t stream) {
  switch (p.H) {
    case 64: return launch_bwd<64>(p, dy, stats, item_padding_idx, user_padding_idx, d_item, d_user, user_rows, d_pos_part, dgb_part, stream);
    case 128: return launch_bwd<128>(p, dy, stats, item_padding_idx, user_padding_idx, d_item, d_user, user_rows, d_pos_part, dgb_part, stream);
    case 256: return launch_bwd<256>(p, dy, stats, item_padding_idx, user_padding_idx, d_item, d_user, user_rows, d_pos_part, dgb_part, stream);
  }
  return -1;
}
