// The TIME-INTERVAL attention core of ACTiSASRec (L <= 64): recbole/model/transformer_layers.py:1010-1422, the encoder
// actisasrec.py:59 builds.  A sibling of acattn_unnorm.hip (same frame, same mixtures, none of the three re-normalising
// soft-maxes), not a flag through it: the frame both share is acattn_row64.h, the time terms are here.  Per head, with
// pk_j / pv_j the head's slices of the dropped absolute-position rows, t_ij = time_index[b, i, j], TK_ij = drop(time_k[t_ij]), TV_ij = drop(time_v[t_ij]):
//     S  = q.(K + pk)^T + q_i.TK_ij + e_order + e_distance       transformer_layers.py:1125-1166 (the spatial terms see the
//                                                                plain k only, :1142-1145)
//     P  = dropout(softmax(S / sqrt(dh) + mask))                 :1168-1176
//     M  = dropout(softmax(qa.Ka^T / sqrt(dh) + mask))           :1065-1082 (no position and no time term)
//     A_att = P M + N (1 - M),  A_w = P (g + (1 - g) exp(1 - M)) :1297-1303, :1274-1275
//     ctx_x[i] = sum_j A_x[i,j] (v_j + pv_j + TV_ij)             :1084-1090
//
// The time terms are not MFMA work: every (i, j) has its own dh-vector.  The reference gathers them as two [B,L,L,H]
// tensors; here the four lanes of a query row each gather THEIR quarter of the table row (KS = dh / 4 contiguous floats,
// the quad reads the whole head slice) from global memory -- both tables are L2-resident (2 x 64 KB at H = 64, span 256) --
// and replay the dropout bits (explicit bytes, or one hash per (pair, table, 32 columns) in counter mode).  A row's quad
// sums the partial dot products with two permlane swaps per key.
//   - k + pk and v + pv are summed while staging; the key halves of the spatial affines are formed from the plain k in the
//     same pass, and the one later use of the plain k (the affine weights' gradients) reads it from global memory again;
//   - every key j < L enters the value sums, padded and future ones included (A_att = N where M = 0); a zero weight of the
//     CALIBRATED mixture skips its TV row (0 x a non-finite row reached only through masked keys stays 0);
//   - for j >= L (tile padding) nothing is read: no index, and TK, TV, pk, pv are zeros;
//   - time_index is clamped into [0, time_span] wherever a table is addressed.
//
// Backward: phase A / phase B of acattn_unnorm.hip.  Phase A also adds d_ctx_x[i].TV_ij to dA_x, adds sum_j dS_ij TK_ij to
// dq, and writes dS, A_att, A_w ([B,nh,L,L] each) for the second launch; phase B writes the product share of dk as d pos_k.
// timeaware_table_grad_kernel owns the two table gradients: a workgroup takes one head and a stride of the sequences, sums
// into a (time_span + 1) x dh fp32 table per time table in its LDS (runs of equal indices are summed in a register first:
// real batches put most pairs on row time_span and row 0), and flushes once with one float atomic per non-zero element.
// Those two outputs alone depend on the order of atomics; everything else gives the same bits in two launches.
#include <algorithm>

#include "acattn_row64.h"

#define ACATTN_L64_WHAT "time-aware attention"
#include "acattn_l64_checks.inc"

namespace {

constexpr int kMaxLds = 160 * 1024;

// ------------------------------------------------------------------------------------------------------------------------
// the time dropout's counter stream: one 32-bit word per (pair = (b L + i) L + j, table, 32 columns).  p == 0.5: column c
// keeps iff bit c % 32 of the word is set; any other p: the high 16 bits of a second-stage hash per column against p * 65536.
// The key is derived with constants of its own: disjoint from rng_group's stream for every seed.
// ------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ RngKey time_rng_key(uint64_t seed) {
  RngKey k = rng_key(seed ^ 0x74696D6562697473ull);
  k.a = mix32(k.a ^ 0x5BD1E995u);
  k.b = mix32(k.b + 0x2545F491u);
  return k;
}
__device__ __forceinline__ uint32_t time_word(const RngKey key, uint32_t pair, uint32_t which, uint32_t chunk, uint32_t nchunk) {
  uint32_t x = ((pair * 2u + which) * nchunk + chunk) ^ key.a;
  x *= 0x7feb352dU;
  x ^= x >> 15;
  x *= 0x846ca68bU;
  x ^= x >> 16;
  return x + key.b;
}
__device__ __forceinline__ uint32_t time_keep1(uint32_t w, int col, float p) {
  if (p == 0.5f) return (w >> (col & 31)) & 1u;
  const uint32_t thr = (uint32_t)(p * 65536.0f);
  return (rng_word(w, 0x9E3779B9u * (uint32_t)((col & 31) + 1), 0x85EBCA77u) >> 16) >= thr ? 1u : 0u;
}

// What the kernels need of acattn_time_ext, per thread.
struct TimeCtx {
  const acattn_time_ext& T;
  int H, L, span;
  bool drop, counter;
  float ks, p;
  RngKey key;
  uint32_t nchunk;
  __device__ __forceinline__ TimeCtx(const acattn_time_ext& T_, int H_, int L_) : T(T_) {
    H = H_;
    L = L_;
    span = T.time_span;
    p = T.p_time;
    drop = p > 0.f;
    counter = drop && !T.keep_time_k;
    ks = drop ? 1.0f / (1.0f - p) : 1.0f;
    nchunk = (uint32_t)((H + 31) >> 5);
    key = time_rng_key(T.time_seed + (T.time_seed_device ? *T.time_seed_device : 0ull));
  }
  // the clamped table row of pair (row = b L + i, j)
  __device__ __forceinline__ int index(size_t pair) const {
    const int t = T.time_index[pair];
    return t < 0 ? 0 : (t > span ? span : t);
  }
  // keep bits of the N columns col0 .. col0 + N - 1 (N <= 16, inside one 32-column chunk) of table `which` at `pair`
  template <int N>
  __device__ __forceinline__ uint32_t keep(int which, size_t pair, int col0) const {
    if (!drop) return 0xFFFFu;
    uint32_t bits = 0;
    if (!counter) {
      const uint8_t* kp = (which ? T.keep_time_v : T.keep_time_k) + pair * H + col0;
#pragma unroll
      for (int e4 = 0; e4 < N / 4; ++e4) {
        const uint32_t v = *(const uint32_t*)(kp + 4 * e4);
#pragma unroll
        for (int e = 0; e < 4; ++e) bits |= (((v >> (8 * e)) & 0xFFu) ? 1u : 0u) << (4 * e4 + e);
      }
      return bits;
    }
    const uint32_t w = time_word(key, (uint32_t)pair, (uint32_t)which, (uint32_t)(col0 >> 5), nchunk);
    if (p == 0.5f) return (w >> (col0 & 31)) & ((1u << N) - 1u);
#pragma unroll
    for (int e = 0; e < N; ++e) bits |= time_keep1(w, col0 + e, p) << e;
    return bits;
  }
  __device__ __forceinline__ uint32_t keep1(int which, size_t pair, int col) const {
    if (!drop) return 1u;
    if (!counter) return (which ? T.keep_time_v : T.keep_time_k)[pair * H + col] ? 1u : 0u;
    return time_keep1(time_word(key, (uint32_t)pair, (uint32_t)which, (uint32_t)(col >> 5), nchunk), col, p);
  }
  // four columns of the dropped row t of table `which`; `bits` = keep<N>() of the lane's columns, e4 = which four of them
  __device__ __forceinline__ f4 row4(int which, int t, int col, uint32_t bits, int e4) const {
    const f4 v = *(const f4*)((which ? T.time_v : T.time_k) + (size_t)t * H + col);
    return v * keep_scale4(bits >> (4 * e4), ks);
  }
};

// blockDim.x == 4 * LP: thread idx + it * blockDim covers the LP x DH/4 16-byte pieces of a matrix in DH / 16 rounds
template <int DH>
__device__ __forceinline__ void stage(const acattn_problem& P, const acattn_time_ext& T, const Staged<DH>& S, size_t rowbase,
                                      int hoff, int L, int LP) {
  constexpr int VS = DH + 4, C4 = DH / 4;
  const f4 w_ko = *(const f4*)(P.w_order + DH + 4 * (threadIdx.x % C4));
  const f4 w_kd = *(const f4*)(P.w_dist + DH + 4 * (threadIdx.x % C4));
#pragma unroll
  for (int it = 0; it < DH / 16; ++it) {
    const int idx = threadIdx.x + it * blockDim.x;
    const int row = idx / C4, c4 = idx - row * C4;
    f4 kv = {0.f, 0.f, 0.f, 0.f}, kav = kv, vv = kv, pk = kv, pv = kv;
    if (row < L) {
      const size_t o = (rowbase + row) * P.H + hoff + 4 * c4;
      kv = *(const f4*)(P.k + o);
      kav = *(const f4*)(P.ka + o);
      vv = *(const f4*)(P.v + o);
      pk = *(const f4*)(T.pos_k + o);
      pv = *(const f4*)(T.pos_v + o);
    }
    *(f4*)(S.Ks + row * VS + 4 * c4) = kv + pk;
    *(f4*)(S.Kas + row * VS + 4 * c4) = kav;
    *(f4*)(S.Vs + row * VS + 4 * c4) = vv + pv;
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

// RowCore plus the time terms.  Of the context cotangents and the time rows the lane holds the columns KS g .. KS g + KS - 1,
// as it does of q and qa.
template <int DH>
struct Row : RowCore<DH> {
  using Core = RowCore<DH>;
  using Core::KS, Core::VS, Core::P, Core::L, Core::c, Core::g, Core::i, Core::row_ok, Core::rowbase, Core::hoff, Core::qf;
  using Core::ll_row;  // this row's L indices of time_index
  const TimeCtx& TC;

  __device__ __forceinline__ Row(const acattn_problem& P_, const Staged<DH>& S_, const TimeCtx& TC_, int b, int h, int qb_,
                                 int lane)
      : Core(P_, S_, b, h, qb_, lane, true), TC(TC_) {}

  // The value the lane that owns key (t, gj, r) of this row holds, in all four lanes of the row (exact: x + 0 + 0 + 0).
  __device__ __forceinline__ float from_owner(float mine, int gj) const { return quad_sum(g == gj ? mine : 0.f); }

  // f(t, gj, r, j, pair) for every key j < L in ascending order; the index a lane reads is its OWN row's (row 0 of the
  // sequence for a row past L: valid memory, and nothing of such a row is stored)
  template <int NTB, class F>
  __device__ __forceinline__ void each_key(F&& f) const {
#pragma unroll
    for (int t = 0; t < NTB; ++t)
#pragma unroll
      for (int gj = 0; gj < 4; ++gj)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int j = 16 * t + 4 * gj + r;
          if (j < L) f(t, gj, r, j, ll_row + j);  // (wave-uniform)
        }
  }
  // acc[t][r] += v[.] . drop(table[t_ij])[.] over the head's columns, for every key of the row; `v0`, `v1`: the lane's KS
  // columns of one or two row vectors (two share the gathered row)
  template <int NTB, bool TWO>
  __device__ __forceinline__ void time_dots(int which, const float (&v0)[KS], const float (&v1)[KS], f4 (&a0)[NTB],
                                            f4 (&a1)[NTB]) const {
    const int col = hoff + KS * g;
    each_key<NTB>([&](int t, int gj, int r, int j, size_t pair) {
      const int ti = TC.index(pair);
      const uint32_t bits = TC.template keep<KS>(which, pair, col);
      float s0 = 0.f, s1 = 0.f;
#pragma unroll
      for (int s4 = 0; s4 < KS / 4; ++s4) {
        const f4 tr = TC.row4(which, ti, col + 4 * s4, bits, s4);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          s0 += v0[4 * s4 + e] * tr[e];
          if (TWO) s1 += v1[4 * s4 + e] * tr[e];
        }
      }
      s0 = quad_sum(s0);
      a0[t][r] += g == gj ? s0 : 0.f;
      if (TWO) {
        s1 = quad_sum(s1);
        a1[t][r] += g == gj ? s1 : 0.f;
      }
    });
  }
  // o0[.] = sum_j w0[i][j] drop(table[t_ij])[.] (and o1 from w1) on the lane's KS columns.  SKIP1: a zero weight of the
  // second sum does not touch the row (the calibrated mixture at masked keys)
  template <int NTB, bool TWO, bool SKIP1>
  __device__ __forceinline__ void time_sums(int which, const f4 (&w0)[NTB], const f4 (&w1)[NTB], float (&o0)[KS],
                                            float (&o1)[KS]) const {
    const int col = hoff + KS * g;
#pragma unroll
    for (int e = 0; e < KS; ++e) o0[e] = o1[e] = 0.f;
    each_key<NTB>([&](int t, int gj, int r, int j, size_t pair) {
      const int ti = TC.index(pair);
      const uint32_t bits = TC.template keep<KS>(which, pair, col);
      const float a = from_owner(w0[t][r], gj);
      const float b = TWO ? from_owner(w1[t][r], gj) : 0.f;
#pragma unroll
      for (int s4 = 0; s4 < KS / 4; ++s4) {
        const f4 tr = TC.row4(which, ti, col + 4 * s4, bits, s4);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          o0[4 * s4 + e] += a * tr[e];
          if (TWO) o1[4 * s4 + e] += (SKIP1 && b == 0.f) ? 0.f : b * tr[e];
        }
      }
    });
  }
  // x = S / sqrt(dh) + mask and y = qa.Ka^T / sqrt(dh) + mask, both in exp2 units
  template <int NTB>
  __device__ __forceinline__ void scores(f4 (&x)[NTB], f4 (&y)[NTB]) const {
    this->template scores_dense<NTB>(x, y);
    time_dots<NTB, false>(0, qf, qf, x, x);  // + q_i . TK_ij
    this->template scores_finish<NTB>(x, y);
  }
  // the lane's KS columns of the row of a [B,L,H] tensor (NULL = zeros)
  __device__ __forceinline__ void load_cols(const float* d, float (&v)[KS]) const {
#pragma unroll
    for (int e = 0; e < KS; ++e) v[e] = 0.f;
    if (!d || !row_ok) return;
    const size_t off = (rowbase + i) * P.H + hoff + KS * g;
#pragma unroll
    for (int s4 = 0; s4 < KS / 4; ++s4) {
      const f4 d4 = *(const f4*)(d + off + 4 * s4);
#pragma unroll
      for (int e = 0; e < 4; ++e) v[4 * s4 + e] = d4[e];
    }
  }
  // w[query c][key] = sum over the head's columns of X[key][.] d[.]  (d: the lane's columns of the row)
  template <int NTB>
  __device__ __forceinline__ void keys_times(const float* X, const float (&d)[KS], f4 (&w)[NTB]) const {
#pragma unroll
    for (int t = 0; t < NTB; ++t) w[t] = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s4 = 0; s4 < KS / 4; ++s4) {
#pragma unroll
      for (int t = 0; t < NTB; ++t) {
        const f4 x4 = *(const f4*)(X + (16 * t + c) * VS + KS * g + 4 * s4);
#pragma unroll
        for (int e = 0; e < 4; ++e) w[t] = mfma16(x4[e], d[4 * s4 + e], w[t]);
      }
    }
  }
  // o[dt] += the row vector `v` (lane layout: columns KS g ..) in the MFMA output layout (columns 16 dt + 4 g + r), through
  // the wave's 16 x (DH + 4) floats of LDS.  Every wave of the workgroup calls this the same number of times.
  __device__ __forceinline__ void add_row_vector(float* tr, const float (&v)[KS], f4 (&o)[DH / 16]) const {
    __syncthreads();
#pragma unroll
    for (int s4 = 0; s4 < KS / 4; ++s4)
      *(f4*)(tr + c * VS + KS * g + 4 * s4) = f4{v[4 * s4], v[4 * s4 + 1], v[4 * s4 + 2], v[4 * s4 + 3]};
    __syncthreads();
#pragma unroll
    for (int dt = 0; dt < DH / 16; ++dt) o[dt] += *(const f4*)(tr + c * VS + 16 * dt + 4 * g);
  }
};

// ------------------------------------------------------------------------------------------------------------------------
// forward
// ------------------------------------------------------------------------------------------------------------------------
template <int DH, int NTB>
__device__ __forceinline__ void fwd_block(const acattn_problem& P, const acattn_fwd_out& O, const Row<DH>& R, float* tr) {
  constexpr int KS = DH / 4;
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
  // sum_j A_x[i,j] TV_ij for both mixtures from one gather of the rows
  float ta[KS], tw[KS];
  R.template time_sums<NTB, true, true>(1, a_att, a_w, ta, tw);
  f4 o[DH / 16];
  const size_t off = (R.rowbase + R.i) * P.H + R.hoff + 4 * R.g;
  R.template times_keys<NTB>(R.S.Vs, a_att, o);
  R.add_row_vector(tr, ta, o);
  if (R.row_ok) {
#pragma unroll
    for (int dt = 0; dt < DH / 16; ++dt) *(f4*)(O.ctx_attacked + off + 16 * dt) = o[dt];
  }
  R.template times_keys<NTB>(R.S.Vs, a_w, o);
  R.add_row_vector(tr, tw, o);
  if (R.row_ok) {
#pragma unroll
    for (int dt = 0; dt < DH / 16; ++dt) *(f4*)(O.ctx_calibrated + off + 16 * dt) = o[dt];
  }
}

template <int DH>
__global__ void __launch_bounds__(256) acattn_timeaware_fwd_kernel(const acattn_problem P, const acattn_time_ext T,
                                                                   const acattn_fwd_out O) {
  const int L = P.L, nT = (L + 15) >> 4, LP = 16 * nT;
  int b, h;
  decode_block(blockIdx.x, P.B, P.n_heads, b, h);
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const Staged<DH> S(smem, LP);
  stage<DH>(P, T, S, (size_t)b * L, h * DH, L, LP);
  __syncthreads();
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  float* tr = smem + Staged<DH>::floats(LP) + wave * 16 * (DH + 4);
  const TimeCtx TC(T, P.H, L);
  const Row<DH> R(P, S, TC, b, h, wave, threadIdx.x & 63);
  switch (nT) {
    case 1: fwd_block<DH, 1>(P, O, R, tr); break;
    case 2: fwd_block<DH, 2>(P, O, R, tr); break;
    case 3: fwd_block<DH, 3>(P, O, R, tr); break;
    default: fwd_block<DH, 4>(P, O, R, tr); break;
  }
}

// ------------------------------------------------------------------------------------------------------------------------
// backward
// ------------------------------------------------------------------------------------------------------------------------
// LDS behind the staged operands: four [LP][LP + 4] matrices (dS, dSa, A_att, A_w), per-wave column sums of the two affine
// cotangents, their totals, three per-row sums, and the waves' 16 x (DH + 4) floats of add_row_vector
struct BwdShared {
  float *mat, *colp, *col, *rows, *tr;
  int LS, LP;
  __device__ __forceinline__ BwdShared(float* base, int LP_) {
    LP = LP_;
    LS = LP + 4;
    mat = base;
    colp = mat + 4 * LP * LS;
    col = colp + 4 * 2 * LP;
    rows = col + 2 * LP;
    tr = rows + 3 * LP;
  }
  static constexpr int floats(int LP, int DH) { return 4 * LP * (LP + 4) + 8 * LP + 2 * LP + 3 * LP + LP * (DH + 4); }
};

template <int DH, int NTB>
__device__ __forceinline__ void bwd_block(const acattn_problem& P, const acattn_bwd_io& IO, const acattn_time_grads& G,
                                          const Row<DH>& R, const BwdShared& W) {
  constexpr int DT = DH / 16, KS = DH / 4;
  const int c = R.c, g = R.g, qb = R.qb;
  float* tr = W.tr + qb * 16 * (DH + 4);
  f4 x[NTB], y[NTB];
  R.template scores<NTB>(x, y);
  float lse_x2 = 0.f, lse_y2 = 0.f;
  if (R.row_ok) {
    const float* sp = IO.row_stats + (R.bh * R.L + R.i) * ACATTN_NSTAT;
    lse_x2 = sp[0];
    lse_y2 = sp[1];
  }
  // dA_x[i,j] = d_ctx_x[i] . (v_j + pv_j + TV_ij)
  f4 dAa[NTB], dAw[NTB];
  {
    float da[KS], dc[KS];
    R.load_cols(IO.d_ctx_attacked, da);
    R.load_cols(IO.d_ctx_calibrated, dc);
    R.template keys_times<NTB>(R.S.Vs, da, dAa);
    R.template keys_times<NTB>(R.S.Vs, dc, dAw);
    if (IO.d_ctx_attacked || IO.d_ctx_calibrated) R.template time_dots<NTB, true>(1, da, dc, dAa, dAw);
  }
  const float* gate = R.gate_row();
  const float dpen2 = IO.d_penalty_part ? 2.0f * IO.d_penalty_part[R.bh * ((R.L + 15) >> 4) + qb] : 0.f;
  const float inv_sqrt = 1.0f / sqrtf((float)DH);
  float r1 = 0.f, r2 = 0.f;
  float* wsS = (float*)G.workspace;
  const size_t n4 = (size_t)P.B * P.n_heads * R.L * R.L;
  // x becomes Pt, then dS; y becomes Mt, then dSa; dAa becomes d Pt, dAw becomes d Mt
#pragma unroll
  for (int t = 0; t < NTB; ++t) {
    f4 n;
    uint32_t ka, km;
    R.draws(t, n, ka, km);
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
    // the two mixtures, for dv (LDS) and for the table gradients (workspace planes 1, 2)
    const f4 aat = R.live(p * m + n * (1.0f - m)), aw = p * mix;
    *(f4*)(W.mat + (2 * W.LP + 16 * qb + c) * W.LS + 16 * t + 4 * g) = aat;
    *(f4*)(W.mat + (3 * W.LP + 16 * qb + c) * W.LS + 16 * t + 4 * g) = aw;
    R.store_seg(wsS + n4, t, aat);
    R.store_seg(wsS + 2 * n4, t, aw);
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
    x[t] = (x[t] * (dAa[t] - r1)) * inv_sqrt;  // dS = d (raw score)
    y[t] = (y[t] * (dAw[t] - r2)) * inv_sqrt;  // dSa
    *(f4*)(W.mat + (0 * W.LP + 16 * qb + c) * W.LS + 16 * t + 4 * g) = x[t];
    *(f4*)(W.mat + (1 * W.LP + 16 * qb + c) * W.LS + 16 * t + 4 * g) = y[t];
    R.store_seg(wsS, t, x[t]);
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
  // dq = dS.(K + pk) + sum_j dS_ij TK_ij + the query halves of the affines; dqa = dSa.Ka
  float tq[KS], unused[KS];
  R.template time_sums<NTB, false, false>(0, x, x, tq, unused);
  f4 o[DT];
  const size_t off = (R.rowbase + R.i) * P.H + R.hoff + 4 * g;
  R.template times_keys<NTB>(R.S.Ks, x, o);
  R.add_row_vector(tr, tq, o);
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
__global__ void __launch_bounds__(256) acattn_timeaware_bwd_kernel(const acattn_problem P, const acattn_time_ext T,
                                                                   const acattn_bwd_io IO, const acattn_time_grads G) {
  constexpr int DT = DH / 16, VS = DH + 4;
  const int L = P.L, H = P.H, nT = (L + 15) >> 4, LP = 16 * nT;
  int b, h;
  decode_block(blockIdx.x, P.B, P.n_heads, b, h);
  const size_t rowbase = (size_t)b * L, bh = (size_t)b * P.n_heads + h;
  const int hoff = h * DH;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const Staged<DH> S(smem, LP);
  const BwdShared W(smem + Staged<DH>::floats(LP), LP);
  stage<DH>(P, T, S, rowbase, hoff, L, LP);
  __syncthreads();
  const int lane = threadIdx.x & 63, c = lane & 15, g = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  {
    const TimeCtx TC(T, H, L);
    const Row<DH> R(P, S, TC, b, h, wave, lane);
    switch (nT) {
      case 1: bwd_block<DH, 1>(P, IO, G, R, W); break;
      case 2: bwd_block<DH, 2>(P, IO, G, R, W); break;
      case 3: bwd_block<DH, 3>(P, IO, G, R, W); break;
      default: bwd_block<DH, 4>(P, IO, G, R, W); break;
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
      *(f4*)(G.d_pos_k + koff + 16 * dt) = o[dt];  // the product share alone
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
    for (int dt = 0; dt < DT; ++dt) *(f4*)(IO.dv + koff + 16 * dt) = o[dt];  // = d pos_v as well
  }

  // ---- the calibrator's parameters: this (sequence, head)'s partial sums, rows and keys in ascending order -------------------
  // (the key halves see the PLAIN k: the staged rows hold k + pk)
  const int wstride = IO.part_stride ? IO.part_stride : 2 * DH, sstride = IO.part_stride ? IO.part_stride : 4;
  if ((int)threadIdx.x < DH) {
    const int d = threadIdx.x;
    float wo_q = 0.f, wd_q = 0.f, wo_k = 0.f, wd_k = 0.f;
    for (int r = 0; r < L; ++r) {
      const float qv = P.q[(rowbase + r) * H + hoff + d], kv = P.k[(rowbase + r) * H + hoff + d];
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

// ------------------------------------------------------------------------------------------------------------------------
// the two table gradients (second launch of the backward)
//   d time_k[t, head cols] += sum_{(b,i,j): t_bij = t} dS_ij q_i * keepK_bij / (1 - p)
//   d time_v[t, head cols] += sum_{(b,i,j): t_bij = t} (A_att_ij d_ctx_att_i + A_w_ij d_ctx_cal_i) * keepV_bij / (1 - p)
// Workgroup (head h, group grp of n_groups) walks the sequences grp, grp + n_groups, ...; thread = (column d, pair slot):
// slot s takes the pairs s, s + 256 / DH, ... of a sequence in ascending (i, j), sums runs of equal t in registers and adds a
// finished run into the workgroup's LDS tables (ds_add_f32).  One flush of the non-zero entries with global float atomics into
// the zero-filled outputs.  The LDS holds nothing else: 2 (time_span + 1) DH floats.
// ------------------------------------------------------------------------------------------------------------------------
template <int DH>
__global__ void __launch_bounds__(256) timeaware_table_grad_kernel(const acattn_problem P, const acattn_time_ext T,
                                                                   const acattn_bwd_io IO, const acattn_time_grads G,
                                                                   int n_groups) {
  constexpr int NS = 256 / DH;
  const int L = P.L, H = P.H, nh = P.n_heads, rows = T.time_span + 1;
  const int h = blockIdx.x % nh, grp = blockIdx.x / nh;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* tabK = smem;
  float* tabV = smem + rows * DH;
  for (int e = threadIdx.x; e < 2 * rows * DH; e += 256) smem[e] = 0.f;
  __syncthreads();
  const TimeCtx TC(T, H, L);
  const int d = threadIdx.x % DH, slot = threadIdx.x / DH, col = h * DH + d;
  const float* wsS = (const float*)G.workspace;
  const size_t n4 = (size_t)P.B * nh * L * L;
  int cur = -1;
  float accK = 0.f, accV = 0.f;
  auto flush_run = [&]() {
    if (cur >= 0) {
      if (accK != 0.f) atomicAdd(tabK + cur * DH + d, accK);
      if (accV != 0.f) atomicAdd(tabV + cur * DH + d, accV);
    }
    accK = accV = 0.f;
  };
  for (int b = grp; b < P.B; b += n_groups) {
    const size_t rowbase = (size_t)b * L, seg = ((size_t)b * nh + h) * L * L;
    for (int pr = slot; pr < L * L; pr += NS) {
      const int i = pr / L;
      const size_t pair = rowbase * L + pr, xo = (rowbase + i) * H + col;
      const int t = TC.index(pair);
      if (t != cur) {
        flush_run();
        cur = t;
      }
      const float ds = wsS[seg + pr], aa = wsS[n4 + seg + pr], aw = wsS[2 * n4 + seg + pr];
      float gv = 0.f;
      if (IO.d_ctx_attacked) gv += aa * IO.d_ctx_attacked[xo];
      if (IO.d_ctx_calibrated && aw != 0.f) gv += aw * IO.d_ctx_calibrated[xo];
      if (TC.keep1(0, pair, col)) accK += ds * P.q[xo] * TC.ks;
      if (TC.keep1(1, pair, col)) accV += gv * TC.ks;
    }
  }
  flush_run();
  __syncthreads();
  for (int e = threadIdx.x; e < rows * DH; e += 256) {
    const int t = e / DH, dd = e - t * DH;
    const float vk = tabK[e], vv = tabV[e];
    if (vk != 0.f) unsafeAtomicAdd(G.d_time_k + (size_t)t * H + h * DH + dd, vk);
    if (vv != 0.f) unsafeAtomicAdd(G.d_time_v + (size_t)t * H + h * DH + dd, vv);
  }
}

// acattn_time_rng_materialize: the bits TimeCtx::keep draws in counter mode, as bytes
__global__ void __launch_bounds__(256) time_rng_kernel(int H, long long n, uint64_t seed, float p, uint8_t* keep_k, uint8_t* keep_v) {
  const long long idx = blockIdx.x * 256LL + threadIdx.x;
  if (idx >= n) return;
  const RngKey key = time_rng_key(seed);
  const uint32_t nchunk = (uint32_t)((H + 31) >> 5);
  const long long pair = idx / H;
  const int col = (int)(idx - pair * H);
  if (keep_k) keep_k[idx] = (uint8_t)(p > 0.f ? time_keep1(time_word(key, (uint32_t)pair, 0u, (uint32_t)(col >> 5), nchunk), col, p) : 1u);
  if (keep_v) keep_v[idx] = (uint8_t)(p > 0.f ? time_keep1(time_word(key, (uint32_t)pair, 1u, (uint32_t)(col >> 5), nchunk), col, p) : 1u);
}

// The configuration this family covers (include/acattn.h): the limit a problem breaks, or NULL.
const char* timeaware_limit(const acattn_problem& p, const acattn_time_ext& t) {
  const char* w = l64_config(p);
  if (w) return w;
  if (t.time_span < 1) return "time-aware attention: time_span must be >= 1";
  if (8LL * ((int64_t)t.time_span + 1) * (p.H / p.n_heads) > kMaxLds) return "time-aware attention: time_span too large: 8 (time_span + 1) head_size must be <= 160 KiB (the table gradients' LDS)";
  if (!(t.p_time >= 0.f && t.p_time < 1.f)) return "time-aware attention: p_time must lie in [0, 1)";
  if ((w = l64_sizes(p))) return w;
  if ((int64_t)p.B * p.L * p.L * 2 * ((p.H + 31) / 32) >= (1LL << 32)) return "time-aware attention: B L L H / 16 must stay below 2^32 (the time dropout's counter)";
  return nullptr;
}

const char* timeaware_pointers(const acattn_problem& p, const acattn_time_ext& t) {
  if (const char* w = l64_pointers(p)) return w;
  if (!t.pos_k || !t.pos_v || !t.time_index || !t.time_k || !t.time_v) return "time-aware attention: pos_k, pos_v, time_index, time_k, time_v must be non-NULL";
  if ((t.keep_time_k == nullptr) != (t.keep_time_v == nullptr)) return "time-aware attention: keep_time_k and keep_time_v must be given together";
  return nullptr;
}

template <int DH>
size_t fwd_lds(int LP) { return sizeof(float) * (Staged<DH>::floats(LP) + LP * (DH + 4)); }
template <int DH>
size_t bwd_lds(int LP) { return sizeof(float) * (Staged<DH>::floats(LP) + BwdShared::floats(LP, DH)); }

}  // namespace

int acattn_timeaware_supported(const acattn_problem& p, const acattn_time_ext& t, const char** why) {
  const char* w = timeaware_limit(p, t);
  if (why) *why = w;
  return w ? 0 : 1;
}

int acattn_launch_timeaware_fwd(const acattn_problem& p, const acattn_time_ext& t, const acattn_fwd_out& o, hipStream_t stream) {
  const char* why = timeaware_limit(p, t);
  if (!why) why = timeaware_pointers(p, t);
  if (!why) why = l64_fwd_out(o);
  if (why) {
    acattn_set_error(why);
    return -1;
  }
  const int nT = (p.L + 15) / 16, LP = 16 * nT, grid = p.B * p.n_heads;
  switch (p.H / p.n_heads) {
    case 16: return launch(acattn_timeaware_fwd_kernel<16>, fwd_lds<16>(LP), grid, 64 * nT, stream, p, t, o);
    case 32: return launch(acattn_timeaware_fwd_kernel<32>, fwd_lds<32>(LP), grid, 64 * nT, stream, p, t, o);
    default: return launch(acattn_timeaware_fwd_kernel<64>, fwd_lds<64>(LP), grid, 64 * nT, stream, p, t, o);
  }
}

int acattn_launch_timeaware_bwd(const acattn_problem& p, const acattn_time_ext& t, const acattn_bwd_io& io,
                                const acattn_time_grads& g, hipStream_t stream) {
  const char* why = timeaware_limit(p, t);
  if (!why) why = timeaware_pointers(p, t);
  if (!why) why = l64_bwd_io(p, io);
  if (!why && (!g.d_pos_k || !g.d_time_k || !g.d_time_v || !g.workspace)) why = "time-aware attention backward: d_pos_k, d_time_k, d_time_v and workspace must be non-NULL";
  if (why) {
    acattn_set_error(why);
    return -1;
  }
  const int dh = p.H / p.n_heads, nT = (p.L + 15) / 16, LP = 16 * nT, grid = p.B * p.n_heads;
  int rc;
  switch (dh) {
    case 16: rc = launch(acattn_timeaware_bwd_kernel<16>, bwd_lds<16>(LP), grid, 64 * nT, stream, p, t, io, g); break;
    case 32: rc = launch(acattn_timeaware_bwd_kernel<32>, bwd_lds<32>(LP), grid, 64 * nT, stream, p, t, io, g); break;
    default: rc = launch(acattn_timeaware_bwd_kernel<64>, bwd_lds<64>(LP), grid, 64 * nT, stream, p, t, io, g); break;
  }
  if (rc != 0) return rc;
  const size_t n_tab = (size_t)(t.time_span + 1) * p.H;
  if ((rc = acattn_launch_zero(g.d_time_k, n_tab, stream)) != 0) return rc;
  if ((rc = acattn_launch_zero(g.d_time_v, n_tab, stream)) != 0) return rc;
  // one head per workgroup, about one workgroup per CU of the 256
  const int n_groups = std::max(1, std::min(p.B, 256 / p.n_heads));
  const size_t lds = sizeof(float) * 2 * (size_t)(t.time_span + 1) * dh;
  switch (dh) {
    case 16: return launch(timeaware_table_grad_kernel<16>, lds, n_groups * p.n_heads, 256, stream, p, t, io, g, n_groups);
    case 32: return launch(timeaware_table_grad_kernel<32>, lds, n_groups * p.n_heads, 256, stream, p, t, io, g, n_groups);
    default: return launch(timeaware_table_grad_kernel<64>, lds, n_groups * p.n_heads, 256, stream, p, t, io, g, n_groups);
  }
}

int acattn_launch_time_rng(int B, int L, int H, uint64_t seed, float p, uint8_t* keep_k, uint8_t* keep_v, hipStream_t stream) {
  const long long n = (long long)B * L * L * H;
  hipLaunchKernelGGL(time_rng_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, H, n, seed, p, keep_k, keep_v);
  return (int)hipGetLastError();
}
