// torch.optim.Adam's update for every parameter of the model in ONE launch (recbole/trainer/trainer.py:590-615 builds
// optim.Adam; the step is part of the measured training step).
//
// The step is a stream over 7 x 4 bytes per parameter element -- 180 MB with the 100k x 64 item table, whose CE gradient is
// dense.  torch's fused multi-tensor implementation takes two launches for the model's ~60 tensors plus one that
// increments the step counters: 55 + 14 + 5 us.  Here: one launch, tensor descriptors in the kernel arguments (a scalar
// scan finds a workgroup's tensor), 16-byte accesses, the step counters incremented by the last workgroup to finish.
//
// Two kernels compute the same bits (tests/test_hip_adam_stream.py):
//   adam_step_kernel (acattn_adam_step): one workgroup per 4,096 elements, every wave evaluates the two double-precision
//     pow() of the bias corrections itself.  In the binary those ~600 of a wave's ~1,600 instructions mostly run BEFORE its
//     first load, the 16 loads per lane are issued in four groups between the arithmetic (the compiler sinks them), and the
//     grid is 1.3 rounds of what fits on the device.
//   adam_step_kernel_cached (acattn_adam_step_cached): a fixed grid walks 1,024-element chunks grid-stride; the next
//     chunk's four 16-byte loads are requested, and pinned, before the current chunk's arithmetic and stores; the bias
//     corrections come from a small device buffer that the last workgroup of the PREVIOUS launch filled (keyed by step and
//     betas, so a stale entry is never used; without a matching entry the wave computes them as above).
//
// The arithmetic follows ATen/native/cuda/fused_adam_utils.cuh (adam_math, ADAM_MODE::ORIGINAL, no amsgrad, no maximize)
// operation by operation, including which products are formed in double (beta1, beta2, lr, eps, weight_decay are doubles
// there and the moments are floats), so that results agree with torch's to the last bit or two
// (tests/test_hip_adam.py).
#include <math.h>
#include <stdlib.h>

#include <algorithm>

#include "acattn_common.h"

namespace {

constexpr int kChunk = 4096;  // elements per workgroup (2048: 75 us; four pipelined trips of 4096 per workgroup: 64 us;
                              // this: 62 us = 2.9 TB/s over the 180 MB of the benchmark model, torch's three launches: 74 us)

struct AdamArgs {
  acattn_adam_group g;
  int block_start[ACATTN_ADAM_MAX_TENSORS + 1];
  double lr, beta1, beta2, eps, weight_decay;
  int* done;
};

__device__ __forceinline__ void adam_math(float& param, float grad, float& exp_avg, float& exp_avg_sq, const AdamArgs& A,
                                          float bias_correction1, float bias_correction2_sqrt) {
  if (A.weight_decay != 0) grad += param * A.weight_decay;
  exp_avg = A.beta1 * exp_avg + (1 - A.beta1) * grad;
  exp_avg_sq = A.beta2 * exp_avg_sq + (1 - A.beta2) * grad * grad;
  const float step_size = A.lr / bias_correction1;
  const float denom = (sqrtf(exp_avg_sq) / bias_correction2_sqrt) + A.eps;
  param -= step_size * exp_avg / denom;
}

__global__ void __launch_bounds__(256) adam_step_kernel(const AdamArgs A) {
  int t = 0;
  while (t + 1 < A.g.n_tensors && (int)blockIdx.x >= A.block_start[t + 1]) ++t;  // (scalar: uniform per workgroup)
  const int64_t n = A.g.numel[t];
  const int64_t base = (int64_t)((int)blockIdx.x - A.block_start[t]) * kChunk;
  float* __restrict__ p = A.g.param[t];
  const float* __restrict__ gr = A.g.grad[t];
  float* __restrict__ m = A.g.exp_avg[t];
  float* __restrict__ v = A.g.exp_avg_sq[t];
  // torch increments the count first (_foreach_add(state_steps, 1)) and corrects with the incremented one
  // (every lane computes the two double-precision pow() itself: one lane per workgroup + a barrier put ~4 us of serial
  // latency in front of every workgroup)
  const float step = *A.g.step[t] + 1.0f;
  const bool aligned = ((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(gr) | reinterpret_cast<uintptr_t>(m) |
                         reinterpret_cast<uintptr_t>(v)) & 15) == 0;
  auto corrections = [&](float& bc1, float& bc2s) {
    bc1 = (float)(1 - pow(A.beta1, (double)step));
    bc2s = (float)sqrt(1 - pow(A.beta2, (double)step));
  };
  float bc1, bc2s;
  if (aligned && base + kChunk <= n) {
    constexpr int NV = kChunk / 1024;
    f4 pv[NV], gv[NV], mv[NV], vv[NV];
#pragma unroll
    for (int k = 0; k < NV; ++k) {
      const int64_t i = base + (int64_t)(threadIdx.x + 256 * k) * 4;
      pv[k] = *(const f4*)(p + i);
      gv[k] = *(const f4*)(gr + i);
      mv[k] = *(const f4*)(m + i);
      vv[k] = *(const f4*)(v + i);
    }
    corrections(bc1, bc2s);
#pragma unroll
    for (int k = 0; k < NV; ++k) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float pe = pv[k][e], me = mv[k][e], ve = vv[k][e];
        adam_math(pe, gv[k][e], me, ve, A, bc1, bc2s);
        pv[k][e] = pe, mv[k][e] = me, vv[k][e] = ve;
      }
      const int64_t i = base + (int64_t)(threadIdx.x + 256 * k) * 4;
      *(f4*)(p + i) = pv[k];
      *(f4*)(m + i) = mv[k];
      *(f4*)(v + i) = vv[k];
    }
  } else {
    corrections(bc1, bc2s);
    for (int64_t i = base + threadIdx.x; i < n && i < base + kChunk; i += 256) {
      float pe = p[i], me = m[i], ve = v[i];
      adam_math(pe, gr[i], me, ve, A, bc1, bc2s);
      p[i] = pe;
      m[i] = me;
      v[i] = ve;
    }
  }
  // The last workgroup to finish advances the counters: every workgroup has read its counter by then (its lanes read it
  // at their start, the barrier below waits for them, then thread 0 counts the workgroup in), and the next launch sees counters and `done` through the
  // kernel boundary.  No fence: a device-scope fence writes the XCD's L2 back on this part, once per workgroup (it made
  // the launch 2x slower than the three launches it replaces).
  __syncthreads();
  if (threadIdx.x == 0) {
    if (atomicAdd(A.done, 1) == (int)gridDim.x - 1) {
      for (int k = 0; k < A.g.n_tensors; ++k) *A.g.step[k] = *A.g.step[k] + 1.0f;
      *A.done = 0;
    }
  }
}

// ---- the persistent form ------------------------------------------------------------------------------------------------

constexpr int kTrip = 1024;        // elements per trip of a workgroup: one 16-byte access per lane and array
constexpr int kGridPerCU = 2;      // workgroups per compute unit: 1: 43-45 us, 2 to 5: 40-42 us (no order among them beyond the
                                   // launch's 3-9 us spread), 8: +3 us, 12: +10 us (86 registers: 5 workgroups per unit are resident)

// One tensor slot of the correction cache (include/acattn.h: ACATTN_ADAM_CACHE_BYTES).  bc1 / bc2s belong to the corrected
// step `step` (>= 1, so an all-zero entry matches nothing) and these betas.
struct AdamCorrection {
  double beta1, beta2;
  float step, bc1, bc2s, pad;
};
static_assert(sizeof(AdamCorrection) * ACATTN_ADAM_MAX_TENSORS == ACATTN_ADAM_CACHE_BYTES, "acattn.h sizes the cache");
static_assert(ACATTN_ADAM_MAX_TENSORS <= 64, "one lane of the last workgroup's first wave per tensor slot");

struct AdamStreamArgs {
  AdamArgs a;  // block_start: the FAST trips (kTrip elements by 16-byte accesses), tensor after tensor
  int slow_start[ACATTN_ADAM_MAX_TENSORS + 1];  // the checked trips: ragged tails, tensors whose pointers are not all aligned
  AdamCorrection* cache;
};

// The ONE evaluation of the corrections behind the cached kernel: the last workgroup fills the cache with it and a wave
// without a matching entry calls it, so both give the same bits (the expressions are adam_step_kernel's).
__device__ __forceinline__ void adam_corrections(double beta1, double beta2, float step, float& bc1, float& bc2s) {
  bc1 = (float)(1 - pow(beta1, (double)step));
  bc2s = (float)sqrt(1 - pow(beta2, (double)step));
}

struct AdamTrip {
  float* p;
  const float* g;
  float* m;
  float* v;
  int64_t base;
  float bc1, bc2s;  // of the trip's tensor, wave-uniform
};

__device__ __forceinline__ float uniform(float x) {  // the same bits in every lane: keep them in a scalar register
  return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, x)));
}

// (Nontemporal accesses for exp_avg, exp_avg_sq and the gradient -- touched once per step, read by nothing else -- were
// measured and not kept: 40.1-40.5 us against 40.6-41.1 us inside the training step, within the launch's own spread.)
__global__ void __launch_bounds__(256) adam_step_kernel_cached(const AdamStreamArgs S) {
  const AdamArgs& A = S.a;
  const int n_tensors = A.g.n_tensors, stride = (int)gridDim.x;
  // A workgroup's trips ascend, so the scalar scan for a trip's tensor resumes where the last one ended.
  int scan = 0;
  auto locate = [&](const int* start, int item, AdamTrip& T) {
    while (scan + 1 < n_tensors && item >= start[scan + 1]) ++scan;
    T.p = A.g.param[scan], T.g = A.g.grad[scan], T.m = A.g.exp_avg[scan], T.v = A.g.exp_avg_sq[scan];
    T.base = (int64_t)(item - start[scan]) * kTrip;
  };
  auto request = [&](const AdamTrip& T, f4& pv, f4& gv, f4& mv, f4& vv) {
    const int64_t i = T.base + (int64_t)threadIdx.x * 4;
    pv = *(const f4*)(T.p + i);
    gv = *(const f4*)(T.g + i);
    mv = *(const f4*)(T.m + i);
    vv = *(const f4*)(T.v + i);
  };
  // torch increments the count first (_foreach_add(state_steps, 1)) and corrects with the incremented one.  The wave keeps
  // the corrections of the last tensor it looked up and looks again only when a trip belongs to another one.
  int have = -1;
  float bc1 = 0.f, bc2s = 0.f;
  auto correct = [&](AdamTrip& T) {
    if (scan != have) {
      have = scan;
      const float step = *A.g.step[scan] + 1.0f;
      const AdamCorrection c = S.cache[scan];
      if (__builtin_expect(c.step == step && c.beta1 == A.beta1 && c.beta2 == A.beta2, 1)) bc1 = c.bc1, bc2s = c.bc2s;
      else adam_corrections(A.beta1, A.beta2, step, bc1, bc2s);
      bc1 = uniform(bc1), bc2s = uniform(bc2s);
    }
    T.bc1 = bc1, T.bc2s = bc2s;
  };
  auto update = [&](const AdamTrip& T, f4& pv, const f4& gv, f4& mv, f4& vv) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float pe = pv[e], me = mv[e], ve = vv[e];
      adam_math(pe, gv[e], me, ve, A, T.bc1, T.bc2s);
      pv[e] = pe, mv[e] = me, vv[e] = ve;
    }
    const int64_t i = T.base + (int64_t)threadIdx.x * 4;
    *(f4*)(T.p + i) = pv;
    *(f4*)(T.m + i) = mv;
    *(f4*)(T.v + i) = vv;
  };
  // ---- the fast trips, two register sets in turn: while one trip is updated and stored, the other's four requests are
  // in flight.  The fences keep the requests in front of the arithmetic (the compiler otherwise sinks loads to their
  // first use).  Every trip here loads unconditionally and a workgroup's last trip has code of its own (the markers keep
  // the copies apart): the compiler counts outstanding requests per code path and waits for the FEWEST any path into a
  // block can have, so one shared block behind "if (more) request" waited for everything and nothing overlapped.
  // A trip's corrections are settled when it is requested: behind the first trip's requests, and in front of a later
  // trip's only when it starts another tensor (a miss there evaluates pow() with one register set live, not two).
  int item = (int)blockIdx.x;
  const int total = A.block_start[n_tensors];
  if (item < total) {
    AdamTrip Ta, Tb;
    f4 pa, ga, ma, va, pb, gb, mb, vb;
    // requests the trip behind `item` into one register set, then updates `item`'s trip from the other
    auto trip = [&](AdamTrip& Tnext, f4& pn, f4& gn, f4& mn, f4& vn, AdamTrip& T, f4& pv, f4& gv, f4& mv, f4& vv) {
      locate(A.block_start, item + stride, Tnext);
      correct(Tnext);
      request(Tnext, pn, gn, mn, vn);
      __builtin_amdgcn_sched_barrier(0);
      update(T, pv, gv, mv, vv);
      item += stride;
    };
    locate(A.block_start, item, Ta);
    request(Ta, pa, ga, ma, va);
    correct(Ta);
    if (total - item <= stride) {
      update(Ta, pa, ga, ma, va);
      asm volatile("; only trip");
    } else {
      // (the first pair stands in front of the loop so that the loop is entered with what its own end leaves in flight)
      trip(Tb, pb, gb, mb, vb, Ta, pa, ga, ma, va);
      for (;;) {
        if (total - item <= stride) {
          update(Tb, pb, gb, mb, vb);
          asm volatile("; last trip, second register set");
          break;
        }
        trip(Ta, pa, ga, ma, va, Tb, pb, gb, mb, vb);
        if (total - item <= stride) {
          update(Ta, pa, ga, ma, va);
          asm volatile("; last trip, first register set");
          break;
        }
        trip(Tb, pb, gb, mb, vb, Ta, pa, ga, ma, va);
      }
    }
  }
  // ---- the checked trips (a tensor's ragged tail; every trip of a tensor whose four pointers are not all 16-byte
  // aligned): scalar accesses, handed out from the far end of the grid, whose workgroups have one fast trip fewer
  const int slow_total = S.slow_start[n_tensors];
  scan = 0;
  for (item = stride - 1 - (int)blockIdx.x; item < slow_total; item += stride) {
    AdamTrip T;
    locate(S.slow_start, item, T);
    correct(T);
    const int64_t n = A.g.numel[scan];
    const int64_t first = T.base + (int64_t)(A.block_start[scan + 1] - A.block_start[scan]) * kTrip;  // behind the fast trips
    for (int64_t i = first + threadIdx.x; i < n && i < first + kTrip; i += 256) {
      float pe = T.p[i], me = T.m[i], ve = T.v[i];
      adam_math(pe, T.g[i], me, ve, A, T.bc1, T.bc2s);
      T.p[i] = pe;
      T.m[i] = me;
      T.v[i] = ve;
    }
  }
  // The last workgroup to finish advances the counters and fills the correction cache for the next launch, one lane of its
  // first wave per tensor slot.  Every workgroup has read every counter and cache entry it needs by then: it reads them
  // in correct(), in front of the arithmetic of the trip that needs them, the barrier below waits for all its waves'
  // trips, and only then is it counted in.  The next launch sees counters, cache and `done` through the kernel boundary.  No
  // fence: a device-scope fence writes the XCD's L2 back on this part, once per workgroup (it made the one-workgroup-per-
  // chunk launch 2x slower than the three launches it replaces).
  __syncthreads();
  if (threadIdx.x < 64) {
    int last = 0;
    if (threadIdx.x == 0) last = atomicAdd(A.done, 1) == (int)gridDim.x - 1;
    if (__shfl(last, 0)) {
      const int k = (int)threadIdx.x;
      if (k < n_tensors) {
        const float now = *A.g.step[k] + 1.0f;
        *A.g.step[k] = now;
        AdamCorrection c;
        c.beta1 = A.beta1, c.beta2 = A.beta2, c.step = now + 1.0f, c.pad = 0.f;
        adam_corrections(A.beta1, A.beta2, c.step, c.bc1, c.bc2s);
        S.cache[k] = c;
      }
      if (k == 0) *A.done = 0;
    }
  }
}

// largest tensors first: a workgroup finds its tensor by a scalar scan over block_start, and nearly all workgroups
// belong to the item table (with the table last in the list the scan cost 70 us per launch)
void sort_tensors(const acattn_adam_group& g, acattn_adam_group& sorted) {
  int order[ACATTN_ADAM_MAX_TENSORS];
  for (int t = 0; t < g.n_tensors; ++t) order[t] = t;
  std::stable_sort(order, order + g.n_tensors, [&](int a, int b) { return g.numel[a] > g.numel[b]; });
  sorted.n_tensors = g.n_tensors;
  for (int t = 0; t < g.n_tensors; ++t) {
    const int s = order[t];
    sorted.param[t] = g.param[s], sorted.grad[t] = g.grad[s], sorted.exp_avg[t] = g.exp_avg[s];
    sorted.exp_avg_sq[t] = g.exp_avg_sq[s], sorted.step[t] = g.step[s], sorted.numel[t] = g.numel[s];
  }
}

int g_adam_grid = getenv("ACATTN_ADAM_GRID") ? atoi(getenv("ACATTN_ADAM_GRID")) : 0;  // 0 = kGridPerCU per compute unit (measurement / test hooks: this and acattn_select_adam_grid)

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

}  // namespace

int acattn_launch_adam_step(const acattn_adam_group& g, double lr, double beta1, double beta2, double eps,
                            double weight_decay, int* done, hipStream_t stream) {
  AdamArgs A;
  sort_tensors(g, A.g);
  int blocks = 0;
  for (int t = 0; t < g.n_tensors; ++t) {
    A.block_start[t] = blocks;
    blocks += (int)((A.g.numel[t] + kChunk - 1) / kChunk);
  }
  A.block_start[g.n_tensors] = blocks;
  A.lr = lr, A.beta1 = beta1, A.beta2 = beta2, A.eps = eps, A.weight_decay = weight_decay;
  A.done = done;
  if (blocks == 0) return 0;
  hipLaunchKernelGGL(adam_step_kernel, dim3(blocks), dim3(256), 0, stream, A);
  return (int)hipGetLastError();
}

int acattn_select_adam_grid_choice(int workgroups) {
  const int old = g_adam_grid;
  g_adam_grid = workgroups;
  return old;
}

int acattn_launch_adam_step_cached(const acattn_adam_group& g, double lr, double beta1, double beta2, double eps,
                                   double weight_decay, int* done, void* cache, hipStream_t stream) {
  AdamStreamArgs S;
  AdamArgs& A = S.a;
  sort_tensors(g, A.g);
  int fast = 0, slow = 0;
  for (int t = 0; t < g.n_tensors; ++t) {
    const bool aligned = ((reinterpret_cast<uintptr_t>(A.g.param[t]) | reinterpret_cast<uintptr_t>(A.g.grad[t]) |
                           reinterpret_cast<uintptr_t>(A.g.exp_avg[t]) | reinterpret_cast<uintptr_t>(A.g.exp_avg_sq[t])) & 15) == 0;
    const int64_t whole = aligned ? A.g.numel[t] / kTrip : 0;
    A.block_start[t] = fast, S.slow_start[t] = slow;
    fast += (int)whole;
    slow += (int)((A.g.numel[t] - whole * kTrip + kTrip - 1) / kTrip);
  }
  A.block_start[g.n_tensors] = fast, S.slow_start[g.n_tensors] = slow;
  A.lr = lr, A.beta1 = beta1, A.beta2 = beta2, A.eps = eps, A.weight_decay = weight_decay;
  A.done = done;
  S.cache = (AdamCorrection*)cache;
  const int trips = fast + slow;
  if (trips == 0) return 0;
  // the grid never follows the element count: a fixed number of workgroups per compute unit, fewer only when there are
  // fewer trips than that
  const int grid = std::min(trips, g_adam_grid > 0 ? g_adam_grid : kGridPerCU * num_cus());
  hipLaunchKernelGGL(adam_step_kernel_cached, dim3(grid), dim3(256), 0, stream, S);
  return (int)hipGetLastError();
}
