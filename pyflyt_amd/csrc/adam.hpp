// pf_adam_step: Adam / AdamW with global gradient-norm clipping over a set of parameter tensors, the optimiser's step of a PPO epoch
// (include/pyflyt_amd.h states the semantics). Two kernels in one call, over the same grid:
//
//   adam_norm_kernel    a workgroup strides over 1024-element chunks, each chunk a piece of ONE tensor (the host puts the per-tensor
//                       chunk prefix into the arguments; the workgroup finds its tensor by a wave-uniform search over at most 33
//                       integers). A thread owns four consecutive elements of a chunk and adds their squares in double, in ascending
//                       index, over its chunks in ascending order; the wave's fixed butterfly (traj_stats.hpp), then the four waves
//                       through LDS in ascending order: ONE double per workgroup to the caller's workspace. Workgroup 0 also reads
//                       what the call needs of `state` (the step counter, the count of skipped calls) and writes it, with b1^t and
//                       b2^t for t = counter + 1, behind the partials: the update kernel never reads `state`, so its one writer of
//                       `state` races with nobody.
//   adam_update_kernel  every workgroup adds the partials in ascending order (all arrive at the same bits), derives the launch-uniform
//                       scalars in double and rounds them to float32, then updates its chunks: per element one fixed float32
//                       sequence. Workgroup 0's first thread writes `state`. With skip_nonfinite and a norm that is not finite the
//                       workgroups return before they touch a tensor.
//
// The tensor pointers travel in the kernel arguments by value (1.4 KB): no descriptor table in device memory, no copy. A chunk's four
// arrays move as one float4 per thread where all four pointers of its tensor are 16-byte aligned and the thread's four elements
// exist, and element by element otherwise: a thread owns the same four elements either way, so the bits agree. The grid is
// min(chunks, kAdamMaxGrid): a function of numel[] alone. No atomics.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../../include/pyflyt_amd.h"
#include "uav_device.hpp"
#include "traj_stats.hpp"  // ts_wave_sum

namespace pf {

constexpr int kAdamBlock = 256;
constexpr int kAdamChunk = 4 * kAdamBlock;  // elements of one tensor a workgroup takes at a time
constexpr int kAdamMaxGrid = 256;           // one workgroup per CU of an MI355X; more chunks are strided over
constexpr int kAdamHeader = 4;              // doubles behind the partials: counter, skipped calls, b1^t, b2^t
constexpr int kAdamWaves = kAdamBlock / 64;

struct AdamK {
  int32_t n_tensors, chunks, skip_nonfinite;
  float lr;
  float beta1, beta2, eps, weight_decay, max_grad_norm;
  const float* lr_dev;
  double* state;
  double* work;                                  // [grid] partials, then kAdamHeader doubles
  int32_t first_chunk[PF_ADAM_MAX_TENSORS + 1];  // tensor i owns the chunks first_chunk[i] .. first_chunk[i + 1] - 1
  int32_t numel[PF_ADAM_MAX_TENSORS];
  float* param[PF_ADAM_MAX_TENSORS];
  const float* grad[PF_ADAM_MAX_TENSORS];
  float* exp_avg[PF_ADAM_MAX_TENSORS];
  float* exp_avg_sq[PF_ADAM_MAX_TENSORS];
  static constexpr bool kGated = false;
};
// pf_adam_step_gated's: one more device word, read by the update kernel (adam_norm_kernel takes the AdamK in it as it is)
struct AdamGatedK : AdamK {
  const uint32_t* gate;
  static constexpr bool kGated = true;
};

// the most workgroups a call over `total` elements can take: a chunk holds at least one element and at most kAdamChunk
inline size_t adam_grid_bound(int64_t total) { return (size_t)(total < (int64_t)kAdamMaxGrid ? total : (int64_t)kAdamMaxGrid); }

typedef float adam_f4 __attribute__((ext_vector_type(4)));

// the tensor that owns `chunk`: the last i with first_chunk[i] <= chunk. Wave-uniform, and said so, so that the argument arrays are
// indexed by a scalar register
PF_DEV int adam_tensor_of(const AdamK& K, const int chunk) {
  int i = 0;
  for (int j = 1; j < PF_ADAM_MAX_TENSORS; ++j)
    if (j < K.n_tensors && K.first_chunk[j] <= chunk) i = j;
  return __builtin_amdgcn_readfirstlane(i);
}

// thread t's four elements of a chunk begin at element e of a tensor: `live` of them exist (4 inside the tensor, fewer at its end, 0
// or less past it)
PF_DEV int adam_live(const int numel, const int64_t e) {
  const int64_t rest = (int64_t)numel - e;
  return rest > 4 ? 4 : (int)rest;
}
template <class T>
PF_DEV void adam_load4(T* base, const bool vec, const int live, float (&x)[4]) {
  if (vec && live >= 4) {
    const adam_f4 q = *reinterpret_cast<const adam_f4*>(base);
    x[0] = q[0], x[1] = q[1], x[2] = q[2], x[3] = q[3];
  } else {
#pragma unroll
    for (int u = 0; u < 4; ++u) x[u] = u < live ? base[u] : 0.0f;
  }
}
PF_DEV void adam_store4(float* base, const bool vec, const int live, const float (&x)[4]) {
  if (vec && live >= 4) {
    adam_f4 q;
    q[0] = x[0], q[1] = x[1], q[2] = x[2], q[3] = x[3];
    *reinterpret_cast<adam_f4*>(base) = q;
  } else {
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (u < live) base[u] = x[u];
  }
}

__global__ void __launch_bounds__(kAdamBlock) adam_norm_kernel(const AdamK K) {
  __shared__ double sh[kAdamWaves];
  const int t = (int)threadIdx.x;
  double s = 0.0;
  for (int chunk = (int)blockIdx.x; chunk < K.chunks; chunk += (int)gridDim.x) {
    const int i = adam_tensor_of(K, chunk);
    const float* g = K.grad[i];
    const int64_t e = (int64_t)(chunk - K.first_chunk[i]) * kAdamChunk + 4 * t;
    float x[4];
    adam_load4(g + e, ((uintptr_t)g & 15) == 0, adam_live(K.numel[i], e), x);  // (elements that do not exist add +0)
#pragma unroll
    for (int u = 0; u < 4; ++u) s = s + (double)x[u] * (double)x[u];
  }
  s = ts_wave_sum(s);
  if ((t & 63) == 0) sh[t >> 6] = s;
  __syncthreads();
  if (t == 0) {
    double v = sh[0];
#pragma unroll
    for (int w = 1; w < kAdamWaves; ++w) v = v + sh[w];
    K.work[blockIdx.x] = v;
    if (blockIdx.x == 0) {
      double* h = K.work + gridDim.x;
      const double step = K.state[0] + 1.0;
      h[0] = K.state[0];
      h[1] = K.state[4];
      h[2] = pow((double)K.beta1, step);
      h[3] = pow((double)K.beta2, step);
    }
  }
}

// KT: AdamK, or AdamGatedK (pf_adam_step_gated: a closed gate is SKIP's rule, counted in slot 5)
template <class KT>
__global__ void __launch_bounds__(kAdamBlock) adam_update_kernel(const KT K) {
  constexpr bool GATED = KT::kGated;
  const int t = (int)threadIdx.x, grid = (int)gridDim.x;
  const double* __restrict__ part = K.work;
  double sum = 0.0;
  int b = 0;
  for (; b + 8 <= grid; b += 8) {
    double v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = part[b + u];
#pragma unroll
    for (int u = 0; u < 8; ++u) sum = sum + v[u];
  }
  for (; b < grid; ++b) sum = sum + part[b];
  const double t_old = part[grid], skipped = part[grid + 1], b1t = part[grid + 2], b2t = part[grid + 3];
  const double lr = K.lr_dev ? (double)*K.lr_dev : (double)K.lr;
  const double norm = sqrt(sum);
  const bool nonfinite = K.skip_nonfinite != 0 && !(norm - norm == 0.0);  // (not finite: an infinity or a NaN)
  bool closed = false;
  if constexpr (GATED) closed = *K.gate == 0u;
  const bool skip = nonfinite || closed;
  const double c = (double)K.max_grad_norm / (norm + 1e-6);
  const double coef = c < 1.0 ? c : (c != c ? c : 1.0);              // min(1, c), a NaN passed on as torch's clamp does
  if (blockIdx.x == 0 && t == 0) {
    double* st = K.state;
    st[0] = skip ? t_old : t_old + 1.0;
    st[1] = norm;
    st[2] = skip ? 0.0 : coef;
    st[3] = lr;
    st[4] = nonfinite ? skipped + 1.0 : skipped;
    if constexpr (GATED) {
      const double gated = st[5];  // (this thread is the only one of the call that touches `state` after the norm kernel)
      st[5] = closed ? gated + 1.0 : gated;
      st[6] = st[7] = 0.0;
    } else {
      st[5] = st[6] = st[7] = 0.0;
    }
  }
  if (skip) return;
  const float coef32 = (float)coef;
  const float b2 = K.beta2;
  const float omb1 = (float)(1.0 - (double)K.beta1), omb2 = (float)(1.0 - (double)K.beta2);
  const float neg_step = (float)(-(lr / (1.0 - b1t)));
  const float bc2_sqrt = (float)sqrt(1.0 - b2t);
  const float eps = K.eps;
  const bool decays = K.weight_decay > 0.0f;
  const float decay = (float)(1.0 - lr * (double)K.weight_decay);
  for (int chunk = (int)blockIdx.x; chunk < K.chunks; chunk += grid) {
    const int i = adam_tensor_of(K, chunk);
    float* p = K.param[i];
    const float* g = K.grad[i];
    float* m = K.exp_avg[i];
    float* v = K.exp_avg_sq[i];
    const bool vec = (((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) == 0;
    const int64_t e = (int64_t)(chunk - K.first_chunk[i]) * kAdamChunk + 4 * t;
    const int live = adam_live(K.numel[i], e);
    float pp[4], gg[4], mm[4], vv[4];
    adam_load4(p + e, vec, live, pp);
    adam_load4(g + e, vec, live, gg);
    adam_load4(m + e, vec, live, mm);
    adam_load4(v + e, vec, live, vv);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const float gc = gg[u] * coef32;
      const float p0 = decays ? pp[u] * decay : pp[u];
      mm[u] = fmaf(omb1, gc - mm[u], mm[u]);
      vv[u] = fmaf(omb2, gc * gc, b2 * vv[u]);
      const float denom = sqrtf(vv[u]) / bc2_sqrt + eps;
      pp[u] = fmaf(neg_step, mm[u] / denom, p0);
    }
    adam_store4(p + e, vec, live, pp);
    adam_store4(m + e, vec, live, mm);
    adam_store4(v + e, vec, live, vv);
  }
}

}  // namespace pf
