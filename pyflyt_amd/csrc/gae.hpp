// pf_gae: generalised advantage estimation over the trajectory buffers of a rollout, and the log-probabilities of its actions
// (include/pyflyt_amd.h states the semantics). Two kernels in one call:
//
//   gae_scan_kernel   the backward recursion adv[s] = delta[s] + gamma lambda (done[s] ? 0 : adv[s + 1]), one lane per env, so that
//                     every [k][n] row is read and written coalesced. The carried dependency is ONE fma per step and no load depends
//                     on it, but at 65 536 envs a lane per env is one wave per SIMD: a loop that loads a step, waits and computes pays
//                     a memory latency per step. So the steps go in windows of kGaeWin, descending: every load of a window (five per
//                     step) is issued, unconditionally, before the first value is used -- about 80 loads of a wave in flight, 64
//                     lanes wide -- and the wave pays one memory latency per window, not per step. Windows do not overlap: a
//                     version that kept a second window's loads in flight while the first was computed compiled to a loop that
//                     waited for those loads at its bottom (the compiler folds the flags' widening and compares into the loop's
//                     phi of the two windows, behind the loads), so it bought registers and no overlap and was dropped.
//   gae_logp_kernel   the Gaussian log-probability: no dependency along s and most of the call's bytes (two action-wide rows per
//                     lane-step), so it runs over the whole k n extent, grid-strided, one row per thread, not inside the scan.
//
// Arithmetic: float32, the same sequence of operations for every lane and step whichever window the step falls in (the build has
// -ffp-contract=off: every fused multiply-add is an fmaf below). Nothing depends on n, on the grid or on the stream.
// Selections are selects: the stale rows of final_values and the reward of a reset step are loaded and then NOT chosen -- they are
// never multiplied by a zero, so a NaN in them reaches nothing.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../../include/pyflyt_amd.h"
#include "uav_device.hpp"

namespace pf {

constexpr int kGaeWin = 16;       // steps per window of the scan
constexpr int kGaeLogpBlock = 256;
constexpr int kGaeLogpMaxGrid = 2048;  // 8 blocks per CU; the rest of the extent is grid-strided
constexpr float kHalfLog2Pi = 0.91893853320467274178f;

struct GaeK {
  float gamma, lambda;
  const float* reward;
  const uint8_t* terminated;
  const uint8_t* truncated;
  const float* values;
  const float* final_values;
  const uint8_t* episode_start;
  float* advantages;
  float* returns;
  uint8_t* valid_out;
};

// One window: slot j holds step s_hi - j; bte | btr = done[s_hi - kGaeWin], the step under the window (NEXT_STEP)
template <int MODE>
struct GaeWindow {
  float r[kGaeWin], v[kGaeWin], fv[kGaeWin];
  uint32_t te[kGaeWin], tr[kGaeWin];  // (a register each: bytes packed four to a register would chain the loads)
  uint32_t bte, btr;                  // the flags under the window, as loaded (combining them here would wait for the loads)
};

// Every load of the window, unconditionally (nothing here waits). The top window of a k that is no multiple of kGaeWin reaches above
// step k - 1: those slots read row k - 1 again and gae_compute skips them.
template <int MODE>
__device__ __forceinline__ void gae_load(GaeWindow<MODE>& w, const GaeK& a, size_t n, size_t i, int s_hi, int k) {
#pragma unroll
  for (int j = 0; j < kGaeWin; ++j) {
    const int s = s_hi - j < k ? s_hi - j : k - 1;
    const size_t o = (size_t)s * n + i;
    w.r[j] = a.reward[o];
    w.v[j] = a.values[o];
    w.te[j] = a.terminated[o];
    w.tr[j] = a.truncated[o];
    if (MODE == PF_AUTORESET_SAME_STEP) w.fv[j] = a.final_values[o];
  }
  if (MODE == PF_AUTORESET_NEXT_STEP) {  // (row 0 again under the bottom window, where gae_compute takes episode_start: no branch here)
    const size_t o = (size_t)(s_hi >= kGaeWin ? s_hi - kGaeWin : 0) * n + i;
    w.bte = a.terminated[o];
    w.btr = a.truncated[o];
  }
}

// start = done[-1]; v_up = values[s + 1], adv_up = advantages[s + 1] of the highest step s < k of the window on entry; the lowest step's own on exit
template <int MODE>
__device__ __forceinline__ void gae_compute(const GaeWindow<MODE>& w, const GaeK& a, float gl, size_t n, size_t i, int s_hi, int k, uint32_t start, float& v_up,
                                            float& adv_up) {
#pragma unroll
  for (int j = 0; j < kGaeWin; ++j) {
    if (s_hi - j < k) {  // (wave-uniform)
      const size_t o = (size_t)(s_hi - j) * n + i;
      const bool term = w.te[j] != 0;
      const bool done = term || w.tr[j] != 0;
      const float nv = (MODE == PF_AUTORESET_SAME_STEP && done) ? w.fv[j] : v_up;
      const float boot = term ? 0.0f : nv;
      const float delta = fmaf(a.gamma, boot, w.r[j]) - w.v[j];
      float adv = fmaf(gl, done ? 0.0f : adv_up, delta);
      bool valid = true;
      if (MODE == PF_AUTORESET_NEXT_STEP)  // a reset step: the step under it finished the episode
        valid = (j + 1 < kGaeWin ? (w.te[(j + 1) % kGaeWin] | w.tr[(j + 1) % kGaeWin]) : (s_hi >= kGaeWin ? (w.bte | w.btr) : start)) == 0;
      adv = valid ? adv : 0.0f;
      a.advantages[o] = adv;
      a.returns[o] = valid ? adv + w.v[j] : w.v[j];
      if (a.valid_out) a.valid_out[o] = valid ? 1 : 0;
      v_up = w.v[j];
      adv_up = adv;
    }
  }
}

template <int MODE>
__global__ __launch_bounds__(64) void gae_scan_kernel(GaeK a, int n_lanes, int k) {
  const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
  const size_t n = (size_t)n_lanes;
  if (i >= n) return;
  const float gl = a.gamma * a.lambda;
  const uint32_t start = (MODE == PF_AUTORESET_NEXT_STEP && a.episode_start) ? a.episode_start[i] : 0u;
  float v_up = a.values[(size_t)k * n + i], adv_up = 0.0f;
  int s = (k + kGaeWin - 1) / kGaeWin * kGaeWin - 1;  // the top slot of the top window; the windows end at step 0
  for (; s >= 0; s -= kGaeWin) {  // (nothing of a window is carried round the loop: only v_up and adv_up)
    GaeWindow<MODE> w;
    gae_load<MODE>(w, a, n, i, s, k);
    gae_compute<MODE>(w, a, gl, n, i, s, k, start, v_up, adv_up);
  }
}

// One component of the log-density; the row's sum adds them in ascending c starting from 0
__device__ __forceinline__ float gae_logp_term(float act, float mean, float log_std, float inv_std) {
  const float z = (act - mean) * inv_std;
  return ((-0.5f * z) * z - log_std) - kHalfLog2Pi;
}

// VEC: action width 4 and 16-byte aligned rows, one float4 per row and operand; otherwise any width, component by component
template <bool VEC>
__global__ __launch_bounds__(kGaeLogpBlock) void gae_logp_kernel(const float* __restrict__ actions, const float* __restrict__ mean,
                                                                  const float* __restrict__ log_std, float* __restrict__ logp, size_t rows, int width) {
  const size_t stride = (size_t)gridDim.x * kGaeLogpBlock;
  if (VEC) {
    float ls[4], inv[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      ls[c] = log_std[c];
      inv[c] = expf(-ls[c]);
    }
    for (size_t r = (size_t)blockIdx.x * kGaeLogpBlock + threadIdx.x; r < rows; r += stride) {
      const float4 x = reinterpret_cast<const float4*>(actions)[r];
      const float4 m = reinterpret_cast<const float4*>(mean)[r];
      float acc = 0.0f;
      acc = acc + gae_logp_term(x.x, m.x, ls[0], inv[0]);
      acc = acc + gae_logp_term(x.y, m.y, ls[1], inv[1]);
      acc = acc + gae_logp_term(x.z, m.z, ls[2], inv[2]);
      acc = acc + gae_logp_term(x.w, m.w, ls[3], inv[3]);
      logp[r] = acc;
    }
  } else {
    for (size_t r = (size_t)blockIdx.x * kGaeLogpBlock + threadIdx.x; r < rows; r += stride) {
      float acc = 0.0f;
      for (int c = 0; c < width; ++c) {
        const float l = log_std[c];
        acc = acc + gae_logp_term(actions[r * width + c], mean[r * width + c], l, expf(-l));
      }
      logp[r] = acc;
    }
  }
}

}  // namespace pf
