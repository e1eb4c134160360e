// pf_traj_stats: episode returns / lengths along the trajectory buffers of a rollout and the running moments of an observation and a
// reward normaliser (include/pyflyt_amd.h states the semantics). Three kernels in one call:
//
//   ts_scan_kernel    the forward recursion ret += r, len += 1, G = fma(gamma, G, r) with cuts at done, one lane per env, so that every
//                     [k][n] row is read and written coalesced. The carried dependency is one add and one fma per step and no load
//                     depends on it; at 65 536 envs a lane per env is one wave per SIMD, so the steps go in windows of kTsWin,
//                     ascending, as in gae_scan_kernel: every load of a window (three per step) is issued, unconditionally, before
//                     the first value is used. Windows do not overlap (gae.hpp says what the overlapping version compiled to). Each
//                     lane keeps its part of `summary` and of the moments of G in registers; a butterfly over the wave (the same
//                     tree for every wave) leaves kTsScanQ doubles per wave in the context's scratch block.
//   ts_obs_kernel     the masked column sums of obs [k n][D], grid-strided over the flat float stream: consecutive threads read
//                     consecutive floats, and the stride is a multiple of D, so a thread stays in one column and its row advances by
//                     a constant. Double sums of (x - shift) and (x - shift)^2, shift = the running mean the block holds before the
//                     call; the loads of eight rows (the float and, under NEXT_STEP, the two flag bytes that
//                     decide the row's validity, from branch-free selected addresses) are issued before the first is used. The threads of a block that share a column are summed in ascending
//                     thread order: 2 D doubles per block in the scratch block.
//   ts_finish_kernel  one block: the wave partials and the block partials summed in ascending order (in kTsSeg contiguous segments,
//                     then the segments in ascending order), `summary` written, the batch moments merged into the running blocks
//                     (Chan et al.).
//
// Arithmetic: the float32 sequences of a lane are fixed (the build has -ffp-contract=off: the one fused multiply-add is an fmaf), the
// same whichever window a step falls in. The double reductions run in an order that (n, k, D) alone decide: the grid of the
// observation kernel is a function of k n D, never of the device. No atomics. Selections are selects: the reward and the observation
// row of an invalid step are loaded and then NOT chosen, so a NaN in them reaches nothing.
//
// pf_traj_stats_masked is the same three launches with a third source of validity (TsValid below): a [k][n] byte mask, pf_world_sync's
// on the multi-agent envs. Its instantiations differ from the other two in where the validity bit comes from and in nothing else --
// the scan loads one more byte per step and so takes windows of kTsWinMask steps, which no float32 sequence and no double sum
// depends on; the observation kernel loads valid[row] where NEXT_STEP loads two flag bytes. With pf_gae's valid_out (NEXT_STEP) or all
// ones (the other modes) as the mask, every output has the bits of pf_traj_stats.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../../include/pyflyt_amd.h"
#include "uav_device.hpp"

namespace pf {

constexpr int kTsWin = 16;            // steps per window of the scan
constexpr int kTsWinMask = 12;        // the same where a step has a fourth load, its byte of `valid`: 48 loads in flight either way (the counter of outstanding vector-memory loads stops at 63)
constexpr int kTsScanQ = 11;          // doubles a wave leaves: summary[8], then count / sum / sum of squares of G - shift over its valid steps
constexpr int kTsScanStride = 12;     // (16-byte aligned rows)
constexpr int kTsObsBlock = 256;
constexpr int kTsObsMaxGrid = 1024;   // 4 blocks per CU; the rest of the extent is grid-strided
constexpr int kTsObsUnroll = 8;       // loads a thread has in flight
constexpr int kTsMaxD = 128;          // widest observation row (the dogfight's is 123)
constexpr int kTsSeg = 8;             // contiguous segments the finish kernel cuts a list of partials into
constexpr int kTsFinishBlock = 256;

struct TsK {
  float gamma;
  const float* reward;
  const uint8_t* terminated;
  const uint8_t* truncated;
  const uint8_t* episode_start;  // (kTsMask: `valid` [k][n] stands here, as in pf_traj_stats_masked_args)
  float* carry_return;
  int32_t* carry_length;
  float* carry_disc;
  float* ep_return_out;
  int32_t* ep_length_out;
  const double* ret_moments;  // (read only here: the shift)
};

// doubles of scratch a context of n lanes needs: the scan's wave partials, then the observation kernel's block partials
__host__ __device__ inline size_t ts_scan_words(int n) { return (size_t)kTsScanStride * (((size_t)n + 63) / 64); }
inline size_t ts_scratch_words(int n, int D) { return ts_scan_words(n) + (size_t)kTsObsMaxGrid * 2 * (size_t)D; }
inline unsigned ts_obs_grid(size_t total) {
  const size_t blocks = (total + kTsObsBlock - 1) / kTsObsBlock;
  return (unsigned)(blocks < (size_t)kTsObsMaxGrid ? blocks : (size_t)kTsObsMaxGrid);
}

// The sum over the wave's 64 lanes by a butterfly: the same tree in every wave, and every lane ends with the same bits
__device__ __forceinline__ double ts_wave_sum(double x) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) x = x + __shfl_xor(x, m, 64);
  return x;
}
__device__ __forceinline__ double ts_wave_min(double x) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) x = fmin(x, __shfl_xor(x, m, 64));
  return x;
}
__device__ __forceinline__ double ts_wave_max(double x) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) x = fmax(x, __shfl_xor(x, m, 64));
  return x;
}

// Where a step's validity comes from. kTsAll: every step is valid (SAME_STEP, OFF); kTsNext: the context's auto-reset mode is NEXT_STEP,
// a step is invalid where the one before it was done; kTsMask: pf_traj_stats_masked, one byte per step and lane says so.
enum TsValid { kTsAll = 0, kTsNext = 1, kTsMask = 2 };

template <TsValid V>
__global__ __launch_bounds__(64) void ts_scan_kernel(TsK a, int n_lanes, int k, double* __restrict__ partials) {
  constexpr bool NEXT = V == kTsNext, MASK = V == kTsMask;
  constexpr int kWin = MASK ? kTsWinMask : kTsWin;
  const size_t n = (size_t)n_lanes;
  const size_t lane = (size_t)blockIdx.x * 64 + threadIdx.x;
  const bool live = lane < n;
  const size_t i = live ? lane : n - 1;  // (the lanes past n read lane n - 1 and select nothing: they stay for the butterfly)
  float ret = a.carry_return[i], G = a.carry_disc[i];
  int32_t len = a.carry_length[i];
  bool prev_done = NEXT && a.episode_start ? a.episode_start[i] != 0 : false;
  const double shift = a.ret_moments ? a.ret_moments[1] : 0.0;
  uint32_t n_ep = 0, n_term = 0, n_trunc = 0, n_valid = 0, sum_len = 0;
  double sum_ret = 0.0, sum_sq = 0.0, g1 = 0.0, g2 = 0.0;
  float lo = INFINITY, hi = -INFINITY;
  for (int s0 = 0; s0 < k; s0 += kWin) {  // (nothing of a window is carried round the loop)
    float r[kWin];
    uint32_t te[kWin], tr[kWin], vb[kWin];  // (a register each, as in gae.hpp; vb: the step's byte of `valid`, kTsMask only)
#pragma unroll
    for (int j = 0; j < kWin; ++j) {  // every load of the window; the slots past step k - 1 read row k - 1 again and are skipped below
      const int s = s0 + j < k ? s0 + j : k - 1;
      const size_t o = (size_t)s * n + i;
      r[j] = a.reward[o];
      te[j] = a.terminated[o];
      tr[j] = a.truncated[o];
      vb[j] = MASK ? a.episode_start[o] : 0u;
    }
#pragma unroll
    for (int j = 0; j < kWin; ++j) {
      if (s0 + j < k) {  // (wave-uniform)
        const size_t o = (size_t)(s0 + j) * n + i;
        const bool term = te[j] != 0;
        const bool done = term || tr[j] != 0;
        const bool valid = MASK ? live && vb[j] != 0 : live && !(NEXT && prev_done);
        const float ret1 = ret + r[j];
        const float G1 = fmaf(a.gamma, G, r[j]);
        ret = valid ? ret1 : ret;
        len = valid ? len + 1 : len;
        G = valid ? G1 : G;
        const double d = (double)G - shift;
        n_valid += valid ? 1u : 0u;
        g1 = g1 + (valid ? d : 0.0);
        g2 = g2 + (valid ? d * d : 0.0);
        const bool fin = valid && done;
        const float er = fin ? ret : 0.0f;
        const int32_t el = fin ? len : 0;
        if (live) {
          if (a.ep_return_out) a.ep_return_out[o] = er;
          if (a.ep_length_out) a.ep_length_out[o] = el;
        }
        n_ep += fin ? 1u : 0u;
        n_term += fin && term ? 1u : 0u;
        n_trunc += fin && !term ? 1u : 0u;
        sum_len += (uint32_t)el;
        sum_ret = sum_ret + (double)er;  // (er is +0 where nothing finished)
        sum_sq = sum_sq + (double)er * (double)er;
        lo = fin ? fminf(lo, ret) : lo;
        hi = fin ? fmaxf(hi, ret) : hi;
        ret = fin ? 0.0f : ret;
        len = fin ? 0 : len;
        G = fin ? 0.0f : G;
        prev_done = done;
      }
    }
  }
  if (live) {
    a.carry_return[i] = ret;
    a.carry_length[i] = len;
    a.carry_disc[i] = G;
  }
  double q[kTsScanQ];
  q[0] = ts_wave_sum((double)n_ep);
  q[1] = ts_wave_sum(sum_ret);
  q[2] = ts_wave_sum(sum_sq);
  q[3] = ts_wave_min((double)lo);
  q[4] = ts_wave_max((double)hi);
  q[5] = ts_wave_sum((double)sum_len);
  q[6] = ts_wave_sum((double)n_term);
  q[7] = ts_wave_sum((double)n_trunc);
  q[8] = ts_wave_sum((double)n_valid);
  q[9] = ts_wave_sum(g1);
  q[10] = ts_wave_sum(g2);
  if (threadIdx.x < kTsScanQ) {  // (every lane holds all eleven: lane t writes the t-th)
    double v = q[0];
#pragma unroll
    for (int t = 1; t < kTsScanQ; ++t) v = threadIdx.x == t ? q[t] : v;
    partials[(size_t)blockIdx.x * kTsScanStride + threadIdx.x] = v;
  }
}

// rows = k n rows of D floats; stride = the threads that work, a multiple of D (the last gridDim.x * kTsObsBlock - stride threads idle)
// kTsMask: episode_start is `valid` [k n], a flat row's index is its index there; terminated and truncated are not read
template <TsValid V>
__global__ __launch_bounds__(kTsObsBlock) void ts_obs_kernel(const float* __restrict__ obs, const uint8_t* __restrict__ terminated,
                                                              const uint8_t* __restrict__ truncated, const uint8_t* __restrict__ episode_start,
                                                              const double* __restrict__ obs_moments, double* __restrict__ partials, size_t rows,
                                                              int n_lanes, int D) {
  constexpr bool NEXT = V == kTsNext, MASK = V == kTsMask;
  __shared__ double sh1[kTsObsBlock], sh2[kTsObsBlock];
  const size_t n = (size_t)n_lanes;
  const size_t g = (size_t)blockIdx.x * kTsObsBlock + threadIdx.x;
  const size_t threads = (size_t)gridDim.x * kTsObsBlock;
  const size_t row_step = threads / (size_t)D, stride = row_step * (size_t)D;
  const int c = (int)(g % (size_t)D);
  double s1 = 0.0, s2 = 0.0;
  const uint8_t* es = episode_start ? episode_start : terminated;
  const uint32_t es_mask = episode_start ? 0xFFu : 0u;
  if (g < stride) {
    const double shift = obs_moments[1 + c];
    size_t row = g / (size_t)D;
    // a row's validity: NEXT_STEP and the lane finished in the step before (row - n), or waited for its reset when the call began.
    // Branch-free, so that the flag loads go out with the observation loads: two byte loads from SELECTED addresses -- the two flag
    // bytes of the row n above, or, for the first n rows, episode_start twice (es: episode_start, or any readable [n] bytes with
    // es_mask 0 where the caller gave none). The bytes are kept as loaded and combined where they are used: combining them next
    // to the loads would wait for them there (gae.hpp).
    // kTsMask: one byte load, valid[row], in the first's place; the second is not issued.
    auto flag_ptr = [&](const uint8_t* flags, size_t rw) { return rw >= n ? flags + (rw - n) : es + rw; };
    auto take = [&](float x, uint32_t b1, uint32_t b2, size_t rw) {
      const bool ok = MASK ? b1 != 0 : !NEXT || ((b1 | b2) & (rw >= n ? 0xFFu : es_mask)) == 0;
      const double d = (double)x - shift;
      s1 = s1 + (ok ? d : 0.0);
      s2 = s2 + (ok ? d * d : 0.0);
    };
    for (; row + (size_t)(kTsObsUnroll - 1) * row_step < rows; row += (size_t)kTsObsUnroll * row_step) {
      float x[kTsObsUnroll];
      uint32_t b1[kTsObsUnroll], b2[kTsObsUnroll];
#pragma unroll
      for (int u = 0; u < kTsObsUnroll; ++u) {  // every load of the eight rows (nothing here waits)
        const size_t rw = row + (size_t)u * row_step;
        x[u] = obs[rw * (size_t)D + c];
        b1[u] = MASK ? episode_start[rw] : NEXT ? *flag_ptr(terminated, rw) : 0u;
        b2[u] = NEXT ? *flag_ptr(truncated, rw) : 0u;
      }
#pragma unroll
      for (int u = 0; u < kTsObsUnroll; ++u) take(x[u], b1[u], b2[u], row + (size_t)u * row_step);
    }
    for (; row < rows; row += row_step) take(obs[row * (size_t)D + c], MASK ? episode_start[row] : NEXT ? *flag_ptr(terminated, row) : 0u, NEXT ? *flag_ptr(truncated, row) : 0u, row);
  }
  sh1[threadIdx.x] = s1;
  sh2[threadIdx.x] = s2;
  __syncthreads();
  if ((int)threadIdx.x < D) {  // the block's threads of column t, in ascending thread order
    const int first = (int)(((size_t)D + threadIdx.x - ((size_t)blockIdx.x * kTsObsBlock) % (size_t)D) % (size_t)D);
    double t1 = 0.0, t2 = 0.0;
    for (int u = first; u < kTsObsBlock; u += D) {
      t1 = t1 + sh1[u];
      t2 = t2 + sh2[u];
    }
    partials[((size_t)blockIdx.x * 2) * (size_t)D + threadIdx.x] = t1;
    partials[((size_t)blockIdx.x * 2 + 1) * (size_t)D + threadIdx.x] = t2;
  }
}

// (count, mean, M2) of a running block merged with a batch given as count nb and the sums s1, s2 of (x - mean) and (x - mean)^2
// about the block's own mean: the batch's mean is mean + s1 / nb and its M2 is s2 - s1^2 / nb, and with delta = s1 / nb
// Chan's M2 + M2_b + delta^2 n nb / (n + nb) follows. nb = 0 leaves the block as it is.
__device__ __forceinline__ void ts_merge(double na, double nb, double s1, double s2, double& mean, double& m2) {
  if (nb > 0.0) {
    const double tot = na + nb, delta = s1 / nb;
    const double m2b = s2 - s1 * delta;
    mean = mean + delta * (nb / tot);
    m2 = m2 + m2b + delta * delta * (na * nb / tot);
  }
}

// One block. scan_partials: n_waves rows of kTsScanStride; obs_partials: n_blocks rows of 2 D (NULL: no observation moments)
__global__ __launch_bounds__(kTsFinishBlock) void ts_finish_kernel(const double* __restrict__ scan_partials, int n_waves,
                                                                    const double* __restrict__ obs_partials, int n_blocks, int D,
                                                                    double* __restrict__ summary, double* __restrict__ ret_moments,
                                                                    double* __restrict__ obs_moments) {
  __shared__ double seg_scan[kTsScanQ * kTsSeg];
  __shared__ double seg_obs[2 * kTsMaxD * kTsSeg];
  const int t = (int)threadIdx.x;
  const double na_obs = obs_moments ? obs_moments[0] : 0.0;
  if (t < kTsScanQ * kTsSeg) {
    const int q = t / kTsSeg, sg = t % kTsSeg, chunk = (n_waves + kTsSeg - 1) / kTsSeg;
    const int w1 = (sg + 1) * chunk < n_waves ? (sg + 1) * chunk : n_waves;
    double v = q == 3 ? (double)INFINITY : q == 4 ? -(double)INFINITY : 0.0;
    for (int w = sg * chunk; w < w1; ++w) {
      const double x = scan_partials[(size_t)w * kTsScanStride + q];
      v = q == 3 ? fmin(v, x) : q == 4 ? fmax(v, x) : v + x;
    }
    seg_scan[t] = v;
  }
  if (obs_partials) {
    const int chunk = (n_blocks + kTsSeg - 1) / kTsSeg;
    for (int item = t; item < 2 * D * kTsSeg; item += kTsFinishBlock) {
      const int q = item / kTsSeg, sg = item % kTsSeg;  // q: which * D + column
      const int b1 = (sg + 1) * chunk < n_blocks ? (sg + 1) * chunk : n_blocks;
      double v = 0.0;
      for (int b = sg * chunk; b < b1; ++b) v = v + obs_partials[(size_t)b * 2 * (size_t)D + q];
      seg_obs[item] = v;
    }
  }
  __syncthreads();
  auto scan_total = [&](int q) {
    double v = seg_scan[q * kTsSeg];
    for (int sg = 1; sg < kTsSeg; ++sg) {
      const double x = seg_scan[q * kTsSeg + sg];
      v = q == 3 ? fmin(v, x) : q == 4 ? fmax(v, x) : v + x;
    }
    return v;
  };
  const double n_valid = scan_total(8);  // (a whole number: the same in every thread)
  if (t < 8) summary[t] = scan_total(t);
  if (t == 8 && ret_moments) {
    double mean = ret_moments[1], m2 = ret_moments[2];
    const double na = ret_moments[0];
    ts_merge(na, n_valid, scan_total(9), scan_total(10), mean, m2);
    ret_moments[0] = na + n_valid;
    ret_moments[1] = mean;
    ret_moments[2] = m2;
  }
  if (obs_partials) {
    for (int c = t; c < D; c += kTsFinishBlock) {
      double s1 = 0.0, s2 = 0.0;
      for (int sg = 0; sg < kTsSeg; ++sg) {
        s1 = s1 + seg_obs[c * kTsSeg + sg];
        s2 = s2 + seg_obs[(D + c) * kTsSeg + sg];
      }
      double mean = obs_moments[1 + c], m2 = obs_moments[1 + D + c];
      ts_merge(na_obs, n_valid, s1, s2, mean, m2);
      obs_moments[1 + c] = mean;
      obs_moments[1 + D + c] = m2;
    }
    __syncthreads();  // (every thread has read the count)
    if (t == 0) obs_moments[0] = na_obs + n_valid;
  }
}

}  // namespace pf
