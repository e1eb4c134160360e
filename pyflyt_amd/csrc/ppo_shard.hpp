// Sharded PPO (include/pyflyt_amd.h: pf_ppo_adv_sums, pf_ppo_grad_shard, pf_ppo_shard_combine, pf_adv_sums_add, pf_moments_merge): one
// gradient call cut at the two places where it reduces over ALL rows, so that shards of a batch -- one per device -- give the joint
// batch's gradient. The per-row kernels are the ones pf_ppo_grad / pf_ppo_grad_rows launch, unchanged; what is here are the small
// kernels in front of and behind them:
//
//   ppo_adv_sums_kernel      one block behind ppo_adv_kernel / ppo_adv_rows_kernel: ppo_adv_finish_kernel's three totals from the same
//                            partials in the same order, written as they are (nothing divided), and the count of out-of-range slots.
//   ppo_shard_fin_kernel     one thread: the advantage block the heads read (c, mu, sigma, mu32, inv32) from the sums of ALL shards,
//                            by ppo_adv_finish_kernel's formulas (ppo_adv_fin below).
//   ppo_shard_finish_kernel  one block behind the heads: ppo_finish's totals of the rows of partials, in its order (eight contiguous
//                            segments, ascending, then the segments, ascending), written raw into the shard's block with the shard's
//                            own valid count and out-of-range count.
//   ppo_shard_combine_kernel one block: the shards' raw totals added in ascending shard order (min / max for the two ratio slots),
//                            the advantage block from the global sums, then ppo_finish itself on that one row of totals.
//   ppo_shard_sum_kernel     grid-strided: grad_out[i] = float32(sum over the shards, ascending, in double, of grads[g][i]).
//   adv_sums_add_kernel      four doubles: the sum of up to 16 blocks in ascending order.
//   moments_merge_kernel     one block: (count, mean[D], M2[D]) blocks merged into dst in order, by ts_finish_kernel's ts_merge.
//
// A total that goes through a one-shard combine is 0.0 + total + seven times 0.0 in ppo_finish (for the ratio slots fmin / fmax with
// +-infinity): the same bits, so one shard is pf_ppo_grad_rows bit for bit. No atomics; every order is a function of the shapes alone.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../../include/pyflyt_amd.h"
#include "uav_device.hpp"
#include "traj_stats.hpp"  // ts_wave_sum, ts_merge
#include "ppo_loss.hpp"    // the partials' layout, ppo_finish

namespace pf {

// a shard's block: the kPpoStride columns of a row of partials as totals, then the shard's valid count and its out-of-range slots
constexpr int kShardColCount = kPpoStride, kShardColBad = kPpoStride + 1;
static_assert(kShardColBad < PF_PPO_SHARD_WORDS, "the block holds the totals and the two counts");
static_assert(kPpoSums == 7 && kPpoQ == 17 && kPpoStride == 20, "include/pyflyt_amd.h states this layout of the shard block");
constexpr int kShardSumBlock = 256;
constexpr int kShardSumMaxGrid = 1024;  // 4 blocks per CU; the rest of the extent is grid-strided
constexpr int kShardSumUnroll = 4;      // elements a thread has in flight, per shard

// ppo_adv_finish_kernel's formulas on its three totals (count, sum, sum of squares): fin = c, mu, sigma, then the float32 roundings
// of mu and of 1 / max(sigma, 1e-8)
PF_DEV void ppo_adv_fin(const double n, const double s1, const double s2, double* fin) {
  const double c = n;
  const double mu = c > 0.0 ? s1 / c : 0.0;
  const double var = c > 0.0 ? s2 / c - mu * mu : 0.0;  // sum (A - mu)^2 / c from the sums about 0
  const double sigma = sqrt(var > 0.0 ? var : 0.0);
  fin[0] = c;
  fin[1] = mu;
  fin[2] = sigma;
  fin[3] = (double)(float)mu;
  fin[4] = (double)(float)(1.0 / (sigma > 1e-8 ? sigma : 1e-8));
}

// One block. partials: n_blocks rows of kPpoAdvStride as ppo_adv_kernel (three columns) or ppo_adv_rows_kernel (four: has_bad) left
// them; sums: count, sum, sum of squares, out-of-range slots
__global__ __launch_bounds__(kPpoBlock) void ppo_adv_sums_kernel(const double* __restrict__ partials, int n_blocks, int has_bad, double* __restrict__ sums) {
  __shared__ double seg[kPpoAdvStride * kPpoSeg];
  const int t = (int)threadIdx.x;
  if (t < kPpoAdvStride * kPpoSeg) {
    const int q = t / kPpoSeg, sg = t % kPpoSeg, chunk = (n_blocks + kPpoSeg - 1) / kPpoSeg;
    const int b1 = (sg + 1) * chunk < n_blocks ? (sg + 1) * chunk : n_blocks;
    double v = 0.0;
    if (q < kPpoAdvQ || has_bad != 0)  // (the contiguous kernel leaves the fourth column as it found it)
      for (int b = sg * chunk; b < b1; ++b) v = v + partials[(size_t)b * kPpoAdvStride + q];
    seg[t] = v;
  }
  __syncthreads();
  if (t < kPpoAdvStride) {
    double v = seg[t * kPpoSeg];
    for (int sg = 1; sg < kPpoSeg; ++sg) v = v + seg[t * kPpoSeg + sg];
    sums[t] = v;
  }
}

__global__ __launch_bounds__(64) void ppo_shard_fin_kernel(const double* __restrict__ adv_sums, double* __restrict__ fin) {
  if (threadIdx.x == 0) ppo_adv_fin(adv_sums[0], adv_sums[1], adv_sums[2], fin);
}

// One block. partials: n_blocks rows of kPpoStride, the first qn columns live (kPpoQ, or kPpoStride with the options); adv_part: the
// shard's own advantage partials, adv_blocks rows (has_bad: with ppo_adv_rows_kernel's fourth column)
__global__ __launch_bounds__(kPpoBlock) void ppo_shard_finish_kernel(const double* __restrict__ partials, int n_blocks, int qn,
                                                                      const double* __restrict__ adv_part, int adv_blocks, int has_bad,
                                                                      double* __restrict__ block) {
  __shared__ double seg[kPpoStride * kPpoSeg];
  const int t = (int)threadIdx.x;
  if (t < qn * kPpoSeg) {
    const int q = t / kPpoSeg, sg = t % kPpoSeg, chunk = (n_blocks + kPpoSeg - 1) / kPpoSeg;
    const int b1 = (sg + 1) * chunk < n_blocks ? (sg + 1) * chunk : n_blocks;
    double v = q == kPpoSums ? (double)INFINITY : q == kPpoSums + 1 ? -(double)INFINITY : 0.0;
    for (int b = sg * chunk; b < b1; ++b) {
      const double x = partials[(size_t)b * kPpoStride + q];
      v = q == kPpoSums ? fmin(v, x) : q == kPpoSums + 1 ? fmax(v, x) : v + x;
    }
    seg[t] = v;
  }
  __syncthreads();
  if (t < PF_PPO_SHARD_WORDS) {
    double v = 0.0;
    if (t < qn) {
      v = seg[t * kPpoSeg];
      for (int sg = 1; sg < kPpoSeg; ++sg) {
        const double x = seg[t * kPpoSeg + sg];
        v = t == kPpoSums ? fmin(v, x) : t == kPpoSums + 1 ? fmax(v, x) : v + x;
      }
    }
    if (t != kShardColCount && t != kShardColBad) block[t] = v;
  }
  const int wave = t / 64, lane = t % 64;
  if (wave == 2) {  // the two counts: whole numbers, their order of summation is free
    double n = 0.0, bad = 0.0;
    for (int b = lane; b < adv_blocks; b += 64) {
      n = n + adv_part[(size_t)b * kPpoAdvStride];
      bad = has_bad != 0 ? bad + adv_part[(size_t)b * kPpoAdvStride + kPpoAdvQ] : bad;
    }
    n = ts_wave_sum(n);
    bad = ts_wave_sum(bad);
    if (lane == 0) {
      block[kShardColCount] = n;
      block[kShardColBad] = bad;
    }
  }
}

struct ShardCombineK {
  int32_t n_shards, width, vclip, bnd;
  float vf_coef, ent_coef, bounds_coef;
  const double* blocks[PF_PPO_MAX_SHARDS];
  const double* adv_sums;
  const float* log_std;
  float* grad_log_std;
  double* stats;
};
// One block: stats and grad_log_std of the joint batch. ppo_finish<true> with both options off is ppo_finish<false> (the columns of
// an option that is off are not used), so the one instantiation serves every call
__global__ __launch_bounds__(kPpoBlock) void ppo_shard_combine_kernel(const ShardCombineK a) {
  __shared__ double row[kPpoStride];
  __shared__ double fin[kPpoFinWords];
  __shared__ double bad;
  const int t = (int)threadIdx.x;
  if (t < kPpoStride) {
    double v = a.blocks[0][t];
    for (int g = 1; g < a.n_shards; ++g) {
      const double x = a.blocks[g][t];
      v = t == kPpoSums ? fmin(v, x) : t == kPpoSums + 1 ? fmax(v, x) : v + x;
    }
    row[t] = v;
  }
  if (t == 64) {
    double v = a.blocks[0][kShardColBad];
    for (int g = 1; g < a.n_shards; ++g) v = v + a.blocks[g][kShardColBad];
    bad = v;
  }
  if (t == 128) ppo_adv_fin(a.adv_sums[0], a.adv_sums[1], a.adv_sums[2], fin);
  __syncthreads();
  ppo_finish<true>(row, 1, fin, a.log_std, a.width, a.vf_coef, a.ent_coef, a.stats, a.grad_log_std, a.vclip != 0, a.bnd != 0, a.bounds_coef, &bad);
}

struct ShardSumK {
  int32_t n_shards;
  const float* grads[PF_PPO_MAX_SHARDS];
  float* out;
};
// Grid-strided; a thread issues the loads of kShardSumUnroll elements of every shard before it adds the first
__global__ __launch_bounds__(kShardSumBlock) void ppo_shard_sum_kernel(const ShardSumK a, size_t numel) {
  const size_t stride = (size_t)gridDim.x * kShardSumBlock;
  for (size_t i0 = (size_t)blockIdx.x * kShardSumBlock + threadIdx.x; i0 < numel; i0 += (size_t)kShardSumUnroll * stride) {
    double v[kShardSumUnroll];
#pragma unroll
    for (int u = 0; u < kShardSumUnroll; ++u) v[u] = 0.0;
    for (int g = 0; g < a.n_shards; ++g) {
      const float* __restrict__ src = a.grads[g];
      float x[kShardSumUnroll];
#pragma unroll
      for (int u = 0; u < kShardSumUnroll; ++u) {
        const size_t i = i0 + (size_t)u * stride;
        x[u] = src[i < numel ? i : numel - 1];
      }
#pragma unroll
      for (int u = 0; u < kShardSumUnroll; ++u) v[u] = g == 0 ? (double)x[u] : v[u] + (double)x[u];
    }
#pragma unroll
    for (int u = 0; u < kShardSumUnroll; ++u) {
      const size_t i = i0 + (size_t)u * stride;
      if (i < numel) a.out[i] = (float)v[u];
    }
  }
}

struct ShardSrcK {
  int32_t n_src;
  const double* src[PF_PPO_MAX_SHARDS];
};
__global__ __launch_bounds__(64) void adv_sums_add_kernel(const ShardSrcK a, double* __restrict__ dst) {
  const int t = (int)threadIdx.x;
  if (t < 4) {
    double v = a.src[0][t];
    for (int g = 1; g < a.n_src; ++g) v = v + a.src[g][t];
    dst[t] = v;
  }
}

// One block, thread c the column c. A block b with count nb goes into ts_merge as the batch it describes: about dst's mean its rows
// sum to nb d and their squares to M2_b + nb d^2, d = mean_b - mean. Into an empty dst a block is copied: its own bits
__global__ __launch_bounds__(kTsMaxD) void moments_merge_kernel(const ShardSrcK a, double* __restrict__ dst, int D) {
  const int c = (int)threadIdx.x;
  double na = dst[0];
  double mean = 0.0, m2 = 0.0;
  if (c < D) mean = dst[1 + c], m2 = dst[1 + D + c];
  for (int g = 0; g < a.n_src; ++g) {
    const double* __restrict__ b = a.src[g];
    const double nb = b[0];
    if (c < D && nb > 0.0) {
      const double mb = b[1 + c], m2b = b[1 + D + c];
      if (na > 0.0) {
        const double d = mb - mean, s1 = nb * d;
        ts_merge(na, nb, s1, m2b + s1 * d, mean, m2);
      } else {
        mean = mb, m2 = m2b;
      }
    }
    na = nb > 0.0 ? na + nb : na;
  }
  __syncthreads();  // (every thread has read dst's count)
  if (c < D) dst[1 + c] = mean, dst[1 + D + c] = m2;
  if (c == 0) dst[0] = na;
}

}  // namespace pf
