// pf_ppo_loss: the clipped PPO objective of a diagonal-Gaussian policy, its statistics and its gradients with respect to the
// actor's means, the critic's values and log_std, in one pass over the M rows of a batch (include/pyflyt_amd.h states the semantics).
// Four kernels in one call:
//
//   ppo_adv_kernel         the count, the sum and the sum of squares of the valid advantages, grid-strided; a thread issues the loads
//                          of eight rows (the float and the validity byte) before it uses the first, and keeps its three sums in double.
//                          The sums are about the shift 0 (DESIGN.md section 14 says what that costs).
//   ppo_adv_finish_kernel  one block: the block partials in ascending order; c, mu, sigma, and the float32 roundings of mu and of
//                          1 / max(sigma, 1e-8) that the main kernel applies.
//   ppo_main_kernel        grid-strided over the rows, U rows per trip: every load of the U rows (mean, action, old log-probability,
//                          advantage, return, value, validity byte; rows past M re-read row M - 1 and select nothing) is issued,
//                          unconditionally, before the first value is used. Per row one fixed float32 sequence (ppo_actor_row and
//                          ppo_critic_row below, which the fused kernels of ppo_grad.hpp run too); the two per-row
//                          gradients leave by streaming stores (nobody in this call reads them again); the sums behind `stats` and
//                          grad_log_std stay per thread in double, are added over the wave by the fixed butterfly of traj_stats.hpp
//                          and over the block's four waves through LDS in ascending order: one row of partials per block.
//                          <W, VEC>: W = the action width; VEC (W = 4 and 16-byte aligned rows) moves one float4 per operand and
//                          row, the other instantiations component by component. Same arithmetic, and a row belongs to the same
//                          thread either way, so the bits agree.
//   ppo_finish_kernel      one block: the block partials cut into eight contiguous segments, summed in ascending order, the
//                          segments added in ascending order; `stats` and grad_log_std written.
//
// The grid of the two strided kernels is min(ceil(M / 256), 1024): a function of M alone, so (M, A) fix the order of every sum. No
// atomics. Selections are selects: every input of an invalid row is loaded and then NOT chosen, so a NaN there reaches nothing.
// A missing `valid` is served without a second instantiation: the byte is read from memory that is readable anyway and masked off.
// pf_ppo_grad_rows (ppo_grad.hpp) has two siblings here, ppo_adv_rows_kernel and ppo_finish_rows_kernel: the first and the last kernel of
// a call on the rows an index list names.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../../include/pyflyt_amd.h"
#include "uav_device.hpp"
#include "gae.hpp"         // gae_logp_term
#include "traj_stats.hpp"  // ts_wave_sum

namespace pf {

constexpr int kPpoBlock = 256;
constexpr int kPpoMaxGrid = 1024;    // 4 blocks per CU; the rest of the extent is grid-strided
constexpr int kPpoMaxA = 8;          // widest action row
constexpr int kPpoAdvUnroll = 8;     // rows a thread of the advantage pass has in flight
constexpr int kPpoRowsVec = 3;       // rows a thread of the main kernel has in flight: float4 rows ...
constexpr int kPpoRowsGen = 2;       // ... and component-wise rows (up to 16 loads each)
constexpr int kPpoAdvQ = 3;          // count, sum, sum of squares
constexpr int kPpoAdvStride = 4;
constexpr int kPpoFinWords = 8;      // c, mu, sigma, mu32, inv32 (the float32 values, held as doubles)
constexpr int kPpoSums = 7;          // sum min(u, v); sum (V - R)^2; sum (r - 1) - d; rows with |r - 1| > clip; sum R; sum R^2; sum (V - R)
constexpr int kPpoQ = kPpoSums + 2 + kPpoMaxA;  // then min r, max r, then the grad_log_std sums
constexpr int kPpoStride = 20;
constexpr int kPpoSeg = 8;           // contiguous segments a finish kernel cuts the list of block partials into
constexpr int kPpoWaves = kPpoBlock / 64;

// doubles of scratch a context holds for the call: advantage partials, the advantage finish's block, the main partials
constexpr size_t kPpoAdvOffset = 0;
constexpr size_t kPpoFinOffset = (size_t)kPpoMaxGrid * kPpoAdvStride;
constexpr size_t kPpoMainOffset = kPpoFinOffset + kPpoFinWords;
constexpr size_t kPpoScratchWords = kPpoMainOffset + (size_t)kPpoMaxGrid * kPpoStride;

inline unsigned ppo_grid(size_t rows) {
  const size_t blocks = (rows + kPpoBlock - 1) / kPpoBlock;
  return (unsigned)(blocks < (size_t)kPpoMaxGrid ? blocks : (size_t)kPpoMaxGrid);
}

typedef float ppo_f4 __attribute__((ext_vector_type(4)));

struct PpoK {
  float clip, vf_coef;
  int32_t normalize;
  const float* mean;
  const float* log_std;
  const float* actions;
  const float* logp_old;
  const float* advantages;
  const float* returns;
  const float* value;
  const uint8_t* vbytes;  // `valid`, or any M readable bytes with vmask 0 where the caller gave none
  uint32_t vmask;
  float* grad_mean;
  float* grad_value;
  static constexpr bool kOpt = false;
};
// what pf_ppo_loss_opt / pf_ppo_grad_opt add (include/pyflyt_amd.h: VALUE CLIPPING, BOUNDS LOSS). The kernels that take it are
// instantiations of their own, so the ones above never see it; an option that is off in such a call is a launch-uniform select
struct PpoOptK {
  const float* values_old;  // [M]; with vclip = 0 any M readable floats (the host gives `returns`), loaded and never chosen
  int32_t vclip, bnd;       // 0 / 1: value clipping, the bounds loss
  float clip_vf, bounds_coef;
  float lo[kPpoMaxA], hi[kPpoMaxA];  // -inf / +inf from the action width on
};
struct PpoOptMainK : PpoK {
  PpoOptK o;
  static constexpr bool kOpt = true;
};
// the columns of a row of partials the options fill: sum of the chosen squared value error, rows with |V - V_old| > clip_vf, sum b
constexpr int kPpoColVc = kPpoQ, kPpoColOut = kPpoQ + 1, kPpoColBnd = kPpoQ + 2;
static_assert(kPpoColBnd < kPpoStride, "the options' sums fit the spare columns");

__global__ __launch_bounds__(kPpoBlock) void ppo_adv_kernel(const float* __restrict__ adv, const uint8_t* __restrict__ vbytes, uint32_t vmask,
                                                             size_t rows, double* __restrict__ partials) {
  __shared__ double sh[kPpoWaves][kPpoAdvQ];
  const size_t stride = (size_t)gridDim.x * kPpoBlock;
  const uint32_t all = vmask == 0u ? 1u : 0u;  // (no branch on it: a bit OR-ed into every row's byte)
  uint32_t n = 0;
  double s1 = 0.0, s2 = 0.0;
  for (size_t r0 = (size_t)blockIdx.x * kPpoBlock + threadIdx.x; r0 < rows; r0 += (size_t)kPpoAdvUnroll * stride) {
    float x[kPpoAdvUnroll];
    uint32_t b[kPpoAdvUnroll];
#pragma unroll
    for (int u = 0; u < kPpoAdvUnroll; ++u) {  // every load of the eight rows (nothing here waits)
      const size_t rw = r0 + (size_t)u * stride;
      const size_t i = rw < rows ? rw : rows - 1;
      x[u] = adv[i];
      b[u] = vbytes[i];
    }
#pragma unroll
    for (int u = 0; u < kPpoAdvUnroll; ++u) {
      const bool ok = r0 + (size_t)u * stride < rows && ((b[u] & vmask) | all) != 0u;
      const double d = (double)x[u];
      n += ok ? 1u : 0u;
      s1 = s1 + (ok ? d : 0.0);
      s2 = s2 + (ok ? d * d : 0.0);
    }
  }
  const double q0 = ts_wave_sum((double)n), q1 = ts_wave_sum(s1), q2 = ts_wave_sum(s2);
  const int wave = (int)threadIdx.x / 64, lane = (int)threadIdx.x % 64;
  if (lane < kPpoAdvQ) sh[wave][lane] = lane == 0 ? q0 : lane == 1 ? q1 : q2;
  __syncthreads();
  if (threadIdx.x < kPpoAdvQ) {
    double v = sh[0][threadIdx.x];
#pragma unroll
    for (int w = 1; w < kPpoWaves; ++w) v = v + sh[w][threadIdx.x];
    partials[(size_t)blockIdx.x * kPpoAdvStride + threadIdx.x] = v;
  }
}

// ppo_adv_kernel through an index list (pf_ppo_grad_rows): slot j of the m takes the advantage and the validity byte of row row_index[j],
// the slots to the same threads in the same order, so the three sums have the bits of ppo_adv_kernel on the gathered copies. An index
// outside [0, rows_total) is not dereferenced: row 0 is loaded in its place and not chosen, and the slot is counted in the partials'
// fourth column (a whole number: its order of summation is free)
__global__ __launch_bounds__(kPpoBlock) void ppo_adv_rows_kernel(const float* __restrict__ adv, const uint8_t* __restrict__ vbytes, uint32_t vmask,
                                                                  const int32_t* __restrict__ row_index, size_t rows, uint32_t rows_total,
                                                                  double* __restrict__ partials) {
  __shared__ double sh[kPpoWaves][kPpoAdvStride];
  const size_t stride = (size_t)gridDim.x * kPpoBlock;
  const uint32_t all = vmask == 0u ? 1u : 0u;
  uint32_t n = 0, n_bad = 0;
  double s1 = 0.0, s2 = 0.0;
  for (size_t r0 = (size_t)blockIdx.x * kPpoBlock + threadIdx.x; r0 < rows; r0 += (size_t)kPpoAdvUnroll * stride) {
    uint32_t g[kPpoAdvUnroll];
    float x[kPpoAdvUnroll];
    uint32_t b[kPpoAdvUnroll];
#pragma unroll
    for (int u = 0; u < kPpoAdvUnroll; ++u) {  // the eight indices, then the eight rows behind them
      const size_t rw = r0 + (size_t)u * stride;
      g[u] = (uint32_t)row_index[rw < rows ? rw : rows - 1];
    }
#pragma unroll
    for (int u = 0; u < kPpoAdvUnroll; ++u) {
      const size_t i = g[u] < rows_total ? g[u] : 0u;  // (a negative index is a large unsigned one)
      x[u] = adv[i];
      b[u] = vbytes[i];
    }
#pragma unroll
    for (int u = 0; u < kPpoAdvUnroll; ++u) {
      const bool in = r0 + (size_t)u * stride < rows, good = g[u] < rows_total;
      const bool ok = in && good && ((b[u] & vmask) | all) != 0u;
      const double d = (double)x[u];
      n += ok ? 1u : 0u;
      n_bad += in && !good ? 1u : 0u;
      s1 = s1 + (ok ? d : 0.0);
      s2 = s2 + (ok ? d * d : 0.0);
    }
  }
  const double q0 = ts_wave_sum((double)n), q1 = ts_wave_sum(s1), q2 = ts_wave_sum(s2), q3 = ts_wave_sum((double)n_bad);
  const int wave = (int)threadIdx.x / 64, lane = (int)threadIdx.x % 64;
  if (lane < kPpoAdvStride) sh[wave][lane] = lane == 0 ? q0 : lane == 1 ? q1 : lane == 2 ? q2 : q3;
  __syncthreads();
  if (threadIdx.x < kPpoAdvStride) {
    double v = sh[0][threadIdx.x];
#pragma unroll
    for (int w = 1; w < kPpoWaves; ++w) v = v + sh[w][threadIdx.x];
    partials[(size_t)blockIdx.x * kPpoAdvStride + threadIdx.x] = v;
  }
}
// (ppo_adv_finish_kernel below, as it is, makes c, mu and sigma of these partials; the fourth column waits for the call's last kernel,
//  ppo_finish_rows_kernel, which adds it up into stats[14])

// One block. fin: c, mu, sigma, then the float32 roundings of mu and of 1 / max(sigma, 1e-8)
__global__ __launch_bounds__(kPpoBlock) void ppo_adv_finish_kernel(const double* __restrict__ partials, int n_blocks, double* __restrict__ fin) {
  __shared__ double seg[kPpoAdvQ * kPpoSeg];
  const int t = (int)threadIdx.x;
  if (t < kPpoAdvQ * kPpoSeg) {
    const int q = t / kPpoSeg, sg = t % kPpoSeg, chunk = (n_blocks + kPpoSeg - 1) / kPpoSeg;
    const int b1 = (sg + 1) * chunk < n_blocks ? (sg + 1) * chunk : n_blocks;
    double v = 0.0;
    for (int b = sg * chunk; b < b1; ++b) v = v + partials[(size_t)b * kPpoAdvStride + q];
    seg[t] = v;
  }
  __syncthreads();
  if (t == 0) {
    double tot[kPpoAdvQ];
#pragma unroll
    for (int q = 0; q < kPpoAdvQ; ++q) {
      double v = seg[q * kPpoSeg];
      for (int sg = 1; sg < kPpoSeg; ++sg) v = v + seg[q * kPpoSeg + sg];
      tot[q] = v;
    }
    const double c = tot[0];
    const double mu = c > 0.0 ? tot[1] / c : 0.0;
    const double var = c > 0.0 ? tot[2] / c - mu * mu : 0.0;  // sum (A - mu)^2 / c from the sums about 0
    const double sigma = sqrt(var > 0.0 ? var : 0.0);
    fin[0] = c;
    fin[1] = mu;
    fin[2] = sigma;
    fin[3] = (double)(float)mu;
    fin[4] = (double)(float)(1.0 / (sigma > 1e-8 ? sigma : 1e-8));
  }
}

// The per-row float32 sequence, in two halves that share nothing but `live`: ppo_main_kernel runs both on a row, the fused kernels of
// ppo_grad.hpp one each (the actor's launch the first, the critic's the second), so a row's gradients are the same bits either way.
//
// The actor's half, over the first `width` of W columns (ppo_main_kernel: width = W, known when it is compiled): the row's gradient
// with respect to its means -> gm, the float32 terms of grad_log_std -> gt, and min(u, v), r and logp - logp_old for the statistics.
// `cf`: lo_clip, hi_clip, w32, mu32, inv32. Every choice is a select: an invalid row's inputs are used and not chosen
template <int W>
PF_DEV void ppo_actor_row(const float (&m)[W], const float (&x)[W], const float (&ls)[W], const float (&inv)[W], const int width, const float lpo,
                          const float ad, const bool live, const bool norm, const float (&cf)[5], float (&gm)[W], float (&gt)[W], float& surr,
                          float& r, float& d) {
  float z[W], logp = 0.0f;
#pragma unroll
  for (int c = 0; c < W; ++c) {
    z[c] = (x[c] - m[c]) * inv[c];
    logp = c < width ? logp + gae_logp_term(x[c], m[c], ls[c], inv[c]) : logp;
  }
  const float adv = norm ? (ad - cf[3]) * cf[4] : ad;
  d = logp - lpo;
  r = expf(d);
  const float su = r * adv;
  const float sv = fminf(fmaxf(r, cf[0]), cf[1]) * adv;
  surr = fminf(su, sv);
  const bool act = live && su <= sv;  // the branch of the minimum that depends on the new policy
  const float gl = act ? ((-cf[2]) * adv) * r : 0.0f;  // d loss / d logp
#pragma unroll
  for (int c = 0; c < W; ++c) {
    gm[c] = act && c < width ? (gl * z[c]) * inv[c] : 0.0f;
    gt[c] = act && c < width ? gl * (z[c] * z[c] - 1.0f) : 0.0f;
  }
}
// its terms of the statistics: sum min(u, v), sum (r - 1) - d, the rows with |r - 1| > clip, min r, max r
PF_DEV void ppo_actor_terms(const bool live, const float surr, const float r, const float d, const float clip, double& s_surr, double& s_kl,
                            uint32_t& n_clip, float& r_lo, float& r_hi) {
  s_surr = s_surr + (live ? (double)surr : 0.0);
  s_kl = s_kl + (live ? (double)((r - 1.0f) - d) : 0.0);
  n_clip += live && fabsf(r - 1.0f) > clip ? 1u : 0u;
  r_lo = live ? fminf(r_lo, r) : r_lo;
  r_hi = live ? fmaxf(r_hi, r) : r_hi;
}
// The critic's half: returns the row's gradient with respect to its value, kv = vf_coef * w32; its terms: sum (V - R)^2, sum R,
// sum R^2, sum (V - R)
PF_DEV float ppo_critic_row(const float vl, const float rt, const float kv, const bool live, double& s_d2, double& s_r, double& s_r2, double& s_d) {
  const float dv = vl - rt;
  const double R = (double)rt, D = (double)dv;
  s_d2 = s_d2 + (live ? D * D : 0.0);
  s_r = s_r + (live ? R : 0.0);
  s_r2 = s_r2 + (live ? R * R : 0.0);
  s_d = s_d + (live ? D : 0.0);
  return live ? kv * dv : 0.0f;
}

// The options' halves, run behind the two above on the same row (so a call without them is the functions above and nothing else).
// The bounds loss: b = sum_c (hx^2 + lx^2) over the first `width` columns, returned for a live row (0 otherwise), and its gradient
// kb (hx - lx), kb = (2 bounds_coef) w32, added to gm on every live row
template <int W>
PF_DEV float ppo_bounds_row(const float (&m)[W], const int width, const bool use, const float kb, const float (&lo)[kPpoMaxA],
                            const float (&hi)[kPpoMaxA], float (&gm)[W]) {
  float b = 0.0f;
#pragma unroll
  for (int c = 0; c < W; ++c) {
    const float hx = fmaxf(m[c] - hi[c], 0.0f), lx = fmaxf(lo[c] - m[c], 0.0f);
    const bool on = use && c < width;
    b = on ? b + (hx * hx + lx * lx) : b;
    gm[c] = on ? gm[c] + kb * (hx - lx) : gm[c];
  }
  return b;
}
// Value clipping: gv = ppo_critic_row's gradient of the row; returns 0 where the clipped branch is the larger one. s_c2: the sum of
// the chosen square; n_out: the live rows with |V - V_old| > clip_vf. |dc| > |dv| is dc^2 > dv^2 decided exactly
PF_DEV float ppo_vclip_row(const float gv, const float vl, const float rt, const float vo, const float clip_vf, const bool use, double& s_c2,
                           uint32_t& n_out) {
  const float e = vl - vo;
  const bool out = fabsf(e) > clip_vf;
  const float vc = e > 0.0f ? vo + clip_vf : vo - clip_vf;
  const float dv = vl - rt, dc = vc - rt;
  const bool use_c = use && out && fabsf(dc) > fabsf(dv);
  const double D = (double)dv, C = (double)dc;
  s_c2 = s_c2 + (use ? (use_c ? C * C : D * D) : 0.0);
  n_out += use && out ? 1u : 0u;
  return use_c ? 0.0f : gv;
}

// (amdgpu_waves_per_eu(4, 4) and kPpoMaxGrid go together: 1024 blocks of four waves are 16 waves per CU on 256 CUs, four per SIMD, so the
//  whole grid is resident at once for every instantiation without options; the float4 one needs the cap for its registers, the generic
//  ones just obey it)
// (with the options the float4 instantiation and the eight-wide one hold three more sums and a fourth per-row stream: at 128 registers
//  they spill, so these two alone run at three waves per SIMD, 768 of the 1024 blocks resident and the rest behind them, and keep their
//  scratch at 0; nothing waits on the whole grid, so residency is a matter of speed only)
// KT: PpoK, or PpoOptMainK (pf_ppo_loss_opt: one more [M] stream, three more sums)
template <int W, bool VEC, class KT>
__global__ __launch_bounds__(kPpoBlock) __attribute__((amdgpu_waves_per_eu(KT::kOpt && (VEC || W == 8) ? 3 : 4, 4))) void ppo_main_kernel(KT a, size_t rows, const double* __restrict__ fin, double* __restrict__ partials) {
  static_assert(!VEC || W == 4, "the float4 path is four wide");
  constexpr bool OPT = KT::kOpt;
  constexpr int U = VEC ? kPpoRowsVec : kPpoRowsGen, QN = OPT ? kPpoStride : kPpoQ;
  __shared__ double sh[kPpoWaves][QN];
  float ls[W], inv[W];
#pragma unroll
  for (int c = 0; c < W; ++c) {
    ls[c] = a.log_std[c];
    inv[c] = expf(-ls[c]);
  }
  const double cnt = fin[0];
  const float w32 = cnt > 0.0 ? (float)(1.0 / cnt) : 0.0f;
  const float mu32 = (float)fin[3], inv32 = (float)fin[4];
  const float cf[5] = {1.0f - a.clip, 1.0f + a.clip, w32, mu32, inv32}, kv = a.vf_coef * w32;
  const uint32_t all = a.vmask == 0u ? 1u : 0u;  // (no branch on it: a bit OR-ed into every row's byte)
  const bool norm = a.normalize != 0;
  const size_t stride = (size_t)gridDim.x * kPpoBlock;
  double sum[kPpoSums], gls[W];
  uint32_t n_clip = 0;  // (sum[3] stays 0 until the end: the count is a whole number)
#pragma unroll
  for (int q = 0; q < kPpoSums; ++q) sum[q] = 0.0;
#pragma unroll
  for (int c = 0; c < W; ++c) gls[c] = 0.0;
  float r_lo = INFINITY, r_hi = -INFINITY;
  double s_c2 = 0.0, s_b = 0.0;  // (the options' sums: dead code without them)
  uint32_t n_out = 0;
  float kb = 0.0f;
  if constexpr (OPT) kb = (2.0f * a.o.bounds_coef) * w32;
  for (size_t r0 = (size_t)blockIdx.x * kPpoBlock + threadIdx.x; r0 < rows; r0 += (size_t)U * stride) {
    float m[U][W], x[U][W], lpo[U], ad[U], rt[U], vl[U], vo[OPT ? U : 1];
    uint32_t b[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {  // every load of the U rows (nothing here waits); the rows past M read row M - 1 again
      const size_t rw = r0 + (size_t)u * stride;
      const size_t i = rw < rows ? rw : rows - 1;
      if constexpr (VEC) {
        const float4 mm = reinterpret_cast<const float4*>(a.mean)[i];
        const float4 xx = reinterpret_cast<const float4*>(a.actions)[i];
        m[u][0] = mm.x, m[u][1] = mm.y, m[u][2] = mm.z, m[u][3] = mm.w;
        x[u][0] = xx.x, x[u][1] = xx.y, x[u][2] = xx.z, x[u][3] = xx.w;
      } else {
#pragma unroll
        for (int c = 0; c < W; ++c) {
          m[u][c] = a.mean[i * W + c];
          x[u][c] = a.actions[i * W + c];
        }
      }
      lpo[u] = a.logp_old[i];
      ad[u] = a.advantages[i];
      rt[u] = a.returns[i];
      vl[u] = a.value[i];
      b[u] = a.vbytes[i];
      if constexpr (OPT) vo[u] = a.o.values_old[i];
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const size_t rw = r0 + (size_t)u * stride;
      const bool in = rw < rows;
      const bool live = in && ((b[u] & a.vmask) | all) != 0u;
      float gm[W], gt[W], surr, r, d;
      ppo_actor_row<W>(m[u], x[u], ls, inv, W, lpo[u], ad[u], live, norm, cf, gm, gt, surr, r, d);
#pragma unroll
      for (int c = 0; c < W; ++c) gls[c] = gls[c] + (double)gt[c];
      ppo_actor_terms(live, surr, r, d, a.clip, sum[0], sum[2], n_clip, r_lo, r_hi);
      float gv = ppo_critic_row(vl[u], rt[u], kv, live, sum[1], sum[4], sum[5], sum[6]);
      if constexpr (OPT) {
        s_b = s_b + (double)ppo_bounds_row<W>(m[u], W, live && a.o.bnd != 0, kb, a.o.lo, a.o.hi, gm);
        gv = ppo_vclip_row(gv, vl[u], rt[u], vo[u], a.o.clip_vf, live && a.o.vclip != 0, s_c2, n_out);
      }
      if (in) {
        if constexpr (VEC) {
          ppo_f4 o;
          o.x = gm[0], o.y = gm[1], o.z = gm[2], o.w = gm[3];
          __builtin_nontemporal_store(o, reinterpret_cast<ppo_f4*>(a.grad_mean) + rw);
        } else {
#pragma unroll
          for (int c = 0; c < W; ++c) __builtin_nontemporal_store(gm[c], a.grad_mean + rw * W + c);
        }
        __builtin_nontemporal_store(gv, a.grad_value + rw);
      }
    }
  }
  sum[3] = (double)n_clip;
  double q[QN];
#pragma unroll
  for (int j = 0; j < kPpoSums; ++j) q[j] = ts_wave_sum(sum[j]);
  q[kPpoSums] = ts_wave_min((double)r_lo);
  q[kPpoSums + 1] = ts_wave_max((double)r_hi);
#pragma unroll
  for (int c = 0; c < kPpoMaxA; ++c) q[kPpoSums + 2 + c] = c < W ? ts_wave_sum(gls[c < W ? c : 0]) : 0.0;
  if constexpr (OPT) {
    q[kPpoColVc] = ts_wave_sum(s_c2);
    q[kPpoColOut] = ts_wave_sum((double)n_out);
    q[kPpoColBnd] = ts_wave_sum(s_b);
  }
  const int wave = (int)threadIdx.x / 64, lane = (int)threadIdx.x % 64;
  if (lane < QN) {  // (every lane holds all of them: lane t writes the t-th)
    double v = q[0];
#pragma unroll
    for (int j = 1; j < QN; ++j) v = lane == j ? q[j] : v;
    sh[wave][lane] = v;
  }
  __syncthreads();
  if (threadIdx.x < QN) {  // the block's four waves in ascending order
    const int j = (int)threadIdx.x;
    double v = sh[0][j];
#pragma unroll
    for (int w = 1; w < kPpoWaves; ++w) v = j == kPpoSums ? fmin(v, sh[w][j]) : j == kPpoSums + 1 ? fmax(v, sh[w][j]) : v + sh[w][j];
    partials[(size_t)blockIdx.x * kPpoStride + j] = v;
  }
}

constexpr double kPpoEntropyConst = 1.41893853320467274178;  // 1/2 (1 + log 2 pi)

// One block. partials: n_blocks rows of kPpoStride; fin: ppo_adv_finish_kernel's. OPT: the options' three columns are summed too, and
// vclip / bnd say which of them are live (a column of an option that is off holds a sum nobody asked for, and is not used).
// bad: null, or a word of LDS written before the call that holds stats[14] (ppo_finish_rows_kernel)
template <bool OPT>
PF_DEV void ppo_finish(const double* __restrict__ partials, const int n_blocks, const double* __restrict__ fin, const float* __restrict__ log_std,
                       const int width, const float vf_coef, const float ent_coef, double* __restrict__ stats, float* __restrict__ grad_log_std,
                       const bool vclip, const bool bnd, const float bounds_coef, const double* bad = nullptr) {
  constexpr int QN = OPT ? kPpoStride : kPpoQ;
  __shared__ double seg[QN * kPpoSeg];
  const int t = (int)threadIdx.x;
  if (t < QN * kPpoSeg) {
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
  auto total = [&](int q) {
    double v = seg[q * kPpoSeg];
    for (int sg = 1; sg < kPpoSeg; ++sg) {
      const double x = seg[q * kPpoSeg + sg];
      v = q == kPpoSums ? fmin(v, x) : q == kPpoSums + 1 ? fmax(v, x) : v + x;
    }
    return v;
  };
  if (t < width) grad_log_std[t] = (float)(total(kPpoSums + 2 + t) - (double)ent_coef);
  if (t == 64) {  // (another wave than the one that writes grad_log_std)
    const double c = fin[0];
    const double w = c > 0.0 ? 1.0 / c : 0.0;
    double H = 0.0;
    for (int k = 0; k < width; ++k) H = H + ((double)log_std[k] + kPpoEntropyConst);
    const double policy_loss = -(w * total(0));
    double value_loss = 0.5 * (w * total(1));
    if constexpr (OPT) value_loss = vclip ? 0.5 * (w * total(kPpoColVc)) : value_loss;
    const double mean_r = w * total(4), mean_d = w * total(6);
    const double var_r = w * total(5) - mean_r * mean_r, var_d = w * total(1) - mean_d * mean_d;
    double loss = (policy_loss + (double)vf_coef * value_loss) - (double)ent_coef * H;
    double clipped = 0.0, bounds_loss = 0.0;
    if constexpr (OPT) {
      clipped = vclip ? w * total(kPpoColOut) : 0.0;
      bounds_loss = bnd ? w * total(kPpoColBnd) : 0.0;
      loss = bnd ? loss + (double)bounds_coef * bounds_loss : loss;
    }
    stats[0] = c;
    stats[1] = loss;
    stats[2] = policy_loss;
    stats[3] = value_loss;
    stats[4] = H;
    stats[5] = w * total(2);
    stats[6] = w * total(3);
    stats[7] = fin[1];
    stats[8] = fin[2];
    stats[9] = 1.0 - var_d / var_r;
    stats[10] = total(kPpoSums);
    stats[11] = total(kPpoSums + 1);
    stats[12] = clipped;
    stats[13] = bounds_loss;
    stats[14] = bad ? *bad : 0.0;
    stats[15] = 0.0;
  }
}
__global__ __launch_bounds__(kPpoBlock) void ppo_finish_kernel(const double* __restrict__ partials, int n_blocks, const double* __restrict__ fin,
                                                                const float* __restrict__ log_std, int width, float vf_coef, float ent_coef,
                                                                double* __restrict__ stats, float* __restrict__ grad_log_std) {
  ppo_finish<false>(partials, n_blocks, fin, log_std, width, vf_coef, ent_coef, stats, grad_log_std, false, false, 0.0f);
}
__global__ __launch_bounds__(kPpoBlock) void ppo_finish_opt_kernel(const double* __restrict__ partials, int n_blocks, const double* __restrict__ fin,
                                                                    const float* __restrict__ log_std, int width, float vf_coef, float ent_coef,
                                                                    double* __restrict__ stats, float* __restrict__ grad_log_std, int vclip, int bnd,
                                                                    float bounds_coef) {
  ppo_finish<true>(partials, n_blocks, fin, log_std, width, vf_coef, ent_coef, stats, grad_log_std, vclip != 0, bnd != 0, bounds_coef);
}
// pf_ppo_grad_rows' last kernel: ppo_finish_kernel (OPT = false) or ppo_finish_opt_kernel, with stats[14] = the slots whose index
// lay outside the batch: the fourth column of ppo_adv_rows_kernel's adv_blocks rows of partials, whole numbers added up by wave 2
template <bool OPT>
__global__ __launch_bounds__(kPpoBlock) void ppo_finish_rows_kernel(const double* __restrict__ partials, int n_blocks, const double* __restrict__ fin,
                                                                     const float* __restrict__ log_std, int width, float vf_coef, float ent_coef,
                                                                     double* __restrict__ stats, float* __restrict__ grad_log_std, int vclip, int bnd,
                                                                     float bounds_coef, const double* __restrict__ adv_part, int adv_blocks) {
  __shared__ double bad;
  const int wave = (int)threadIdx.x / 64, lane = (int)threadIdx.x % 64;
  if (wave == 2) {
    double v = 0.0;
    for (int b = lane; b < adv_blocks; b += 64) v = v + adv_part[(size_t)b * kPpoAdvStride + kPpoAdvQ];
    v = ts_wave_sum(v);
    if (lane == 0) bad = v;
  }
  ppo_finish<OPT>(partials, n_blocks, fin, log_std, width, vf_coef, ent_coef, stats, grad_log_std, vclip != 0, bnd != 0, bounds_coef, &bad);  // (its barrier orders the word)
}

}  // namespace pf
