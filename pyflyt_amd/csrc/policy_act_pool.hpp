// pf_policy_act_pool: pf_policy_act's network (policy_act.hpp) for a POOL of up to PF_POLICY_POOL_MAX policies in one launch, every
// row evaluated once by the policy its entry of row_policy names. And pf_policy_pool_plan, which sorts the rows by policy.
//
// The plan (device, opaque to the caller; T = ceil(n / 64) + P tiles, which always suffice):
//     int32 tile_policy[T]     the policy tile j runs, or -1 for a tile nobody uses
//     int32 row[T][64]         the rows of tile j, -1 in the padding slots
// Policy p owns the tiles first[p] .. first[p + 1] - 1, first[p + 1] - first[p] = ceil(count[p] / 64), and its rows stand in them
// in ascending order; the slots behind the last row of its last tile, and every slot of the unused tiles, hold -1. Every byte is
// written exactly once by every call and nothing depends on the order threads run in: the plan's BYTES are a function of row_policy.
//
// policy_pool_plan_kernel: one workgroup of sixteen waves, a counting sort in three phases. Each wave owns a contiguous range of
// 64-row chunks. (1) it counts its rows per policy, one ballot per policy and chunk, lane p keeping policy p's count; (2) thread 0
// turns the 16 x P counts into each policy's first tile and each wave's first slot for each policy; (3) each wave walks its chunks
// again and writes a row to its policy's next slot plus its rank in the chunk's ballot. It is built once per assignment, so it is
// written to be read, not to be fast (profiles/policy_pool/bench.json has what it costs).
//
// policy_act_pool_kernel is policy_act_kernel with four differences, and everything that computes a bit is the text that kernel
// runs (mlp_tile.hpp: tile_fill, tile_chain, act_store_hidden, tile_out_pair, act_barrier; policy_mlp.hpp: pol_tanh, philox, bm16):
//   * a tile's 64 row indices come from the plan. The observation rows are gathered (a lane per column, so a row's columns are
//     still coalesced; the index of a wave's row is the same in all its lanes and is loaded as a scalar) and the stores are
//     scattered to the row's own index; a padding slot (-1) loads zeros and stores nothing, as the ragged last tile does there.
//   * a workgroup walks a CONTIGUOUS range of plan tiles and stages W0 / W1 / WO / the biases / exp(log_std) again only when the
//     tile's policy differs from the one staged: the plan is sorted by policy, so that is once per workgroup and once more per
//     policy boundary inside its range. (D > 64 restages the first layer's chunks per tile, as policy_act_kernel does.)
//   * the P pf_policy blocks are kernel arguments (17 x 88 bytes); the tile's block is read from there with a uniform index.
//   * the Philox key is the row's global lane, lane0 + row, not its position in the tile.
// Both indices that come out of the plan are range-checked before they address anything: (unsigned)row < n, (unsigned)p < P. A
// stale plan gives wrong actions, never an access outside the caller's tensors.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../../include/pyflyt_amd.h"
#include "uav_device.hpp"
#include "policy_mlp.hpp"
#include "mlp_tile.hpp"
#include "policy_act.hpp"

namespace pf {

constexpr int kPoolMax = PF_POLICY_POOL_MAX;
constexpr int kPoolPlanWaves = 16;  // policy_pool_plan_kernel's one workgroup

// the tiles of a plan for n rows and P policies
inline int pool_plan_tiles(const int n, const int P) { return (n - 1) / kActRows + 1 + P; }
// the most rows a plan is made for: its slots are counted in 32 bits
constexpr int kPoolMaxRows = INT32_MAX - kActRows * (kPoolMax + 1);

__global__ void __launch_bounds__(64 * kPoolPlanWaves) policy_pool_plan_kernel(const int32_t* row_policy, const int n, const int P, int32_t* plan, const int T) {
  __shared__ int cnt[kPoolPlanWaves][kPoolMax];  // phase 1: wave w's rows of policy p; phase 2 on: the slot its first one goes to
  __shared__ int first[kPoolMax + 1];            // the first tile of policy p; first[P]: the first unused tile
  __shared__ int total[kPoolMax];                // the rows of policy p
  const int t = (int)threadIdx.x, lane = t & 63, wv = t >> 6;
  int32_t* tile_policy = plan;
  int32_t* rows = plan + T;
  const int chunks = (n - 1) / 64 + 1;
  const int c0 = (int)((int64_t)chunks * wv / kPoolPlanWaves), c1 = (int)((int64_t)chunks * (wv + 1) / kPoolPlanWaves);
  const uint64_t below = (1ull << lane) - 1ull;

  int mine = 0;  // lane p: this wave's rows of policy p so far
  for (int c = c0; c < c1; ++c) {
    const int i = c * 64 + lane;
    const int v = i < n ? row_policy[i] : -1;
    for (int p = 0; p < P; ++p) {
      const uint64_t m = __ballot(v == p);
      if (lane == p) mine += __popcll(m);
    }
  }
  if (lane < kPoolMax) cnt[wv][lane] = lane < P ? mine : 0;
  __syncthreads();
  if (t == 0) {
    int tile = 0;
    for (int p = 0; p < P; ++p) {
      int sum = 0;
      for (int w = 0; w < kPoolPlanWaves; ++w) {
        const int x = cnt[w][p];
        cnt[w][p] = tile * kActRows + sum;
        sum += x;
      }
      first[p] = tile, total[p] = sum;
      tile += (sum + kActRows - 1) / kActRows;
    }
    first[P] = tile;
  }
  __syncthreads();
  const int slots = T * kActRows;
  int next = lane < P ? cnt[wv][lane] : 0;  // lane p: the slot this wave's next row of policy p goes to
  for (int c = c0; c < c1; ++c) {
    const int i = c * 64 + lane;
    const int v = i < n ? row_policy[i] : -1;
    for (int p = 0; p < P; ++p) {
      const uint64_t m = __ballot(v == p);
      const int o = __shfl(next, p) + __popcll(m & below);
      if (v == p && o < slots) rows[o] = i;
      if (lane == p) next += __popcll(m);
    }
  }
  // the padding behind each policy's last row, the unused tiles, and which policy a tile runs
  for (int p = 0; p < P; ++p)
    for (int j = first[p] * kActRows + total[p] + t; j < first[p + 1] * kActRows && j < slots; j += 64 * kPoolPlanWaves) rows[j] = -1;
  for (int j = first[P] * kActRows + t; j < slots; j += 64 * kPoolPlanWaves) rows[j] = -1;
  for (int j = t; j < T; j += 64 * kPoolPlanWaves) {
    int p = -1;
    for (int q = 0; q < P; ++q)
      if (j >= first[q] && j < first[q + 1]) p = q;
    tile_policy[j] = p;
  }
}

struct ActPoolK {
  pf_policy Q[kPoolMax];
  const float* obs;
  float* mean_out;
  float* actions_out;
  const int32_t* plan;
  int n, D, A, P, T;
  uint32_t seed_lo, seed_hi, step;
  uint64_t lane0;
};

__global__ void __launch_bounds__(256) policy_act_pool_kernel(const ActPoolK K) {
  __shared__ float Wc[kPolH * kPolH];      // the first layer's chunk [k][(unit + k) & 63]
  __shared__ float W1s[kPolH * kPolH];     // the second layer, likewise
  __shared__ float WOs[kPolH * kActMaxA];  // the output layer [i][c]
  __shared__ float Bs[2 * kPolH + 2 * kActMaxA];  // b0, b1, the output bias, exp(log_std)
  __shared__ float T[kActRows * kActTS];
  const int t = (int)threadIdx.x, lane = t & 63, wv = __builtin_amdgcn_readfirstlane(t >> 6);
  const int l31 = lane & 31, h = lane >> 5, mt = wv & 1, nt = wv >> 1;
  const int D = K.D, A = K.A, n = K.n;
  const int32_t* tile_policy = K.plan;
  const int32_t* rows = K.plan + K.T;
  const int nchunks = (D + kPolH - 1) / kPolH;
  // this workgroup's tiles: a contiguous range, so that a policy's weights are staged once for all of its tiles in the range
  const int tile0 = (int)((int64_t)K.T * (int)blockIdx.x / (int)gridDim.x), tile1 = (int)((int64_t)K.T * ((int)blockIdx.x + 1) / (int)gridDim.x);

  // a [64][64] block of a layer: thread t reads (unit j = 4 i + wv, input k = lane) for i = 0 .. 15, all sixteen loads in flight
  auto stage_block = [&](float* dst, const float* w, const int stride, const int k0, const int n_in, const int n_out) {
    float v[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int j = 4 * i + wv;
      v[i] = (k0 + lane < n_in && j < n_out) ? w[(size_t)j * stride + k0 + lane] : 0.0f;
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) dst[lane * kPolH + ((4 * i + wv + lane) & 63)] = v[i];
  };
  // the observation chunk of a tile: wave wv the slots 16 wv .. 16 wv + 15, a lane per column; columns from D on, and padding slots, are zero
  auto load_x = [&](const int tile, const int ch, float (&x)[16]) {
    const int c = ch * kPolH + lane;
#pragma unroll
    for (int rr = 0; rr < 16; ++rr) {
      const int g = rows[(size_t)tile * kActRows + wv * 16 + rr];
      x[rr] = ((unsigned)g < (unsigned)n && c < D) ? K.obs[(size_t)g * D + c] : 0.0f;
    }
  };

  const float* arow = T + (mt * 32 + l31) * kActTS;  // A operand: this lane's row of the tile
  const int bcol = nt * 32 + l31;                    // B operand and C/D: this lane's hidden unit
  float* hcol = T + (mt * 32) * kActTS + bcol;       // where the lane's accumulator registers go
  int staged = -1;  // the policy whose weights are in LDS
  float xc[16];     // the next observation chunk, loaded one chunk ahead of its use: the matrix phase covers the loads' latency
  if (tile0 < tile1) load_x(tile0, 0, xc);
  for (int tile = tile0; tile < tile1; ++tile) {
    const int p = __builtin_amdgcn_readfirstlane(tile_policy[tile]);
    if ((unsigned)p >= (unsigned)K.P) {  // a tile nobody uses (the same verdict in every lane: no barrier is skipped by some)
      if (tile + 1 < tile1) load_x(tile + 1, 0, xc);
      continue;
    }
    const pf_policy& Q = K.Q[p];
    const bool three = Q.n_layers == 3;
    const int w0 = Q.width[0], w1 = Q.width[1];
    const int hl = three ? w1 : w0;  // the width the output layer reads
    const bool restage = p != staged;
    staged = p;
    act_f16v acc;
    for (int ch = 0; ch < nchunks; ++ch) {
      const int c0 = ch * kPolH;
      act_barrier();  // the previous readers of T, of Wc and (behind a tile's last phase) of every other staged block are done
      if (restage || nchunks > 1) stage_block(Wc, Q.w[0], D, c0, D, w0);
      if (restage && ch == 0) {
        const float* wo = Q.w[three ? 2 : 1];
        const float* bo = Q.b[three ? 2 : 1];
        if (three) stage_block(W1s, Q.w[1], w0, 0, w0, w1);
        for (int idx = t; idx < kPolH * kActMaxA; idx += 256) {
          const int i = idx / kActMaxA, c = idx % kActMaxA;
          WOs[idx] = (i < hl && c < A) ? wo[(size_t)c * hl + i] : 0.0f;
        }
        if (t < kPolH) {
          Bs[t] = t < w0 ? Q.b[0][t] : 0.0f;
          Bs[kPolH + t] = (three && t < w1) ? Q.b[1][t] : 0.0f;
        }
        if (t < kActMaxA) {
          Bs[2 * kPolH + t] = t < A ? bo[t] : 0.0f;
          Bs[2 * kPolH + kActMaxA + t] = (Q.log_std && t < A) ? expf(Q.log_std[t]) : 0.0f;
        }
      }
#pragma unroll
      for (int rr = 0; rr < 16; ++rr) T[(wv * 16 + rr) * kActTS + lane] = xc[rr];
      {
        const bool last = ch + 1 == nchunks;
        const int nt_tile = last ? tile + 1 : tile;
        if (nt_tile < tile1) load_x(nt_tile, last ? 0 : ch + 1, xc);
      }
      act_barrier();
      if (ch == 0) acc = tile_fill(Bs[bcol]);
      const int np = (min(kPolH, D - c0) + 1) >> 1;
      acc = tile_chain(acc, arow, Wc, bcol, h, np);
    }
    act_barrier();
    act_store_hidden(Q.activation, acc, hcol, h);
    act_barrier();
    if (three) {
      acc = tile_fill(Bs[kPolH + bcol]);
      acc = tile_chain(acc, arow, W1s, bcol, h, kPolH / 2);
      act_barrier();
      act_store_hidden(Q.activation, acc, hcol, h);
      act_barrier();
    }
    // the affine output layer and the draw: lane = slot, this wave the outputs ca and ca + 1
    const int ca = 2 * wv;
    if (ca < A) {
      float m0 = Bs[2 * kPolH + ca], m1 = Bs[2 * kPolH + ca + 1];
      tile_out_pair(WOs, T + lane * kActTS, ca, m0, m1);
      const int g = rows[(size_t)tile * kActRows + lane];  // the slot's row, or -1
      float a0 = m0, a1 = m1;
      if (Q.log_std != nullptr) {
        // pf_policy_act's draw: one Philox call per row keyed by its GLOBAL lane, stream 4; this wave the Box-Muller pair of word wv
        const u32x4 r = philox4x32(K.seed_lo, K.seed_hi, (uint32_t)(K.lane0 + (uint64_t)g), K.step, 0u, 4u);
        float e0, e1;
        bm16(wv == 0 ? r.a : wv == 1 ? r.b : wv == 2 ? r.c : r.d, e0, e1);
        a0 = fmaf(Bs[2 * kPolH + kActMaxA + ca], e0, m0);
        a1 = fmaf(Bs[2 * kPolH + kActMaxA + ca + 1], e1, m1);
      }
      if ((unsigned)g < (unsigned)n) {
        const size_t o = (size_t)g * A;
        K.actions_out[o + ca] = a0;
        if (K.mean_out != nullptr) K.mean_out[o + ca] = m0;
        if (ca + 1 < A) {
          K.actions_out[o + ca + 1] = a1;
          if (K.mean_out != nullptr) K.mean_out[o + ca + 1] = m1;
        }
      }
    }
  }
}

}  // namespace pf
