// pf_policy_act: pf_rollout_policy's MLP as a launch of its own -- [n][D] observation rows in, [n][A] actions and means out, for any
// context with an env task (policy_mlp.hpp evaluates the same network inside the QuadX rollout launch, one lane per env).
//
// How it is laid out: a batched matrix product on the f32-input matrix instruction, v_mfma_f32_32x32x2_f32, whose result is bit for
// bit a k-ordered fmaf chain from its C operand: accumulator = bias, k ascending is exactly the contract's "bias first, then the
// inputs in ascending index, one fused multiply-add each, float32".
//   * a workgroup of four waves owns a tile of 64 rows: wave (mt, nt) computes rows 32 mt .. 32 mt + 31 x hidden units
//     32 nt .. 32 nt + 31, one 32x32 accumulator (16 registers); rows on M, hidden units on N.
//   * the weights are staged into LDS once per workgroup, transposed from torch's [out][in] to [k][unit] with the unit index
//     rotated by k ((unit + k) & 63): the staging reads global memory along k (contiguous) and the lanes of a write differ in k, so
//     without the rotation all 64 would hit one bank. Workgroups stride over the tiles, so the staging is paid once per
//     workgroup, not once per tile. The first layer is staged in chunks of 64 inputs: D <= 64 is one chunk, staged once; a wider
//     observation (the dogfight's, up to 128) restages its chunks for every tile -- 32 KB of first-layer weights would not leave
//     room for the tile under the 64 KB of static LDS.
//   * the tile T[64][65] holds the observation chunk, then the first hidden layer, then the second: the accumulator (C/D layout:
//     unit on the lane, rows in the registers) goes through the activation into T and is read back in the A-operand layout (row on
//     the lane, k in the lane half). The row stride is odd: with 64 the 32 rows of an A read would share a bank.
//   * the observation rows of the NEXT chunk (the next tile's, for D <= 64) are loaded into registers before the matrix phase of the
//     current one and stored to T after it: sixteen loads in flight per lane, their latency behind the tile's matrix and activation phases.
//   * the ragged last tile clamps the row it reads and masks its stores: all 64 lanes are live at every matrix instruction.
//   * an odd D gets a zero last k-pair (T's column D and the weights' row D are zero): an exact term.
//   * the output layer (4, 6 or 7 wide) is plain fmaf: lane = row, wave w the outputs 2w and 2w + 1, the weights broadcast from LDS.
//   * nothing is kept between calls: no packed block in the context, the caller's tensors are read at every call.
//   * the tile constants, the barrier, the accumulator's fill, row map and activation store, the matrix chain and the output pair's
//     fmaf chain are mlp_tile.hpp's (mlp.hpp and ppo_grad.hpp run them too).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../../include/pyflyt_amd.h"
#include "uav_device.hpp"
#include "policy_mlp.hpp"
#include "mlp_tile.hpp"

namespace pf {

struct ActK {
  pf_policy Q;
  float* actions_out;
  int n, D, A;
  uint32_t seed_lo, seed_hi, step;
  uint64_t lane0;
};

__global__ void __launch_bounds__(256) policy_act_kernel(const ActK K) {
  __shared__ float Wc[kPolH * kPolH];      // the first layer's chunk [k][(unit + k) & 63]
  __shared__ float W1s[kPolH * kPolH];     // the second layer, likewise
  __shared__ float WOs[kPolH * kActMaxA];  // the output layer [i][c]
  __shared__ float Bs[2 * kPolH + 2 * kActMaxA];  // b0, b1, the output bias, exp(log_std)
  __shared__ float T[kActRows * kActTS];
  const int t = (int)threadIdx.x, lane = t & 63, wv = t >> 6;
  const int l31 = lane & 31, h = lane >> 5, mt = wv & 1, nt = wv >> 1;
  const pf_policy& Q = K.Q;
  const int D = K.D, A = K.A, n = K.n;
  const bool three = Q.n_layers == 3;
  const int w0 = Q.width[0], w1 = Q.width[1];
  const int hl = three ? w1 : w0;  // the width the output layer reads
  const float* wo = Q.w[three ? 2 : 1];
  const float* bo = Q.b[three ? 2 : 1];
  const int nchunks = (D + kPolH - 1) / kPolH;
  const int ntiles = (n + kActRows - 1) / kActRows;

  // a [64][64] block of a layer: thread t reads (unit j = 4 i + wv, input k = lane) for i = 0 .. 15, all sixteen loads in flight
  auto stage_block = [&](float* dst, const float* w, const int stride, const int k0, const int n_in, const int n_out, const bool on) {
    float v[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int j = 4 * i + wv;
      v[i] = (on && k0 + lane < n_in && j < n_out) ? w[(size_t)j * stride + k0 + lane] : 0.0f;
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) dst[lane * kPolH + ((4 * i + wv + lane) & 63)] = v[i];
  };
  auto stage_w0 = [&](const int c0) { stage_block(Wc, Q.w[0], D, c0, D, w0, true); };
  // the observation chunk of a tile: wave wv rows 16 wv .. 16 wv + 15, a lane per column; columns from D on are zero
  auto load_x = [&](const int tile, const int ch, float (&x)[16]) {
    const int c = ch * kPolH + lane;
#pragma unroll
    for (int rr = 0; rr < 16; ++rr) {
      const int g = min(tile * kActRows + wv * 16 + rr, n - 1);
      x[rr] = c < D ? Q.obs0[(size_t)g * D + c] : 0.0f;
    }
  };
  stage_block(W1s, Q.w[1], w0, 0, w0, w1, three);
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

  const float* arow = T + (mt * 32 + l31) * kActTS;  // A operand: this lane's row of the tile
  const int bcol = nt * 32 + l31;                    // B operand and C/D: this lane's hidden unit
  float* hcol = T + (mt * 32) * kActTS + bcol;       // where the lane's accumulator registers go
  bool first = true;
  float xc[16];  // the next observation chunk, loaded one chunk ahead of its use: the matrix phase covers the loads' latency
  if ((int)blockIdx.x < ntiles) load_x((int)blockIdx.x, 0, xc);
  for (int tile = (int)blockIdx.x; tile < ntiles; tile += (int)gridDim.x) {
    const int r0 = tile * kActRows;
    act_f16v acc;
    for (int ch = 0; ch < nchunks; ++ch) {
      const int c0 = ch * kPolH;
      act_barrier();  // the previous readers of T and Wc are done
      if (first || nchunks > 1) stage_w0(c0);
#pragma unroll
      for (int rr = 0; rr < 16; ++rr) T[(wv * 16 + rr) * kActTS + lane] = xc[rr];
      {
        const bool last = ch + 1 == nchunks;
        const int nt_tile = last ? tile + (int)gridDim.x : tile;
        if (nt_tile < ntiles) load_x(nt_tile, last ? 0 : ch + 1, xc);
      }
      act_barrier();
      if (ch == 0) acc = tile_fill(Bs[bcol]);
      const int np = (min(kPolH, D - c0) + 1) >> 1;
      acc = tile_chain(acc, arow, Wc, bcol, h, np);
    }
    first = false;
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
    // the affine output layer and the draw: lane = row, this wave the outputs ca and ca + 1 (a wave whose outputs lie beyond A -- waves
    // 2 and 3 of a four-wide head -- goes straight to the next tile's first barrier)
    const int ca = 2 * wv;
    if (ca < A) {
      float m0 = Bs[2 * kPolH + ca], m1 = Bs[2 * kPolH + ca + 1];
      tile_out_pair(WOs, T + lane * kActTS, ca, m0, m1);
      const int g = r0 + lane;
      float a0 = m0, a1 = m1;
      if (Q.log_std != nullptr) {
        // one Philox call per row, stream 4: normal c of normal8's eight for output c (policy_mlp.hpp: policy_action). Normals 2 w and
        // 2 w + 1 are the Box-Muller pair of the call's word w: this wave evaluates that pair only
        const u32x4 r = philox4x32(K.seed_lo, K.seed_hi, (uint32_t)(K.lane0 + (uint64_t)g), K.step, 0u, 4u);
        float e0, e1;
        bm16(wv == 0 ? r.a : wv == 1 ? r.b : wv == 2 ? r.c : r.d, e0, e1);
        a0 = fmaf(Bs[2 * kPolH + kActMaxA + ca], e0, m0);
        a1 = fmaf(Bs[2 * kPolH + kActMaxA + ca + 1], e1, m1);
      }
      if (g < n) {
        const size_t o = (size_t)g * A;
        K.actions_out[o + ca] = a0;
        if (Q.mean_out != nullptr) Q.mean_out[o + ca] = m0;
        if (ca + 1 < A) {
          K.actions_out[o + ca + 1] = a1;
          if (Q.mean_out != nullptr) Q.mean_out[o + ca + 1] = m1;
        }
      }
    }
  }
}

}  // namespace pf
