// What policy_act_kernel (policy_act.hpp) and mlp_backward_kernel (mlp.hpp) share of the 64-row tile code: the constants, the barrier
// between phases, the 32x32 accumulator's fill, register-to-row map and activation store, the matrix chain of a layer and the fmaf
// chain of a pair of outputs -- so the h0 / h1 the backward computes again, and the means and values the fused heads of ppo_grad.hpp
// compute in the tile, come from the text the forward runs. Everything is force-inlined. The staging of the weights and
// biases and the row loads are still written per kernel: each of them, as a shared function, made pf_mlp_backward measurably slower
// (profiles/mlp_tile/nothing_moved.txt). Layouts: policy_act.hpp's top comment.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../../include/pyflyt_amd.h"
#include "uav_device.hpp"
#include "policy_mlp.hpp"  // kPolH

namespace pf {

constexpr int kActRows = 64;       // rows of a workgroup's tile
constexpr int kActTS = kPolH + 1;  // the tile's row stride in floats
constexpr int kActMaxA = 8;        // the output layer's block holds eight columns (action widths 4, 6, 7)
constexpr int kActMaxIn = 128;     // the widest observation (an eight-aircraft dogfight with six-wide actions: 123)

typedef float act_f16v __attribute__((ext_vector_type(16)));

// The workgroup barrier between the phases of a tile. Everything the phases exchange goes through LDS, so it waits for the LDS counter
// only: __syncthreads() also waits for the vector-memory counter, i.e. for the next tile's loads, issued one phase ahead on purpose.
PF_DEV void act_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// the row (of the wave's 32) that register r of the 32x32 accumulator holds in lane half h
PF_DEV int tile_row(const int r, const int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

// an accumulator that starts from a bias (or from zero)
PF_DEV act_f16v tile_fill(const float b) {
  act_f16v acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = b;
  return acc;
}

// np k-pairs of a layer's chain, k ascending: the A operand from this lane's tile row, the B operand unit bcol of the staged block W
PF_DEV act_f16v tile_chain(act_f16v acc, const float* arow, const float* W, const int bcol, const int h, const int np) {
  for (int kk = 0; kk < np; ++kk) {
    const int k = 2 * kk + h;
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(arow[k], (W + k * kPolH)[(bcol + k) & 63], acc, 0, 0, 0);
  }
  return acc;
}

// the 32x32 accumulator through the activation into the tile; trow0 is the lane's unit in the first of the wave's 32 rows
PF_DEV void act_store_hidden(const int activation, const act_f16v& acc, float* trow0, const int h) {
#pragma unroll
  for (int r = 0; r < 16; ++r) trow0[tile_row(r, h) * kActTS] = activation == PF_ACT_RELU ? __builtin_fmaxf(acc[r], 0.0f) : pol_tanh(acc[r]);
}

// the affine output layer of one row: outputs ca and ca + 1, each from its bias (m0, m1 on entry) over the 64 columns of the row's last
// hidden layer xr (zero past the layer's width), i ascending, one fmaf each; WOs is the staged [i][c] block
PF_DEV void tile_out_pair(const float* WOs, const float* xr, const int ca, float& m0, float& m1) {
#pragma unroll 8
  for (int i = 0; i < kPolH; ++i) {
    const float x = xr[i];
    m0 = fmaf(WOs[i * kActMaxA + ca], x, m0);
    m1 = fmaf(WOs[i * kActMaxA + ca + 1], x, m1);
  }
}

}  // namespace pf
