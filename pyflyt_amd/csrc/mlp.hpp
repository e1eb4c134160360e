// pf_mlp_forward / pf_mlp_backward: the networks of a PPO epoch without a GEMM library -- rows in, rows out, and from the
// output-gradients of those rows the gradients of every weight and bias (include/pyflyt_amd.h states the semantics).
//
// The forward IS policy_act_kernel (policy_act.hpp), launched with the draw off, the caller's rows as obs0 and A = out_dim: no second
// forward exists. The backward is two kernels:
//
//   mlp_backward_kernel  a workgroup of four waves strides over 64-row tiles with policy_act_kernel's tile and operand layouts. Per tile:
//                          1. the forward again, by the chain function policy_act_kernel runs (mlp_tile.hpp: tile_chain): X -> TX, h0 -> TH0, h1 -> TH1; nothing was saved;
//                          2. the rows of grad_out -> G, the rows past `rows` as exact zeros (x is clamped, the gradient is masked);
//                          3. grad_w[last] += G^T h_last   (the rows are the contraction: wave (mt, nt) takes the rows 32 mt .. 32 mt + 31);
//                          4. delta_last = (G WO) * act'(h_last), at most eight fmaf per element, written over h_last IN PLACE: an
//                             element of delta needs the element of h under it and nothing else of that tile;
//                          5. grad_w[1] += delta1^T h0; delta0 = (delta1 W1) * act'(h0) over h0 in place -- W1 is read from the block the
//                             forward staged, [k][(unit + k) & 63], along the other index: both directions are conflict-free;
//                          6. grad_w[0] += delta0^T X, one 32x32 accumulator per 64-column chunk of X.
//                        Every product of a tile starts from a zero accumulator and is then added to the workgroup's running sum in
//                        registers: a sum's chain is 64 rows long, not (rows / grid) long. The bias gradients are column sums of the
//                        deltas, taken from the accumulator registers as they pass. At the end the workgroup writes ONE block of
//                        partial sums, laid out like the parameters (w0, b0, w1, b1, ...), to the caller's workspace.
//   mlp_reduce_kernel    one thread per parameter: the workgroups' partials in ascending workgroup order, in double; float32 out.
//
// The grid is min(tiles, kMlpMaxGrid): a function of `rows` alone. No atomics. LDS: both chunks of the first layer, the second
// layer, X (two chunks), h0, h1 and G are 118 KB of the CU's 160 KB, declared statically (gfx950 admits it): one workgroup per CU.
// The tile constants, the barrier, the accumulator's fill, row map and activation store and the forward's matrix chain are mlp_tile.hpp's,
// shared with policy_act_kernel; the staging and the row loads are this file's own copies (profiles/mlp_tile/nothing_moved.txt: why).
//
// mlp_backward_kernel is a template over its argument block. With MlpK it is pf_mlp_backward's kernel, instruction for instruction what
// it was as a plain function (profiles/ppo_grad/nothing_moved.txt). With a block derived from MlpK that has a head (ppo_grad.hpp:
// PpoGradK), step 2 is replaced: the head loads its own row data a tile ahead, and once h_last stands in LDS it computes the output
// layer and from it the tile's rows of G. Steps 1 and 3 - 6, the running sums and the block of partials are this one text either way.
// A head with kIndexed (ppo_grad.hpp: PpoGradRowsK) names its rows by an index list: slot j of the n is row row_index[j] of x. Every
// wave holds a tile's 64 indices, lane = slot, in ONE register, loaded TWO tiles ahead: when the loads of the next tile's rows are
// issued at the top of a tile, their addresses come from a register that was filled a whole tile earlier, so no dependent load
// stands on a tile's path. A row number of load_x is uniform over the wave: v_readlane of that register.
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

constexpr int kMlpMaxGrid = 256;       // one workgroup per CU of an MI355X (the LDS admits no second); more rows are strided over
constexpr int kMlpGS = kActMaxA + 1;   // the row stride of the grad_out tile
constexpr int kMlpTile = kActRows * kActTS;

struct MlpNone {};
struct MlpK {
  typedef MlpNone Rows;
  typedef MlpNone Sums;
  static constexpr int kHead = 0;  // the rows of G are the caller's grad_out (ppo_grad.hpp: the heads that compute them in the tile)
  static constexpr bool kIndexed = false;  // a tile's rows are the rows tile * 64 ... of x (ppo_grad.hpp: the heads that take them through an index list)
  pf_mlp Q;
  const float* x;
  const float* grad_out;
  float* partials;  // [grid][mlp_param_count]
  int n;
};
struct MlpOutK {
  float* p[6];      // grad_w[0], grad_b[0], grad_w[1], grad_b[1], grad_w[2], grad_b[2]
  int end[6];       // where each ends in a block of partials
};

// parameters of the network = floats of one block of partials; seg_end (may be null): where each of w0, b0, w1, b1, w2, b2 ends
inline __host__ __device__ int mlp_param_count(const pf_mlp& q, int* seg_end) {
  int off = 0;
  for (int l = 0; l < 3; ++l) {
    if (l < q.n_layers) {
      const int n_in = l == 0 ? q.in_dim : q.width[l - 1];
      const int n_out = l + 1 == q.n_layers ? q.out_dim : q.width[l];
      off += n_out * n_in;
      if (seg_end) seg_end[2 * l] = off;
      off += n_out;
      if (seg_end) seg_end[2 * l + 1] = off;
    } else if (seg_end) {
      seg_end[2 * l] = seg_end[2 * l + 1] = off;
    }
  }
  return off;
}
inline int mlp_grid(int64_t rows) {
  const int64_t tiles = (rows + kActRows - 1) / kActRows;
  return (int)(tiles < (int64_t)kMlpMaxGrid ? tiles : (int64_t)kMlpMaxGrid);
}

// delta = pre * act'(h) over the h of this lane's sixteen accumulator positions, in place; returns the sum of the sixteen
PF_DEV float mlp_delta_store(const int activation, const act_f16v& pre, float* hcol, const int h) {
  float cs = 0.0f;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    float* p = hcol + tile_row(r, h) * kActTS;
    const float hv = *p;
    const float d = activation == PF_ACT_RELU ? (hv > 0.0f ? pre[r] : 0.0f) : fmaf(-hv, hv, 1.0f) * pre[r];
    *p = d;
    cs = cs + d;
  }
  return cs;
}

// a^T b over the 64 rows of two tiles: this wave's 32 x 32 block, columns ca .. ca + 31 of `a` by cb .. cb + 31 of `b`, from zero
PF_DEV act_f16v mlp_outer(const float* a, const float* b, const int ca, const int cb, const int l31, const int h) {
  act_f16v acc = tile_fill(0.0f);
  for (int kk = 0; kk < kActRows / 2; ++kk) {
    const int row = 2 * kk + h;
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[row * kActTS + ca + l31], b[row * kActTS + cb + l31], acc, 0, 0, 0);
  }
  return acc;
}

// KT: MlpK, or a block derived from it whose head makes the tile's rows of G itself (step 2'; ppo_grad.hpp: PpoGradK)
template <class KT>
__global__ void __launch_bounds__(256) mlp_backward_kernel(const KT K) {
  constexpr int HEAD = KT::kHead;
  __shared__ float W0s[2 * kPolH * kPolH];  // the first layer, two chunks of 64 inputs: [k][(unit + k) & 63]
  __shared__ float W1s[kPolH * kPolH];      // the second layer, likewise
  __shared__ float WOs[kPolH * kActMaxA];   // the output layer [i][c]
  __shared__ float Bs[2 * kPolH];           // b0, b1
  __shared__ float TX[2 * kMlpTile];        // the rows of x, two chunks of 64 columns; at the very end the scratch of the last sums
  __shared__ float TH0[kMlpTile];           // h0, then delta0
  __shared__ float TH1[kMlpTile];           // h1, then delta1
  __shared__ float G[kActRows * kMlpGS];    // the rows of grad_out
  float* HS = nullptr;                      // a head's own LDS: its rows' data and the output bias
  if constexpr (HEAD != 0) {
    __shared__ float head_lds[KT::kLdsFloats];
    HS = head_lds;
  }
  const int t = (int)threadIdx.x, lane = t & 63, wv = t >> 6;
  const int l31 = lane & 31, h = lane >> 5, mt = wv & 1, nt = wv >> 1;
  const pf_mlp& Q = K.Q;
  const int D = Q.in_dim, A = Q.out_dim, n = K.n;
  const bool three = Q.n_layers == 3;
  const int w0 = Q.width[0], w1 = three ? Q.width[1] : 0;
  const int hl = three ? w1 : w0;  // the width the output layer reads
  const float* wo = Q.w[three ? 2 : 1];
  const int nchunks = (D + kPolH - 1) / kPolH;
  const int ntiles = (n + kActRows - 1) / kActRows;

  // (a copy of policy_act_kernel's staging, to be kept in step with it: thread t reads (unit j = 4 i + wv, input k = lane), sixteen loads in flight)
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
  // a chunk of the tile's rows of x: wave wv rows 16 wv .. 16 wv + 15, a lane per column; columns from D on are zero. Rows past n
  // re-read row n - 1 (finite where the caller's rows are): their delta is zero, so what they hold is multiplied by zero
  auto load_x = [&](const int tile, const int ch, float (&x)[16]) {
    const int c = ch * kPolH + lane;
#pragma unroll
    for (int rr = 0; rr < 16; ++rr) {
      const int g = min(tile * kActRows + wv * 16 + rr, n - 1);
      x[rr] = (ch < nchunks && c < D) ? K.x[(size_t)g * D + c] : 0.0f;
    }
  };
  // the same through the index list: `s` = this wave's copy of the tile's 64 row numbers, lane = slot (slots past n repeat slot n - 1's),
  // -1 where the list's number lay outside the batch: row 0 is loaded in its place and zeros are chosen
  auto load_x_rows = [&](const int s, const int ch, float (&x)[16]) {
    const int c = ch * kPolH + lane, wu = __builtin_amdgcn_readfirstlane(wv);
#pragma unroll
    for (int rr = 0; rr < 16; ++rr) {
      const int g = __builtin_amdgcn_readlane(s, wu * 16 + rr);
      const float v = (ch < nchunks && c < D) ? K.x[(size_t)max(g, 0) * D + c] : 0.0f;
      x[rr] = g < 0 ? 0.0f : v;
    }
  };
  // the tile's rows of grad_out: two elements per thread; rows past n and columns past A are exact zeros, never read
  auto load_g = [&](const int tile, float (&g)[2]) {
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int idx = t + 256 * u, row = idx / kActMaxA, c = idx % kActMaxA;
      const int gr = tile * kActRows + row;
      g[u] = (gr < n && c < A) ? K.grad_out[(size_t)gr * A + c] : 0.0f;
    }
  };
  stage_block(W0s, Q.w[0], D, 0, D, w0, true);
  stage_block(W0s + kPolH * kPolH, Q.w[0], D, kPolH, D, w0, nchunks > 1);
  stage_block(W1s, Q.w[1], w0, 0, w0, w1, three);
  for (int idx = t; idx < kPolH * kActMaxA; idx += 256) {
    const int i = idx / kActMaxA, c = idx % kActMaxA;
    WOs[idx] = (i < hl && c < A) ? wo[(size_t)c * hl + i] : 0.0f;
  }
  if (t < kPolH) {
    Bs[t] = t < w0 ? Q.b[0][t] : 0.0f;
    Bs[kPolH + t] = (three && t < w1) ? Q.b[1][t] : 0.0f;
  }
  if constexpr (HEAD != 0) K.stage_head(t, HS);

  const int arow = (mt * 32 + l31) * kActTS;     // A operand of a forward-shaped product: this lane's row of a tile
  const int bcol = nt * 32 + l31;                // B operand and C/D: this lane's unit
  const int hpos = (mt * 32) * kActTS + bcol;    // where the lane's accumulator registers sit in a tile
  float* TL = three ? TH1 : TH0;                 // the last hidden layer's tile

  // the workgroup's running sums: this wave's blocks of grad_w[0] (per chunk), grad_w[1], the output layer's (rows 32 mt .. of the
  // contraction: the two mt halves meet at the end), and this lane's share of the column sums
  act_f16v gw0[2], gw1;
  float gwo[4] = {0.0f, 0.0f, 0.0f, 0.0f}, gbh0 = 0.0f, gbh1 = 0.0f, gbo = 0.0f;
#pragma unroll
  for (int r = 0; r < 16; ++r) gw0[0][r] = gw0[1][r] = gw1[r] = 0.0f;

  float xc[2][16], gq[2];  // the next tile's rows, loaded a tile ahead of their use
  typename KT::Rows hq;    // (a head's rows likewise; its sums for `stats`)
  typename KT::Sums hsum;
  int nraw = 0;            // an indexed head: the index list's 64 numbers of the next tile, lane = slot, as loaded
  if constexpr (KT::kIndexed) {
    const int s = K.row_of(K.load_index((int)blockIdx.x, lane));  // (the one dependent load of the launch)
    if ((int)blockIdx.x + (int)gridDim.x < ntiles) nraw = K.load_index((int)blockIdx.x + (int)gridDim.x, lane);
    load_x_rows(s, 0, xc[0]);
    load_x_rows(s, 1, xc[1]);
    K.load_rows((int)blockIdx.x, t, s, hq);
  } else {
    load_x((int)blockIdx.x, 0, xc[0]);
    load_x((int)blockIdx.x, 1, xc[1]);
    if constexpr (HEAD == 0) load_g((int)blockIdx.x, gq); else K.load_rows((int)blockIdx.x, t, hq);
  }
  __syncthreads();  // the staged weights
  for (int tile = (int)blockIdx.x; tile < ntiles; tile += (int)gridDim.x) {
    act_barrier();  // the previous tile's readers of TX, TH0 and G are done
#pragma unroll
    for (int ch = 0; ch < 2; ++ch)
      if (ch < nchunks) {
#pragma unroll
        for (int rr = 0; rr < 16; ++rr) TX[ch * kMlpTile + (wv * 16 + rr) * kActTS + lane] = xc[ch][rr];
      }
    if constexpr (HEAD == 0) {
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int idx = t + 256 * u;
        G[(idx / kActMaxA) * kMlpGS + idx % kActMaxA] = gq[u];
      }
    } else {
      K.stage_rows(t, hq, HS);
    }
    if constexpr (KT::kIndexed) {
      if (tile + (int)gridDim.x < ntiles) {
        const int s = K.row_of(nraw);  // (arrived during the previous tile)
        if (tile + 2 * (int)gridDim.x < ntiles) nraw = K.load_index(tile + 2 * (int)gridDim.x, lane);
        load_x_rows(s, 0, xc[0]);
        load_x_rows(s, 1, xc[1]);
        K.load_rows(tile + (int)gridDim.x, t, s, hq);
      }
    } else if (tile + (int)gridDim.x < ntiles) {
      load_x(tile + (int)gridDim.x, 0, xc[0]);
      load_x(tile + (int)gridDim.x, 1, xc[1]);
      if constexpr (HEAD == 0) load_g(tile + (int)gridDim.x, gq); else K.load_rows(tile + (int)gridDim.x, t, hq);
    }
    act_barrier();

    // ---- the forward again: tile_fill and tile_chain, as in policy_act_kernel
    act_f16v acc;
    acc = tile_fill(Bs[bcol]);
    for (int ch = 0; ch < nchunks; ++ch) {
      const int np = (min(kPolH, D - ch * kPolH) + 1) >> 1;
      acc = tile_chain(acc, TX + ch * kMlpTile + arow, W0s + ch * kPolH * kPolH, bcol, h, np);
    }
    act_store_hidden(Q.activation, acc, TH0 + hpos, h);
    act_barrier();
    if (three) {
      acc = tile_fill(Bs[kPolH + bcol]);
      acc = tile_chain(acc, TH0 + arow, W1s, bcol, h, kPolH / 2);
      act_store_hidden(Q.activation, acc, TH1 + hpos, h);
      act_barrier();
    }
    // ---- step 2': a head computes the output layer from h_last and from it the tile's rows of G
    if constexpr (HEAD != 0) K.make_g(tile, t, TL, WOs, HS, G, hsum);

    // ---- the output layer: grad_w = G^T h_last over this wave's half of the rows, grad_b = the column sums of G
    if (32 * nt < hl) {
      acc = tile_fill(0.0f);
      for (int kk = 0; kk < 16; ++kk) {
        const int row = 32 * mt + 2 * kk + h;
        const float a = l31 < kActMaxA ? G[row * kMlpGS + l31] : 0.0f;
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, TL[row * kActTS + bcol], acc, 0, 0, 0);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) gwo[r] = gwo[r] + acc[r];  // (outputs 0 .. 7 are registers 0 .. 3 of the two lane halves)
    }
    if (t < kActRows) {  // thread t: output t & 7, rows 8 (t >> 3) .. + 7
      float s = 0.0f;
#pragma unroll
      for (int rr = 0; rr < 8; ++rr) s = s + G[((t >> 3) * 8 + rr) * kMlpGS + (t & 7)];
      gbo = gbo + s;
    }
    act_barrier();  // every read of h_last above is done: delta goes over it

    // ---- delta of the last hidden layer: (G WO) * act'(h)
    {
      float wr[kActMaxA];
#pragma unroll
      for (int c = 0; c < kActMaxA; ++c) wr[c] = WOs[bcol * kActMaxA + c];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float* g = G + (32 * mt + tile_row(r, h)) * kMlpGS;
        float d = g[0] * wr[0];
#pragma unroll
        for (int c = 1; c < kActMaxA; ++c) d = fmaf(g[c], wr[c], d);
        acc[r] = d;
      }
      const float cs = mlp_delta_store(Q.activation, acc, TL + hpos, h);
      if (three) gbh1 = gbh1 + cs; else gbh0 = gbh0 + cs;
    }
    act_barrier();

    if (three) {
      // ---- grad_w[1] += delta1^T h0; then delta0 = (delta1 W1) * act'(h0)
      if (32 * mt < w1 && 32 * nt < w0) {
        acc = mlp_outer(TH1, TH0, 32 * mt, 32 * nt, l31, h);
#pragma unroll
        for (int r = 0; r < 16; ++r) gw1[r] = gw1[r] + acc[r];
      }
      acc = tile_fill(0.0f);
      for (int kk = 0; kk < kPolH / 2; ++kk) {
        const int j = 2 * kk + h;  // W1[j][i = bcol] sits at row i of the staged block, rotated by i
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(TH1[arow + j], W1s[bcol * kPolH + ((j + bcol) & 63)], acc, 0, 0, 0);
      }
      act_barrier();  // grad_w[1]'s reads of h0 are done
      gbh0 = gbh0 + mlp_delta_store(Q.activation, acc, TH0 + hpos, h);
      act_barrier();
    }

    // ---- grad_w[0] += delta0^T X
#pragma unroll
    for (int ch = 0; ch < 2; ++ch)
      if (ch < nchunks && 32 * mt < w0 && ch * kPolH + 32 * nt < D) {
        acc = mlp_outer(TH0, TX + ch * kMlpTile, 32 * mt, 32 * nt, l31, h);
#pragma unroll
        for (int r = 0; r < 16; ++r) gw0[ch][r] = gw0[ch][r] + acc[r];
      }
  }

  // ---- one block of partial sums per workgroup, laid out like the parameters
  int end[6];
  const int P = mlp_param_count(Q, end);
  float* part = K.partials + (size_t)blockIdx.x * P;
  float* S = TX;  // scratch: [0, 512) the output layer's second half; [512, 768) and [768, 1024) the hidden column sums; [1024, 1088) the output's
  act_barrier();
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int j = 32 * mt + tile_row(r, h);
#pragma unroll
    for (int ch = 0; ch < 2; ++ch) {
      const int i = ch * kPolH + bcol;
      if (j < w0 && i < D) part[(size_t)j * D + i] = gw0[ch][r];
    }
    if (three && j < w1 && bcol < w0) part[end[1] + j * w0 + bcol] = gw1[r];
  }
  if (mt == 1) {
#pragma unroll
    for (int r = 0; r < 4; ++r) S[(r + 4 * h) * kPolH + bcol] = gwo[r];
  }
  S[512 + (2 * mt + h) * kPolH + bcol] = gbh0;  // (every lane writes: bcol covers 0 .. 63 over nt and l31, (mt, h) the four holders)
  S[768 + (2 * mt + h) * kPolH + bcol] = gbh1;
  if (t < kActRows) S[1024 + t] = gbo;
  act_barrier();
  const int ow = three ? end[3] : end[1];  // where the output layer's weights begin
  if (mt == 0) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int c = r + 4 * h;
      if (c < A && bcol < hl) part[ow + c * hl + bcol] = gwo[r] + S[c * kPolH + bcol];
    }
  }
  if (t < kPolH) {
    float s0 = S[512 + t], s1 = S[768 + t];
#pragma unroll
    for (int q = 1; q < 4; ++q) {
      s0 = s0 + S[512 + q * kPolH + t];
      s1 = s1 + S[768 + q * kPolH + t];
    }
    if (t < w0) part[end[0] + t] = s0;
    if (three && t < w1) part[end[2] + t] = s1;
  }
  if (t < A) {
    float s = S[1024 + t];
#pragma unroll
    for (int q = 1; q < 8; ++q) s = s + S[1024 + 8 * q + t];
    part[(three ? end[4] : end[2]) + t] = s;
  }
  if constexpr (HEAD != 0) K.write_sums(t, hsum);
}

// One thread per parameter: the workgroups' partials in ascending workgroup order, in double
__global__ void __launch_bounds__(256) mlp_reduce_kernel(const float* __restrict__ partials, const int n_blocks, const int P, const MlpOutK O) {
  const int e = (int)blockIdx.x * 256 + (int)threadIdx.x;
  if (e >= P) return;
  double s = 0.0;
  int g = 0;
  for (; g + 8 <= n_blocks; g += 8) {
    float v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = partials[(size_t)(g + u) * P + e];
#pragma unroll
    for (int u = 0; u < 8; ++u) s = s + (double)v[u];
  }
  for (; g < n_blocks; ++g) s = s + (double)partials[(size_t)g * P + e];
  int seg = 0, begin = 0;
#pragma unroll
  for (int q = 0; q < 5; ++q)
    if (e >= O.end[q]) {
      seg = q + 1;
      begin = O.end[q];
    }
  float* dst = seg == 0 ? O.p[0] : seg == 1 ? O.p[1] : seg == 2 ? O.p[2] : seg == 3 ? O.p[3] : seg == 4 ? O.p[4] : O.p[5];
  dst[e - begin] = (float)s;
}

}  // namespace pf
