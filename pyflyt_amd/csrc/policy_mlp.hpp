// pf_rollout_policy's MLP: one policy evaluation per lane between two env steps, inside the rollout launch (quadx_fast.hpp, ROLL == 3).
//
// How it is laid out for one wavefront lane per env:
//   * the weights are wave-uniform. A lone wave per SIMD cannot afford them in LDS: the rollout instantiations already hold 21 KB
//     of LDS per wave, four waves share a CU's 160 KB, and a 21 -> 64 -> 64 -> 4 network is 23 KB more -- the fourth wave would not
//     fit. They come through the SCALAR cache instead (s_load_dwordx16, sixteen weights per load; the source asks for each
//     load one ahead of its use, the compiler emits them two at a time per half input: see pol_layer64) and enter the multiply-adds as scalar operands: acc[j] = fma(s_w[j], v_x, acc[j]), no vector register and no
//     LDS traffic per weight. (A packed v_pk_fma_f32 takes ONE 64-bit scalar operand for both halves, so two different scalar
//     weights cannot feed one packed op: the price of this layout is one issue slot per multiply-add instead of one per two.)
//   * pf_rollout_policy first runs policy_pack_kernel: the caller's torch.nn.Linear tensors ([out][in], any hidden width up to 64)
//     -> one block the context owns, input-major ([in][out], so that a load serves sixteen accumulators), hidden widths padded to
//     64 with zero weights and zero biases (a padded unit is act(0) = 0 and adds exact zeros downstream), exp(log_std) evaluated
//     once. The caller's tensors are read at every call -- an optimiser step in place is seen -- and the env launch itself has no
//     vector-memory load in its loop: the scalar loads count in lgkmcnt, not in the vmcnt the observation stores sit in.
//   * the lane's input is its own observation row in the LDS tile (written by the step that has just ended; obs0 staged there
//     once in the prologue); hidden activations go through a [64][64 lanes] LDS block, a lane reading and writing its own column
//     only (conflict-free, no cross-lane dependency: no wave barrier inside the evaluation).
//   * summation order, fixed: acc = bias, then the inputs in ascending index, one fmaf each, float32. It does not depend on the
//     launch shape or on where in a launch the step falls: splitting a rollout leaves every bit as it was.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../../include/pyflyt_amd.h"
#include "uav_device.hpp"
#include "uav_vehicles.hpp"  // lds_fptr

namespace pf {

constexpr int kPolH = PF_POLICY_MAX_HIDDEN;
constexpr int kPolMaxIn = 40;  // rows of the first layer's block (>= the widest observation of the supported tasks, 37)
constexpr int kPolAct = 4;     // action width
static_assert(kPolH == 64, "the layer routines are written for 64 accumulators: four scalar loads of sixteen weights");
// the packed block, in floats
constexpr int kPolW0 = 0;                          // [kPolMaxIn][64]
constexpr int kPolB0 = kPolW0 + kPolMaxIn * kPolH;  // [64]
constexpr int kPolW1 = kPolB0 + kPolH;             // [64][64]
constexpr int kPolB1 = kPolW1 + kPolH * kPolH;     // [64]
constexpr int kPolWO = kPolB1 + kPolH;             // [64][4]
constexpr int kPolBO = kPolWO + kPolH * kPolAct;   // [4]
constexpr int kPolStd = kPolBO + kPolAct;          // [4] exp(log_std), or 0
constexpr int kPolWords = kPolStd + kPolAct + 16;  // (+ one load's worth: the layer routines request one load ahead)

// What the env kernel gets (by value: scalar registers)
struct PolicyK {
  const float* packed;  // the context's packed block
  const float* obs0;
  float* mean_out;
  int n_layers, activation, has_std;
};

__global__ void __launch_bounds__(256) policy_pack_kernel(const pf_policy Q, const int D, float* __restrict__ dst) {
  const int t = (int)threadIdx.x;
  const int w0 = Q.width[0], w1 = Q.width[1];
  const bool three = Q.n_layers == 3;
  const int hl = three ? w1 : w0;  // the width the output layer reads
  const float* wo = Q.w[three ? 2 : 1];
  const float* bo = Q.b[three ? 2 : 1];
  for (int idx = t; idx < kPolMaxIn * kPolH; idx += 256) {
    const int i = idx / kPolH, j = idx % kPolH;
    dst[kPolW0 + idx] = (i < D && j < w0) ? Q.w[0][(size_t)j * D + i] : 0.0f;
  }
  for (int idx = t; idx < kPolH * kPolH; idx += 256) {
    const int i = idx / kPolH, j = idx % kPolH;
    dst[kPolW1 + idx] = (three && i < w0 && j < w1) ? Q.w[1][(size_t)j * w0 + i] : 0.0f;
  }
  for (int idx = t; idx < kPolH * kPolAct; idx += 256) {
    const int i = idx / kPolAct, c = idx % kPolAct;
    dst[kPolWO + idx] = i < hl ? wo[(size_t)c * hl + i] : 0.0f;
  }
  if (t < kPolH) {
    dst[kPolB0 + t] = t < w0 ? Q.b[0][t] : 0.0f;
    dst[kPolB1 + t] = (three && t < w1) ? Q.b[1][t] : 0.0f;
  }
  if (t < kPolAct) {
    dst[kPolBO + t] = bo[t];
    dst[kPolStd + t] = Q.log_std ? expf(Q.log_std[t]) : 0.0f;
  }
  if (t < 16) dst[kPolStd + kPolAct + t] = 0.0f;
}

typedef float pol_f16v __attribute__((ext_vector_type(16)));
typedef const float __attribute__((address_space(4)))* pol_cptr;
typedef const pol_f16v __attribute__((address_space(4)))* pol_c16ptr;
PF_DEV pol_cptr pol_uniform(const float* p) {  // (uav_vehicles.hpp: uniform_params)
  const uintptr_t a = reinterpret_cast<uintptr_t>(p);
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)a), hi = __builtin_amdgcn_readfirstlane((uint32_t)(a >> 32));
  return (pol_cptr)(((uintptr_t)hi << 32) | (uintptr_t)lo);
}

// tanh in float32: an odd polynomial below 0.25 (truncation 2e-9 relative), 1 - 2 / (exp(2|x|) + 1) above (v_exp_f32 and v_rcp_f32,
// one ulp each; the subtraction from 1 halves their relative errors or better from |x| = 0.25 on). Absolute error below 2e-7.
PF_DEV float pol_tanh(const float x) {
  const float ax = __builtin_fabsf(x);
  const float x2 = x * x;
  const float p = fmaf(x2, fmaf(x2, fmaf(x2, fmaf(x2, 0.021869488f, -0.053968254f), 0.13333334f), -0.33333334f), 1.0f);
  const float e = __builtin_amdgcn_exp2f(__builtin_fminf(ax, 20.0f) * 2.8853900817779268f);  // exp(2|x|)
  const float big = fmaf(-2.0f, __builtin_amdgcn_rcpf(e + 1.0f), 1.0f);
  return ax < 0.25f ? x * p : __builtin_copysignf(big, x);
}

// acc[64] = bias + W x: x_i = in[i * stride] (LDS), the layer's block input-major, sixteen weights per scalar load. The source requests
// each load one ahead of the multiply-adds that use it (the last request of a layer reads the first words of what follows it in the
// block). WHAT THE COMPILER EMITS is not that pipeline: per input, two s_load_dwordx16 and the ds_read at the loop head, s_waitcnt
// lgkmcnt(0), 32 v_fmac, and the other two loads issued between them, waited for before the last 32 -- the first pair's latency of
// every input is exposed, the second pair's is covered by 16-32 multiply-adds. Scalar loads return out of order, so any use needs
// lgkmcnt(0); a real double buffer needs the loads of input i + 1 in flight across the back edge, which this source shape does not get.
PF_DEV void pol_layer64(const pol_cptr Wt, const pol_cptr bias, const lds_fptr in, const int stride, const int n_in, float (&acc)[kPolH]) {
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const pol_f16v bq = reinterpret_cast<pol_c16ptr>(bias)[q];
#pragma unroll
    for (int t = 0; t < 16; ++t) acc[16 * q + t] = bq[t];
  }
  pol_c16ptr w = reinterpret_cast<pol_c16ptr>(Wt);
  pol_f16v cur = w[0];
#pragma nounroll
  for (int i = 0; i < n_in; ++i) {
    const float x = in[i * stride];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const pol_f16v nxt = w[4 * i + q + 1];
#pragma unroll
      for (int t = 0; t < 16; ++t) acc[16 * q + t] = fmaf(cur[t], x, acc[16 * q + t]);
      cur = nxt;
    }
  }
}

PF_DEV void pol_activate_store(const int activation, float (&acc)[kPolH], const lds_fptr hcol) {
  if (activation == PF_ACT_RELU) {
#pragma unroll
    for (int j = 0; j < kPolH; ++j) hcol[j * 64] = __builtin_fmaxf(acc[j], 0.0f);
  } else {
#pragma unroll
    for (int j = 0; j < kPolH; ++j) hcol[j * 64] = pol_tanh(acc[j]);
  }
}

// the affine output layer: four inputs x four outputs per scalar load
PF_DEV float4 pol_output(const pol_cptr Wt, const pol_cptr bias, const lds_fptr hcol) {
  float o0 = bias[0], o1 = bias[1], o2 = bias[2], o3 = bias[3];
  pol_c16ptr w = reinterpret_cast<pol_c16ptr>(Wt);
  pol_f16v cur = w[0];
#pragma nounroll
  for (int g = 0; g < kPolH / 4; ++g) {
    const pol_f16v nxt = w[g + 1];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float x = hcol[(4 * g + r) * 64];
      o0 = fmaf(cur[4 * r + 0], x, o0); o1 = fmaf(cur[4 * r + 1], x, o1);
      o2 = fmaf(cur[4 * r + 2], x, o2); o3 = fmaf(cur[4 * r + 3], x, o3);
    }
    cur = nxt;
  }
  return float4{o0, o1, o2, o3};
}

// The policy's mean for this lane: `row` its observation (D floats, LDS), `hcol` its column of the [64][64] activation block.
PF_DEV float4 policy_mean(const PolicyK& PK, const pol_cptr P, const lds_fptr row, const int D, const lds_fptr hcol) {
  float acc[kPolH];
  pol_layer64(P + kPolW0, P + kPolB0, row, 1, D, acc);
  pol_activate_store(PK.activation, acc, hcol);
  if (PK.n_layers == 3) {
    pol_layer64(P + kPolW1, P + kPolB1, hcol, 64, kPolH, acc);
    pol_activate_store(PK.activation, acc, hcol);
  }
  return pol_output(P + kPolWO, P + kPolBO, hcol);
}

}  // namespace pf
