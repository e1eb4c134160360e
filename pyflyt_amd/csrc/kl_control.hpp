// pf_kl_control: what a PPO recipe decides from the measured KL, on the device (include/pyflyt_amd.h states the semantics): whether
// the optimiser's next step is taken (the gate pf_adam_step_gated reads) and, with `adapt`, the new learning rate in *lr_dev. One
// launch of one thread: two comparisons and at most one float32 multiplication or division. It reads `stats` behind the loss's
// finish kernel on the same stream and writes three small blocks; nothing here waits for the host.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/pyflyt_amd.h"

namespace pf {

struct KlControlK {
  const double* stats;
  float target_kl, stop_factor;
  int32_t adapt;
  float lr_factor, lr_low, lr_high, lr_min, lr_max;
  float* lr_dev;
  uint32_t* gate;
  double* state;
};

__global__ void __launch_bounds__(64) kl_control_kernel(const KlControlK K) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const double kl = K.stats[5], target = (double)K.target_kl;
  const bool open = kl <= (double)K.stop_factor * target;  // (false for a NaN)
  float lr = K.lr_dev ? *K.lr_dev : 0.0f;
  if (K.adapt != 0) {
    const bool cut = kl > (double)K.lr_high * target, raise = kl < (double)K.lr_low * target;  // (both false for a NaN)
    const float down = fmaxf(lr / K.lr_factor, K.lr_min), up = fminf(lr * K.lr_factor, K.lr_max);
    lr = cut ? down : raise ? up : lr;
    *K.lr_dev = lr;
  }
  *K.gate = open ? 1u : 0u;
  const double closed = K.state[3];
  K.state[0] = kl;
  K.state[1] = (double)lr;
  K.state[2] = open ? 1.0 : 0.0;
  K.state[3] = open ? closed : closed + 1.0;
}

}  // namespace pf
