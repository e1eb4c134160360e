// aviary_kernels.hpp -- the Aviary-level kernels (pf_aviary_*, pf_body_tick), the settled spawn template of the env kernels'
// lane-independent resets, and pf_sample_actions' kernel. One lane per drone, one wavefront per workgroup (env_generic.hpp: kWave).
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>
#include <cstdint>

#include "../../include/pyflyt_amd.h"
#include "uav_device.hpp"
#include "uav_vehicles.hpp"
#include "shared_world.hpp"
#include "env_generic.hpp"

namespace pf {

// Aviary-level kernels (where bodies land and stay landed): 30 KB of LDS for the contact solve -- every lane of a wave of
// quadrotors (the incident face's 4 vertices + the sentinel, 24 floats each) in one round, six worst-case airframes (48
// vertices) side by side
constexpr int kAviaryContactFloats = 64 * 5 * kContactWords;

// Settled spawn state for contexts whose settle phase is lane-independent (see env_kernel).
template <class VEH>
__global__ void settle_template_kernel(const pf_params P, float4* tmpl, const pf_params* __restrict__ Pdev) {
  __shared__ __attribute__((aligned(16))) float ktab[VEH::TABLE_FLOATS];
  __shared__ __attribute__((aligned(16))) float cws[kAviaryContactFloats];
  VEH V;
  bind_vehicle(V, P, Pdev, ktab, cws, kAviaryContactFloats);
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  float sp[6] = {0, 0, 0, 0, 0, 0};
  V.reset(P, nullptr, sp);
  V.set_mode(P.flight_mode, sp);
  Noise nz;
  nz.mode = PF_NOISE_OFF; nz.n = 1; nz.lane = 0; nz.k0 = nz.k1 = nz.c0 = 0; nz.nmot = 0.f; nz.cached = -1; nz.xi = nullptr;
  nz.begin_event(0u, 1u, nullptr);
  for (int s = 0; s < P.settle_steps; ++s) V.template aviary_step<kRuntimeMode>(P, sp, nz, 0);
  V.store(tmpl, 1, 0, 7, INFINITY, int4{0, 0, 0, 0});
}

// ------------------------------------------------------------------ Aviary-level kernels
// Each one: bind the vehicle to its LDS, load the lane, its own loop, store the lane, write the outputs (helpers: uav_vehicles.hpp).
template <class VEH>
__global__ void __launch_bounds__(kWave) aviary_reset_kernel(const pf_params P, const pf_buffers B, const int n,
                                                             const float* pose) {
  const int lane = blockIdx.x * kWave + threadIdx.x;
  if (lane >= n) return;
  const size_t li = lane;
  VEH V;
  bind_no_tick(V);
  float sp[8];
  V.reset(P, pose ? pose + li * 7 : nullptr, sp, B.start_vel ? B.start_vel + li * 3 : nullptr);
  V.store(reinterpret_cast<float4*>(B.state), (size_t)n, li, /*mode=*/7, INFINITY, int4{0, 0, 0, 0});
  if (B.out_state) write_out_state(V, B, li);
  if (B.out_link_pos) write_out_link_pos(V, P, B, li);
  if (B.out_aux) write_out_aux(V, B, li);
}

template <class VEH>
__global__ void __launch_bounds__(kWave) aviary_set_mode_kernel(const pf_params P, const pf_buffers B, const int n,
                                                                const int sp_dim, const int new_mode, float* sp_out) {
  const int lane = blockIdx.x * kWave + threadIdx.x;
  if (lane >= n) return;
  VEH V;
  bind_no_tick(V);
  float nd;
  int4 ints;
  // load everything (old mode 7 == all groups), re-initialise the controllers, store everything
  V.load(reinterpret_cast<const float4*>(B.state), (size_t)n, (size_t)lane, 7, nd, ints);
  V.b.rpy = euler_from_quat(V.b.q);
  float sp[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (sp_out)
    for (int k = 0; k < 8; ++k)
      if (k < sp_dim) sp[k] = sp_out[(size_t)lane * sp_dim + k];
  V.set_mode(B.modes ? B.modes[lane] : new_mode, sp);
  V.store(reinterpret_cast<float4*>(B.state), (size_t)n, (size_t)lane, 7, nd, ints);
  if (sp_out)
    for (int k = 0; k < 8; ++k)
      if (k < sp_dim) sp_out[(size_t)lane * sp_dim + k] = sp[k];
  (void)P;
}

template <class VEH>
__global__ void __launch_bounds__(kWave) aviary_step_kernel(const pf_params P, const pf_buffers B, const int n,
                                                            const uint64_t lane0, const int n_steps,
                                                            const pf_params* __restrict__ Pdev) {
  __shared__ __attribute__((aligned(16))) float ktab[VEH::TABLE_FLOATS];
  __shared__ __attribute__((aligned(16))) float cws[kAviaryContactFloats];  // the contact solver's LDS regions (uav_vehicles.hpp)
  VEH V;
  bind_vehicle(V, P, Pdev, ktab, cws, kAviaryContactFloats);
  const int lane = blockIdx.x * kWave + threadIdx.x;
  if (lane >= n) return;
  const size_t li = lane, N = n;
  int mode;
  float nd, sp[8];
  int4 ints;
  uint32_t rng_ctr;
  Noise nz;
  load_lane(V, P, B, n, li, lane0, mode, nd, ints, rng_ctr, nz);
  read_setpoints(P, B, li, mode, sp);
  const int ratio = lane_ctrl_ratio(B, li, 0);
  const bool armed = lane_armed(B, li);
  bool contact = false;
  for (int s = 0; s < n_steps; ++s) {
    nz.begin_event(rng_ctr, 0u, B.xi ? B.xi + (size_t)s * P.ticks_per_control * N : nullptr);
    if (!armed) {  // no control, no forces, no state read-back: gravity only (aviary.py:510-521 skip it, Bullet does not)
      V.b.contact_step = false;
      for (int t = 0; t < P.ticks_per_control; ++t) V.tick_unarmed(P);
    } else if (ratio > 0 || B.modes) {  // this drone's own control rate (period ratio * dt) and / or flight mode
      const int rr = ratio > 0 ? ratio : P.ticks_per_control;
      V.b.contact_step = false;
      for (int t = 0; t < P.ticks_per_control; ++t) {
        if (t % rr == 0) {
          if (t > 0) V.b.rpy = euler_from_quat_fast(V.b.q);
          V.template control<kRuntimeMode>(P, sp, ratio > 0 ? ratio * P.dt : 0.0f, B.modes ? mode : kNoModeOverride);
        }
        V.tick(P, nz.get(t));
      }
      V.b.rpy = euler_from_quat_fast(V.b.q);
    } else {
      V.template aviary_step<kRuntimeMode>(P, sp, nz, 0);
    }
    rng_ctr += 1;
    contact = V.b.contact_step;
  }
  store_lane(V, B, n, li, mode, nd, ints, rng_ctr);
  if (B.out_state && armed) write_out_state(V, B, li);
  if (B.out_aux && armed) write_out_aux(V, B, li);
  if (B.out_contact) B.out_contact[li] = contact ? 1 : 0;
}

// Aviary.step for drones that share a world (pf_params.agents_per_world = K > 1 with PF_TASK_NONE): the reference's N-drone Aviary
// is ONE Bullet world, whose drones hit each other and whose rotational-drag gate looks at every contact point in it (quadx.py:509).
// A world's K drones are adjacent lanes of one wave (K divides 64 and n: a world never straddles a wave, and a partial last wave
// holds whole worlds only). Before every physics tick the lanes exchange pose and contact bit through LDS (world_exchange: the
// drone-drone box tests, the drag gate from the previous tick's world-wide contact bit), then tick<true> runs the pair stage with
// its impulses (contact_response) between the velocity update and the ground solve. Every lane of a world runs every tick -- a
// disarmed drone with zero force and torque, as PyBullet still integrates it -- so that the wave-wide exchange and pair stage see
// all of them. With no contact anywhere in a world the tick does the solo kernel's arithmetic (the pair stage's shift is +0).
// out_contact: the floor part of the last Aviary step's contacts; out_contact_peers: bit j = touched drone j of the world.
template <class VEH>
__global__ void __launch_bounds__(kWave) aviary_world_step_kernel(const pf_params P, const pf_buffers B, const int n,
                                                                  const uint64_t lane0, const int n_steps,
                                                                  const pf_params* __restrict__ Pdev) {
  __shared__ __attribute__((aligned(16))) float ktab[VEH::TABLE_FLOATS];
  __shared__ __attribute__((aligned(16))) float cws[kAviaryContactFloats];  // the contact solvers' LDS regions (floor and pair stage)
  __shared__ float wpose[kWave * 8];                                         // each lane's pose and contact bit, once per tick
  __shared__ float wvel[kWave * kPairVelStride];                             // ... and its new velocities for the pair stage
  VEH V;
  bind_vehicle(V, P, Pdev, ktab, cws, kAviaryContactFloats);
  const int tid = threadIdx.x;
  const int lane = blockIdx.x * kWave + tid;
  if (lane >= n) return;  // (whole worlds: the lanes that stay are every lane of their worlds)
  const size_t li = lane, N = n;
  const int K = P.agents_per_world;
  V.b.wpose_ = wpose; V.b.wvel_ = wvel; V.b.wtid = tid; V.b.wA = K;
  int mode;
  float nd, sp[8];
  int4 ints;
  uint32_t rng_ctr;
  Noise nz;
  load_lane(V, P, B, n, li, lane0, mode, nd, ints, rng_ctr, nz);
  read_setpoints(P, B, li, mode, sp);
  const int ratio = lane_ctrl_ratio(B, li, 0);
  const int rr = ratio > 0 ? ratio : P.ticks_per_control;  // this drone's own control rate, or once per Aviary step
  const bool armed = lane_armed(B, li);
  // The QuadX controller reads its constants from the device copy of the parameter block: taken from the kernel argument, the
  // compiler keeps them in registers across the tick loop, whose pair-stage call leaves half the register file to the values that
  // live across it, and the instantiation spilled to scratch memory. The copy's flight_mode is the one of pf_ctx_create: the lane's
  // mode is passed to control() explicitly. (Fixedwing: stateless mixing that reads flight_mode itself, and no pressure to relieve.)
  const pf_params& Pc = std::is_same<VEH, QuadX>::value ? *Pdev : P;
  bool floor = false;
  uint32_t peers = 0u;
  for (int s = 0; s < n_steps; ++s) {
    nz.begin_event(rng_ctr, 0u, B.xi ? B.xi + (size_t)s * P.ticks_per_control * N : nullptr);
    floor = false;  // (aviary.py:507: the contact array of the last Aviary step)
    peers = 0u;
    for (int t = 0; t < P.ticks_per_control; ++t) {
      if (armed && t % rr == 0) {
        if (t > 0) V.b.rpy = euler_from_quat_fast(V.b.q);
        V.template control<kRuntimeMode>(Pc, sp, ratio > 0 ? ratio * P.dt : 0.0f, mode);
      }
      uint32_t bits;
      world_exchange(V.b, wpose, tid, K, P.bound_radius, Pdev, false, nullptr, false, &bits);  // (shared_world.hpp)
      v3 F{0.0f, 0.0f, 0.0f}, tau{0.0f, 0.0f, 0.0f};
      if (armed) V.forces(P, nz.get(t), nullptr, F, tau);  // (a disarmed drone: no control, no forces -- gravity only)
      V.b.template tick<true>(P, F, tau);                   // (every lane of the world together: the pair stage is wave-wide)
      floor = floor || V.b.floor_now;
      peers |= bits;
    }
    V.b.peer_contact = false;
    if (armed) V.b.rpy = euler_from_quat_fast(V.b.q);
    rng_ctr += 1;
  }
  store_lane(V, B, n, li, mode, nd, ints, rng_ctr);
  if (B.out_state && armed) write_out_state(V, B, li);
  if (B.out_aux && armed) write_out_aux(V, B, li);
  if (B.out_contact) B.out_contact[li] = floor ? 1 : 0;
  if (B.out_contact_peers) B.out_contact_peers[li] = (uint8_t)peers;
}

// One physics tick of Aviary.step (pf_aviary_tick): the wind-field protocol needs the host between
// ticks. QuadX carries the motor commands of the step's control tick in state group 12.
template <class VEH>
__global__ void __launch_bounds__(kWave) aviary_tick_kernel(const pf_params P, const pf_buffers B, const int n,
                                                            const uint64_t lane0, const int tick_index,
                                                            const pf_params* __restrict__ Pdev) {
  __shared__ __attribute__((aligned(16))) float ktab[VEH::TABLE_FLOATS];
  __shared__ __attribute__((aligned(16))) float cws[kAviaryContactFloats];  // the contact solver's LDS regions (uav_vehicles.hpp)
  VEH V;
  bind_vehicle(V, P, Pdev, ktab, cws, kAviaryContactFloats);
  const int lane = blockIdx.x * kWave + threadIdx.x;
  if (lane >= n) return;
  const size_t li = lane, N = n;
  constexpr bool kQuad = VEH::AUX == 4;
  constexpr int kCmdGroup = 12;
  float4* S = reinterpret_cast<float4*>(B.state);
  int mode;
  float nd, sp[8];
  int4 ints;
  uint32_t rng_ctr;
  Noise nz;
  load_lane(V, P, B, n, li, lane0, mode, nd, ints, rng_ctr, nz);
  nz.begin_event(rng_ctr, 0u, B.xi);
  read_setpoints(P, B, li, mode, sp);
  const int ratio = lane_ctrl_ratio(B, li, P.ticks_per_control);
  const bool armed = lane_armed(B, li);
  if (!armed) {
    V.tick_unarmed(P);
  } else {
  if (tick_index % ratio == 0 || !kQuad) {
    V.template control<kRuntimeMode>(P, sp, B.ctrl_ratio ? ratio * P.dt : 0.0f, B.modes ? mode : kNoModeOverride);  // Fixedwing: stateless mixing, recomputed every tick
  } else {
    const float4 c = S[(size_t)kCmdGroup * N + li];
    V.set_cmd(c);
  }
  const float xi = nz.get(P.noise_mode == PF_NOISE_INJECT ? 0 : tick_index);
  V.tick(P, xi, B.wind ? B.wind + li * (size_t)(VEH::WIND_LINKS * 3) : nullptr);
  }
  V.b.rpy = euler_from_quat_fast(V.b.q);
  if (tick_index == P.ticks_per_control - 1) rng_ctr += 1;
  store_lane(V, B, n, li, mode, nd, ints, rng_ctr);
  if (kQuad) S[(size_t)kCmdGroup * N + li] = V.get_cmd();
  if (B.out_state && armed) write_out_state(V, B, li);
  if (B.out_aux && armed) write_out_aux(V, B, li);
  if (B.out_contact) B.out_contact[li] = V.b.contact_now ? 1 : 0;
  if (B.out_link_pos) write_out_link_pos(V, P, B, li);
}

// applyExternalForce / applyExternalTorque on the base link (LINK_FRAME) + stepSimulation, n_ticks times
// (pf_body_tick): the free-body tick by itself, for the integrator's known-answer tests.
template <class VEH>
__global__ void __launch_bounds__(kWave) body_tick_kernel(const pf_params P, const pf_buffers B, const int n, const int n_ticks,
                                                          const pf_params* __restrict__ Pdev) {
  const int lane = blockIdx.x * kWave + threadIdx.x;
  if (lane >= n) return;
  const size_t li = lane;
  __shared__ __attribute__((aligned(16))) float cws[kAviaryContactFloats];
  VEH V;
  bind_contact(V, P, Pdev, cws, kAviaryContactFloats);  // (no constant table: the vehicle's forces are not run)
  float nd;
  int4 ints;
  V.load(reinterpret_cast<const float4*>(B.state), (size_t)n, li, 7, nd, ints);
  const float* wr = B.wrench + li * 6;
  const v3 F{wr[0], wr[1], wr[2]}, tau{wr[3], wr[4], wr[5]};
  bool contact = false;
  for (int t = 0; t < n_ticks; ++t) {
    V.b.tick(P, F, tau);
    contact |= V.b.contact_now;
  }
  V.b.rpy = euler_from_quat_fast(V.b.q);
  store_lane(V, B, n, li, 7, nd, ints, (uint32_t)ints.z);
  if (B.out_state) write_out_state(V, B, li);
  if (B.out_contact) B.out_contact[li] = contact ? 1 : 0;
}

__global__ void __launch_bounds__(256) sample_actions_kernel(const pf_params P, float* actions, const int n,
                                                             const uint64_t lane0, const uint32_t step_index) {
  const int lane = blockIdx.x * 256 + threadIdx.x;
  if (lane >= n) return;
  reinterpret_cast<float4*>(actions)[lane] =
      sampled_action4<true>((uint32_t)P.seed, (uint32_t)(P.seed >> 32), (uint32_t)(lane0 + lane), step_index, P.action_low, P.action_high);
}

}  // namespace pf
