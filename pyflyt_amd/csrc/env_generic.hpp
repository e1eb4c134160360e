// env_generic.hpp -- the generic fused env kernel: every (vehicle, task, flight mode) that has no specialised kernel
// (quadx_fast.hpp, fixedwing_fast.hpp, dogfight.hpp), and the per-task side block it keeps in registers.
//
// Execution model: one wavefront lane per drone, one 64-lane wavefront per workgroup (no
// inter-wave synchronisation anywhere), persistent state as float4 groups [group][lane][4] so that
// every state access is a 16 B/lane, 1 KiB/wave coalesced global_load/store_dwordx4. The whole env
// step (env_step_ratio x ticks_per_control physics ticks, controller, reward, termination,
// auto-reset with its settle ticks) stays in registers; the row-major observation tile is
// transposed through LDS so that the [n][obs_dim] output is written with full-width stores.
// No MFMA: there is no dense contraction on this path (3x3 work only).
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>
#include <cstdint>

#include "../../include/pyflyt_amd.h"
#include "uav_device.hpp"
#include "uav_vehicles.hpp"
#include "shared_world.hpp"

namespace pf {

constexpr int kWave = 64;
constexpr int kMaxObs = 40;  // 13 + 4 + 6 + 3*4 = 35 (Fixedwing), 13 + 4 + 4 + 4*4 = 37 (QuadX with yaw targets)

// ------------------------------------------------------------------ per-task side block
// 12 floats per lane in state groups G_TGT..G_TGT+2:
//   waypoint tasks : the 4 x 3 target positions (waypoint_handler.py:70-83)
//   MA hover       : spawn position (3), spawn quaternion (4), the action of the previous call (4)
struct SideBlock {
  float t[4][3];
  float yaw[4];  // QuadX-Waypoints yaw targets (waypoint_handler.py:85-89), state group G_TGT + 3
  int n_left;
  PF_DEV void load(const float4* S, size_t n, size_t i, int g) {
    float4 a = S[(size_t)(g + 0) * n + i], b = S[(size_t)(g + 1) * n + i], c = S[(size_t)(g + 2) * n + i];
    t[0][0] = a.x; t[0][1] = a.y; t[0][2] = a.z; t[1][0] = a.w;
    t[1][1] = b.x; t[1][2] = b.y; t[2][0] = b.z; t[2][1] = b.w;
    t[2][2] = c.x; t[3][0] = c.y; t[3][1] = c.z; t[3][2] = c.w;
  }
  PF_DEV void store(float4* S, size_t n, size_t i, int g) const {
    S[(size_t)(g + 0) * n + i] = float4{t[0][0], t[0][1], t[0][2], t[1][0]};
    S[(size_t)(g + 1) * n + i] = float4{t[1][1], t[1][2], t[2][0], t[2][1]};
    S[(size_t)(g + 2) * n + i] = float4{t[2][2], t[3][0], t[3][1], t[3][2]};
  }
  PF_DEV void pop() {  // waypoint_handler.py:181-188
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
      for (int c = 0; c < 3; ++c) t[k][c] = t[k + 1][c];
    yaw[0] = yaw[1]; yaw[1] = yaw[2]; yaw[2] = yaw[3];
    n_left -= 1;
  }
};
PF_DEV float wrap_pi(float e) {  // waypoint_handler.py:147-149
  e = e > kPi ? e - 2.0f * kPi : e;
  return e < -kPi ? e + 2.0f * kPi : e;
}

// One Aviary.step out of line: used only by the rarely taken SAME_STEP settle loop so that the hot
// loop below keeps the single inlined copy.
template <class VEH, int MODE_T>
__device__ __noinline__ void aviary_step_outlined(VEH* V, const pf_params* P, const float* sp, Noise* nz, int flat_base) {
  V->template aviary_step<MODE_T>(*P, sp, *nz, flat_base);
}

// ------------------------------------------------------------------ the generic fused env kernel
// Every (vehicle, task, flight mode) the specialised QuadX mode-0 kernel (quadx_fast.hpp) does not
// cover. Flat control flow: reset preamble, ONE loop of Aviary steps with a single per-lane
// predicate (stepping lanes run env_step_ratio iterations with the env logic, lanes that are being
// reset run their settle iterations through the same loop body), epilogue.
// `tmpl`: a settled spawn state (GROUPS float4s) computed once per context when the settle phase
// cannot depend on the lane (Fixedwing: the settle throttle command is 0, so motor noise has
// nothing to scale; any vehicle with noise off) -- a reset is then a copy.
// roll_steps > 0: pf_rollout -- that many env steps in this one launch, the lane's state resident in registers between them (what a
// relaunch would re-derive from the stored groups is re-derived by VEH::relaunch, so the trajectory is the one of roll_steps x
// (pf_sample_actions + pf_env_step), bit for bit); step k's actions are B.actions[k] or drawn here with pf_sample_actions' keys
// (step index step0 + k), its outputs go to slot k of the trajectory buffers. 0: one step (pf_env_step / pf_env_reset).
template <class VEH, int TASK, int MODE_T>
__global__ void __launch_bounds__(kWave) env_kernel(const pf_params P, const pf_buffers B, const int n,
                                                    const uint64_t lane0, const int op, const uint8_t* mask,
                                                    const float4* __restrict__ tmpl, const pf_params* __restrict__ Pdev,
                                                    const int roll_steps, const uint32_t step0) {
  __shared__ __attribute__((aligned(16))) float tile[kWave * kMaxObs];
  __shared__ __attribute__((aligned(16))) float ktab[VEH::TABLE_FLOATS];
  __shared__ float wpose[kWave * 8];  // shared worlds: each lane's pose and contact bit, exchanged once per tick
  __shared__ float wvel[TASK == PF_TASK_MA_HOVER ? kWave * kPairVelStride : 1];  // ... and the new velocities for the pair stage
  const int tid = threadIdx.x;
  VEH::fill_table(ktab, Pdev, tid);
  __syncthreads();
  const int wave_base = blockIdx.x * kWave;
  const int lane = wave_base + tid;
  const bool valid = lane < n;
  const size_t li = valid ? lane : n - 1;
  const size_t N = (size_t)n;
  const float4* Sin = reinterpret_cast<const float4*>(B.state);
  float4* Sout = reinterpret_cast<float4*>(B.state);
  const int mode = (MODE_T == kRuntimeMode) ? P.flight_mode : MODE_T;
  constexpr bool kSide = (TASK == PF_TASK_WAYPOINTS || TASK == PF_TASK_MA_HOVER);

  static_assert(kWave * kMaxObs >= kContactSlotFloats, "the contact solver's LDS regions alias the observation tile: at least one worst-case region");
  VEH V;
  bind_contact(V, P, Pdev, tile, kWave * kMaxObs);  // (the tile is idle during the physics ticks)
  V.bind(ktab);
  if (TASK == PF_TASK_MA_HOVER && P.agents_per_world > 1) { V.b.wpose_ = wpose; V.b.wvel_ = wvel; V.b.wtid = tid; V.b.wA = P.agents_per_world; }
  SideBlock tg;
  float new_dist;
  int4 ints;
  V.load(Sin, N, li, mode, new_dist, ints);
  if (kSide) tg.load(Sin, N, li, VEH::G_TGT);
  const bool kYaw = (TASK == PF_TASK_WAYPOINTS) && P.use_yaw_targets != 0;
  tg.yaw[0] = tg.yaw[1] = tg.yaw[2] = tg.yaw[3] = 0.0f;
  float yaw_err0 = 0.0f;  // waypoint_handler.py:156
  if (kYaw) { float4 y = Sin[(size_t)(VEH::G_TGT + 3) * N + li]; tg.yaw[0] = y.x; tg.yaw[1] = y.y; tg.yaw[2] = y.z; tg.yaw[3] = y.w; }
  float4 ma_past = float4{0.f, 0.f, 0.f, 0.f};  // MA hover: self.past_actions (ma_quadx_base_env.py:326)
  if (TASK == PF_TASK_MA_HOVER) ma_past = Sin[(size_t)(VEH::G_TGT + 3) * N + li];
  int step_count = ints.x, flags = ints.y;
  uint32_t rng_ctr = (uint32_t)ints.z;
  // QuadX Hover / Waypoints: a reset's draws are keyed by the event counter at the lane's PREVIOUS reset (oracle/uav_oracle.c:
  // orc_env_reset; quadx_fast.hpp: QuadSpare). The key word lives in group 7's fourth word (flight modes -1, 0) or, where groups
  // 7-11 hold the cascade's memories, in group 11's third; this kernel prepares nothing ahead: it writes the word back with the
  // "spare valid" bit clear.
  constexpr bool REKEY = std::is_same<VEH, QuadX>::value && (TASK == PF_TASK_HOVER || TASK == PF_TASK_WAYPOINTS);
  const bool key_in11 = REKEY && mode > 0;
  uint32_t reset_kw = 0u;
  bool reset_kw_dirty = false;
  if (REKEY) {
    const float4 gk = Sin[(size_t)(key_in11 ? 11 : 7) * N + li];
    reset_kw = (uint32_t)__float_as_int(key_in11 ? gk.z : gk.w) & 0x7fffffffu;
  }
  tg.n_left = ints.w;
  bool term = (flags & PF_F_TERMINATED) != 0, trunc = (flags & PF_F_TRUNCATED) != 0;
  float old_dist = new_dist;

  Noise nz;
  nz.init(P, n, li, lane0);

  bool active = false, do_reset = false, wave_all = false;  // (per env step: set at the top of the step loop below)

  float sp[6] = {0, 0, 0, 0, 0, 0};
  float act4[4] = {0, 0, 0, 0};   // action slots of the observation
  float reward = 0.0f;
  bool pop_pending = false;
  bool rpy_valid = false;
  const int D = (P.angle_repr ? 13 : 12) + 4 + VEH::AUX +
                (TASK == PF_TASK_WAYPOINTS ? (kYaw ? 4 : 3) * P.num_targets : (TASK == PF_TASK_MA_HOVER ? 3 : 0));

  // env.reset() up to (not including) the settle phase: quadx_base_env.py:149-206,
  // ma_quadx_base_env.py:206-241. Returns with `sp` = the mode's default setpoint.
  auto begin_reset = [&]() {
    if (tmpl != nullptr) {
      float nd_;
      int4 i_;
      V.load(tmpl, 1, 0, 7, nd_, i_);  // settled spawn state incl. controller memories (mode 7 == every group)
      V.b.rpy = euler_from_quat_fast(V.b.q);
    } else if (TASK == PF_TASK_MA_HOVER) {
      const float pose[7] = {tg.t[0][0], tg.t[0][1], tg.t[0][2], tg.t[1][0], tg.t[1][1], tg.t[1][2], tg.t[2][0]};
      V.reset(P, pose, sp);
      V.set_mode(mode, sp);
    } else {
      V.reset(P, nullptr, sp);
      V.set_mode(mode, sp);
    }
    rpy_valid = true;
    step_count = 0; term = false; trunc = false; flags = 0; pop_pending = false;
    if (TASK != PF_TASK_MA_HOVER) act4[0] = act4[1] = act4[2] = act4[3] = 0.0f;
    nz.begin_event(REKEY ? reset_kw : rng_ctr, 1u, B.xi_reset);
    if (REKEY) { reset_kw = (rng_ctr + 1u) & 0x7fffffffu; reset_kw_dirty = true; }  // (the NEXT reset's key: the counter as this reset leaves it -- strictly increasing)
    if (TASK == PF_TASK_WAYPOINTS) {  // waypoint_handler.py:53-83
      const int nt = P.num_targets;
      tg.n_left = nt;
      new_dist = INFINITY; old_dist = INFINITY;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if (i < nt) {
          float theta, phi, dist;
          if (P.noise_mode == PF_NOISE_INJECT && B.u_targets != nullptr) {
            theta = B.u_targets[(size_t)i * N + li];
            phi = B.u_targets[(size_t)(nt + i) * N + li];
            dist = B.u_targets[(size_t)(2 * nt + i) * N + li];
          } else {
            theta = (2.0f * kPi) * nz.uniform(i, 2u);
            phi = (2.0f * kPi) * nz.uniform(nt + i, 2u);
            dist = fmaf(P.dome * 0.9f - 1.0f, nz.uniform(2 * nt + i, 2u), 1.0f);
          }
          float st, ct, sph, cph;
          sincosf(theta, &st, &ct);
          sincosf(phi, &sph, &cph);
          float zz = __builtin_fabsf(dist * cph);
          tg.t[i][0] = dist * sph * ct; tg.t[i][1] = dist * sph * st; tg.t[i][2] = zz > P.min_height ? zz : P.min_height;
        }
      }
      if (kYaw) {  // waypoint_handler.py:85-89: uniform(-pi, pi), drawn after all the positions
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (i < nt)
            tg.yaw[i] = (P.noise_mode == PF_NOISE_INJECT && B.u_targets != nullptr) ? B.u_targets[(size_t)(3 * nt + i) * N + li]
                                                                                    : fmaf(2.0f * kPi, nz.uniform(3 * nt + i, 2u), -kPi);
      }
    }
  };
  // compute_state's waypoint bookkeeping (waypoint_handler.py:135-142); ||R^T d|| = ||d||
  auto wp_distance = [&]() {
    if (TASK != PF_TASK_WAYPOINTS) return;
    if (pop_pending) { tg.pop(); pop_pending = false; }
    float dx = tg.t[0][0] - V.b.p.x, dy = tg.t[0][1] - V.b.p.y, dz = tg.t[0][2] - V.b.p.z;
    old_dist = new_dist;
    new_dist = sqrtf(fmaf(dx, dx, fmaf(dy, dy, dz * dz)));
    if (kYaw) yaw_err0 = __builtin_fabsf(wrap_pi(tg.yaw[0] - V.b.rpy.z));
  };
  // compute_term_trunc_reward: quadx_base_env.py:251-267, quadx_hover_env.py:117-138,
  // quadx_waypoints_env.py:177-204, fixedwing_waypoints_env.py:169-190, ma_quadx_hover_env.py:168-205
  auto term_trunc_reward = [&]() {
    if (step_count > P.max_steps) trunc = true;
    if (TASK == PF_TASK_MA_HOVER) {
      if (V.b.contact_step) { reward -= 100.0f; flags |= PF_F_INFO_COLLISION; term = true; }
      if (sqrtf(dot(V.b.p, V.b.p)) > P.dome) { reward -= 100.0f; flags |= PF_F_INFO_OOB; term = true; }
      if (!P.sparse_reward) {
        v3 d{V.b.p.x - tg.t[0][0], V.b.p.y - tg.t[0][1], V.b.p.z - tg.t[0][2]};
        float lin = sqrtf(dot(d, d));
        float ang = sqrtf(fmaf(V.b.rpy.x, V.b.rpy.x, V.b.rpy.y * V.b.rpy.y));
        reward -= lin + ang * 0.1f;
        reward += 1.0f;
      }
      return;
    }
    if (V.b.contact_step) { reward = -100.0f; flags |= PF_F_INFO_COLLISION; term = true; }
    if (sqrtf(dot(V.b.p, V.b.p)) > P.dome) { reward = -100.0f; flags |= PF_F_INFO_OOB; term = true; }
    if (TASK == PF_TASK_HOVER) {
      if (!P.sparse_reward) {
        v3 d{V.b.p.x, V.b.p.y, V.b.p.z - 1.0f};
        float lin = sqrtf(dot(d, d));
        float yaw_rate = __builtin_fabsf(V.b.wb.z);
        reward -= 0.01f * (yaw_rate * yaw_rate);
        float ang = sqrtf(fmaf(V.b.rpy.x, V.b.rpy.x, V.b.rpy.y * V.b.rpy.y));
        reward -= lin + ang;
        reward += 1.0f;
      }
    } else if (TASK == PF_TASK_WAYPOINTS) {
      if (!P.sparse_reward) {
        float progress = (isinf(old_dist + new_dist)) ? 0.0f : old_dist - new_dist;
        reward += __builtin_fmaxf(3.0f * progress, 0.0f);
        reward += P.wp_dist_reward / new_dist;
        if (P.wp_yaw_penalty != 0.0f) {
          float yaw_rate = __builtin_fabsf(V.b.wb.z);
          reward -= P.wp_yaw_penalty * (yaw_rate * yaw_rate);
        }
      }
      if (new_dist < P.goal_reach_distance && (!kYaw || yaw_err0 < P.goal_reach_angle)) {  // waypoint_handler.py:167-179
        reward = 100.0f;
        pop_pending = true;  // the observation of this step still shows the reached target
        if ((tg.n_left - 1) == 0) { trunc = true; flags |= PF_F_INFO_COMPLETE; }
      }
    }
  };
  // flattened observation row of this lane -> LDS tile (Appendix A of SURVEY.md)
  auto write_obs_row = [&]() {
    if (!rpy_valid) { V.b.rpy = euler_from_quat_fast(V.b.q); rpy_valid = true; }
    float* row = tile + tid * D;
    int k = 0;
    row[k++] = V.b.wb.x; row[k++] = V.b.wb.y; row[k++] = V.b.wb.z;
    quat qe = canon_quat(V.b.q);
    if (P.angle_repr) { row[k++] = qe.x; row[k++] = qe.y; row[k++] = qe.z; row[k++] = qe.w; }
    else { row[k++] = V.b.rpy.x; row[k++] = V.b.rpy.y; row[k++] = V.b.rpy.z; }
    row[k++] = V.b.vb.x; row[k++] = V.b.vb.y; row[k++] = V.b.vb.z;
    row[k++] = V.b.p.x; row[k++] = V.b.p.y; row[k++] = V.b.p.z;
    float aux[VEH::AUX];
    V.aux(aux);
    if (TASK == PF_TASK_MA_HOVER) {  // ma_quadx_hover_env.py:141-166: aux, past action, start_pos
#pragma unroll
      for (int a = 0; a < VEH::AUX; ++a) row[k++] = aux[a];
      row[k++] = ma_past.x; row[k++] = ma_past.y; row[k++] = ma_past.z; row[k++] = ma_past.w;
      row[k++] = tg.t[0][0]; row[k++] = tg.t[0][1]; row[k++] = tg.t[0][2];
    } else {
      row[k++] = act4[0]; row[k++] = act4[1]; row[k++] = act4[2]; row[k++] = act4[3];
#pragma unroll
      for (int a = 0; a < VEH::AUX; ++a) row[k++] = aux[a];
    }
    if (TASK == PF_TASK_WAYPOINTS) {
      m3 Re = rot_from_quat(qe);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if (i < P.num_targets) {
          v3 d = mulT(Re, v3{tg.t[i][0] - V.b.p.x, tg.t[i][1] - V.b.p.y, tg.t[i][2] - V.b.p.z});
          bool live = i < tg.n_left;
          row[k++] = live ? d.x : 0.0f; row[k++] = live ? d.y : 0.0f; row[k++] = live ? d.z : 0.0f;
          if (kYaw) row[k++] = live ? wrap_pi(tg.yaw[i] - V.b.rpy.z) : 0.0f;  // waypoint_handler.py:144-153
        }
      }
    }
  };

  const int n_env_steps = roll_steps > 0 ? roll_steps : 1;
  for (int ks = 0; ks < n_env_steps; ++ks) {
  const size_t toff = (size_t)ks * N;  // this env step's slot in the trajectory buffers, in lanes
  if (ks > 0) {  // what the next launch would start from: the stored groups, re-derived
    V.relaunch(mode, flags);
    rpy_valid = false;
    old_dist = new_dist;
    yaw_err0 = 0.0f;
    reward = 0.0f;
#pragma unroll
    for (int k = 0; k < 6; ++k) sp[k] = 0.0f;
    act4[0] = act4[1] = act4[2] = act4[3] = 0.0f;
  }
  if (op == OP_RESET) {
    do_reset = (mask == nullptr) || (mask[li] != 0);
    // (shared worlds: a mask that names some agents of a world resets the world)
    if (TASK == PF_TASK_MA_HOVER && P.agents_per_world > 1) do_reset = widen_to_world(do_reset && valid, tid, P.agents_per_world);
    active = do_reset;
  } else {
    do_reset = (P.autoreset == PF_AUTORESET_NEXT_STEP) && (term || trunc);
    active = true;
  }
  active = active && valid;
  do_reset = do_reset && active;
  wave_all = __all(active || !valid);

  // ---------------------------------------------------------------- what each lane runs
  bool settling = false;  // in the settle phase of a reset (no env logic after an Aviary step)
  int my_its = 0;         // Aviary steps this lane still has to run in the loop below
  float4 a = float4{0.f, 0.f, 0.f, 0.f};
  if (roll_steps > 0 && B.actions == nullptr) {  // pf_sample_actions' draw for (lane, step0 + ks): every lane's, restarting or not
    a = sampled_action4<true>((uint32_t)P.seed, (uint32_t)(P.seed >> 32), (uint32_t)(lane0 + li), step0 + (uint32_t)ks, P.action_low, P.action_high);
    if (B.actions_out != nullptr && valid) reinterpret_cast<float4*>(B.actions_out)[toff + li] = a;
  } else if (active && !do_reset) {
    a = reinterpret_cast<const float4*>(B.actions)[toff + li];
  }
  // (wave-uniform guard: most waves of most launches restart nobody. It also takes the reset's divergent region out of the path into
  //  the Aviary-step loop: with `if (do_reset) ... else if (active) ...` the allocator's copies of the zeroed PID memories landed in
  //  front of the join block's exec restore in the QuadX-Hover instantiations -- tools/isa_exec_check.py, 25 of round 5's 186 sites)
  if (__builtin_expect(__any(do_reset), 0)) {
    if (do_reset) {
      begin_reset();
      settling = true;
      my_its = (tmpl != nullptr) ? 0 : P.settle_steps;
    }
  }
  if (active && !do_reset) {
    if (TASK == PF_TASK_MA_HOVER) {  // past <- current, current <- action (ma_quadx_base_env.py:326-332)
      ma_past = float4{tg.t[2][1], tg.t[2][2], tg.t[3][0], tg.t[3][1]};
      tg.t[2][1] = a.x; tg.t[2][2] = a.y; tg.t[3][0] = a.z; tg.t[3][1] = a.w;
      reward = 0.0f;
      term = false; trunc = false;  // per-call flags (ma_quadx_base_env.py:336-337)
      my_its = P.env_step_ratio;    // no early exit in the multi-agent base (:342-361)
    } else {
      act4[0] = a.x; act4[1] = a.y; act4[2] = a.z; act4[3] = a.w;
      reward = -0.1f;
      my_its = (term || trunc) ? 0 : P.env_step_ratio;  // quadx_base_env.py:289-290
    }
    sp[0] = a.x; sp[1] = a.y; sp[2] = a.z;
    sp[3] = P.throttle_remap ? fmaf(a.w, 0.5f, 0.5f) : a.w;  // fixedwing_base_env.py:260
    nz.begin_event(rng_ctr, 0u, B.xi);
  }

  // Shared world (pz_envs: every agent's drone in ONE Bullet world): the A lanes of a world sit next to each other in the
  // wave; before every tick they exchange pose and contact bit through LDS, test their collision boxes against each other
  // (15 axes, in the peer's frame, behind a bounding-sphere test) and OR the world's contact bits into the gate of the
  // rotational drag. One Aviary.step = control + ticks_per_control x (exchange, tick).
  const int A = (TASK == PF_TASK_MA_HOVER && P.agents_per_world > 1) ? P.agents_per_world : 1;
  auto world_aviary_step = [&](int flat_base) {
    V.b.contact_step = false;
    V.template control<MODE_T>(P, sp);
    for (int t = 0; t < P.ticks_per_control; ++t) {
      world_exchange(V.b, wpose, tid, A, P.bound_radius, Pdev);  // (shared_world.hpp)
      if constexpr (TASK == PF_TASK_MA_HOVER) V.template tick<true>(P, nz.get(flat_base + t));  // (with the contact response between the drones)
      else V.tick(P, nz.get(flat_base + t));
    }
    V.b.peer_contact = false;
    V.b.rpy = euler_from_quat_fast(V.b.q);
  };
  int it = 0;
  while (__any(my_its > 0)) {
    if (my_its > 0) {
      if (A > 1) world_aviary_step(it * P.ticks_per_control);
      else V.template aviary_step<MODE_T>(P, sp, nz, it * P.ticks_per_control);
      rpy_valid = true;
      my_its -= 1;
      if (!settling) {
        wp_distance();
        term_trunc_reward();
        if (TASK != PF_TASK_MA_HOVER && (term || trunc)) my_its = 0;
      }
    }
    it += 1;
  }
  const bool stepped = active && !settling && op == OP_STEP;
  const float out_reward = stepped ? reward : 0.0f;
  const bool out_term = stepped && term, out_trunc = stepped && trunc;
  if (stepped) {
    step_count += 1; rng_ctr += 1;  // quadx_base_env.py:299
    if (V.nonfinite()) flags |= PF_F_NONFINITE;  // NaN / Inf guard (see quadx_fast.hpp)
  }

  // ---------------------------------------------------------------- SAME_STEP auto-reset (rare path)
  if (P.autoreset == PF_AUTORESET_SAME_STEP) {
    const bool same = stepped && (term || trunc);
    if (__any(same)) {
      if (B.final_obs != nullptr) {  // terminal observation, before the state is re-initialised
        if (active) write_obs_row();
        flush_obs_tile(tile, B.final_obs + toff * D, D, kWave, n, wave_base, tid, wave_all, active);
      }
      if (B.final_info != nullptr && same) {  // gymnasium's final_info: the episode's flags / targets left, pre-reset
        B.final_info[2 * (toff + li) + 0] = done_flags(flags, term, trunc, V.b.contact_now);
        B.final_info[2 * (toff + li) + 1] = tg.n_left - (pop_pending ? 1 : 0);
      }
      if (same) {
        begin_reset();
        settling = true;
        if (tmpl == nullptr) {
          // through copies: handing &V itself to an out-of-line call would pin the whole vehicle
          // state in scratch memory for the entire kernel (measured: 1.9 KB/lane, 2x slower)
          VEH Vc = V;
          Noise nc = nz;
          float spc[6] = {sp[0], sp[1], sp[2], sp[3], sp[4], sp[5]};
          for (int s = 0; s < P.settle_steps; ++s) aviary_step_outlined<VEH, MODE_T>(&Vc, Pdev, spc, &nc, s * P.ticks_per_control);
          V = Vc;
        }
      }
    }
  }
  if (active && settling) {  // end_reset: compute_state after the settle steps (quadx_base_env.py:212)
    wp_distance();
    rng_ctr += 1;
  }

  // ---------------------------------------------------------------- outputs: obs tile first, state after
  if (active) write_obs_row();
  flush_obs_tile(tile, B.obs + toff * D, D, kWave, n, wave_base, tid, wave_all, active);
  if (active) {
    if (pop_pending) { tg.pop(); pop_pending = false; }
    flags = done_flags(flags, term, trunc, V.b.contact_now);
    if (ks == n_env_steps - 1) {  // the state goes back to HBM once per launch
      V.store(Sout, N, li, mode, new_dist, int4{step_count, flags, (int)rng_ctr, tg.n_left});
      if constexpr (REKEY) {
        if (key_in11) Sout[(size_t)11 * N + li] = float4{V.zE[0], V.zE[1], __int_as_float((int)reset_kw), 0.0f};
        else if (reset_kw_dirty) Sout[(size_t)7 * N + li] = float4{0.0f, 0.0f, 0.0f, __int_as_float((int)reset_kw)};
      }
      if (kSide) tg.store(Sout, N, li, VEH::G_TGT);
      if (kYaw) Sout[(size_t)(VEH::G_TGT + 3) * N + li] = float4{tg.yaw[0], tg.yaw[1], tg.yaw[2], tg.yaw[3]};
      if (TASK == PF_TASK_MA_HOVER) Sout[(size_t)(VEH::G_TGT + 3) * N + li] = ma_past;
    }
    step_outputs(B, op, toff, li, out_reward, out_term, out_trunc);
  }
  }  // (env steps of this launch)
}

}  // namespace pf
