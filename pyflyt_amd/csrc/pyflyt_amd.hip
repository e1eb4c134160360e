// pyflyt_amd.hip -- kernels + C ABI (include/pyflyt_amd.h) of the MI355X-native batched UAV step.
//
// Execution model: one wavefront lane per drone, one 64-lane wavefront per workgroup (no
// inter-wave synchronisation anywhere), persistent state as float4 groups [group][lane][4] so that
// every state access is a 16 B/lane, 1 KiB/wave coalesced global_load/store_dwordx4. The whole env
// step (env_step_ratio x ticks_per_control physics ticks, controller, reward, termination,
// auto-reset with its settle ticks) stays in registers; the row-major observation tile is
// transposed through LDS so that the [n][obs_dim] output is written with full-width stores.
// No MFMA: there is no dense contraction on this path (3x3 work only).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <type_traits>

#include "../../include/pyflyt_amd.h"
#include "uav_vehicles.hpp"
#include "quadx_fast.hpp"
#include "fixedwing_fast.hpp"
#include "dogfight.hpp"
#include "rocket.hpp"

namespace pf {

constexpr int kWave = 64;
constexpr int kMaxObs = 40;  // 13 + 4 + 6 + 3*4 = 35 (Fixedwing), 13 + 4 + 4 + 4*4 = 37 (QuadX with yaw targets)

// Aviary-level kernels (where bodies land and stay landed): 30 KB of LDS for the contact solve -- every lane of a wave of
// quadrotors (the incident face's 4 vertices + the sentinel, 24 floats each) in one round, six worst-case airframes (48
// vertices) side by side
constexpr int kAviaryContactFloats = 64 * 5 * kContactWords;

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
// Rocket-Landing: env_kernel<Rocket, PF_TASK_ROCKET_LANDING, kRuntimeMode> and the landing pad
#include "rocket_landing.hpp"
namespace pf {

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
#include "gae.hpp"
#include "traj_stats.hpp"
#include "ppo_loss.hpp"
#include "mlp_tile.hpp"
#include "policy_act.hpp"
#include "mlp.hpp"
#include "ppo_grad.hpp"
#include "adam.hpp"
#include "world_sync.hpp"

// ====================================================================== C ABI
// The env kernel a context runs, chosen once at pf_ctx_create (select_env_kernel).
enum class env_family : uint8_t {
  none,              // no env task: the pf_aviary_* calls only
  quadx,             // quadx_m0_env_kernel (quadx_fast.hpp)
  fixedwing_wp,      // fixedwing_wp_env_kernel (fixedwing_fast.hpp)
  dogfight_fast,     // dogfight_env_kernel<A, DfFastVeh>: the aircraft run on the specialised Fixedwing tick (dogfight.hpp)
  dogfight_generic,  // dogfight_env_kernel<A, DfGenericVeh>
  rocket_landing,    // env_kernel<Rocket, PF_TASK_ROCKET_LANDING, kRuntimeMode> (rocket_landing.hpp)
  generic,           // env_kernel<QuadX / Fixedwing, TASK, MODE_T>
};
struct env_choice {
  env_family family;
  bool cr, md, sh;  // quadx: quadx_m0_env_kernel's CR / MD / SH, as K implies them
  bool wps1;        // quadx, fixedwing_wp: the one-wave-per-SIMD instantiation (WPS = 1, 512 registers)
  bool fixed;       // quadx: pf_env_step without a mask runs the instantiation with the call shape pinned (quadx_fast.hpp: FIXED)
};

struct pf_ctx {
  pf_params P;
  int n;
  int device;
  uint64_t lane0;
  char err[256];
  env_choice ek;
  uint32_t* launch_ctr;  // device, one word per workgroup of the specialised QuadX kernel: env steps taken so far -- the cadence its waves refill their spares on (quadx_fast.hpp: QuadSpare)
  pf::QuadK K;
  pf_params* P_dev;  // device copy of P for the rarely-taken floor paths (contact detection and response) and the LDS constant tables
  float4* tmpl;      // settled spawn state for lane-independent resets (env_kernel), or null
  pf::FwK FK;
  pf::FwTable* surf_dev;  // pre-combined surface + body constants (scalar-loaded per tick)
  float* policy_dev;      // the specialised QuadX kernel: pf_rollout_policy's packed weights (policy_mlp.hpp), rewritten by every call
  double* ts_scratch;     // contexts with an env task: pf_traj_stats's partial sums between its launches (traj_stats.hpp: ts_scratch_words)
  double* ppo_scratch;    // every context: pf_ppo_loss's partial sums between its launches (ppo_loss.hpp: kPpoScratchWords)
  uint8_t* sync_latch;    // every context: pf_world_sync's staging buffer, n bytes -- the new latch, copied over the caller's behind the kernel (world_sync.hpp)
  int act_grid_cap;       // pf_policy_act: the most workgroups a launch takes, two per CU of the device: what its registers admit (two waves per SIMD; profiles/policy_act/resources.txt) (policy_act.hpp)
};
static thread_local char g_err[256] = "";

static int fail(pf_ctx* ctx, int code, const char* msg) {
  snprintf(ctx ? ctx->err : g_err, 256, "%s", msg);
  if (ctx) snprintf(g_err, 256, "%s", msg);
  return code;
}
static int hip_fail(pf_ctx* ctx, hipError_t e, const char* where) {
  char buf[256];
  snprintf(buf, sizeof(buf), "%s: %s", where, hipGetErrorString(e));
  return fail(ctx, (int)e, buf);
}
#define PF_HIP(ctx, call)                                   \
  do {                                                      \
    hipError_t e__ = (call);                                \
    if (e__ != hipSuccess) return hip_fail(ctx, e__, #call); \
  } while (0)

// Which env kernel a context runs, and its launch-invariant template arguments; fills K, FK and fsurf for the specialised kernels.
// The only reader of the environment overrides, which exist for the tests: PF_DISABLE_FAST forces the generic kernels,
// PF_NO_LEAN_KERNEL the two-wave instantiations, PF_NO_CALM_PATH turns the specialised QuadX kernel's calm-wave ticks off,
// PF_NO_FIXED_STEP keeps pf_env_step on the general one-step instantiation.
static env_choice select_env_kernel(const pf_params& P, int n_lanes, int device, pf::QuadK& K, pf::FwK& FK, pf::FwTable& fsurf) {
  env_choice c{env_family::generic, false, false, false, false, false};
  const bool fast = getenv("PF_DISABLE_FAST") == nullptr;
  int cus = 0;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess) cus = 0;
  // the batch is at most one wave per SIMD of the device (4 SIMDs per CU): a second resident wave would have nothing to run
  const bool one_wave = cus > 0 && ((long)n_lanes + 63) / 64 <= 4L * cus && getenv("PF_NO_LEAN_KERNEL") == nullptr;
  if (P.task == PF_TASK_NONE) {
    c.family = env_family::none;
  } else if (P.task == PF_TASK_ROCKET_LANDING) {
    c.family = env_family::rocket_landing;
  } else if (P.task == PF_TASK_DOGFIGHT) {
    c.family = fast && pf::fw_table_from_params(P, fsurf) ? env_family::dogfight_fast : env_family::dogfight_generic;
  } else if (fast && pf::quadk_from_params(P, K)) {
    c.family = env_family::quadx;
    if (getenv("PF_NO_CALM_PATH") != nullptr) K.calm_on = 0;
    // (flight modes other than 0: the MODES instantiation, contact response compiled in; shared worlds: PF_TASK_MA_HOVER with the
    //  contact response on -- quadk_from_params)
    c.md = K.mode != 0;
    c.cr = c.md || P.contact_response;
    c.sh = P.task == PF_TASK_MA_HOVER && c.cr && K.apw > 1;
    // (the one-wave-per-SIMD instantiation -- quadx_fast.hpp, WPS -- exists where CR && !SH: since round 6 the PettingZoo task with
    //  independent lanes as well; since round 5 the cascaded flight modes: their fp64 controller needs the 512 registers -- 408 B of
    //  stack per lane under 256. It solves floor contacts in registers, four slots = the incident face: quad_floor_solve)
    c.wps1 = one_wave && P.contact_manifold_points < 8 && c.cr && !c.sh;
    // (the fixed call shape -- quadx_fast.hpp, FIXED -- is instantiated for what the training loops run: Hover / Waypoints with the contact
    //  response on, noise drawn on the device or off, and exactly the values it pins)
    const int fixed_ratio = P.task == PF_TASK_HOVER ? pf::kQuadFixedRatio<PF_TASK_HOVER> : pf::kQuadFixedRatio<PF_TASK_WAYPOINTS>;
    c.fixed = (P.task == PF_TASK_HOVER || P.task == PF_TASK_WAYPOINTS) && c.cr && !c.md && !c.sh && P.noise_mode != PF_NOISE_INJECT &&
              P.autoreset == PF_AUTORESET_NEXT_STEP && P.env_step_ratio == fixed_ratio && P.angle_repr == 1 && P.sparse_reward == 0 &&
              getenv("PF_NO_FIXED_STEP") == nullptr;
  } else if (fast && pf::fwk_from_params(P, FK, fsurf)) {
    c.family = env_family::fixedwing_wp;
    c.wps1 = one_wave;
  }
  return c;
}

// The instantiation of a per-vehicle kernel for the context's vehicle. Each call passes those of the vehicles it admits (none for
// the Rocket where the call or pf_ctx_create refuses it).
template <class KERNEL>
static KERNEL vehicle_kernel(const pf_ctx* ctx, KERNEL quadx, KERNEL fixedwing, KERNEL rocket = nullptr) {
  return ctx->P.vehicle == PF_QUADX ? quadx : (ctx->P.vehicle == PF_ROCKET && rocket) ? rocket : fixedwing;
}

// The env kernels' instantiations. A launch takes the context's choice (env_choice) and the call's ROLL: 0 for pf_env_reset and
// pf_env_step, 1 for pf_rollout with the actions drawn on the device, 2 for pf_rollout over the given b->actions. The pickers
// name exactly the instantiations that can run.
template <int V>
using int_c = std::integral_constant<int, V>;

// pick(NOISE, ROLL) (pf_rollout refuses PF_NOISE_INJECT: the rollouts have no such instantiation)
template <class Pick>
static auto by_noise_roll(int noise, int roll, Pick pick) {
  const bool philox = noise == PF_NOISE_PHILOX;
  if (roll == 1) return philox ? pick(int_c<PF_NOISE_PHILOX>{}, int_c<1>{}) : pick(int_c<PF_NOISE_OFF>{}, int_c<1>{});
  if (roll == 2) return philox ? pick(int_c<PF_NOISE_PHILOX>{}, int_c<2>{}) : pick(int_c<PF_NOISE_OFF>{}, int_c<2>{});
  if (noise == PF_NOISE_INJECT) return pick(int_c<PF_NOISE_INJECT>{}, int_c<0>{});
  return philox ? pick(int_c<PF_NOISE_PHILOX>{}, int_c<0>{}) : pick(int_c<PF_NOISE_OFF>{}, int_c<0>{});
}

// fixed_call: a pf_env_step without a mask of a context inside the fixed shape's envelope (c.fixed: CR, mode 0, independent lanes)
template <int TASK, int NZ, int R>
static auto quadx_m0_kernel(const env_choice& c, bool fixed_call) {
  constexpr bool MA = TASK == PF_TASK_MA_HOVER;  // (c.sh: a shared world, the PettingZoo task only)
  using namespace pf;
  if constexpr (R == 0 && NZ != PF_NOISE_INJECT && !MA)
    if (fixed_call)
      return c.wps1 ? quadx_m0_env_kernel<TASK, NZ, 64, 0, true, false, false, 1, true> : quadx_m0_env_kernel<TASK, NZ, 64, 0, true, false, false, 2, true>;
  if (c.md)
    return c.sh ? quadx_m0_env_kernel<TASK, NZ, 64, R, true, true, MA, 2>
                : c.wps1 ? quadx_m0_env_kernel<TASK, NZ, 64, R, true, true, false, 1> : quadx_m0_env_kernel<TASK, NZ, 64, R, true, true, false, 2>;
  if (c.cr)
    return c.sh ? quadx_m0_env_kernel<TASK, NZ, 64, R, true, false, MA, 2>
                : c.wps1 ? quadx_m0_env_kernel<TASK, NZ, 64, R, true, false, false, 1> : quadx_m0_env_kernel<TASK, NZ, 64, R, true, false, false, 2>;
  return quadx_m0_env_kernel<TASK, NZ, 64, R, false, false, false, 2>;
}

template <class VEH, bool ROLLOUT>
static auto dogfight_kernel(int agents_per_world) {
  switch (agents_per_world) {
    case 2: return pf::dogfight_env_kernel<2, VEH, ROLLOUT>;
    case 4: return pf::dogfight_env_kernel<4, VEH, ROLLOUT>;
    case 6: return pf::dogfight_env_kernel<6, VEH, ROLLOUT>;
    default: return pf::dogfight_env_kernel<8, VEH, ROLLOUT>;
  }
}

// env_kernel: MODE_T = 0 for a QuadX in flight mode 0, else the runtime mode -- the context's flight mode at this call, which
// pf_aviary_set_mode and pf_aviary_reset change
static auto generic_env_kernel(const pf_ctx* ctx) {
  using namespace pf;
  const pf_params& P = ctx->P;
  if (ctx->ek.family == env_family::rocket_landing) return env_kernel<Rocket, PF_TASK_ROCKET_LANDING, kRuntimeMode>;
  if (P.vehicle != PF_QUADX) return env_kernel<Fixedwing, PF_TASK_WAYPOINTS, kRuntimeMode>;
  const bool m0 = P.flight_mode == 0;
  if (P.task == PF_TASK_HOVER) return m0 ? env_kernel<QuadX, PF_TASK_HOVER, 0> : env_kernel<QuadX, PF_TASK_HOVER, kRuntimeMode>;
  if (P.task == PF_TASK_MA_HOVER) return m0 ? env_kernel<QuadX, PF_TASK_MA_HOVER, 0> : env_kernel<QuadX, PF_TASK_MA_HOVER, kRuntimeMode>;
  return m0 ? env_kernel<QuadX, PF_TASK_WAYPOINTS, 0> : env_kernel<QuadX, PF_TASK_WAYPOINTS, kRuntimeMode>;
}

static int ensure_device(pf_ctx* ctx) {
  int cur = -1;
  PF_HIP(ctx, hipGetDevice(&cur));
  if (cur != ctx->device) PF_HIP(ctx, hipSetDevice(ctx->device));
  return PF_OK;
}

// One launch of the context's env kernel: a reset or a step (roll 0, op and mask) or a rollout (roll 1 / 2, k_steps steps from step
// index step0). The callers have checked the arguments.
static int launch_env(pf_ctx* ctx, const pf_buffers* b, int op, const uint8_t* mask, int roll, int k_steps, uint32_t step0, void* stream) {
  int rc = ensure_device(ctx);
  if (rc) return rc;
  const pf_params& P = ctx->P;
  const env_choice& c = ctx->ek;
  hipStream_t s = (hipStream_t)stream;
  switch (c.family) {
    case env_family::quadx: {
      const bool fixed_call = c.fixed && roll == 0 && op == pf::OP_STEP && mask == nullptr;
      const auto kernel = by_noise_roll(P.noise_mode, roll, [&](auto NZ, auto R) {
        if (P.task == PF_TASK_HOVER) return quadx_m0_kernel<PF_TASK_HOVER, NZ, R>(c, fixed_call);
        if (P.task == PF_TASK_MA_HOVER) return quadx_m0_kernel<PF_TASK_MA_HOVER, NZ, R>(c, fixed_call);
        return quadx_m0_kernel<PF_TASK_WAYPOINTS, NZ, R>(c, fixed_call);
      });
      const int grid = (ctx->n + 64 * pf::kQuadWPB - 1) / (64 * pf::kQuadWPB);
      hipLaunchKernelGGL(kernel, dim3(grid), dim3(64 * pf::kQuadWPB), 0, s, ctx->K, *b, ctx->P_dev, ctx->n, ctx->lane0, op, mask, k_steps, step0,
                         ctx->launch_ctr, pf::PolicyK{});
      break;
    }
    case env_family::fixedwing_wp: {
      const auto kernel = by_noise_roll(P.noise_mode, roll, [&](auto NZ, auto R) {
        return c.wps1 ? pf::fixedwing_wp_env_kernel<NZ, R, 1> : pf::fixedwing_wp_env_kernel<NZ, R, 2>;
      });
      hipLaunchKernelGGL(kernel, dim3((ctx->n + 63) / 64), dim3(64), 0, s, ctx->FK, ctx->surf_dev, *b, ctx->P_dev, ctx->tmpl, ctx->n, ctx->lane0, op,
                         mask, k_steps, step0);
      break;
    }
    case env_family::dogfight_fast:
    case env_family::dogfight_generic: {
      const int apw = P.agents_per_world, lpw = (64 / apw) * apw;  // whole worlds per wave
      const bool fast = c.family == env_family::dogfight_fast;
      const auto kernel = roll ? (fast ? dogfight_kernel<pf::DfFastVeh, true>(apw) : dogfight_kernel<pf::DfGenericVeh, true>(apw))
                               : (fast ? dogfight_kernel<pf::DfFastVeh, false>(apw) : dogfight_kernel<pf::DfGenericVeh, false>(apw));
      hipLaunchKernelGGL(kernel, dim3((ctx->n + lpw - 1) / lpw), dim3(64), 0, s, ctx->P, *b, ctx->n, ctx->lane0, op, mask, ctx->P_dev, ctx->surf_dev,
                         k_steps, step0);
      break;
    }
    case env_family::rocket_landing:
    case env_family::generic:  // (roll_steps 0: one step)
      hipLaunchKernelGGL(generic_env_kernel(ctx), dim3((ctx->n + pf::kWave - 1) / pf::kWave), dim3(pf::kWave), 0, s, ctx->P, *b, ctx->n, ctx->lane0,
                         op, mask, ctx->tmpl, ctx->P_dev, roll ? k_steps : 0, step0);
      break;
    case env_family::none:  // (refused by the callers)
      break;
  }
  PF_HIP(ctx, hipGetLastError());
  return PF_OK;
}

// pf_rollout_policy's instantiations: the one-wave-per-SIMD register budget at every batch size (the evaluation's 64 accumulators on top
// of the env step leave no room under two waves' 256 registers without scratch, and its LDS -- 21 KB of the rollout + 16 KB of activations --
// admits four waves per CU whatever the budget), with the contact response compiled in or not as the context has it. Zero scratch, all eight.
template <int TASK>
static auto quadx_policy_kernel(bool philox, bool cr) {
  using namespace pf;
  if (cr)
    return philox ? quadx_m0_env_kernel<TASK, PF_NOISE_PHILOX, 64, 3, true, false, false, 1> : quadx_m0_env_kernel<TASK, PF_NOISE_OFF, 64, 3, true, false, false, 1>;
  return philox ? quadx_m0_env_kernel<TASK, PF_NOISE_PHILOX, 64, 3, false, false, false, 1> : quadx_m0_env_kernel<TASK, PF_NOISE_OFF, 64, 3, false, false, false, 1>;
}

extern "C" {

int pf_abi_version(void) { return PF_ABI_VERSION; }
size_t pf_sizeof_params(void) { return sizeof(pf_params); }
size_t pf_sizeof_buffers(void) { return sizeof(pf_buffers); }
size_t pf_sizeof_policy(void) { return sizeof(pf_policy); }
size_t pf_sizeof_gae(void) { return sizeof(pf_gae_args); }
size_t pf_sizeof_traj_stats(void) { return sizeof(pf_traj_stats_args); }
size_t pf_sizeof_ppo_loss(void) { return sizeof(pf_ppo_loss_args); }
size_t pf_sizeof_mlp(void) { return sizeof(pf_mlp); }
size_t pf_sizeof_ppo_grad(void) { return sizeof(pf_ppo_grad_args); }
size_t pf_sizeof_adam(void) { return sizeof(pf_adam_args); }
size_t pf_sizeof_world_sync(void) { return sizeof(pf_world_sync_args); }
const char* pf_last_error(const pf_ctx* ctx) { return ctx ? ctx->err : g_err; }

int pf_ctx_create(const pf_params* params, int n_lanes, int device, uint64_t lane_offset, pf_ctx** out) {
  if (!params || !out || n_lanes <= 0) return fail(nullptr, PF_ERR_ARG, "pf_ctx_create: bad argument");
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count == 0)
    return fail(nullptr, PF_ERR_NO_DEVICE, "pf_ctx_create: no HIP device (this library has no CPU fallback)");
  if (device < 0 || device >= count) return fail(nullptr, PF_ERR_ARG, "pf_ctx_create: bad device index");
  const pf_params& P = *params;
  if (P.vehicle != PF_QUADX && P.vehicle != PF_FIXEDWING && P.vehicle != PF_ROCKET) return fail(nullptr, PF_ERR_ARG, "unknown vehicle");
  if (P.vehicle == PF_ROCKET && P.task != PF_TASK_NONE && P.task != PF_TASK_ROCKET_LANDING)
    return fail(nullptr, PF_ERR_UNSUPPORTED, "the Rocket flies the Aviary-level entry points and the Rocket-Landing task (PF_TASK_ROCKET_LANDING) only");
  if (P.task == PF_TASK_ROCKET_LANDING) {  // gym_envs/rocket_envs/rocket_landing_env.py
    if (P.vehicle != PF_ROCKET) return fail(nullptr, PF_ERR_UNSUPPORTED, "the Rocket-Landing task flies the Rocket");
    if (!(P.pad_radius > 0.0f) || !(P.pad_half_height >= 0.0f)) return fail(nullptr, PF_ERR_ARG, "Rocket-Landing: pad_radius must be > 0, pad_half_height >= 0");
    if ((P.rl_reset_options & ~(PF_RL_RANDOMIZE_DROP | PF_RL_ACCELERATE_DROP)) != 0) return fail(nullptr, PF_ERR_ARG, "Rocket-Landing: unknown reset option bits");
  }
  if (P.vehicle == PF_ROCKET && P.flight_mode != 0) return fail(nullptr, PF_ERR_ARG, "rocket flight_mode must be 0");
  if (P.task == PF_TASK_WAYPOINTS && (P.num_targets < 1 || P.num_targets > 4))
    return fail(nullptr, PF_ERR_UNSUPPORTED, "num_targets must be in 1..4");
  if (P.vehicle == PF_QUADX && (P.flight_mode < -1 || P.flight_mode > 7)) return fail(nullptr, PF_ERR_ARG, "quadx flight_mode must be in -1..7");
  if (P.vehicle == PF_FIXEDWING && (P.flight_mode < -1 || P.flight_mode > 0)) return fail(nullptr, PF_ERR_ARG, "fixedwing flight_mode must be -1 or 0");
  if (P.vehicle == PF_FIXEDWING && (P.task == PF_TASK_HOVER || P.task == PF_TASK_MA_HOVER)) return fail(nullptr, PF_ERR_UNSUPPORTED, "no fixedwing hover task in the reference");
  if (P.task == PF_TASK_DOGFIGHT) {  // ma_fixedwing_dogfight_env.py
    if (P.vehicle != PF_FIXEDWING) return fail(nullptr, PF_ERR_UNSUPPORTED, "the dogfight task flies fixedwing aircraft (ma_fixedwing_base_env.py:201)");
    if (P.df_team_size < 1 || 2 * P.df_team_size > pf::kDfMaxAgents || P.agents_per_world != 2 * P.df_team_size)
      return fail(nullptr, PF_ERR_ARG, "dogfight: agents_per_world must be 2 * df_team_size, at most 8");
    if (P.autoreset != PF_AUTORESET_OFF) return fail(nullptr, PF_ERR_ARG, "the multi-agent env has no auto-reset (PettingZoo parallel API)");
    if (P.angle_repr != 0) return fail(nullptr, PF_ERR_UNSUPPORTED, "the dogfight env observes Euler angles (ma_fixedwing_dogfight_env.py:92)");
    if (P.n_surf != PF_MAX_SURF || P.n_motors != 1) return fail(nullptr, PF_ERR_ARG, "dogfight: a five-surface, one-motor airframe");
    if (P.df_action_dim != 0 && P.df_action_dim != 4 && P.df_action_dim != 6) return fail(nullptr, PF_ERR_ARG, "dogfight: df_action_dim is 4 or 6");
  }
  if (P.agents_per_world > 1) {
    if (!((P.vehicle == PF_QUADX && P.task == PF_TASK_MA_HOVER) || P.task == PF_TASK_DOGFIGHT || (P.task == PF_TASK_NONE && P.vehicle != PF_ROCKET)))
      return fail(nullptr, PF_ERR_UNSUPPORTED, "agents_per_world > 1 (a shared world) exists for the Aviary (QuadX, Fixedwing) and the PettingZoo tasks (QuadX hover, fixedwing dogfight)");
    if ((P.task != PF_TASK_DOGFIGHT && 64 % P.agents_per_world != 0) || n_lanes % P.agents_per_world != 0)
      return fail(nullptr, PF_ERR_ARG, "agents_per_world must divide 64 (the lanes of a world share a wavefront) and the lane count");
    // (the pair stage keeps one deepest-contact slot per agent of a world in registers: shared_world.hpp, pair_stage_dev)
    if (P.agents_per_world > 8) return fail(nullptr, PF_ERR_UNSUPPORTED, "a shared world holds at most 8 agents (ORC_MAX_WORLD in the oracle)");
    for (int k = 0; k < P.n_boxes; ++k)
      if (P.boxes[k].kind != 0 || P.boxes[k].yaw != 0.0f)
        return fail(nullptr, PF_ERR_UNSUPPORTED, "shared worlds test plain box colliders against each other (cf2x); this airframe has cylinders / yawed boxes");
  }
  if (P.use_yaw_targets && !(P.vehicle == PF_QUADX && P.task == PF_TASK_WAYPOINTS))
    return fail(nullptr, PF_ERR_UNSUPPORTED, "use_yaw_targets exists for QuadX-Waypoints only (fixedwing_waypoints_env.py:77 hard-wires False)");
  if (P.task == PF_TASK_MA_HOVER && P.autoreset != PF_AUTORESET_OFF) return fail(nullptr, PF_ERR_ARG, "the multi-agent env has no auto-reset (PettingZoo parallel API)");
  if (P.task != PF_TASK_NONE && P.vehicle == PF_FIXEDWING && P.flight_mode != 0) return fail(nullptr, PF_ERR_UNSUPPORTED, "fixedwing env uses flight_mode 0");
  // quat_integrate()'s polynomial range: |w| dt / 2 <= pi/8 given the per-coordinate clamp
  if (1.7320508f * P.max_coord_vel * P.dt * 0.5f > 0.3926991f + 1e-6f)
    return fail(nullptr, PF_ERR_UNSUPPORTED, "max_coord_vel * dt too large for the exponential-map polynomial");
  if (P.ticks_per_control < 1 || P.env_step_ratio < 0 || P.n_boxes > PF_MAX_BOXES) return fail(nullptr, PF_ERR_ARG, "bad loop constants");
  // the contact model's parameters (params.py: build_params checks the same for Python callers; a C caller gets the same answer
  // here): a negative residual threshold is sqrt -> NaN and ends every solve after one sweep, negative distances shrink the slab,
  // a manifold size other than 4 or 8 would be mapped silently
  if (P.contact_manifold_points != 4 && P.contact_manifold_points != 8) return fail(nullptr, PF_ERR_ARG, "contact_manifold_points must be 4 or 8");
  if (P.contact_response && P.contact_iters < 1) return fail(nullptr, PF_ERR_ARG, "contact_iters must be at least 1");
  if (!(P.contact_residual_threshold >= 0.0f) || !(P.contact_report_distance >= 0.0f) || !(P.contact_break_distance >= 0.0f) ||
      !(P.contact_margin >= 0.0f) || !(P.contact_slop >= 0.0f) || !(P.contact_erp >= 0.0f) || !(P.contact_friction >= 0.0f) ||
      !(P.contact_restitution >= 0.0f))
    return fail(nullptr, PF_ERR_ARG, "the contact model's distances, threshold, erp, friction and restitution must be >= 0");
  pf_ctx* c = new (std::nothrow) pf_ctx;
  if (!c) return fail(nullptr, PF_ERR_ARG, "out of host memory");
  c->P = P; c->n = n_lanes; c->device = device; c->lane0 = lane_offset; c->err[0] = 0; c->launch_ctr = nullptr; c->policy_dev = nullptr; c->ts_scratch = nullptr; c->ppo_scratch = nullptr; c->sync_latch = nullptr;
  {  // the airframe's worst-case contact count (collider vertices), see pf_params.contact_max_points
    int pts = 0;
    for (int k = 0; k < P.n_boxes; ++k) pts += P.boxes[k].kind == 1 ? 16 : (P.contact_manifold_points >= 8 ? 8 : 4);
    c->P.contact_max_points = pts < 1 ? 1 : (pts > PF_MAX_CONTACTS ? PF_MAX_CONTACTS : pts);
  }
  c->P_dev = nullptr; c->tmpl = nullptr; c->surf_dev = nullptr;
  pf::FwTable fsurf;
  c->ek = select_env_kernel(P, n_lanes, device, c->K, c->FK, fsurf);
  {
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || cus < 1) cus = 256;
    c->act_grid_cap = 2 * cus;
  }
  const env_family fam = c->ek.family;
  {  // device copy of the parameter block (LDS constant tables, the out-of-line floor test)
    int cur = -1;
    (void)hipGetDevice(&cur);
    (void)hipSetDevice(device);
    // (behind the block: what the specialised QuadX kernel's in-register floor solve reads -- quadx_fast.hpp: quad_solve_consts)
    hipError_t e = hipMalloc((void**)&c->P_dev, pf::kQuadSolveOffset + sizeof(float) * pf::kQuadSolveWords);
    if (e == hipSuccess) e = hipMemcpy(c->P_dev, &c->P, sizeof(pf_params), hipMemcpyHostToDevice);
    if (e == hipSuccess) {
      float sw[pf::kQuadSolveWords] = {0};
      if (fam == env_family::quadx) pf::quad_solve_words(c->P, sw);
      e = hipMemcpy(reinterpret_cast<char*>(c->P_dev) + pf::kQuadSolveOffset, sw, sizeof(sw), hipMemcpyHostToDevice);
    }
    if (e == hipSuccess && fam == env_family::quadx) {  // (quadx_fast.hpp: launch_ctr)
      const size_t words = (size_t)pf::kCtrStride * (((size_t)n_lanes + 63) / 64);
      e = hipMalloc((void**)&c->launch_ctr, sizeof(uint32_t) * words);
      if (e == hipSuccess) e = hipMemset(c->launch_ctr, 0, sizeof(uint32_t) * words);
      if (e == hipSuccess) e = hipMalloc((void**)&c->policy_dev, sizeof(float) * pf::kPolWords);
    }
    if (e == hipSuccess && (fam == env_family::fixedwing_wp || fam == env_family::dogfight_fast)) {
      e = hipMalloc((void**)&c->surf_dev, sizeof(fsurf));
      if (e == hipSuccess) e = hipMemcpy(c->surf_dev, &fsurf, sizeof(fsurf), hipMemcpyHostToDevice);
    }
    if (e == hipSuccess && fam != env_family::none)
      e = hipMalloc((void**)&c->ts_scratch, sizeof(double) * pf::ts_scratch_words(n_lanes, pf_obs_dim(c)));
    if (e == hipSuccess) e = hipMalloc((void**)&c->ppo_scratch, sizeof(double) * pf::kPpoScratchWords);
    if (e == hipSuccess) e = hipMalloc((void**)&c->sync_latch, (size_t)n_lanes);
    if (cur >= 0) (void)hipSetDevice(cur);
    if (e != hipSuccess) { if (c->P_dev) hipFree(c->P_dev); if (c->launch_ctr) hipFree(c->launch_ctr); if (c->policy_dev) hipFree(c->policy_dev); if (c->surf_dev) hipFree(c->surf_dev); if (c->ts_scratch) hipFree(c->ts_scratch); if (c->ppo_scratch) hipFree(c->ppo_scratch); if (c->sync_latch) hipFree(c->sync_latch); delete c; return hip_fail(nullptr, e, "pf_ctx_create: device parameter block"); }
  }
  if ((fam == env_family::fixedwing_wp || fam == env_family::generic) && (P.task == PF_TASK_HOVER || P.task == PF_TASK_WAYPOINTS) &&
      (P.vehicle == PF_FIXEDWING || P.noise_mode == PF_NOISE_OFF)) {
    // the settle phase cannot depend on the lane (fixedwing: throttle command 0 during settle, so the
    // motor noise scales nothing; or noise off): settle once here, resets copy the result
    int cur = -1;
    hipGetDevice(&cur);
    hipSetDevice(device);
    const int groups = P.vehicle == PF_QUADX ? pf::QuadX::GROUPS : pf::Fixedwing::GROUPS;
    hipError_t e = hipMalloc((void**)&c->tmpl, sizeof(float4) * groups);
    if (e == hipSuccess) e = hipMemset(c->tmpl, 0, sizeof(float4) * groups);
    if (e == hipSuccess) {
      hipLaunchKernelGGL(vehicle_kernel(c, pf::settle_template_kernel<pf::QuadX>, pf::settle_template_kernel<pf::Fixedwing>), dim3(1), dim3(64), 0, 0, c->P,
                         c->tmpl, c->P_dev);
      e = hipDeviceSynchronize();
    }
    if (cur >= 0) hipSetDevice(cur);
    if (e != hipSuccess) { if (c->tmpl) hipFree(c->tmpl); if (c->surf_dev) hipFree(c->surf_dev); if (c->ts_scratch) hipFree(c->ts_scratch); if (c->ppo_scratch) hipFree(c->ppo_scratch); if (c->sync_latch) hipFree(c->sync_latch); hipFree(c->P_dev); delete c; return hip_fail(nullptr, e, "pf_ctx_create: settle template"); }
  }
  *out = c;
  return PF_OK;
}
void pf_ctx_destroy(pf_ctx* ctx) {
  if (!ctx) return;
  if (ctx->P_dev) hipFree(ctx->P_dev);
  if (ctx->launch_ctr) hipFree(ctx->launch_ctr);
  if (ctx->policy_dev) hipFree(ctx->policy_dev);
  if (ctx->tmpl) hipFree(ctx->tmpl);
  if (ctx->surf_dev) hipFree(ctx->surf_dev);
  if (ctx->ts_scratch) hipFree(ctx->ts_scratch);
  if (ctx->ppo_scratch) hipFree(ctx->ppo_scratch);
  if (ctx->sync_latch) hipFree(ctx->sync_latch);
  delete ctx;
}
int pf_state_groups(const pf_ctx* ctx) {
  const env_family f = ctx->ek.family;
  if (f == env_family::dogfight_fast || f == env_family::dogfight_generic) return pf::kDfGroups;
  if (f == env_family::rocket_landing) return pf::kRlGroups;
  // (the specialised QuadX kernel in a cascaded flight mode, no shared world: eleven more groups, the float32 remainders of its fp64
  //  rigid-body state and PID memories -- quadx_fast.hpp: QuadStateD)
  if (f == env_family::quadx && ctx->K.mode != 0 && ctx->K.apw == 1) return pf::QuadX::GROUPS + 11;  // (16-19 state, 20-21 rate PID, 22-26 cascade)
  return ctx->P.vehicle == PF_QUADX ? pf::QuadX::GROUPS : (ctx->P.vehicle == PF_ROCKET ? pf::Rocket::GROUPS : pf::Fixedwing::GROUPS);
}
int pf_obs_dim(const pf_ctx* ctx) {
  const pf_params& P = ctx->P;
  if (P.task == PF_TASK_DOGFIGHT) return 19 + (P.df_action_dim == 6 ? 6 : 4) + (P.agents_per_world - 1) * 14;  // ma_fixedwing_dogfight_env.py:128-160
  if (P.task == PF_TASK_ROCKET_LANDING) return (P.angle_repr ? 13 : 12) + pf::kRlActionDim + pf::Rocket::AUX + 1;  // rocket_landing_env.py:141-169
  int aux = P.vehicle == PF_QUADX ? 4 : 6;
  return (P.angle_repr ? 13 : 12) + 4 + aux + (P.task == PF_TASK_WAYPOINTS ? (P.use_yaw_targets ? 4 : 3) * P.num_targets : (P.task == PF_TASK_MA_HOVER ? 3 : 0));
}
int pf_n_lanes(const pf_ctx* ctx) { return ctx->n; }
int pf_ctx_is_specialised(const pf_ctx* ctx) {
  const env_family f = ctx->ek.family;
  return f == env_family::quadx ? 1 : ((f == env_family::fixedwing_wp || f == env_family::dogfight_fast) ? 2 : 0);
}
int pf_ctx_step_is_fixed(const pf_ctx* ctx) { return ctx->ek.family == env_family::quadx && ctx->ek.fixed ? 1 : 0; }

static int env_reset_or_step(pf_ctx* ctx, const pf_buffers* b, int op, const uint8_t* mask, void* stream) {
  if (!ctx || !b || !b->state || !b->obs) return fail(ctx, PF_ERR_ARG, "pf_env_*: state and obs buffers are required");
  const pf_params& P = ctx->P;
  if (P.task == PF_TASK_NONE) return fail(ctx, PF_ERR_ARG, "pf_env_*: context has no env task (use the pf_aviary_* calls)");
  if (op == pf::OP_STEP && (!b->actions || !b->reward || !b->terminated || !b->truncated))
    return fail(ctx, PF_ERR_ARG, "pf_env_step: actions/reward/terminated/truncated buffers are required");
  if (P.noise_mode == PF_NOISE_INJECT && ((op == pf::OP_STEP && !b->xi) || !b->xi_reset))
    if (!(op == pf::OP_STEP && P.autoreset == PF_AUTORESET_OFF && b->xi))
      return fail(ctx, PF_ERR_ARG, "PF_NOISE_INJECT needs xi (step) and xi_reset (reset/auto-reset)");
  return launch_env(ctx, b, op, mask, 0, 1, 0u, stream);
}
int pf_env_reset(pf_ctx* ctx, const pf_buffers* b, const uint8_t* mask, void* stream) {
  return env_reset_or_step(ctx, b, pf::OP_RESET, mask, stream);
}
int pf_env_step(pf_ctx* ctx, const pf_buffers* b, void* stream) { return env_reset_or_step(ctx, b, pf::OP_STEP, nullptr, stream); }

int pf_aviary_reset(pf_ctx* ctx, const pf_buffers* b, void* stream) {
  if (!ctx || !b || !b->state) return fail(ctx, PF_ERR_ARG, "pf_aviary_reset: state buffer required");
  int rc = ensure_device(ctx);
  if (rc) return rc;
  const int grid = (ctx->n + pf::kWave - 1) / pf::kWave;
  hipStream_t s = (hipStream_t)stream;
  const float* pose = b->start_pose;
  const auto kernel = vehicle_kernel(ctx, pf::aviary_reset_kernel<pf::QuadX>, pf::aviary_reset_kernel<pf::Fixedwing>, pf::aviary_reset_kernel<pf::Rocket>);
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(pf::kWave), 0, s, ctx->P, *b, ctx->n, pose);
  ctx->P.flight_mode = 0;  // drone.reset() -> set_mode(0) (quadx.py:224, fixedwing.py:196)
  PF_HIP(ctx, hipGetLastError());
  return PF_OK;
}
int pf_aviary_set_mode(pf_ctx* ctx, const pf_buffers* b, int mode, float* setpoints_out, void* stream) {
  if (!ctx || !b || !b->state) return fail(ctx, PF_ERR_ARG, "pf_aviary_set_mode: state buffer required");
  if (ctx->P.vehicle == PF_QUADX && (mode < -1 || mode > 7)) return fail(ctx, PF_ERR_ARG, "`mode` must be between -1 and 7");
  if (ctx->P.vehicle == PF_FIXEDWING && (mode < -1 || mode > 0)) return fail(ctx, PF_ERR_ARG, "`mode` must be between -1 and 0");
  if (ctx->P.vehicle == PF_ROCKET && mode != 0) return fail(ctx, PF_ERR_ARG, "`mode` must be 0 (rocket.py:238-247)");
  if (b->modes && ctx->P.vehicle != PF_QUADX) return fail(ctx, PF_ERR_UNSUPPORTED, "per-drone flight modes are supported for QuadX only (Fixedwing modes differ in setpoint width)");
  int rc = ensure_device(ctx);
  if (rc) return rc;
  const int grid = (ctx->n + pf::kWave - 1) / pf::kWave;
  hipStream_t s = (hipStream_t)stream;
  const int sp_dim = pf::setpoint_width(ctx->P.vehicle, mode);
  const auto kernel = vehicle_kernel(ctx, pf::aviary_set_mode_kernel<pf::QuadX>, pf::aviary_set_mode_kernel<pf::Fixedwing>, pf::aviary_set_mode_kernel<pf::Rocket>);
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(pf::kWave), 0, s, ctx->P, *b, ctx->n, sp_dim, mode, setpoints_out);
  ctx->P.flight_mode = mode;
  PF_HIP(ctx, hipGetLastError());
  return PF_OK;
}
int pf_aviary_step(pf_ctx* ctx, const pf_buffers* b, int n_steps, void* stream) {
  if (!ctx || !b || !b->state || !b->setpoints) return fail(ctx, PF_ERR_ARG, "pf_aviary_step: state and setpoints required");
  if (n_steps < 1) return fail(ctx, PF_ERR_ARG, "pf_aviary_step: n_steps must be >= 1");
  if (ctx->P.noise_mode == PF_NOISE_INJECT && !b->xi) return fail(ctx, PF_ERR_ARG, "PF_NOISE_INJECT needs xi");
  int rc = ensure_device(ctx);
  if (rc) return rc;
  const int grid = (ctx->n + pf::kWave - 1) / pf::kWave;
  hipStream_t s = (hipStream_t)stream;
  const auto kernel = ctx->P.agents_per_world > 1  // shared worlds (pf_ctx_create admitted QuadX / Fixedwing with plain boxes only)
                          ? vehicle_kernel(ctx, pf::aviary_world_step_kernel<pf::QuadX>, pf::aviary_world_step_kernel<pf::Fixedwing>)
                          : vehicle_kernel(ctx, pf::aviary_step_kernel<pf::QuadX>, pf::aviary_step_kernel<pf::Fixedwing>, pf::aviary_step_kernel<pf::Rocket>);
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(pf::kWave), 0, s, ctx->P, *b, ctx->n, ctx->lane0, n_steps, ctx->P_dev);
  PF_HIP(ctx, hipGetLastError());
  return PF_OK;
}
int pf_aviary_tick(pf_ctx* ctx, const pf_buffers* b, int tick_index, void* stream) {
  if (!ctx || !b || !b->state || !b->setpoints) return fail(ctx, PF_ERR_ARG, "pf_aviary_tick: state and setpoints buffers are required");
  if (tick_index < 0 || tick_index >= ctx->P.ticks_per_control) return fail(ctx, PF_ERR_ARG, "pf_aviary_tick: tick_index must be in [0, ticks_per_control)");
  if (ctx->P.agents_per_world > 1) return fail(ctx, PF_ERR_UNSUPPORTED, "pf_aviary_tick: no per-tick protocol (wind field) in shared worlds; use pf_aviary_step");
  if (ctx->P.noise_mode == PF_NOISE_INJECT && !b->xi) return fail(ctx, PF_ERR_ARG, "pf_aviary_tick: PF_NOISE_INJECT needs b->xi");
  int rc = ensure_device(ctx);
  if (rc) return rc;
  const int grid = (ctx->n + pf::kWave - 1) / pf::kWave;
  hipStream_t s = (hipStream_t)stream;
  const auto kernel = vehicle_kernel(ctx, pf::aviary_tick_kernel<pf::QuadX>, pf::aviary_tick_kernel<pf::Fixedwing>, pf::aviary_tick_kernel<pf::Rocket>);
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(pf::kWave), 0, s, ctx->P, *b, ctx->n, ctx->lane0, tick_index, ctx->P_dev);
  PF_HIP(ctx, hipGetLastError());
  return PF_OK;
}
int pf_wind_links(const pf_ctx* ctx) {
  return ctx->P.vehicle == PF_QUADX ? pf::QuadX::WIND_LINKS : (ctx->P.vehicle == PF_ROCKET ? pf::Rocket::WIND_LINKS : pf::Fixedwing::WIND_LINKS);
}
int pf_sample_actions(pf_ctx* ctx, float* actions, uint32_t step_index, void* stream) {
  if (!ctx || !actions) return fail(ctx, PF_ERR_ARG, "pf_sample_actions: bad argument");
  int rc = ensure_device(ctx);
  if (rc) return rc;
  if (ctx->P.task == PF_TASK_ROCKET_LANDING)
    hipLaunchKernelGGL(pf::sample_actions7_kernel, dim3((ctx->n + 255) / 256), dim3(256), 0, (hipStream_t)stream, ctx->P, actions, ctx->n, ctx->lane0, step_index);
  else
    hipLaunchKernelGGL(pf::sample_actions_kernel, dim3((ctx->n + 255) / 256), dim3(256), 0, (hipStream_t)stream, ctx->P, actions, ctx->n, ctx->lane0, step_index);
  PF_HIP(ctx, hipGetLastError());
  return PF_OK;
}

int pf_rollout(pf_ctx* ctx, const pf_buffers* b, int k_steps, uint32_t step_index0, void* stream) {
  if (!ctx || !b || !b->state || !b->obs || !b->reward || !b->terminated || !b->truncated)
    return fail(ctx, PF_ERR_ARG, "pf_rollout: state, obs, reward, terminated and truncated buffers are required");
  if (k_steps < 1) return fail(ctx, PF_ERR_ARG, "pf_rollout: k_steps must be >= 1");
  const pf_params& P = ctx->P;
  const env_family f = ctx->ek.family;
  if (P.noise_mode == PF_NOISE_INJECT) return fail(ctx, PF_ERR_UNSUPPORTED, "pf_rollout: PF_NOISE_INJECT is a per-step protocol; use pf_env_step");
  if (P.task == PF_TASK_NONE) return fail(ctx, PF_ERR_UNSUPPORTED, "pf_rollout: this context has no env task");
  // Every env kernel is state-resident in a rollout: one launch for the k_steps (the dogfight on either aircraft model: four-wide
  // actions sampled on device, or the given sequence of either width; the generic env kernel: roll_steps)
  if ((f == env_family::dogfight_fast || f == env_family::dogfight_generic) && !b->actions && P.df_action_dim == 6)
    return fail(ctx, PF_ERR_UNSUPPORTED, "pf_rollout: on-device sampling draws four-wide actions; pass the six-wide sequence in b->actions");
  // (the PettingZoo task has no auto-reset: finished agents are culled by the caller, their drones fly on in the shared world)
  if ((f == env_family::quadx || f == env_family::fixedwing_wp) && P.autoreset == PF_AUTORESET_OFF && P.task != PF_TASK_MA_HOVER)
    return fail(ctx, PF_ERR_UNSUPPORTED, "pf_rollout: needs an auto-reset mode (finished lanes would idle for the rest of the launch)");
  return launch_env(ctx, b, pf::OP_STEP, nullptr, b->actions ? 2 : 1, k_steps, step_index0, stream);
}

// ---- what the training-side entry points below share: refusals, argument tables, the policy network's checks, policy_act_kernel's launch
// a refusal with the text "<who>: <what>"; arg_fail: the usual code
static int who_fail(pf_ctx* ctx, int code, const char* who, const char* what) {
  char buf[256];
  snprintf(buf, sizeof(buf), "%s: %s", who, what);
  return fail(ctx, code, buf);
}
static int arg_fail(pf_ctx* ctx, const char* who, const char* what) { return who_fail(ctx, PF_ERR_ARG, who, what); }
// a call's required pointers, a table that ends with a null name: the first missing one is refused as "<who>: <name> is required"
struct arg_ptr {
  const char* name;
  const void* p;
};
static int require_args(pf_ctx* ctx, const char* who, const arg_ptr* args) {
  for (; args->name; ++args)
    if (!args->p) {
      char what[64];
      snprintf(what, sizeof(what), "%s is required", args->name);
      return arg_fail(ctx, who, what);
    }
  return PF_OK;
}
struct arg_span {
  const char* name;
  const void* p;
  size_t bytes;
};
// the first pair of spans that share a byte, or null; the spans before `first_written` are only read and may share bytes with one another
static const char* spans_overlap(const arg_span* s, int count, char* buf, size_t len, int first_written = 0) {
  for (int i = 0; i < count; ++i)
    for (int j = i + 1 > first_written ? i + 1 : first_written; j < count; ++j) {
      const uintptr_t a = (uintptr_t)s[i].p, b = (uintptr_t)s[j].p;
      if (a < b + s[j].bytes && b < a + s[i].bytes) {
        snprintf(buf, len, "%s and %s overlap", s[i].name, s[j].name);
        return buf;
      }
    }
  return nullptr;
}
// what pf_rollout_policy and pf_policy_act check of the network, in this order
static int policy_net_check(pf_ctx* ctx, const char* who, const pf_policy* q) {
  if (q->n_layers != 2 && q->n_layers != 3) return arg_fail(ctx, who, "n_layers must be 2 or 3");
  for (int l = 0; l + 1 < q->n_layers; ++l) {
    if (q->width[l] > PF_POLICY_MAX_HIDDEN) return who_fail(ctx, PF_ERR_UNSUPPORTED, who, "hidden widths over PF_POLICY_MAX_HIDDEN (64) are not supported");
    if (q->width[l] < 1) return arg_fail(ctx, who, "hidden widths must be >= 1");
  }
  if (q->activation != PF_ACT_TANH && q->activation != PF_ACT_RELU) return arg_fail(ctx, who, "activation must be PF_ACT_TANH or PF_ACT_RELU");
  for (int l = 0; l < q->n_layers; ++l)
    if (!q->w[l] || !q->b[l]) return arg_fail(ctx, who, "every layer needs w and b");
  return PF_OK;
}
// the env's action width: what pf_policy_act writes per row and pf_gae's log-probabilities sum over
static int env_action_dim(const pf_params& P) { return P.task == PF_TASK_ROCKET_LANDING ? pf::kRlActionDim : (P.task == PF_TASK_DOGFIGHT && P.df_action_dim == 6) ? 6 : 4; }
static_assert(pf::kRlActionDim <= pf::kActMaxA, "the output layer's block holds the widest action");
// policy_act_kernel's one launch site: workgroups stride over the 64-row tiles, two per CU at the most (all resident), so the weight staging is paid once per workgroup
static int launch_policy_act(pf_ctx* ctx, const pf::ActK& AK, int64_t rows, void* stream) {
  const int64_t tiles = (rows + pf::kActRows - 1) / pf::kActRows;
  const int grid = tiles < (int64_t)ctx->act_grid_cap ? (int)tiles : ctx->act_grid_cap;
  hipLaunchKernelGGL(pf::policy_act_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, AK);
  PF_HIP(ctx, hipGetLastError());
  return PF_OK;
}

int pf_rollout_policy(pf_ctx* ctx, const pf_buffers* b, const pf_policy* q, int k_steps, uint32_t step_index0, void* stream) {
  if (!ctx || !b || !q || !b->state || !b->obs || !b->reward || !b->terminated || !b->truncated)
    return fail(ctx, PF_ERR_ARG, "pf_rollout_policy: policy, state, obs, reward, terminated and truncated buffers are required");
  if (k_steps < 1) return fail(ctx, PF_ERR_ARG, "pf_rollout_policy: k_steps must be >= 1");
  if (b->actions) return fail(ctx, PF_ERR_ARG, "pf_rollout_policy: b->actions must be NULL (the policy computes the actions; b->actions_out receives them)");
  const pf_params& P = ctx->P;
  const env_choice& c = ctx->ek;
  if (P.vehicle != PF_QUADX || (P.task != PF_TASK_HOVER && P.task != PF_TASK_WAYPOINTS))
    return fail(ctx, PF_ERR_UNSUPPORTED, "pf_rollout_policy: QuadX-Hover and QuadX-Waypoints only (no on-device policy for this task / vehicle)");
  if (c.family != env_family::quadx)
    return fail(ctx, PF_ERR_UNSUPPORTED, "pf_rollout_policy: needs the specialised QuadX kernel (pf_ctx_is_specialised() == 1); this context runs the generic one");
  if (c.md) return fail(ctx, PF_ERR_UNSUPPORTED, "pf_rollout_policy: flight mode 0 only (no instantiation with the cascaded flight modes)");
  // (shared worlds exist for PF_TASK_MA_HOVER and the dogfight only: refused by the task check above)
  if (P.noise_mode == PF_NOISE_INJECT) return fail(ctx, PF_ERR_UNSUPPORTED, "pf_rollout_policy: PF_NOISE_INJECT is a per-step protocol; use pf_env_step");
  if (P.autoreset == PF_AUTORESET_OFF)
    return fail(ctx, PF_ERR_UNSUPPORTED, "pf_rollout_policy: needs an auto-reset mode (auto-reset OFF: finished lanes would idle for the rest of the launch)");
  // (the contact response with every vertex in the manifold runs the out-of-line solve, whose argument block is stack: no zero-scratch instantiation)
  if (c.cr && P.contact_manifold_points >= 8)
    return fail(ctx, PF_ERR_UNSUPPORTED, "pf_rollout_policy: contact_response with contact_manifold_points = 8 is not supported (the in-register floor solve holds the 4-point manifold)");
  if (int rc = policy_net_check(ctx, "pf_rollout_policy", q)) return rc;
  if (!q->obs0) return fail(ctx, PF_ERR_ARG, "pf_rollout_policy: obs0 (the observation the previous call left) is required");
  const int D = pf_obs_dim(ctx);
  if (D > pf::kPolMaxIn) return fail(ctx, PF_ERR_UNSUPPORTED, "pf_rollout_policy: observation wider than the first layer's block");
  int rc = ensure_device(ctx);
  if (rc) return rc;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(pf::policy_pack_kernel, dim3(1), dim3(256), 0, s, *q, D, ctx->policy_dev);
  const pf::PolicyK PK{ctx->policy_dev, q->obs0, q->mean_out, q->n_layers, q->activation, q->log_std != nullptr ? 1 : 0};
  const bool philox = P.noise_mode == PF_NOISE_PHILOX;
  const auto kernel = P.task == PF_TASK_HOVER ? quadx_policy_kernel<PF_TASK_HOVER>(philox, c.cr) : quadx_policy_kernel<PF_TASK_WAYPOINTS>(philox, c.cr);
  const int grid = (ctx->n + 64 * pf::kQuadWPB - 1) / (64 * pf::kQuadWPB);
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(64 * pf::kQuadWPB), 0, s, ctx->K, *b, ctx->P_dev, ctx->n, ctx->lane0, (int)pf::OP_STEP, (const uint8_t*)nullptr,
                     k_steps, step_index0, ctx->launch_ctr, PK);
  PF_HIP(ctx, hipGetLastError());
  return PF_OK;
}
int pf_policy_act(pf_ctx* ctx, const pf_policy* q, float* actions_out, uint32_t step_index, void* stream) {
  if (!ctx) return fail(ctx, PF_ERR_ARG, "pf_policy_act: ctx is required");
  if (!q) return fail(ctx, PF_ERR_ARG, "pf_policy_act: policy is required");
  const pf_params& P = ctx->P;
  if (P.task == PF_TASK_NONE) return fail(ctx, PF_ERR_UNSUPPORTED, "pf_policy_act: needs a context with an env task (this one drives the Aviary level only)");
  if (!actions_out) return fail(ctx, PF_ERR_ARG, "pf_policy_act: actions_out is required");
  if (!q->obs0) return fail(ctx, PF_ERR_ARG, "pf_policy_act: obs0 (the [n][pf_obs_dim()] input rows) is required");
  if (int rc = policy_net_check(ctx, "pf_policy_act", q)) return rc;
  const int D = pf_obs_dim(ctx);
  if (D > pf::kActMaxIn) return fail(ctx, PF_ERR_UNSUPPORTED, "pf_policy_act: observation wider than 128");
  int rc = ensure_device(ctx);
  if (rc) return rc;
  const pf::ActK AK{*q, actions_out, ctx->n, D, env_action_dim(P), (uint32_t)P.seed, (uint32_t)(P.seed >> 32), step_index, ctx->lane0};
  return launch_policy_act(ctx, AK, ctx->n, stream);
}
int pf_gae(pf_ctx* ctx, const pf_gae_args* a, int k_steps, void* stream) {
  if (!ctx || !a) return fail(ctx, PF_ERR_ARG, "pf_gae: ctx and the argument block are required");
  const pf_params& P = ctx->P;
  if (P.task == PF_TASK_NONE) return fail(ctx, PF_ERR_UNSUPPORTED, "pf_gae: needs a context with an env task (this one drives the Aviary level only)");
  if (k_steps < 1) return fail(ctx, PF_ERR_ARG, "pf_gae: k_steps must be >= 1");
  const arg_ptr required[] = {{"reward", a->reward}, {"terminated", a->terminated}, {"truncated", a->truncated}, {"values", a->values},
                              {"advantages", a->advantages}, {"returns", a->returns}, {nullptr, nullptr}};
  if (int rc = require_args(ctx, "pf_gae", required)) return rc;
  if (!(a->gamma >= 0.0f && a->gamma <= 1.0f)) return fail(ctx, PF_ERR_ARG, "pf_gae: gamma must be finite and in [0, 1]");
  if (!(a->lambda >= 0.0f && a->lambda <= 1.0f)) return fail(ctx, PF_ERR_ARG, "pf_gae: lambda must be finite and in [0, 1]");
  if (P.autoreset == PF_AUTORESET_SAME_STEP && !a->final_values)
    return fail(ctx, PF_ERR_ARG, "pf_gae: final_values is required under SAME_STEP (the value of the terminal observation in final_obs)");
  if (P.autoreset != PF_AUTORESET_SAME_STEP && a->final_values)
    return fail(ctx, PF_ERR_ARG, "pf_gae: final_values must be NULL outside SAME_STEP (there is no final_obs)");
  if (P.autoreset != PF_AUTORESET_NEXT_STEP && a->episode_start)
    return fail(ctx, PF_ERR_ARG, "pf_gae: episode_start must be NULL outside NEXT_STEP (no other mode has reset steps)");
  const int n_logp = (a->actions != nullptr) + (a->mean != nullptr) + (a->log_std != nullptr) + (a->logp_out != nullptr);
  if (n_logp != 0 && n_logp != 4)
    return fail(ctx, PF_ERR_ARG, "pf_gae: actions, mean, log_std and logp_out come together or are all NULL");
  int rc = ensure_device(ctx);
  if (rc) return rc;
  hipStream_t s = (hipStream_t)stream;
  const pf::GaeK K{a->gamma, a->lambda, a->reward, a->terminated, a->truncated, a->values, a->final_values, a->episode_start,
                   a->advantages, a->returns, a->valid_out};
  const auto scan = P.autoreset == PF_AUTORESET_NEXT_STEP   ? pf::gae_scan_kernel<PF_AUTORESET_NEXT_STEP>
                    : P.autoreset == PF_AUTORESET_SAME_STEP ? pf::gae_scan_kernel<PF_AUTORESET_SAME_STEP>
                                                            : pf::gae_scan_kernel<PF_AUTORESET_OFF>;
  hipLaunchKernelGGL(scan, dim3((ctx->n + 63) / 64), dim3(64), 0, s, K, ctx->n, k_steps);
  if (n_logp) {
    const int width = env_action_dim(P);
    const size_t rows = (size_t)k_steps * (size_t)ctx->n;
    const size_t blocks = (rows + pf::kGaeLogpBlock - 1) / pf::kGaeLogpBlock;
    const dim3 grid((unsigned)(blocks < (size_t)pf::kGaeLogpMaxGrid ? blocks : (size_t)pf::kGaeLogpMaxGrid));
    // (one float4 per row where the rows are four wide and the caller's pointers allow it; the same arithmetic either way)
    const bool vec = width == 4 && (((uintptr_t)a->actions | (uintptr_t)a->mean) & 15) == 0;
    hipLaunchKernelGGL(vec ? pf::gae_logp_kernel<true> : pf::gae_logp_kernel<false>, grid, dim3(pf::kGaeLogpBlock), 0, s, a->actions, a->mean,
                       a->log_std, a->logp_out, rows, width);
  }
  PF_HIP(ctx, hipGetLastError());
  return PF_OK;
}
int pf_traj_stats(pf_ctx* ctx, const pf_traj_stats_args* a, int k_steps, void* stream) {
  if (!ctx || !a) return fail(ctx, PF_ERR_ARG, "pf_traj_stats: ctx and the argument block are required");
  const pf_params& P = ctx->P;
  if (P.task == PF_TASK_NONE) return fail(ctx, PF_ERR_UNSUPPORTED, "pf_traj_stats: needs a context with an env task (this one drives the Aviary level only)");
  if (k_steps < 1) return fail(ctx, PF_ERR_ARG, "pf_traj_stats: k_steps must be >= 1");
  const arg_ptr required[] = {{"reward", a->reward}, {"terminated", a->terminated}, {"truncated", a->truncated}, {"summary", a->summary},
                              {"carry_return", a->carry_return}, {"carry_length", a->carry_length}, {"carry_disc", a->carry_disc}, {nullptr, nullptr}};
  if (int rc = require_args(ctx, "pf_traj_stats", required)) return rc;
  if (!(a->gamma >= 0.0f && a->gamma <= 1.0f)) return fail(ctx, PF_ERR_ARG, "pf_traj_stats: gamma must be finite and in [0, 1]");
  if (P.autoreset != PF_AUTORESET_NEXT_STEP && a->episode_start)
    return fail(ctx, PF_ERR_ARG, "pf_traj_stats: episode_start must be NULL outside NEXT_STEP (no other mode has reset steps)");
  if (a->obs && !a->obs_moments) return fail(ctx, PF_ERR_ARG, "pf_traj_stats: obs comes with obs_moments (the block its moments are merged into)");
  if (!a->obs && a->obs_moments) return fail(ctx, PF_ERR_ARG, "pf_traj_stats: obs_moments comes with obs");
  const int D = pf_obs_dim(ctx);
  if (a->obs && D > pf::kTsMaxD) return fail(ctx, PF_ERR_UNSUPPORTED, "pf_traj_stats: observation rows wider than 128 have no moments kernel");
  int rc = ensure_device(ctx);
  if (rc) return rc;
  hipStream_t s = (hipStream_t)stream;
  const bool next = P.autoreset == PF_AUTORESET_NEXT_STEP;
  const int waves = (ctx->n + 63) / 64;
  double* scan_part = ctx->ts_scratch;
  double* obs_part = ctx->ts_scratch + pf::ts_scan_words(ctx->n);
  const pf::TsK K{a->gamma, a->reward, a->terminated, a->truncated, a->episode_start, a->carry_return, a->carry_length, a->carry_disc,
                  a->ep_return_out, a->ep_length_out, a->ret_moments};
  hipLaunchKernelGGL(next ? pf::ts_scan_kernel<true> : pf::ts_scan_kernel<false>, dim3(waves), dim3(64), 0, s, K, ctx->n, k_steps, scan_part);
  unsigned grid = 0;
  if (a->obs) {
    const size_t rows = (size_t)k_steps * (size_t)ctx->n;
    grid = pf::ts_obs_grid(rows * (size_t)D);
    hipLaunchKernelGGL(next ? pf::ts_obs_kernel<true> : pf::ts_obs_kernel<false>, dim3(grid), dim3(pf::kTsObsBlock), 0, s, a->obs, a->terminated,
                       a->truncated, a->episode_start, a->obs_moments, obs_part, rows, ctx->n, D);
  }
  hipLaunchKernelGGL(pf::ts_finish_kernel, dim3(1), dim3(pf::kTsFinishBlock), 0, s, scan_part, waves, a->obs ? obs_part : nullptr, (int)grid, D,
                     a->summary, a->ret_moments, a->obs_moments);
  PF_HIP(ctx, hipGetLastError());
  return PF_OK;
}
// what pf_ppo_loss and pf_ppo_grad check of the loss's coefficients
static int ppo_coef_check(pf_ctx* ctx, const char* who, float clip, float vf_coef, float ent_coef, int32_t normalize_advantage) {
  if (!(clip > 0.0f && clip < INFINITY)) return arg_fail(ctx, who, "clip must be finite and > 0");
  if (!(vf_coef >= 0.0f && vf_coef < INFINITY)) return arg_fail(ctx, who, "vf_coef must be finite and >= 0");
  if (!(ent_coef >= 0.0f && ent_coef < INFINITY)) return arg_fail(ctx, who, "ent_coef must be finite and >= 0");
  if (normalize_advantage != 0 && normalize_advantage != 1) return arg_fail(ctx, who, "normalize_advantage must be 0 or 1");
  return PF_OK;
}
int pf_ppo_loss(pf_ctx* ctx, const pf_ppo_loss_args* a, size_t rows, int width, void* stream) {
  if (!ctx || !a) return fail(ctx, PF_ERR_ARG, "pf_ppo_loss: ctx and the argument block are required");
  if (rows < 1) return fail(ctx, PF_ERR_ARG, "pf_ppo_loss: rows must be >= 1");
  if (width < 1 || width > pf::kPpoMaxA) return fail(ctx, PF_ERR_ARG, "pf_ppo_loss: width must be in 1..8");
  const arg_ptr required[] = {{"mean", a->mean}, {"log_std", a->log_std}, {"actions", a->actions}, {"logp_old", a->logp_old},
                              {"advantages", a->advantages}, {"returns", a->returns}, {"value", a->value}, {"grad_mean", a->grad_mean},
                              {"grad_value", a->grad_value}, {"grad_log_std", a->grad_log_std}, {"stats", a->stats}, {nullptr, nullptr}};
  if (int rc = require_args(ctx, "pf_ppo_loss", required)) return rc;
  if (int rc = ppo_coef_check(ctx, "pf_ppo_loss", a->clip, a->vf_coef, a->ent_coef, a->normalize_advantage)) return rc;
  int rc = ensure_device(ctx);
  if (rc) return rc;
  hipStream_t s = (hipStream_t)stream;
  double* adv_part = ctx->ppo_scratch + pf::kPpoAdvOffset;
  double* fin = ctx->ppo_scratch + pf::kPpoFinOffset;
  double* main_part = ctx->ppo_scratch + pf::kPpoMainOffset;
  // (no valid: the byte loads read the advantages' first M bytes and the mask drops them)
  const uint8_t* vbytes = a->valid ? a->valid : reinterpret_cast<const uint8_t*>(a->advantages);
  const uint32_t vmask = a->valid ? 0xFFu : 0u;
  const unsigned grid = pf::ppo_grid(rows);
  hipLaunchKernelGGL(pf::ppo_adv_kernel, dim3(grid), dim3(pf::kPpoBlock), 0, s, a->advantages, vbytes, vmask, rows, adv_part);
  hipLaunchKernelGGL(pf::ppo_adv_finish_kernel, dim3(1), dim3(pf::kPpoBlock), 0, s, adv_part, (int)grid, fin);
  const pf::PpoK K{a->clip, a->vf_coef, a->normalize_advantage, a->mean, a->log_std, a->actions, a->logp_old, a->advantages, a->returns, a->value,
                   vbytes, vmask, a->grad_mean, a->grad_value};
  // (one float4 per row where the rows are four wide and the caller's pointers allow it; the same arithmetic either way)
  const bool vec = width == 4 && (((uintptr_t)a->actions | (uintptr_t)a->mean | (uintptr_t)a->grad_mean) & 15) == 0;
  void (*main_kernel)(pf::PpoK, size_t, const double*, double*) = nullptr;
  switch (width) {
    case 1: main_kernel = pf::ppo_main_kernel<1, false>; break;
    case 2: main_kernel = pf::ppo_main_kernel<2, false>; break;
    case 3: main_kernel = pf::ppo_main_kernel<3, false>; break;
    case 4: main_kernel = vec ? pf::ppo_main_kernel<4, true> : pf::ppo_main_kernel<4, false>; break;
    case 5: main_kernel = pf::ppo_main_kernel<5, false>; break;
    case 6: main_kernel = pf::ppo_main_kernel<6, false>; break;
    case 7: main_kernel = pf::ppo_main_kernel<7, false>; break;
    default: main_kernel = pf::ppo_main_kernel<8, false>; break;
  }
  hipLaunchKernelGGL(main_kernel, dim3(grid), dim3(pf::kPpoBlock), 0, s, K, rows, (const double*)fin, main_part);
  hipLaunchKernelGGL(pf::ppo_finish_kernel, dim3(1), dim3(pf::kPpoBlock), 0, s, (const double*)main_part, (int)grid, (const double*)fin, a->log_std, width,
                     a->vf_coef, a->ent_coef, a->stats, a->grad_log_std);
  PF_HIP(ctx, hipGetLastError());
  return PF_OK;
}
// pf_mlp_forward / pf_mlp_backward: what both check of the network; `who` is the call's name
static const char* mlp_shape_error(const pf_mlp* q) {
  if (q->n_layers != 2 && q->n_layers != 3) return "n_layers must be 2 or 3";
  for (int l = 0; l + 1 < q->n_layers; ++l)
    if (q->width[l] < 1 || q->width[l] > PF_POLICY_MAX_HIDDEN) return "width: hidden widths must be in 1..PF_POLICY_MAX_HIDDEN (64)";
  if (q->activation != PF_ACT_TANH && q->activation != PF_ACT_RELU) return "activation must be PF_ACT_TANH or PF_ACT_RELU";
  if (q->in_dim < 1 || q->in_dim > pf::kActMaxIn) return "in_dim must be in 1..128";
  if (q->out_dim < 1 || q->out_dim > pf::kActMaxA) return "out_dim must be in 1..8";
  return nullptr;
}
static int mlp_check(pf_ctx* ctx, const char* who, const pf_mlp* q, int64_t rows) {
  if (!q) return arg_fail(ctx, who, "mlp is required");
  if (const char* e = mlp_shape_error(q)) return arg_fail(ctx, who, e);
  for (int l = 0; l < q->n_layers; ++l)
    if (!q->w[l] || !q->b[l]) return arg_fail(ctx, who, "w / b: every layer needs w and b");
  if (rows < 1) return arg_fail(ctx, who, "rows must be >= 1");
  if (rows > (int64_t)INT32_MAX - pf::kActRows) return arg_fail(ctx, who, "rows must be below 2^31 - 64 (the kernels index rows with 32 bits)");
  return PF_OK;
}
int pf_mlp_forward(pf_ctx* ctx, const pf_mlp* q, const float* x, int64_t rows, float* out, void* stream) {
  static const char* who = "pf_mlp_forward";
  if (!ctx) return arg_fail(ctx, who, "ctx is required");
  int rc = mlp_check(ctx, who, q, rows);
  if (rc) return rc;
  if (!x) return arg_fail(ctx, who, "x is required");
  if (!out) return arg_fail(ctx, who, "out is required");
  char buf[128];
  const arg_span spans[2] = {{"x", x, sizeof(float) * (size_t)rows * q->in_dim}, {"out", out, sizeof(float) * (size_t)rows * q->out_dim}};
  if (const char* e = spans_overlap(spans, 2, buf, sizeof(buf))) return arg_fail(ctx, who, e);
  rc = ensure_device(ctx);
  if (rc) return rc;
  // policy_act_kernel itself, the draw off (no log_std), the caller's rows as its observations and out_dim as its action width
  pf_policy P;
  P.n_layers = q->n_layers;
  P.width[0] = q->width[0];
  P.width[1] = q->width[1];
  P.activation = q->activation;
  for (int l = 0; l < 3; ++l) {
    P.w[l] = l < q->n_layers ? q->w[l] : nullptr;
    P.b[l] = l < q->n_layers ? q->b[l] : nullptr;
  }
  P.log_std = nullptr;
  P.obs0 = x;
  P.mean_out = nullptr;
  const pf::ActK AK{P, out, (int)rows, q->in_dim, q->out_dim, 0u, 0u, 0u, 0ull};
  return launch_policy_act(ctx, AK, rows, stream);
}
size_t pf_mlp_backward_workspace_bytes(const pf_mlp* q, int64_t rows) {
  if (!q || mlp_shape_error(q) || rows < 1) return 0;
  return sizeof(float) * (size_t)pf::mlp_grid(rows) * (size_t)pf::mlp_param_count(*q, nullptr);
}
int pf_mlp_backward(pf_ctx* ctx, const pf_mlp* q, const float* x, const float* grad_out, int64_t rows, float* const grad_w[3], float* const grad_b[3],
                    void* workspace, size_t workspace_bytes, void* stream) {
  static const char* who = "pf_mlp_backward";
  if (!ctx) return arg_fail(ctx, who, "ctx is required");
  int rc = mlp_check(ctx, who, q, rows);
  if (rc) return rc;
  if (!x) return arg_fail(ctx, who, "x is required");
  if (!grad_out) return arg_fail(ctx, who, "grad_out is required");
  if (!grad_w) return arg_fail(ctx, who, "grad_w is required");
  if (!grad_b) return arg_fail(ctx, who, "grad_b is required");
  for (int l = 0; l < q->n_layers; ++l) {
    if (!grad_w[l]) return arg_fail(ctx, who, "grad_w: every layer needs its output");
    if (!grad_b[l]) return arg_fail(ctx, who, "grad_b: every layer needs its output");
  }
  if (!workspace) return arg_fail(ctx, who, "workspace is required");
  const size_t need = pf_mlp_backward_workspace_bytes(q, rows);
  if (workspace_bytes < need) return arg_fail(ctx, who, "workspace_bytes is below pf_mlp_backward_workspace_bytes(mlp, rows)");
  static const char* const wn[3] = {"grad_w[0]", "grad_w[1]", "grad_w[2]"};
  static const char* const bn[3] = {"grad_b[0]", "grad_b[1]", "grad_b[2]"};
  arg_span spans[9];
  int ns = 0;
  spans[ns++] = {"x", x, sizeof(float) * (size_t)rows * q->in_dim};
  spans[ns++] = {"grad_out", grad_out, sizeof(float) * (size_t)rows * q->out_dim};
  spans[ns++] = {"workspace", workspace, need};
  for (int l = 0; l < q->n_layers; ++l) {
    const size_t n_in = l == 0 ? q->in_dim : q->width[l - 1], n_out = l + 1 == q->n_layers ? q->out_dim : q->width[l];
    spans[ns++] = {wn[l], grad_w[l], sizeof(float) * n_in * n_out};
    spans[ns++] = {bn[l], grad_b[l], sizeof(float) * n_out};
  }
  char buf[128];
  if (const char* e = spans_overlap(spans, ns, buf, sizeof(buf))) return arg_fail(ctx, who, e);
  rc = ensure_device(ctx);
  if (rc) return rc;
  hipStream_t s = (hipStream_t)stream;
  const int grid = pf::mlp_grid(rows);
  const pf::MlpK K{*q, x, grad_out, (float*)workspace, (int)rows};
  hipLaunchKernelGGL(pf::mlp_backward_kernel<pf::MlpK>, dim3(grid), dim3(256), 0, s, K);
  pf::MlpOutK O;
  const int P = pf::mlp_param_count(*q, O.end);
  for (int l = 0; l < 3; ++l) {
    O.p[2 * l] = l < q->n_layers ? grad_w[l] : nullptr;
    O.p[2 * l + 1] = l < q->n_layers ? grad_b[l] : nullptr;
  }
  hipLaunchKernelGGL(pf::mlp_reduce_kernel, dim3((P + 255) / 256), dim3(256), 0, s, (const float*)workspace, grid, P, O);
  PF_HIP(ctx, hipGetLastError());
  return PF_OK;
}
// pf_ppo_grad: the shape checks of the two networks; null, or the refusal with the network named (buf holds it)
static const char* ppo_grad_shape_error(const pf_mlp* actor, const pf_mlp* critic, char* buf, size_t len) {
  if (const char* e = mlp_shape_error(actor)) {
    snprintf(buf, len, "actor: %s", e);
    return buf;
  }
  if (const char* e = mlp_shape_error(critic)) {
    snprintf(buf, len, "critic: %s", e);
    return buf;
  }
  if (critic->out_dim != 1) return "critic: out_dim must be 1";
  if (critic->in_dim != actor->in_dim) return "critic: in_dim must equal the actor's in_dim (both read x)";
  return nullptr;
}
size_t pf_ppo_grad_workspace_bytes(const pf_mlp* actor, const pf_mlp* critic, int64_t rows) {
  char buf[160];
  if (!actor || !critic || ppo_grad_shape_error(actor, critic, buf, sizeof(buf)) || rows < 1) return 0;
  const int grid = pf::mlp_grid(rows);
  return pf::ppo_grad_stat_bytes(grid) + sizeof(float) * (size_t)grid * ((size_t)pf::mlp_param_count(*actor, nullptr) + (size_t)pf::mlp_param_count(*critic, nullptr));
}
int pf_ppo_grad(pf_ctx* ctx, const pf_ppo_grad_args* a, int64_t rows, void* workspace, size_t workspace_bytes, void* stream) {
  static const char* who = "pf_ppo_grad";
  if (!ctx) return arg_fail(ctx, who, "ctx is required");
  if (!a) return arg_fail(ctx, who, "the argument block is required");
  if (!a->actor) return arg_fail(ctx, who, "actor is required");
  if (!a->critic) return arg_fail(ctx, who, "critic is required");
  char buf[160];
  if (const char* e = ppo_grad_shape_error(a->actor, a->critic, buf, sizeof(buf))) return arg_fail(ctx, who, e);
  const pf_mlp* nets[2] = {a->actor, a->critic};
  for (int k = 0; k < 2; ++k)
    for (int l = 0; l < nets[k]->n_layers; ++l)
      if (!nets[k]->w[l] || !nets[k]->b[l]) return arg_fail(ctx, who, k == 0 ? "actor: w / b: every layer needs w and b" : "critic: w / b: every layer needs w and b");
  if (rows < 1) return arg_fail(ctx, who, "rows must be >= 1");
  if (rows > (int64_t)INT32_MAX - pf::kActRows) return arg_fail(ctx, who, "rows must be below 2^31 - 64 (the kernels index rows with 32 bits)");
  const arg_ptr required[] = {{"x", a->x}, {"log_std", a->log_std}, {"actions", a->actions}, {"logp_old", a->logp_old}, {"advantages", a->advantages},
                              {"returns", a->returns}, {"grad_log_std", a->grad_log_std}, {"stats", a->stats}, {"workspace", workspace}, {nullptr, nullptr}};
  if (int rc = require_args(ctx, who, required)) return rc;
  static const char* const gn[2][2][3] = {{{"actor_grad_w[0]", "actor_grad_w[1]", "actor_grad_w[2]"}, {"actor_grad_b[0]", "actor_grad_b[1]", "actor_grad_b[2]"}},
                                          {{"critic_grad_w[0]", "critic_grad_w[1]", "critic_grad_w[2]"}, {"critic_grad_b[0]", "critic_grad_b[1]", "critic_grad_b[2]"}}};
  float* const* gw[2] = {a->actor_grad_w, a->critic_grad_w};
  float* const* gb[2] = {a->actor_grad_b, a->critic_grad_b};
  for (int k = 0; k < 2; ++k)
    for (int l = 0; l < nets[k]->n_layers; ++l) {
      const arg_ptr outs[] = {{gn[k][0][l], gw[k][l]}, {gn[k][1][l], gb[k][l]}, {nullptr, nullptr}};
      if (int rc = require_args(ctx, who, outs)) return rc;
    }
  if (int rc = ppo_coef_check(ctx, who, a->clip, a->vf_coef, a->ent_coef, a->normalize_advantage)) return rc;
  const size_t need = pf_ppo_grad_workspace_bytes(a->actor, a->critic, rows);
  if (workspace_bytes < need) return arg_fail(ctx, who, "workspace_bytes is below pf_ppo_grad_workspace_bytes(actor, critic, rows)");
  if (((uintptr_t)workspace & 7) != 0) return arg_fail(ctx, who, "workspace must be 8-byte aligned (it holds rows of double partial sums)");
  const size_t M = (size_t)rows, A = (size_t)a->actor->out_dim;
  arg_span spans[7 + 15];
  int ns = 0;
  spans[ns++] = {"x", a->x, sizeof(float) * M * a->actor->in_dim};
  spans[ns++] = {"log_std", a->log_std, sizeof(float) * A};
  spans[ns++] = {"actions", a->actions, sizeof(float) * M * A};
  spans[ns++] = {"logp_old", a->logp_old, sizeof(float) * M};
  spans[ns++] = {"advantages", a->advantages, sizeof(float) * M};
  spans[ns++] = {"returns", a->returns, sizeof(float) * M};
  if (a->valid) spans[ns++] = {"valid", a->valid, M};
  const int n_read = ns;
  spans[ns++] = {"workspace", workspace, need};
  spans[ns++] = {"grad_log_std", a->grad_log_std, sizeof(float) * A};
  spans[ns++] = {"stats", a->stats, sizeof(double) * 16};
  for (int k = 0; k < 2; ++k)
    for (int l = 0; l < nets[k]->n_layers; ++l) {
      const pf_mlp* q = nets[k];
      const size_t n_in = l == 0 ? q->in_dim : q->width[l - 1], n_out = l + 1 == q->n_layers ? q->out_dim : q->width[l];
      spans[ns++] = {gn[k][0][l], gw[k][l], sizeof(float) * n_in * n_out};
      spans[ns++] = {gn[k][1][l], gb[k][l], sizeof(float) * n_out};
    }
  if (const char* e = spans_overlap(spans, ns, buf, sizeof(buf), n_read)) return arg_fail(ctx, who, e);
  int rc = ensure_device(ctx);
  if (rc) return rc;
  hipStream_t s = (hipStream_t)stream;
  double* adv_part = ctx->ppo_scratch + pf::kPpoAdvOffset;
  double* fin = ctx->ppo_scratch + pf::kPpoFinOffset;
  // (no valid: the byte loads read the advantages' first M bytes and the mask drops them)
  const uint8_t* vbytes = a->valid ? a->valid : reinterpret_cast<const uint8_t*>(a->advantages);
  const uint32_t vmask = a->valid ? 0xFFu : 0u;
  const unsigned adv_grid = pf::ppo_grid(M);
  hipLaunchKernelGGL(pf::ppo_adv_kernel, dim3(adv_grid), dim3(pf::kPpoBlock), 0, s, a->advantages, vbytes, vmask, M, adv_part);
  hipLaunchKernelGGL(pf::ppo_adv_finish_kernel, dim3(1), dim3(pf::kPpoBlock), 0, s, adv_part, (int)adv_grid, fin);
  const int grid = pf::mlp_grid(rows);
  double* stat_part = (double*)workspace;
  float* part[2];
  part[0] = (float*)((char*)workspace + pf::ppo_grad_stat_bytes(grid));
  part[1] = part[0] + (size_t)grid * (size_t)pf::mlp_param_count(*a->actor, nullptr);
  const pf::PpoGradK<pf::kGradActor> KA{pf::MlpK{*a->actor, a->x, nullptr, part[0], (int)rows}, a->clip, a->vf_coef, a->normalize_advantage, a->log_std, a->actions,
                                        a->logp_old, a->advantages, a->returns, vbytes, vmask, fin, stat_part};
  const pf::PpoGradK<pf::kGradCritic> KC{pf::MlpK{*a->critic, a->x, nullptr, part[1], (int)rows}, a->clip, a->vf_coef, a->normalize_advantage, a->log_std, a->actions,
                                         a->logp_old, a->advantages, a->returns, vbytes, vmask, fin, stat_part};
  hipLaunchKernelGGL(pf::mlp_backward_kernel<pf::PpoGradK<pf::kGradActor>>, dim3(grid), dim3(256), 0, s, KA);
  hipLaunchKernelGGL(pf::mlp_backward_kernel<pf::PpoGradK<pf::kGradCritic>>, dim3(grid), dim3(256), 0, s, KC);
  for (int k = 0; k < 2; ++k) {
    pf::MlpOutK O;
    const int P = pf::mlp_param_count(*nets[k], O.end);
    for (int l = 0; l < 3; ++l) {
      O.p[2 * l] = l < nets[k]->n_layers ? gw[k][l] : nullptr;
      O.p[2 * l + 1] = l < nets[k]->n_layers ? gb[k][l] : nullptr;
    }
    hipLaunchKernelGGL(pf::mlp_reduce_kernel, dim3((P + 255) / 256), dim3(256), 0, s, (const float*)part[k], grid, P, O);
  }
  hipLaunchKernelGGL(pf::ppo_finish_kernel, dim3(1), dim3(pf::kPpoBlock), 0, s, (const double*)stat_part, grid, (const double*)fin, a->log_std, (int)A, a->vf_coef,
                     a->ent_coef, a->stats, a->grad_log_std);
  PF_HIP(ctx, hipGetLastError());
  return PF_OK;
}
size_t pf_adam_workspace_bytes(int64_t total_numel) {
  if (total_numel < 1 || total_numel > (int64_t)INT32_MAX) return 0;
  return sizeof(double) * (pf::adam_grid_bound(total_numel) + pf::kAdamHeader);
}
// what pf_adam_step refuses, or null; `buf` holds a composed message
static const char* adam_error(const pf_adam_args* a, const void* workspace, size_t workspace_bytes, char* buf, size_t len) {
  if (!a) return "the argument block is required";
  if (a->n_tensors < 1 || a->n_tensors > PF_ADAM_MAX_TENSORS) return "n_tensors must be in 1..PF_ADAM_MAX_TENSORS (32)";
  if (a->skip_nonfinite != 0 && a->skip_nonfinite != 1) return "skip_nonfinite must be 0 or 1";
  if (!a->lr_dev && !(a->lr >= 0.0f && a->lr < INFINITY)) return "lr must be finite and >= 0";
  if (!(a->beta1 >= 0.0f && a->beta1 < 1.0f)) return "beta1 must be in [0, 1)";
  if (!(a->beta2 >= 0.0f && a->beta2 < 1.0f)) return "beta2 must be in [0, 1)";
  if (!(a->eps > 0.0f && a->eps < INFINITY)) return "eps must be finite and > 0";
  if (!(a->weight_decay >= 0.0f && a->weight_decay < INFINITY)) return "weight_decay must be finite and >= 0";
  if (!(a->max_grad_norm > 0.0f)) return "max_grad_norm must be > 0 (+infinity: no clipping)";
  if (!a->state) return "state is required";
  if (!workspace) return "workspace is required";
  static const char* const kinds[4] = {"param", "grad", "exp_avg", "exp_avg_sq"};
  arg_span spans[4 * PF_ADAM_MAX_TENSORS + 3];
  char names[4 * PF_ADAM_MAX_TENSORS][16];
  int ns = 0;
  int64_t total = 0;
  for (int i = 0; i < a->n_tensors; ++i) {
    if (a->numel[i] < 1) {
      snprintf(buf, len, "numel[%d] must be >= 1", i);
      return buf;
    }
    total += a->numel[i];
    if (total > (int64_t)INT32_MAX) return "numel: the total must be below 2^31";
    const void* const ptrs[4] = {a->param[i], a->grad[i], a->exp_avg[i], a->exp_avg_sq[i]};
    for (int k = 0; k < 4; ++k) {
      snprintf(names[ns], sizeof(names[ns]), "%s[%d]", kinds[k], i);
      if (!ptrs[k]) {
        snprintf(buf, len, "%s is required", names[ns]);
        return buf;
      }
      spans[ns] = {names[ns], ptrs[k], sizeof(float) * (size_t)a->numel[i]};
      ++ns;
    }
  }
  const size_t need = pf_adam_workspace_bytes(total);
  if (workspace_bytes < need) return "workspace_bytes is below pf_adam_workspace_bytes(the total of numel)";
  spans[ns++] = {"state", a->state, sizeof(double) * 8};
  spans[ns++] = {"workspace", workspace, need};
  if (a->lr_dev) spans[ns++] = {"lr_dev", a->lr_dev, sizeof(float)};
  return spans_overlap(spans, ns, buf, len);
}
int pf_adam_step(pf_ctx* ctx, const pf_adam_args* a, void* workspace, size_t workspace_bytes, void* stream) {
  static const char* who = "pf_adam_step";
  if (!ctx) return arg_fail(ctx, who, "ctx is required");
  char buf[128];
  if (const char* e = adam_error(a, workspace, workspace_bytes, buf, sizeof(buf))) return arg_fail(ctx, who, e);
  int rc = ensure_device(ctx);
  if (rc) return rc;
  pf::AdamK K;
  K.n_tensors = a->n_tensors;
  K.skip_nonfinite = a->skip_nonfinite;
  K.lr = a->lr;
  K.beta1 = a->beta1, K.beta2 = a->beta2, K.eps = a->eps, K.weight_decay = a->weight_decay, K.max_grad_norm = a->max_grad_norm;
  K.lr_dev = a->lr_dev;
  K.state = a->state;
  K.work = (double*)workspace;
  int chunks = 0;
  for (int i = 0; i < PF_ADAM_MAX_TENSORS; ++i) {
    const bool on = i < a->n_tensors;
    K.first_chunk[i] = chunks;
    K.numel[i] = on ? (int32_t)a->numel[i] : 0;
    K.param[i] = on ? a->param[i] : nullptr;
    K.grad[i] = on ? a->grad[i] : nullptr;
    K.exp_avg[i] = on ? a->exp_avg[i] : nullptr;
    K.exp_avg_sq[i] = on ? a->exp_avg_sq[i] : nullptr;
    if (on) chunks += (int)((a->numel[i] + pf::kAdamChunk - 1) / pf::kAdamChunk);
  }
  K.first_chunk[PF_ADAM_MAX_TENSORS] = chunks;
  K.chunks = chunks;
  const int grid = chunks < pf::kAdamMaxGrid ? chunks : pf::kAdamMaxGrid;  // (<= adam_grid_bound(total): a chunk holds an element or more)
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(pf::adam_norm_kernel, dim3(grid), dim3(pf::kAdamBlock), 0, s, K);
  hipLaunchKernelGGL(pf::adam_update_kernel, dim3(grid), dim3(pf::kAdamBlock), 0, s, K);
  PF_HIP(ctx, hipGetLastError());
  return PF_OK;
}
int pf_world_sync(pf_ctx* ctx, const pf_world_sync_args* a, int agents_per_world, void* stream) {
  static const char* who = "pf_world_sync";
  if (!ctx) return arg_fail(ctx, who, "ctx is required");
  if (!a) return arg_fail(ctx, who, "the argument block is required");
  const arg_ptr required[] = {{"terminated", a->terminated}, {"truncated", a->truncated}, {"reward", a->reward}, {"done", a->done},
                              {"valid_out", a->valid_out}, {"reset_out", a->reset_out}, {nullptr, nullptr}};
  if (int rc = require_args(ctx, who, required)) return rc;
  if (agents_per_world < 1 || agents_per_world > pf::kWorldSyncMaxA) return arg_fail(ctx, who, "agents_per_world must be in 1..64");
  if (ctx->n % agents_per_world != 0) return arg_fail(ctx, who, "agents_per_world must divide the context's lane count n");
  int rc = ensure_device(ctx);
  if (rc) return rc;
  hipStream_t s = (hipStream_t)stream;
  // (the new latch goes to the context's staging buffer and is copied over the caller's behind the kernel: world_sync.hpp)
  const pf::WorldSyncK K{a->terminated, a->truncated, a->reward, a->done, a->exclude, a->valid_out, a->reset_out, ctx->sync_latch};
  hipLaunchKernelGGL(pf::world_sync_kernel, dim3((ctx->n + pf::kWorldSyncBlock - 1) / pf::kWorldSyncBlock), dim3(pf::kWorldSyncBlock), 0, s, K, ctx->n,
                     agents_per_world);
  PF_HIP(ctx, hipGetLastError());
  PF_HIP(ctx, hipMemcpyAsync(a->done, ctx->sync_latch, (size_t)ctx->n, hipMemcpyDeviceToDevice, s));
  return PF_OK;
}
int pf_body_tick(pf_ctx* ctx, const pf_buffers* b, int n_ticks, void* stream) {
  if (!ctx || !b || !b->state || !b->wrench) return fail(ctx, PF_ERR_ARG, "pf_body_tick: state and wrench buffers are required");
  if (n_ticks < 1) return fail(ctx, PF_ERR_ARG, "pf_body_tick: n_ticks must be >= 1");
  if (ctx->P.vehicle == PF_ROCKET) return fail(ctx, PF_ERR_UNSUPPORTED, "pf_body_tick: the Rocket's mass properties change per tick; QuadX / Fixedwing only");
  int rc = ensure_device(ctx);
  if (rc) return rc;
  const int grid = (ctx->n + pf::kWave - 1) / pf::kWave;
  hipStream_t s = (hipStream_t)stream;
  const auto kernel = vehicle_kernel(ctx, pf::body_tick_kernel<pf::QuadX>, pf::body_tick_kernel<pf::Fixedwing>);
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(pf::kWave), 0, s, ctx->P, *b, ctx->n, n_ticks, ctx->P_dev);
  PF_HIP(ctx, hipGetLastError());
  return PF_OK;
}

#ifdef PF_PHASE_TRACE
// diagnostic variant only (profiles/tools/solver_trace.py): read (and clear) the contact solver's call statistics
int pf_debug_solver_trace(unsigned long long* out) {
  hipError_t e = hipMemcpyFromSymbol(out, HIP_SYMBOL(pf::g_solver_trace), sizeof(unsigned long long) * 8, 0, hipMemcpyDeviceToHost);
  unsigned long long z[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (e == hipSuccess) e = hipMemcpyToSymbol(HIP_SYMBOL(pf::g_solver_trace), z, sizeof(z), 0, hipMemcpyHostToDevice);
  return (int)e;
}
// diagnostic variant only: (waves that were not calm, waves that took the calm test) since the last call; clears
int pf_debug_calm_trace(unsigned long long* out) {
  hipError_t e = hipMemcpyFromSymbol(out, HIP_SYMBOL(pf::g_calm_trace), sizeof(unsigned long long) * 2, 0, hipMemcpyDeviceToHost);
  unsigned long long z[2] = {0, 0};
  if (e == hipSuccess) e = hipMemcpyToSymbol(HIP_SYMBOL(pf::g_calm_trace), z, sizeof(z), 0, hipMemcpyHostToDevice);
  return (int)e;
}
// diagnostic variant only (profiles/tools/phase_trace.py): copy out the per-wave phase stamps of the last quadx_m0 launch
int pf_debug_phase_trace(unsigned long long* out, int n_words) {
  return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(pf::g_phase_trace), sizeof(unsigned long long) * (size_t)n_words, 0, hipMemcpyDeviceToHost);
}
#endif

}  // extern "C"
