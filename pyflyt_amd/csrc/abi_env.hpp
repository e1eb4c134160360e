// abi_env.hpp -- the C ABI's environment side: which env kernel a context runs and its one launch site, the context's lifetime and queries,
// and the entry points that step environments (pf_env_*, pf_aviary_*, pf_body_tick, pf_sample_actions, pf_rollout, pf_rollout_policy). Host code.
#pragma once
#include <cstdlib>
#include <new>
#include <type_traits>

#include "abi_ctx.hpp"  // (with the HIP runtime, quadx_fast.hpp, fixedwing_fast.hpp, env_generic.hpp)
#include "dogfight.hpp"
#include "rocket_landing.hpp"
#include "aviary_kernels.hpp"
#include "policy_mlp.hpp"  // policy_pack_kernel
#include "traj_stats.hpp"  // ts_scratch_words
#include "ppo_loss.hpp"    // kPpoScratchWords

// Which env kernel a context runs, and its launch-invariant template arguments; fills K, FK and fsurf for the specialised kernels.
// The only reader of the environment overrides, which exist for the tests: PF_DISABLE_FAST forces the generic kernels,
// PF_NO_LEAN_KERNEL the two-wave instantiations, PF_NO_CALM_PATH turns the specialised QuadX kernel's calm-wave ticks off,
// PF_NO_FIXED_STEP keeps pf_env_step on the general one-step instantiation. `cus`: the device's CU count, 0 where it is unknown.
static env_choice select_env_kernel(const pf_params& P, int n_lanes, int cus, pf::QuadK& K, pf::FwK& FK, pf::FwTable& fsurf) {
  env_choice c{env_family::generic, false, false, false, false, false};
  const bool fast = getenv("PF_DISABLE_FAST") == nullptr;
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

// One launch of the context's env kernel: a reset or a step (roll 0, op and mask) or a rollout (roll 1 / 2, k_steps steps from step
// index step0). The callers have checked the arguments.
static int launch_env(pf_ctx* ctx, const pf_buffers* b, int op, const uint8_t* mask, int roll, int k_steps, uint32_t step0, void* stream) {
  if (int rc = ensure_device(ctx)) return rc;
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
  return launched(ctx);
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
size_t pf_sizeof_traj_stats_masked(void) { return sizeof(pf_traj_stats_masked_args); }
size_t pf_sizeof_ppo_loss(void) { return sizeof(pf_ppo_loss_args); }
size_t pf_sizeof_mlp(void) { return sizeof(pf_mlp); }
size_t pf_sizeof_ppo_grad(void) { return sizeof(pf_ppo_grad_args); }
size_t pf_sizeof_adam(void) { return sizeof(pf_adam_args); }
size_t pf_sizeof_world_sync(void) { return sizeof(pf_world_sync_args); }
size_t pf_sizeof_outcome(void) { return sizeof(pf_outcome_args); }
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
  pf_ctx* c = new (std::nothrow) pf_ctx();
  if (!c) return fail(nullptr, PF_ERR_ARG, "out of host memory");
  c->P = P; c->n = n_lanes; c->device = device; c->lane0 = lane_offset;
  {  // the airframe's worst-case contact count (collider vertices), see pf_params.contact_max_points
    int pts = 0;
    for (int k = 0; k < P.n_boxes; ++k) pts += P.boxes[k].kind == 1 ? 16 : (P.contact_manifold_points >= 8 ? 8 : 4);
    c->P.contact_max_points = pts < 1 ? 1 : (pts > PF_MAX_CONTACTS ? PF_MAX_CONTACTS : pts);
  }
  int cus = 0;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess) cus = 0;
  pf::FwTable fsurf;
  c->ek = select_env_kernel(P, n_lanes, cus, c->K, c->FK, fsurf);
  c->act_grid_cap = 2 * (cus < 1 ? 256 : cus);
  const env_family fam = c->ek.family;
  {  // device copy of the parameter block (LDS constant tables, the out-of-line floor test)
    const device_scope on(device);
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
    if (e != hipSuccess) return pf_ctx_destroy(c), hip_fail(nullptr, e, "pf_ctx_create: device parameter block");  // (frees what was allocated)
  }
  if ((fam == env_family::fixedwing_wp || fam == env_family::generic) && (P.task == PF_TASK_HOVER || P.task == PF_TASK_WAYPOINTS) &&
      (P.vehicle == PF_FIXEDWING || P.noise_mode == PF_NOISE_OFF)) {
    // the settle phase cannot depend on the lane (fixedwing: throttle command 0 during settle, so the
    // motor noise scales nothing; or noise off): settle once here, resets copy the result
    const device_scope on(device);
    const int groups = P.vehicle == PF_QUADX ? pf::QuadX::GROUPS : pf::Fixedwing::GROUPS;
    hipError_t e = hipMalloc((void**)&c->tmpl, sizeof(float4) * groups);
    if (e == hipSuccess) e = hipMemset(c->tmpl, 0, sizeof(float4) * groups);
    if (e == hipSuccess) {
      hipLaunchKernelGGL(vehicle_kernel(c, pf::settle_template_kernel<pf::QuadX>, pf::settle_template_kernel<pf::Fixedwing>), dim3(1), dim3(64), 0, 0, c->P,
                         c->tmpl, c->P_dev);
      e = hipDeviceSynchronize();
    }
    if (e != hipSuccess) return pf_ctx_destroy(c), hip_fail(nullptr, e, "pf_ctx_create: settle template");
  }
  *out = c;
  return PF_OK;
}
void pf_ctx_destroy(pf_ctx* ctx) {
  if (!ctx) return;
  for (void* p : {(void*)ctx->P_dev, (void*)ctx->launch_ctr, (void*)ctx->policy_dev, (void*)ctx->tmpl, (void*)ctx->surf_dev, (void*)ctx->ts_scratch,
                  (void*)ctx->ppo_scratch, (void*)ctx->sync_latch})
    if (p) hipFree(p);
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
  if (P.task == PF_TASK_NONE) return arg_fail(ctx, "pf_env_*", "context has no env task (use the pf_aviary_* calls)");
  if (op == pf::OP_STEP && (!b->actions || !b->reward || !b->terminated || !b->truncated))
    return fail(ctx, PF_ERR_ARG, "pf_env_step: actions/reward/terminated/truncated buffers are required");
  if (P.noise_mode == PF_NOISE_INJECT && ((op == pf::OP_STEP && !b->xi) || !b->xi_reset))
    if (!(op == pf::OP_STEP && P.autoreset == PF_AUTORESET_OFF && b->xi))
      return fail(ctx, PF_ERR_ARG, "PF_NOISE_INJECT needs xi (step) and xi_reset (reset/auto-reset)");
  return launch_env(ctx, b, op, mask, 0, 1, 0u, stream);
}
int pf_env_reset(pf_ctx* ctx, const pf_buffers* b, const uint8_t* mask, void* stream) { return env_reset_or_step(ctx, b, pf::OP_RESET, mask, stream); }
int pf_env_step(pf_ctx* ctx, const pf_buffers* b, void* stream) { return env_reset_or_step(ctx, b, pf::OP_STEP, nullptr, stream); }

int pf_aviary_reset(pf_ctx* ctx, const pf_buffers* b, void* stream) {
  if (!ctx || !b || !b->state) return fail(ctx, PF_ERR_ARG, "pf_aviary_reset: state buffer required");
  const auto kernel = vehicle_kernel(ctx, pf::aviary_reset_kernel<pf::QuadX>, pf::aviary_reset_kernel<pf::Fixedwing>, pf::aviary_reset_kernel<pf::Rocket>);
  const int rc = launch_per_lane(ctx, b, stream, kernel, b->start_pose);
  ctx->P.flight_mode = 0;  // (behind the launch) drone.reset() -> set_mode(0) (quadx.py:224, fixedwing.py:196)
  return rc;
}
int pf_aviary_set_mode(pf_ctx* ctx, const pf_buffers* b, int mode, float* setpoints_out, void* stream) {
  if (!ctx || !b || !b->state) return fail(ctx, PF_ERR_ARG, "pf_aviary_set_mode: state buffer required");
  if (ctx->P.vehicle == PF_QUADX && (mode < -1 || mode > 7)) return fail(ctx, PF_ERR_ARG, "`mode` must be between -1 and 7");
  if (ctx->P.vehicle == PF_FIXEDWING && (mode < -1 || mode > 0)) return fail(ctx, PF_ERR_ARG, "`mode` must be between -1 and 0");
  if (ctx->P.vehicle == PF_ROCKET && mode != 0) return fail(ctx, PF_ERR_ARG, "`mode` must be 0 (rocket.py:238-247)");
  if (b->modes && ctx->P.vehicle != PF_QUADX) return fail(ctx, PF_ERR_UNSUPPORTED, "per-drone flight modes are supported for QuadX only (Fixedwing modes differ in setpoint width)");
  const int sp_dim = pf::setpoint_width(ctx->P.vehicle, mode);
  const auto kernel = vehicle_kernel(ctx, pf::aviary_set_mode_kernel<pf::QuadX>, pf::aviary_set_mode_kernel<pf::Fixedwing>, pf::aviary_set_mode_kernel<pf::Rocket>);
  const int rc = launch_per_lane(ctx, b, stream, kernel, sp_dim, mode, setpoints_out);
  ctx->P.flight_mode = mode;  // (behind the launch: the kernel takes the mode it leaves)
  return rc;
}
int pf_aviary_step(pf_ctx* ctx, const pf_buffers* b, int n_steps, void* stream) {
  if (!ctx || !b || !b->state || !b->setpoints) return fail(ctx, PF_ERR_ARG, "pf_aviary_step: state and setpoints required");
  if (n_steps < 1) return arg_fail(ctx, "pf_aviary_step", "n_steps must be >= 1");
  if (ctx->P.noise_mode == PF_NOISE_INJECT && !b->xi) return fail(ctx, PF_ERR_ARG, "PF_NOISE_INJECT needs xi");
  const auto kernel = ctx->P.agents_per_world > 1  // shared worlds (pf_ctx_create admitted QuadX / Fixedwing with plain boxes only)
                          ? vehicle_kernel(ctx, pf::aviary_world_step_kernel<pf::QuadX>, pf::aviary_world_step_kernel<pf::Fixedwing>)
                          : vehicle_kernel(ctx, pf::aviary_step_kernel<pf::QuadX>, pf::aviary_step_kernel<pf::Fixedwing>, pf::aviary_step_kernel<pf::Rocket>);
  return launch_per_lane(ctx, b, stream, kernel, ctx->lane0, n_steps, ctx->P_dev);
}
int pf_aviary_tick(pf_ctx* ctx, const pf_buffers* b, int tick_index, void* stream) {
  static const char* who = "pf_aviary_tick";
  if (!ctx || !b || !b->state || !b->setpoints) return fail(ctx, PF_ERR_ARG, "pf_aviary_tick: state and setpoints buffers are required");
  if (tick_index < 0 || tick_index >= ctx->P.ticks_per_control) return arg_fail(ctx, who, "tick_index must be in [0, ticks_per_control)");
  if (ctx->P.agents_per_world > 1) return who_fail(ctx, PF_ERR_UNSUPPORTED, who, "no per-tick protocol (wind field) in shared worlds; use pf_aviary_step");
  if (ctx->P.noise_mode == PF_NOISE_INJECT && !b->xi) return arg_fail(ctx, who, "PF_NOISE_INJECT needs b->xi");
  const auto kernel = vehicle_kernel(ctx, pf::aviary_tick_kernel<pf::QuadX>, pf::aviary_tick_kernel<pf::Fixedwing>, pf::aviary_tick_kernel<pf::Rocket>);
  return launch_per_lane(ctx, b, stream, kernel, ctx->lane0, tick_index, ctx->P_dev);
}
int pf_wind_links(const pf_ctx* ctx) {
  return ctx->P.vehicle == PF_QUADX ? pf::QuadX::WIND_LINKS : (ctx->P.vehicle == PF_ROCKET ? pf::Rocket::WIND_LINKS : pf::Fixedwing::WIND_LINKS);
}
int pf_sample_actions(pf_ctx* ctx, float* actions, uint32_t step_index, void* stream) {
  if (!ctx || !actions) return fail(ctx, PF_ERR_ARG, "pf_sample_actions: bad argument");
  if (int rc = ensure_device(ctx)) return rc;
  const auto kernel = ctx->P.task == PF_TASK_ROCKET_LANDING ? pf::sample_actions7_kernel : pf::sample_actions_kernel;
  hipLaunchKernelGGL(kernel, dim3((ctx->n + 255) / 256), dim3(256), 0, (hipStream_t)stream, ctx->P, actions, ctx->n, ctx->lane0, step_index);
  return launched(ctx);
}

int pf_rollout(pf_ctx* ctx, const pf_buffers* b, int k_steps, uint32_t step_index0, void* stream) {
  static const char* who = "pf_rollout";
  if (!ctx || !b || !b->state || !b->obs || !b->reward || !b->terminated || !b->truncated)
    return fail(ctx, PF_ERR_ARG, "pf_rollout: state, obs, reward, terminated and truncated buffers are required");
  if (k_steps < 1) return arg_fail(ctx, who, "k_steps must be >= 1");
  const pf_params& P = ctx->P;
  const env_family f = ctx->ek.family;
  if (P.noise_mode == PF_NOISE_INJECT) return who_fail(ctx, PF_ERR_UNSUPPORTED, who, "PF_NOISE_INJECT is a per-step protocol; use pf_env_step");
  if (P.task == PF_TASK_NONE) return who_fail(ctx, PF_ERR_UNSUPPORTED, who, "this context has no env task");
  // Every env kernel is state-resident in a rollout: one launch for the k_steps (the dogfight on either aircraft model: four-wide
  // actions sampled on device, or the given sequence of either width; the generic env kernel: roll_steps)
  if ((f == env_family::dogfight_fast || f == env_family::dogfight_generic) && !b->actions && P.df_action_dim == 6)
    return who_fail(ctx, PF_ERR_UNSUPPORTED, who, "on-device sampling draws four-wide actions; pass the six-wide sequence in b->actions");
  // (the PettingZoo task has no auto-reset: finished agents are culled by the caller, their drones fly on in the shared world)
  if ((f == env_family::quadx || f == env_family::fixedwing_wp) && P.autoreset == PF_AUTORESET_OFF && P.task != PF_TASK_MA_HOVER)
    return who_fail(ctx, PF_ERR_UNSUPPORTED, who, "needs an auto-reset mode (finished lanes would idle for the rest of the launch)");
  return launch_env(ctx, b, pf::OP_STEP, nullptr, b->actions ? 2 : 1, k_steps, step_index0, stream);
}
int pf_rollout_policy(pf_ctx* ctx, const pf_buffers* b, const pf_policy* q, int k_steps, uint32_t step_index0, void* stream) {
  static const char* who = "pf_rollout_policy";
  if (!ctx || !b || !q || !b->state || !b->obs || !b->reward || !b->terminated || !b->truncated)
    return fail(ctx, PF_ERR_ARG, "pf_rollout_policy: policy, state, obs, reward, terminated and truncated buffers are required");
  if (k_steps < 1) return arg_fail(ctx, who, "k_steps must be >= 1");
  if (b->actions) return arg_fail(ctx, who, "b->actions must be NULL (the policy computes the actions; b->actions_out receives them)");
  const pf_params& P = ctx->P;
  const env_choice& c = ctx->ek;
  if (P.vehicle != PF_QUADX || (P.task != PF_TASK_HOVER && P.task != PF_TASK_WAYPOINTS))
    return who_fail(ctx, PF_ERR_UNSUPPORTED, who, "QuadX-Hover and QuadX-Waypoints only (no on-device policy for this task / vehicle)");
  if (c.family != env_family::quadx)
    return who_fail(ctx, PF_ERR_UNSUPPORTED, who, "needs the specialised QuadX kernel (pf_ctx_is_specialised() == 1); this context runs the generic one");
  if (c.md) return who_fail(ctx, PF_ERR_UNSUPPORTED, who, "flight mode 0 only (no instantiation with the cascaded flight modes)");
  // (shared worlds exist for PF_TASK_MA_HOVER and the dogfight only: refused by the task check above)
  if (P.noise_mode == PF_NOISE_INJECT) return who_fail(ctx, PF_ERR_UNSUPPORTED, who, "PF_NOISE_INJECT is a per-step protocol; use pf_env_step");
  if (P.autoreset == PF_AUTORESET_OFF)
    return who_fail(ctx, PF_ERR_UNSUPPORTED, who, "needs an auto-reset mode (auto-reset OFF: finished lanes would idle for the rest of the launch)");
  // (the contact response with every vertex in the manifold runs the out-of-line solve, whose argument block is stack: no zero-scratch instantiation)
  if (c.cr && P.contact_manifold_points >= 8)
    return who_fail(ctx, PF_ERR_UNSUPPORTED, who, "contact_response with contact_manifold_points = 8 is not supported (the in-register floor solve holds the 4-point manifold)");
  if (int rc = policy_net_check(ctx, "pf_rollout_policy", q)) return rc;
  if (!q->obs0) return arg_fail(ctx, who, "obs0 (the observation the previous call left) is required");
  const int D = pf_obs_dim(ctx);
  if (D > pf::kPolMaxIn) return who_fail(ctx, PF_ERR_UNSUPPORTED, who, "observation wider than the first layer's block");
  if (int rc = ensure_device(ctx)) return rc;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(pf::policy_pack_kernel, dim3(1), dim3(256), 0, s, *q, D, ctx->policy_dev);
  const pf::PolicyK PK{ctx->policy_dev, q->obs0, q->mean_out, q->n_layers, q->activation, q->log_std != nullptr ? 1 : 0};
  const bool philox = P.noise_mode == PF_NOISE_PHILOX;
  const auto kernel = P.task == PF_TASK_HOVER ? quadx_policy_kernel<PF_TASK_HOVER>(philox, c.cr) : quadx_policy_kernel<PF_TASK_WAYPOINTS>(philox, c.cr);
  const int grid = (ctx->n + 64 * pf::kQuadWPB - 1) / (64 * pf::kQuadWPB);
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(64 * pf::kQuadWPB), 0, s, ctx->K, *b, ctx->P_dev, ctx->n, ctx->lane0, (int)pf::OP_STEP, (const uint8_t*)nullptr,
                     k_steps, step_index0, ctx->launch_ctr, PK);
  return launched(ctx);
}
int pf_body_tick(pf_ctx* ctx, const pf_buffers* b, int n_ticks, void* stream) {
  if (!ctx || !b || !b->state || !b->wrench) return fail(ctx, PF_ERR_ARG, "pf_body_tick: state and wrench buffers are required");
  if (n_ticks < 1) return arg_fail(ctx, "pf_body_tick", "n_ticks must be >= 1");
  if (ctx->P.vehicle == PF_ROCKET) return who_fail(ctx, PF_ERR_UNSUPPORTED, "pf_body_tick", "the Rocket's mass properties change per tick; QuadX / Fixedwing only");
  const auto kernel = vehicle_kernel(ctx, pf::body_tick_kernel<pf::QuadX>, pf::body_tick_kernel<pf::Fixedwing>);
  return launch_per_lane(ctx, b, stream, kernel, n_ticks, ctx->P_dev);
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
