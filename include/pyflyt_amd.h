/*
 * pyflyt_amd.h -- C ABI of the MI355X-native batched UAV-physics step.
 *
 * Drop-in boundary for ONE hot path of jjshoots/PyFlyt (reference @ v0.30.0): `Aviary.step()` and
 * the per-drone `update_control / update_physics / update_state` loop plus the 6-DoF integrator
 * PyBullet supplies underneath it, for N independent drones at one wavefront lane per drone.
 * The reference is pure Python and has no FFI of its own; each entry point below names the
 * reference interface it replaces (file:line relative to /root/reference/PyFlyt/), and
 * INTEGRATION.md shows the ctypes binding a maintainer would add.
 *
 * Conventions
 *   - plain C, no C++/torch types; every pointer in pf_buffers is a DEVICE pointer into memory the
 *     caller owns (PyTorch-ROCm tensors: tensor.data_ptr()); the library only borrows them for the
 *     duration of a call and owns nothing but its context.
 *   - every call is asynchronous on the caller's HIP stream (`stream` = hipStream_t, e.g.
 *     torch.cuda.current_stream().cuda_stream); no internal threads, no hidden synchronisation.
 *   - every function returns 0 on success, a negative pf_status or a positive hipError_t
 *     otherwise; pf_last_error() gives the message. No exceptions cross the boundary.
 *   - one context per GPU; a context is not re-entrant.
 *   - there is NO CPU fallback: without a gfx950 device pf_ctx_create fails.
 */
#ifndef PYFLYT_AMD_H
#define PYFLYT_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PF_ABI_VERSION 10
#define PF_MAX_TARGETS 8
#define PF_MAX_BOXES 12
#define PF_MAX_SURF 5
#define PF_MAX_CONTACTS 48 /* contact vertices solved per body per tick (first in collider / vertex order) */

enum pf_status { PF_OK = 0, PF_ERR_ARG = -1, PF_ERR_UNSUPPORTED = -2, PF_ERR_NO_DEVICE = -3 };
enum pf_vehicle { PF_QUADX = 0, PF_FIXEDWING = 1, PF_ROCKET = 2 /* Aviary-level entry points and PF_TASK_ROCKET_LANDING */ };
enum pf_task { PF_TASK_NONE = 0, PF_TASK_HOVER = 1, PF_TASK_WAYPOINTS = 2, PF_TASK_MA_HOVER = 3,
               PF_TASK_DOGFIGHT = 4 /* MAFixedwingDogfightEnv (pz_envs/fixedwing_envs/ma_fixedwing_dogfight_env.py), fixedwing only */,
               PF_TASK_ROCKET_LANDING = 5 /* RocketLandingEnv (gym_envs/rocket_envs/rocket_landing_env.py), rocket + flight mode 0 only */ };
/* bits of pf_params.rl_reset_options (PF_TASK_ROCKET_LANDING): the reset's `options` (rocket_base_env.py:177-214). The reference's
 * reset(options=None) -- what gymnasium.make passes -- turns on both; options={} neither. */
enum pf_rl_option { PF_RL_RANDOMIZE_DROP = 1, PF_RL_ACCELERATE_DROP = 2 };
enum pf_noise { PF_NOISE_OFF = 0, PF_NOISE_INJECT = 1, PF_NOISE_PHILOX = 2 };
enum pf_autoreset { PF_AUTORESET_OFF = 0, PF_AUTORESET_NEXT_STEP = 1, PF_AUTORESET_SAME_STEP = 2 };

/* bits of the per-lane `flags` word (state group PF_G_INT, .y) */
enum pf_flag {
  PF_F_TERMINATED = 1, PF_F_TRUNCATED = 2, PF_F_CONTACT = 4, /* contact after the last tick */
  PF_F_INFO_COLLISION = 8, PF_F_INFO_OOB = 16, PF_F_INFO_COMPLETE = 32,
  /* a state word of the lane is NaN/Inf after an env step (the reference would carry the NaN on silently:
   * e.g. 0 * inf in the mixer's saturation rescale, quadx.py:490-491, when hi == pmin). Sticky until the
   * lane is reset; surfaced as infos["nonfinite"]; counted by bench.py. */
  PF_F_NONFINITE = 64,
  /* PF_TASK_ROCKET_LANDING: the landing-pad contact value the observation shows (its last entry). It is set by the pad check of the
   * previous Aviary step (rocket_landing_env.py:222-226 runs after compute_state), so it lags one Aviary step and is 0 after a reset. */
  PF_F_PAD_CONTACT = 128
};

typedef struct pf_pid {
  float kp[3], ki[3], kd[3], lim[3];
} pf_pid;

typedef struct pf_box {
  float c[3], h[3]; /* centre in the base frame; box: half extents, cylinder: radius, radius, half length */
  int32_t kind;     /* 0 box, 1 cylinder along the link z axis (primitive_drone.urdf:42-47 prop discs) */
  float yaw;        /* rotation of the shape's link about the base z axis (rocket.urdf:251,277 legs) */
} pf_box;

/* one lifting surface: abstractions/lifting_surfaces.py:141-239 (constants precomputed on host) */
typedef struct pf_surface {
  float r[3];                       /* link COM offset in the base frame */
  float lift[3], drag[3], torque[3]; /* unit vectors */
  float Cl_alpha_3D, inv_Cl_alpha_3D, aero_tau_eta; /* Cl3D, 1/Cl3D, aero_tau*eta */
  float flap_to_chord, inv_pi_aspect, exp_term;     /* 1/(pi*AR), 0.41*(1-exp(-17/AR)) */
  float alpha_0_base, alpha_stall_P_base, alpha_stall_N_base; /* radians */
  float Cd_0, deflection_limit_rad, dt_over_tau;
  float half_rho_area, chord;
} pf_surface;

/* All constants of one batched simulation. Filled by the host from its own parameter tables
 * (pyflyt_amd/params.py; numbers from cf2x.yaml/.urdf and fixedwing.yaml/.urdf, cited there). */
/* Rocket (drones/rocket.py, abstractions/boosters.py, gimbals.py, models/vehicles/rocket/): the fuel
 * tank's mass and inertia change every tick (boosters.py:193-198), so the composite body is rebuilt per
 * tick from these aggregates over the other ("dry") links. */
typedef struct pf_rocket {
  float dry_mass;              /* sum m_i */
  float dry_mr[3];             /* sum m_i r_i */
  float dry_S[6];              /* sum m_i ((r_i.r_i) 1 - r_i r_i^T), symmetric xx xy xz yy yz zz */
  float dry_I[3];              /* sum of the links' own (diagonal) inertias */
  float tank_r[3];             /* fuel tank link COM in the base frame */
  float total_fuel, fuel_rate_ratio /* max_fuel_rate / total_fuel */, fuel_inertia[3];
  float thrust_min_ratio /* min_thrust / max_thrust */, max_thrust, booster_dt_over_tau, booster_noise;
  int32_t reignitable;
  float booster_r[3];          /* booster link COM */
  float gimbal_dt_over_tau, gimbal_range_rad;
  float finlet_map[4][3];      /* rocket.py:152-159 */
  float starting_fuel_ratio;   /* rocket.py:47 */
} pf_rocket;

typedef struct pf_params {
  int32_t vehicle;  /* pf_vehicle */
  int32_t task;     /* pf_task */
  int32_t flight_mode;        /* quadx: -1..7 (quadx.py:233-259); fixedwing: -1, 0 */
  int32_t noise_mode;         /* pf_noise */
  int32_t autoreset;          /* pf_autoreset */
  int32_t angle_repr;         /* 0 euler, 1 quaternion (quadx_base_env.py:62-69) */
  int32_t sparse_reward;
  int32_t num_targets;
  int32_t max_steps;          /* agent_hz * max_duration_seconds (quadx_base_env.py:121) */
  int32_t env_step_ratio;     /* 120 / agent_hz (quadx_base_env.py:122) */
  int32_t settle_steps;       /* 10 (quadx_base_env.py:209) */
  int32_t ticks_per_control;  /* physics_hz / control_hz (base_drone.py:102) */
  int32_t use_gyro_term;      /* [BULLET-FROM-MEMORY] btMultiBody::m_useGyroTerm */
  int32_t throttle_remap;     /* fixedwing_base_env.py:260 */
  int32_t n_motors, n_surf, n_boxes;
  int32_t has_com_offset;
  uint64_t seed;

  /* world / integrator: aviary.py:79,226 + Bullet defaults */
  float dt, gravity_z, max_coord_vel;
  float plane_half_xy, plane_half_z;
  /* Contact RESPONSE -- what stepSimulation (core/aviary.py:516) does after collision detection. [BULLET-FROM-MEMORY]
   * throughout: a named-parameter model (NOT btMultiBodyConstraintSolver digit for digit), every doubtful Bullet fact a field
   * with the best-known default (pyflyt_amd/params.py: WORLD; the argument for each default: DESIGN.md section 3;
   * tests/golden/capture_pybullet.py prints getPhysicsEngineParameters() so that one run where PyBullet exists settles them).
   *  - Contact points against the ground slab, at the pre-integration pose: per collider BOX the four vertices of the face
   *    that looks down the most (contact_manifold_points = 4: dBoxBox2 clips the incident face and is called with maxc = 4,
   *    btPersistentManifold holds four points; 8 = every vertex), per cylinder 8 rim points on either end disc; a vertex is a
   *    point when it is at most `reach` above the slab's top face (and over the slab), reach = contact_margin for a body
   *    without contact points after the previous tick (0: dBoxBox2 returns nothing while an axis separates the boxes),
   *    contact_break_distance for one that had some (btPersistentManifold keeps a point until the gap exceeds the contact
   *    breaking threshold, 0.02 m -- what lets a body REST instead of rattling on the two corners it has not just lifted).
   *  - Rows: normal impulse >= 0 towards contact_restitution x approach speed, or towards -(gap + slop) / dt for a point
   *    still above face - slop ("do not close more than the gap this tick"); two world-axis friction rows clamped to
   *    contact_friction x normal impulse. Projected Gauss-Seidel at the velocity level in collider / vertex order: at most
   *    contact_iters sweeps (50 = PyBullet's numSolverIterations), ended early once the largest squared change of a row's
   *    velocity within a sweep is <= contact_residual_threshold (1e-7 = PyBullet's solverResidualThreshold, i.e. 3.2e-4 m/s;
   *    0: only an idle sweep ends it). Every solve starts from zero impulses: no warm start, as in Bullet's multibody
   *    solver, where it is switched off (setupMultiBodyContactConstraint: `if (0)`) [BULLET-FROM-MEMORY].
   *  - After the position update a translation of contact_erp x (deepest penetration - contact_slop) along +z.
   *  - contact_response = 0: detection only (bodies fall through the floor).
   * Contact REPORT (getContactPoints, core/aviary.py:523-525): the 15-axis box-box verdict against the other box ENLARGED by
   * contact_report_distance (0: reported from touching on) -- by contact_break_distance for a body that held contact points
   * after the previous tick.
   * Shared worlds (agents_per_world > 1, the QuadX PettingZoo task): the same model BETWEEN the drones, one stage earlier in
   * the tick -- velocities after the forces -> pair stage -> ground solve per body -> integration. Pair contacts at the
   * pre-integration poses: for every ordered pair (a, b), a != b, in agent order, every box of a against every box of b, the
   * 8 vertices of a's box in vertex order: a vertex within `reach` of being inside b's box is a contact (reach as above, the
   * breaking distance when either body held contact points), its normal the face of b with the least penetration (first axis
   * on a tie) pointing out of b, its depth that penetration; at most 16 per world and tick. Rows: the normal and Bullet's
   * btPlaneSpace1 tangents on the relative point velocity; the ground rows' targets, sweeps and residual exit, friction clamp
   * contact_friction^2 x normal impulse; after the position update each body moves half of contact_erp x (its deepest pair
   * penetration - slop) along that normal (a: +, b: -).
   * (pz_envs/quadx_envs/ma_quadx_base_env.py:365-369: a culled drone that lands on a live one.) */
  int32_t contact_response, contact_iters;
  float contact_restitution, contact_friction, contact_erp;
  float contact_margin;              /* fresh contact points: how far above the face (0) */
  float contact_slop;                /* allowed overlap (1e-5 = PyBullet's m_linearSlop): what a resting body sinks in by */
  float contact_report_distance;     /* fresh pairs are reported from this gap on (0) */
  float contact_break_distance;      /* ... persisting ones up to this gap (0.02), and keep their points up to it */
  float contact_residual_threshold;  /* squared row-velocity change that ends the sweeps (1e-7) */
  int32_t contact_manifold_points;   /* 4: the incident face of a box; 8: every vertex */
  /* composite body */
  float inv_mass;
  float com[3];
  float I_own[6], I_pa[6], I_inv[6]; /* symmetric: xx xy xz yy yz zz */
  float bound_radius;
  pf_box boxes[PF_MAX_BOXES];
  /* motors: motors.py:110-195 */
  float motor_r[4][3];
  float thrust_unit[4][3];
  float motor_dt_over_tau[4], motor_fmax[4] /* Ct*max_rpm^2 */, motor_tmax[4] /* Cq*max_rpm^2, signed */;
  float motor_noise[4];
  /* quadx */
  float motor_map[4][4];      /* quadx.py:130-137 */
  float drag_const[3];        /* boring_bodies.py:63 */
  float drag_coef_pqr;        /* cf2x.yaml:11 */
  pf_pid pid[4];              /* ang_vel, ang_pos, lin_vel, lin_pos (cf2x.yaml:13-41) */
  pf_pid zpid[2];             /* z_vel, z_pos (cf2x.yaml:43-54) */
  float control_period, inv_control_period;
  /* fixedwing */
  pf_surface surf[PF_MAX_SURF];
  int32_t assist_ids[6];      /* fixedwing.py:143 */
  float assist_signs[6];      /* fixedwing.py:144 */
  /* env */
  float start_pos[3], start_quat[4], start_vel[3];
  float dome, goal_reach_distance, min_height;
  float wp_dist_reward, wp_yaw_penalty;
  /* QuadX-Waypoints yaw targets (quadx_waypoints_env.py:40-42, waypoint_handler.py:85-89,144-156,167-179): one more
   * uniform per target at reset (drawn after all the positions), target deltas 4 wide (body-frame delta + wrapped
   * yaw error), a target counts as reached only when the yaw error is under goal_reach_angle as well */
  int32_t use_yaw_targets;
  float goal_reach_angle;
  float action_low[4], action_high[4]; /* action space box (quadx_base_env.py:80-102) */
  /* PF_TASK_MA_HOVER: agents per SHARED world (pz_envs put every agent's drone in one Bullet world,
   * ma_quadx_base_env.py:206-241). 0 / 1 = every lane alone in its world. A > 1: lanes [w A, (w+1) A) are one world -- a hit
   * between two of its drones enters both contact arrays and ends both episodes (ma_quadx_hover_env.py:181), and a contact
   * point anywhere in the world switches off every drone's rotational drag (quadx.py:509); the drones push each other (the
   * pair stage above; box colliders). A must divide 64 and the lane count, and be at most 8.
   * PF_TASK_NONE (the Aviary-level calls; QuadX or Fixedwing with plain box colliders): A in {1, 2, 4, 8} -- consecutive groups of A
   * drones are one world, the reference's N-drone Aviary (core/aviary.py:69-216) is A = N; pf_aviary_step launches the shared-world
   * step (drone-drone contacts reported in pf_buffers.out_contact_peers), pf_aviary_tick (the wind-field protocol) is unsupported. */
  int32_t agents_per_world;
  /* PF_TASK_DOGFIGHT (ma_fixedwing_dogfight_env.py:42-60): two teams of df_team_size aircraft in one shared world,
   * agents_per_world = 2 df_team_size <= 8 adjacent lanes, lanes [0, team) of a world one team, the rest the other.
   * df_sample_spawn: 1 = every reset draws the world's spawn circle (_get_start_pos_orn :176-213) from the counter RNG keyed
   * by the world's first lane; 0 = the spawn pose is read from the state's spawn groups (pos, rpy). The
   * spawn velocity is 20 m/s along the nose (:216-222). Observation = [attitude 12, surfaces + throttle 6, health, past
   * action 4] + 14 per other ACTIVE aircraft in index order (its attitude in the own body frame 12, its health, same-team
   * flag), zero padded to 23 + 14 (A - 1) (:519-549, :724-752). pf_env_step pops reward / terminated / truncated for the
   * agents still in the episode (PettingZoo parallel API: finished agents are culled, their aircraft fly on with zero
   * commands, ma_fixedwing_base_env.py:289-330); pf_params.autoreset must be PF_AUTORESET_OFF. */
  /* Filled in by pf_ctx_create (callers leave it 0): the most contact points the contact solve can see for this airframe --
   * its collider vertices (contact_manifold_points per box, 16 per cylinder), at most PF_MAX_CONTACTS. Sizes the solver's LDS regions, i.e. how many
   * lanes of a wave can be solved side by side. */
  int32_t contact_max_points;
  /* df_freeze_wrecks (default 0 = the reference's behaviour: a crashed aircraft keeps tumbling in the physics until it comes
   * to rest): 1 = an aircraft stops where it hits the ground -- velocities zeroed, not integrated any further, `inactive` from
   * the next update on. Nothing an agent is rewarded for depends on a wreck's tumbling; it spares the contact solve, which
   * otherwise dominates the step time of every wave that has an aircraft on the ground. */
  /* df_action_dim: 4 (assisted_flight=True, the default; 0 means 4) or 6 (assisted_flight=False). pf_buffers.actions is then
   * [n][df_action_dim]. With 6 the reference still leaves the Aviary in flight mode 0 (ma_fixedwing_base_env.py:229), which reads
   * setpoint[0:4] (fixedwing.py:246-250): entries 4 and 5 only appear in the observation's past action, and the thrust remap
   * of :300-301 lands on entry 5 -- the thrust command is action[3] as given. Reproduced as it is. */
  int32_t df_team_size, df_sample_spawn, df_freeze_wrecks, df_action_dim;
  float df_spawn_min_radius, df_spawn_max_radius;
  float df_damage_per_hit, df_lethal_distance, df_lethal_angle, df_aggressiveness, df_cooperativeness;
  pf_rocket rocket;
  /* ABI 10: PF_TASK_ROCKET_LANDING (gym_envs/rocket_envs/rocket_landing_env.py, rocket_base_env.py). The landing pad
   * (models/landing_pad.urdf loaded at basePosition (0, 0, 0.1), fixed): a static upright cylinder, the second collider of the world
   * next to the ground slab. A collider vertex touches the pad when its horizontal distance from the pad's axis is <= pad_radius and
   * its height lies in [pad bottom, pad top + reach] (reach: the ground slab's margin / report / break distance rule); the top face,
   * normal +z, is a contact plane of the same Gauss-Seidel solve as the slab's. The rim and the side wall are not modelled. */
  float pad_pos[3];          /* centre (0, 0, 0.1) */
  float pad_radius;          /* 2 */
  float pad_half_height;     /* 0.05: the top face at z = 0.15 */
  float ceiling;             /* z above this: out of bounds (500) */
  float max_displacement;    /* |xy| above this: out of bounds (200) */
  int32_t rl_reset_options;  /* pf_rl_option bits */
} pf_params;

/* Device buffers of one call. state layout: float4 groups, [n_groups][n_lanes][4]. The state belongs to the
 * library between calls: besides the lane's physical state it holds what the kernels prepare ahead -- for the QuadX Hover /
 * Waypoints tasks groups 7-11 carry the lane's "spare" (the random part of its NEXT episode: settled spawn state, targets) and the key
 * its next reset draws from. A caller that writes a state by hand clears bit 31 of group 7's fourth word (group 11's third in the
 * cascaded flight modes) and leaves the key in bits 0-30: the kernels then generate at the reset. A spare is only valid for the
 * context that made it (seed, lane offset, spawn pose, settle length, dome, number of targets): pf_env_reset with a NULL mask -- every
 * lane -- therefore ignores the spares it finds and prepares fresh ones, which is what a caller does first with a state buffer that
 * another context has used; a MASKED reset trusts them. The key is the event counter as the lane's previous reset left it: strictly
 * increasing from reset to reset (0 before the first).
 * QuadX env contexts in a cascaded flight mode (flight_mode != 0) on the specialised kernel without a shared world have 27 groups
 * (pf_state_groups): groups 16-26 hold the float32 REMAINDERS of values the kernel carries in fp64 -- 16-19 position, quaternion,
 * velocities, motor states; 20-21 the rate PID's memories; 22-26 the cascade's memories in the packing of groups 7-11 -- next to
 * their float32 roundings in groups 0-5 / 7-11. A hand-written state leaves them zero (the value is then its float32 word). */
typedef struct pf_buffers {
  float* state;            /* [pf_state_groups()][n][4] fp32/int32, persistent */
  const float* actions;    /* [n][4]   gym action (quadx_base_env.py:269); PF_TASK_DOGFIGHT with df_action_dim 6: [n][6];
                            * PF_TASK_ROCKET_LANDING: [n][7] finlet x, finlet y, finlet roll, ignition, throttle, gimbal 1, gimbal 2 */
  float* obs;              /* [n][pf_obs_dim()] row-major */
  float* final_obs;        /* [n][pf_obs_dim()] or NULL; written for finished lanes under SAME_STEP */
  float* reward;           /* [n] */
  uint8_t* terminated;     /* [n] */
  uint8_t* truncated;      /* [n] */
  const float* xi;         /* PF_NOISE_INJECT: [env_step_ratio*ticks_per_control][n] raw motor-noise draws */
  const float* xi_reset;   /* PF_NOISE_INJECT: [settle_steps*ticks_per_control][n] */
  const float* u_targets;  /* PF_NOISE_INJECT, waypoint tasks: [3*num_targets][n] theta|phi|dist draws (+ [num_targets][n] yaw with use_yaw_targets);
                            * PF_TASK_ROCKET_LANDING: [6][n] the reset's spawn draws as the reference takes them (rocket_base_env.py:184-189) --
                            * x, y (in +-0.1 max_displacement), z (in [0.8, 0.9] ceiling), roll, pitch, yaw (in +-0.3); read with
                            * PF_RL_RANDOMIZE_DROP only */
  /* Aviary-level calls only */
  const float* setpoints;  /* [n][4] (quadx, fixedwing mode 0), [n][6] (fixedwing mode -1) or [n][7] (rocket) */
  float* out_state;        /* [n][12]: ang_vel, ang_pos, lin_vel, lin_pos rows of Aviary.state(i) */
  float* out_aux;          /* [n][4] quadx throttle | [n][6] fixedwing surfaces + throttle | [n][9] rocket fins, ignition, fuel, throttle, gimbal */
  uint8_t* out_contact;    /* [n] contact_array[planeId] after the step, or NULL */
  const float* start_pose; /* pf_aviary_reset: [n][7] per-lane spawn (pos xyz, quat xyzw) or NULL = pf_params */
  /* wind field (pf_aviary_tick / pf_aviary_reset; ABI 2). K = pf_wind_links(): the links the reference
   * samples its wind field at -- QuadX 1 (body link, boring_bodies.py:93-96), Fixedwing 5 (surface
   * links, lifting_surfaces.py:88-93) */
  const float* wind;       /* [n][K][3] world-frame wind velocity at those links as of the previous update_state, or NULL */
  float* out_link_pos;     /* [n][K][3] world positions of those links after the call, or NULL */
  /* per-drone control rate (pf_aviary_step / pf_aviary_tick): physics ticks between controller updates of
   * each drone, a divisor of ticks_per_control (= physics_hz / the SLOWEST drone's control_hz,
   * aviary.py:288-289; drones given different `control_hz`, tests/test_core.py:34-62). NULL = uniform. */
  const int32_t* ctrl_ratio; /* [n] */
  /* per-drone flight modes (QuadX; Aviary.set_mode with a list, core/aviary.py:440-458): read by
   * pf_aviary_set_mode / _step / _tick instead of the context's mode. NULL = one mode for all. */
  const int32_t* modes;      /* [n] */
  /* per-drone spawn velocity for pf_aviary_reset (drone_options[i]["starting_velocity"], fixedwing.py:35,
   * ma_fixedwing_dogfight_env.py:218-222): world-frame linear velocity [n][3], NULL = pf_params.start_vel */
  const float* start_vel;
  /* Aviary.set_armed (core/aviary.py:423-438,510-521): a disarmed drone gets no controller update, no motor /
   * aerodynamic / drag forces and no state read-back -- PyBullet still integrates it under gravity, its
   * out_state / out_aux rows keep their last values. [n] bytes, NULL = all armed. */
  const uint8_t* armed;
  /* ABI 3 */
  /* SAME_STEP auto-reset: [n][2] int32 (flags word, targets left) of the finished episode as they were BEFORE the
   * lane was re-initialised -- gymnasium's `final_info` next to `final_obs`; NULL = not reported */
  int32_t* final_info;
  /* pf_rollout only: the sampled / consumed action of every step, [k_steps][n][4], or NULL = not stored */
  float* actions_out;
  /* pf_body_tick only: [n][6] body-frame force (3) and torque (3) applied at the base link for every tick */
  const float* wrench;
  /* ABI 9: pf_aviary_step on a context with agents_per_world = K > 1 (shared worlds, PF_TASK_NONE): [n] bytes, bit j = this drone
   * touched drone j of its world (local index 0..K-1) in some physics tick of the last Aviary step -- the drone rows of the
   * reference's contact_array (core/aviary.py:523-525); out_contact keeps its meaning (the floor). NULL = not reported. */
  uint8_t* out_contact_peers;
} pf_buffers;

typedef struct pf_ctx pf_ctx;

int pf_abi_version(void);
/* struct sizes as compiled, so that a foreign-language binding can verify its mirror of the structs */
size_t pf_sizeof_params(void);
size_t pf_sizeof_buffers(void);
/* message of the last failing call (per context, or global when ctx is NULL) */
const char* pf_last_error(const pf_ctx* ctx);

/* Replaces constructing `Aviary(...)` + the drone objects (core/aviary.py:69-216,
 * core/drones/quadx.py:22-220, fixedwing.py:18-192): binds the parameter block to a device.
 * lane_offset = global index of lane 0 (multi-GPU sharding; keys the counter-based RNG).
 * The context owns one device allocation: a copy of the parameter block (read by the rarely-taken floor paths). */
int pf_ctx_create(const pf_params* params, int n_lanes, int device, uint64_t lane_offset, pf_ctx** out);
void pf_ctx_destroy(pf_ctx* ctx);
int pf_state_groups(const pf_ctx* ctx); /* float4 groups per lane in pf_buffers.state */
int pf_obs_dim(const pf_ctx* ctx);
int pf_n_lanes(const pf_ctx* ctx);
/* which env kernel pf_env_step / pf_env_reset launch for this context: 0 the generic env_kernel, 1 the
 * specialised QuadX mode-0 kernel (Hover / Waypoints / MA-Hover), 2 the specialised Fixedwing-Waypoints kernel */
int pf_ctx_is_specialised(const pf_ctx* ctx);
/* 1 when this context's pf_env_step launches (no mask; pf_env_reset never) run the specialised QuadX kernel with the call shape fixed
 * at compile time: Hover / Waypoints, flight mode 0, contact response on, PF_NOISE_OFF or PF_NOISE_PHILOX, NEXT_STEP auto-reset,
 * the task's default env_step_ratio (Hover 3, Waypoints 4), quaternion observations, dense reward. Same state, same results bit for bit; 0 everywhere else. */
int pf_ctx_step_is_fixed(const pf_ctx* ctx);

/* env.reset(): gym_envs/quadx_envs/quadx_base_env.py:149-212 (begin_reset + end_reset incl. the
 * 10 settle Aviary steps), quadx_hover_env.py:70-83, quadx_waypoints_env.py:112-125,
 * fixedwing_waypoints_env.py:101-114. mask (device, [n] bytes) selects lanes; NULL = all. Shared worlds (agents_per_world > 1):
 * the agents of a world are reset together -- a mask that selects some of them is widened to the whole world on the device. */
int pf_env_reset(pf_ctx* ctx, const pf_buffers* b, const uint8_t* mask, void* stream);
/* env.step(action): quadx_base_env.py:269-301 / fixedwing_base_env.py:244-278 with the task's
 * compute_state + compute_term_trunc_reward, env_step_ratio x Aviary.step() (core/aviary.py:480-531)
 * fused in one launch; auto-reset per pf_params.autoreset. */
int pf_env_step(pf_ctx* ctx, const pf_buffers* b, void* stream);

/* Aviary-level surface (core/aviary.py): reset :218-312, set_mode :440-458, step :480-531 with
 * set_all_setpoints :470-478 folded in (b->setpoints), state/aux_state :335-369 -> out_state/out_aux.
 * n_steps Aviary steps are fused in one launch (setpoints held, as the reference holds them). */
int pf_aviary_reset(pf_ctx* ctx, const pf_buffers* b, void* stream);
/* setpoints_out: [n][4] (or [n][6] for fixedwing mode -1), read-modify-written with the mode's default
 * setpoint (quadx.py:275-290) */
int pf_aviary_set_mode(pf_ctx* ctx, const pf_buffers* b, int mode, float* setpoints_out, void* stream);
/* agents_per_world = K > 1: the K drones of a world exchange poses before every physics tick, collide with each other (pair
 * contacts with impulses when contact_response is on) and share the world-wide rotational-drag gate (quadx.py:509); b->out_contact
 * is the floor, b->out_contact_peers the drone-drone part of the last Aviary step's contacts. */
int pf_aviary_step(pf_ctx* ctx, const pf_buffers* b, int n_steps, void* stream);

/* ONE physics tick of Aviary.step (aviary.py:510-531), for callers that must get between the ticks:
 * a wind field (aviary.py:266-285,324-333; base_wind_field.py) is sampled by the reference in every
 * update_state at the link positions, and feeds the next tick's drag / aerodynamic velocities.
 * tick_index = position of the tick inside the Aviary step (0 .. ticks_per_control-1): the controller
 * runs at tick 0 (quadx.py:409), the motor commands are carried to the later ticks in state group 12
 * (QuadX) or recomputed from the setpoint (Fixedwing, stateless mixing). b->wind (may be NULL) is
 * subtracted from the link velocities; b->out_link_pos receives where to sample the field next;
 * b->out_contact the contact verdict of this tick. PF_NOISE_INJECT: b->xi holds this tick's draws [n].
 * The host side of the protocol is pyflyt_amd/core/aviary.py (Aviary.step with a wind field). */
/* PF_ERR_UNSUPPORTED on a context with agents_per_world > 1 (a per-tick wind field in a shared world is not implemented). */
int pf_aviary_tick(pf_ctx* ctx, const pf_buffers* b, int tick_index, void* stream);
int pf_wind_links(const pf_ctx* ctx);

/* Synthetic uniform actions inside [action_low, action_high] for benchmark rollouts
 * (the role of env.action_space.sample(), tests/test_gym_envs.py:104), keyed by
 * (seed, global lane, step_index). [n][4]; PF_TASK_ROCKET_LANDING: [n][7] in low = (-1, -1, -1, 0, 0, -1, -1), high = 1
 * (rocket_base_env.py:95-119). */
int pf_sample_actions(pf_ctx* ctx, float* actions, uint32_t step_index, void* stream);

/* k_steps consecutive env.step() calls (quadx_base_env.py:269-301 incl. auto-reset) in ONE launch with the
 * per-lane state resident in registers between the steps: the synthetic random-action rollout of
 * tests/test_gym_envs.py:100-110 (`env.step(env.action_space.sample())` in a loop) without the per-step
 * round trip of the state through HBM. Nothing is skipped: every step writes its observation, reward and
 * flags. Buffers are trajectories: b->obs [k_steps][n][obs_dim], b->reward / terminated / truncated
 * [k_steps][n], b->final_obs / final_info (SAME_STEP) [k_steps][n][..]. Actions: b->actions == NULL samples
 * step s of lane i exactly as pf_sample_actions(step_index0 + s) would (same Philox keys) and, if
 * b->actions_out != NULL, stores it there; otherwise b->actions is a given open-loop sequence
 * [k_steps][n][4] ([k_steps][n][7] for PF_TASK_ROCKET_LANDING, actions_out likewise). Results are bit-identical to
 * k_steps x (pf_sample_actions + pf_env_step).
 * State-resident on every env kernel: the specialised ones (QuadX Hover / Waypoints / multi-agent Hover with level spawns in any
 * flight mode, Fixedwing-Waypoints), the dogfight on either aircraft model (ma_fixedwing_base_env.py:272-334 in a loop,
 * tests/test_pz_envs.py:71-93; sampled actions four-wide, or a given sequence of either width [k_steps][n][4 | 6]) and the generic
 * env kernel behind every other configuration. PF_NOISE_OFF / PHILOX; PF_ERR_UNSUPPORTED for PF_NOISE_INJECT, for contexts without
 * an env task, for an auto-reset mode of OFF on the specialised single-agent kernels, and for sampling six-wide dogfight actions. */
int pf_rollout(pf_ctx* ctx, const pf_buffers* b, int k_steps, uint32_t step_index0, void* stream);

/* Closed-loop rollouts: pf_rollout with every action computed ON THE DEVICE, inside the same launch, by a small MLP policy from the
 * observation the env has just written -- the loop an on-policy learner runs (obs -> policy -> action -> env.step), without a launch
 * or a trip through HBM between the env step and the policy. (Added without a new PF_ABI_VERSION: pf_params and pf_buffers are as
 * they were, and a new function breaks no existing binding.)
 *   - WHICH OBSERVATION. Step s of lane i consumes a = mean + exp(log_std) * eps with mean = MLP(o): for s = 0, o is the lane's row
 *     of obs0; for s >= 1 the observation the env wrote for step s - 1, i.e. the row of b->obs[s - 1] (under SAME_STEP the reset
 *     observation of a lane that finished in step s - 1).
 *   - NO CLIPPING: the action is used as sampled, as the reference env uses what it is given (quadx_base_env.py:280).
 *   - RESET STEPS: a lane that NEXT_STEP resets at step s ignores its action, as in pf_env_step; actions_out still holds the sample.
 *   - NOISE: eps is standard normal, ONE Philox call per lane and step keyed by (seed, global lane, step_index0 + s, 0), stream
 *     constant 4, which no other draw uses (DESIGN.md lists them); the first four of the call's eight Box-Muller normals (16-bit
 *     uniforms: |eps| <= 4.86, resolution 2^-16 in the radius and angle draws). log_std == NULL: no call, a = mean exactly.
 *   - THE MLP: n_layers affine layers with `activation` between them, torch.nn.Linear's layout. Every sum runs bias first, then
 *     the inputs in ascending index, one fused multiply-add each, in float32; hidden widths are padded with zero weights to
 *     PF_POLICY_MAX_HIDDEN (exact). The order is fixed: results do not depend on the launch shape, and k steps in one call give
 *     the same bits as two calls of k / 2 with step_index0 advanced and obs0 pointing at the first call's last observation row.
 *     tanh is evaluated in float32 (absolute error below 2e-7).
 *   - OUTPUTS: b->actions_out [k_steps][n][4] the consumed actions, mean_out the means; every trajectory buffer as for pf_rollout.
 *     b->actions must be NULL (PF_ERR_ARG). The weights are read at every call: an optimiser step in place is seen by the next one.
 *   - ALIASING: obs0 may point INTO b->obs -- continuing a rollout in the same trajectory buffer makes it row k_steps - 1 of the very
 *     buffer the call overwrites. That is safe because each wavefront reads the obs0 rows of its own 64 lanes in its prologue, before
 *     its first step, and is the only writer of those lanes' rows of b->obs (at step k_steps - 1, last). A change that lets another
 *     wave write a lane's rows, or moves the obs0 read behind the first flush, breaks the splitting contract.
 *   - SUPPORTED: QuadX-Hover and QuadX-Waypoints on the specialised kernel (pf_ctx_is_specialised() == 1), flight mode 0, PF_NOISE_OFF
 *     or PF_NOISE_PHILOX, NEXT_STEP or SAME_STEP auto-reset, contact response on (4-point manifold) or off. Everything else -- other
 *     tasks and vehicles (shared worlds among them), the generic kernel, cascaded flight modes, PF_NOISE_INJECT, auto-reset OFF, widths
 *     over PF_POLICY_MAX_HIDDEN, and contact_response with contact_manifold_points = 8 (its solve runs out of line with a stack
 *     argument block) -- is PF_ERR_UNSUPPORTED with a message that names what is missing. */
#define PF_POLICY_MAX_HIDDEN 64
enum pf_activation { PF_ACT_TANH = 0, PF_ACT_RELU = 1 };
typedef struct pf_policy {
  int32_t n_layers;            /* 2 or 3 affine layers = 1 or 2 hidden layers */
  int32_t width[2];            /* hidden widths, 1..PF_POLICY_MAX_HIDDEN */
  int32_t activation;          /* pf_activation, on the hidden layers; the output layer is affine */
  const float* w[3];           /* device, row-major [out][in] = torch.nn.Linear.weight; in of layer 0 = pf_obs_dim(), out of the last = action width */
  const float* b[3];           /* device, [out] */
  const float* log_std;        /* device, [action width], or NULL = deterministic (action = mean) */
  const float* obs0;           /* device, [n][pf_obs_dim()]: the observation the previous call left (reset, step, or the last row of a rollout) */
  float* mean_out;             /* device, [k_steps][n][action width], or NULL */
} pf_policy;
size_t pf_sizeof_policy(void);
int pf_rollout_policy(pf_ctx* ctx, const pf_buffers* b, const pf_policy* policy, int k_steps, uint32_t step_index0, void* stream);

/* The policy of pf_rollout_policy as a launch of its own: rows in, rows out, for ANY context with an env task -- the closed loop
 * k x (pf_policy_act, pf_env_step) where pf_rollout_policy has no instantiation (Fixedwing-Waypoints, Rocket-Landing, the dogfight
 * and the multi-agent hover, the cascaded flight modes, the generic kernel, the 8-point manifold). (Added without a new
 * PF_ABI_VERSION: a new function; pf_policy is used as it is.)
 *   - ARGUMENTS: policy->obs0 the [n][D] input rows, D = pf_obs_dim(ctx) (at most 128; the widest env, an eight-aircraft dogfight
 *     with six-wide actions, has 123); actions_out [n][A], required; policy->mean_out [n][A] or NULL. A is the context's action
 *     width: 4, 6 (PF_TASK_DOGFIGHT with df_action_dim 6) or 7 (PF_TASK_ROCKET_LANDING); the last layer's `out` must equal it.
 *   - THE MLP is pf_rollout_policy's, word for word: 2 or 3 affine layers, hidden widths 1..PF_POLICY_MAX_HIDDEN, tanh or ReLU,
 *     torch.nn.Linear's [out][in] layout, read at every call. Every sum starts with the bias, then takes the inputs in ascending
 *     index with one fused multiply-add each, in float32 (computed by the float32-input matrix instruction, which is that chain bit
 *     for bit); the same float32 tanh, exp(log_std) from the same expf, a_c = fmaf(std_c, eps_c, mean_c). No clipping.
 *   - NOISE: the same draw -- ONE Philox call per lane keyed by (seed, global lane, step_index, 0), stream constant 4; eps_c is
 *     normal c of the call's eight for c < A, so six- and seven-wide heads use normals 4-6 of the same call. log_std == NULL: no
 *     call, a = mean exactly.
 *   - CONSEQUENCE: on a context that pf_rollout_policy serves, k x (pf_policy_act(step_index0 + s) on the current observation, then
 *     pf_env_step on actions_out) gives the same actions, means, observations, rewards, flags and state as
 *     pf_rollout_policy(k, step_index0).
 *   - NO RESTRICTION on vehicle, kernel family, flight mode, noise mode, auto-reset mode or manifold: it only maps rows to rows.
 *     obs0 and the outputs must not overlap.
 *   - ERRORS: PF_ERR_UNSUPPORTED for a context without an env task or a hidden width over PF_POLICY_MAX_HIDDEN; PF_ERR_ARG, the
 *     argument named, for a NULL policy / obs0 / actions_out / layer's w or b, n_layers not 2 or 3, a width below 1, an unknown
 *     activation.
 *   - Enqueued on `stream`: no host synchronisation, no allocation, no copy -- capturable in a HIP graph. The call keeps nothing in
 *     the context (no packed block: the kernel stages the caller's tensors itself), so calls on one context may run on different
 *     streams as long as their outputs are distinct. */
int pf_policy_act(pf_ctx* ctx, const pf_policy* policy, float* actions_out, uint32_t step_index, void* stream);

/* What an on-policy learner needs for every step of a rollout's trajectory before it can take a gradient step: which steps are real
 * transitions, advantages and returns by generalised advantage estimation (GAE) with the bootstrap that tells terminated from
 * truncated, and the log-probability of the action taken. Reads the trajectory buffers of pf_rollout / pf_rollout_policy (k_steps
 * rows of n lanes) and the caller's value estimates; any context with an env task. (Added without a new PF_ABI_VERSION: a new
 * function, pf_params and pf_buffers as they were.) Below, done[s] = terminated[s] | truncated[s], and done[-1] = episode_start
 * under NEXT_STEP (NULL: 0), 0 otherwise.
 *   - WHICH ROW HOLDS WHAT. values[s] is V of the observation the policy saw at step s: obs0 for s = 0, b->obs[s - 1] after;
 *     values[k_steps] is V(b->obs[k_steps - 1]). Under NEXT_STEP the row b->obs[s] of a lane that finished in step s is its TERMINAL
 *     observation, and step s + 1 ignores its action and only resets the lane (pf_env_step writes reward 0 and both flags 0 for it): it
 *     is no transition. Under SAME_STEP b->obs[s] is already the reset observation and the terminal one is b->final_obs[s]:
 *     final_values[s] = V(b->final_obs[s]), defined where done[s]; its other rows are stale and are never used.
 *   - VALID. NEXT_STEP: step s is invalid if and only if done[s - 1] (the reset step). SAME_STEP and OFF: every step is valid.
 *   - NEXT VALUE. nv[s] = values[s + 1]; under SAME_STEP nv[s] = done[s] ? final_values[s] : values[s + 1].
 *   - VALID STEPS. delta = reward[s] + gamma * (terminated[s] ? 0 : nv[s]) - values[s];
 *     advantages[s] = delta + gamma * lambda * (done[s] ? 0 : advantages[s + 1]), advantages[k_steps] = 0;
 *     returns[s] = advantages[s] + values[s]. Truncation bootstraps, termination does not; both cut the recursion.
 *   - INVALID STEPS. advantages[s] = 0, returns[s] = values[s] (the same bits), valid_out[s] = 0. Their reward goes into nothing; no
 *     output of a valid step depends on an input of an invalid one (the step under an invalid step is done: the recursion is cut there).
 *   - SELECTS. Every `?` above is a selection, not a multiplication by a mask: a NaN in a stale row of final_values, or in the
 *     reward of an invalid step, reaches no output.
 *   - LOG-PROBABILITY. logp_out[s] = sum over the A components c, in ascending c, of -1/2 z_c^2 - log_std_c - 1/2 log(2 pi) with
 *     z_c = (actions_c - mean_c) * exp(-log_std_c): the diagonal Gaussian of pf_rollout_policy's head (|z_c| <= 4.86 for the actions
 *     it sampled). For every step, valid or not. A = the context's action width (4; 6 for six-wide dogfight actions; 7 for
 *     Rocket-Landing). actions, mean, log_std and logp_out come together or are all NULL.
 *   - ARITHMETIC. float32, one fixed sequence of operations per lane: delta = fma(gamma, bootstrap, reward) - value,
 *     advantage = fma(gamma * lambda, next advantage, delta). The bits do not depend on n, on the launch shape or on the stream. No
 *     random draw.
 *   - ERRORS. PF_ERR_ARG, pf_last_error naming the argument: k_steps < 1; a NULL reward, terminated, truncated, values, advantages
 *     or returns; gamma or lambda outside [0, 1] or not finite; final_values NULL under SAME_STEP or non-NULL otherwise;
 *     episode_start non-NULL outside NEXT_STEP; some but not all of the four log-probability pointers. PF_ERR_UNSUPPORTED: a
 *     context without an env task.
 *   - Enqueued on `stream`: no host synchronisation, no allocation, no copy -- capturable in a HIP graph. */
typedef struct pf_gae_args {
  float gamma, lambda;             /* both in [0, 1] */
  const float*   reward;           /* [k][n]    */
  const uint8_t* terminated;       /* [k][n]    */
  const uint8_t* truncated;        /* [k][n]    */
  const float*   values;           /* [k+1][n]: row s = V(observation the policy saw at step s); row k = V(obs row k-1) */
  const float*   final_values;     /* [k][n] V(final_obs[s]); required under SAME_STEP, must be NULL otherwise */
  const uint8_t* episode_start;    /* [n] or NULL(= all 0): NEXT_STEP only, 1 = the lane was waiting for its reset when the rollout began */
  const float*   actions;          /* [k][n][A] consumed actions, A = the context's action width; NULL with mean/log_std/logp_out = no log-probs */
  const float*   mean;             /* [k][n][A] */
  const float*   log_std;          /* [A] */
  float* advantages;               /* [k][n] */
  float* returns;                  /* [k][n] */
  float* logp_out;                 /* [k][n] or NULL */
  uint8_t* valid_out;              /* [k][n] or NULL */
} pf_gae_args;
size_t pf_sizeof_gae(void);
int pf_gae(pf_ctx* ctx, const pf_gae_args* a, int k_steps, void* stream);

/* What a learner wraps around an env before it trains on pf_gae's batches: the return and the length of every episode that finished
 * inside a trajectory (gymnasium's RecordEpisodeStatistics), and the running moments an observation and a reward normaliser need
 * (NormalizeObservation, NormalizeReward). Reads the trajectory buffers of pf_rollout / pf_rollout_policy (k_steps rows of n lanes);
 * any context with an env task. (Added without a new PF_ABI_VERSION: a new function, pf_params and pf_buffers as they were.) Below,
 * done[s] = terminated[s] | truncated[s], and done[-1] = episode_start under NEXT_STEP (NULL: 0), 0 otherwise.
 *   - VALID. Exactly pf_gae's: under NEXT_STEP step s is invalid if and only if done[s - 1] (the step that only resets the lane);
 *     under SAME_STEP and OFF every step is valid.
 *   - CARRY. carry_return, carry_length and carry_disc [n] are the caller's, read and written: the running return, length and
 *     discounted return of every lane's open episode, so that a trajectory may be split over calls. Zero them where a lane is
 *     reset from outside.
 *   - RECURSION, ascending s, on VALID steps only: ret = ret + reward[s] (a plain float32 add, in step order); len = len + 1;
 *     G = fma(gamma, G, reward[s]). Where done[s], the finished episode is (ret, len), and then ret = 0, len = 0, G = 0. An invalid
 *     step changes nothing and contributes nothing.
 *   - PER-STEP OUTPUTS. ep_return_out[s], ep_length_out[s] = the finished episode's (ret, len) where valid[s] && done[s], 0
 *     elsewhere: done itself is their mask. Either may be NULL.
 *   - SUMMARY. summary[8], overwritten, over the episodes that finished in THIS call: count, sum of returns, sum of squared returns,
 *     min return (+inf when count is 0), max return (-inf when count is 0), sum of lengths, number that ended terminated, number
 *     that ended truncated (terminated wins when both are set).
 *   - RUNNING MOMENTS. ret_moments[3] = (count, mean, M2) of G -- after the step's update, before the cut -- over the valid steps;
 *     obs_moments[1 + 2 D] = (count, mean[D], M2[D]) of the columns of obs over the valid rows, D = pf_obs_dim(). Row s of obs is the
 *     observation the policy SAW at step s (values[s]'s observation in pf_gae). Both are updated in place: the batch's count, mean
 *     and M2 are merged into what the block holds (Chan et al.'s parallel update), so a zeroed block is the empty state and calls
 *     accumulate. variance = M2 / count. ret_moments may be NULL; obs and obs_moments come together or are both NULL.
 *   - SELECTS. The reward and the observation row of an invalid step are loaded and not selected: a NaN in them reaches no output,
 *     no carry and no moment.
 *   - ARITHMETIC. The float32 sequences above are fixed per lane: ep_return_out, ep_length_out and the carries are bit-identical
 *     whether k steps go in one call or in two of k / 2, and do not depend on n, on the launch shape or on the stream. The sums
 *     behind summary and the moments are double, about the mean the block held before the call, in an order that (n, k_steps, D)
 *     alone decide (no atomics): the same call on the same inputs gives the same bits; splitting a call moves the moments by
 *     rounding only.
 *   - ERRORS. PF_ERR_ARG, pf_last_error naming the argument: k_steps < 1; a NULL reward, terminated, truncated, summary,
 *     carry_return, carry_length or carry_disc; gamma outside [0, 1] or not finite; episode_start non-NULL outside NEXT_STEP; obs
 *     without obs_moments or the reverse. PF_ERR_UNSUPPORTED: a context without an env task; obs given on a context whose
 *     observation rows are wider than 128 floats (no env of this library is: the widest, an eight-agent dogfight's, is 123).
 *   - Enqueued on `stream`: three launches, no host synchronisation, no allocation, no copy -- capturable in a HIP graph. The
 *     partial sums between the launches live in a block the context owns (sized at pf_ctx_create from n): calls on one context
 *     must not overlap on different streams. */
typedef struct pf_traj_stats_args {
  float gamma;                     /* in [0, 1] */
  const float*   reward;           /* [k][n]    */
  const uint8_t* terminated;       /* [k][n]    */
  const uint8_t* truncated;        /* [k][n]    */
  const uint8_t* episode_start;    /* [n] or NULL(= all 0): NEXT_STEP only, as for pf_gae */
  const float*   obs;              /* [k][n][D] policy inputs, or NULL (with obs_moments) = no observation moments */
  float*   carry_return;           /* [n] in / out */
  int32_t* carry_length;           /* [n] in / out */
  float*   carry_disc;             /* [n] in / out */
  float*   ep_return_out;          /* [k][n] or NULL */
  int32_t* ep_length_out;          /* [k][n] or NULL */
  double*  summary;                /* [8] out */
  double*  ret_moments;            /* [3] in / out, or NULL */
  double*  obs_moments;            /* [1 + 2 D] in / out, or NULL */
} pf_traj_stats_args;
size_t pf_sizeof_traj_stats(void);
int pf_traj_stats(pf_ctx* ctx, const pf_traj_stats_args* a, int k_steps, void* stream);

/* pf_traj_stats with the validity of every step given by the caller: what the multi-agent envs need, whose valid steps are
 * pf_world_sync's valid_out -- zero where an agent sits a step out after its episode ended, on the step that resets its world and
 * on an opponent's lanes -- and follow from no auto-reset mode. The contract is pf_traj_stats's, word for word, except:
 *   - VALID. Step s of lane i is valid if and only if valid[s][i] != 0: in every auto-reset mode, on any context with an env task.
 *     There is no episode_start and no done[-1].
 *   - INVALID STEPS. terminated, truncated, reward and the observation row of an invalid step are loaded and NOT selected: a flag
 *     set there ends no episode (it is in no count of summary), and a NaN there reaches no output, no carry and no moment.
 *   - ERRORS. pf_traj_stats's list without the episode_start case, and PF_ERR_ARG naming `valid` when valid is NULL.
 *   - Three launches, no host synchronisation, no allocation, no copy -- capturable in a HIP graph. The partial sums live in the
 *     same context-owned block: calls on one context, of this function and of pf_traj_stats, must not overlap on different streams.
 *   - EQUIVALENCE. With valid = the mask pf_gae writes to valid_out for a NEXT_STEP trajectory (the same episode_start), or all
 *     ones under SAME_STEP / OFF, every per-step output, carry, summary word and moment has the SAME BITS as pf_traj_stats's on
 *     those inputs: a lane's sums run in step order, and the order of the double sums is decided by (n, k_steps, D) alone here too.
 *   (Added without a new PF_ABI_VERSION: a new function and a new block; pf_traj_stats_args as it was.) */
typedef struct pf_traj_stats_masked_args {
  float gamma;                     /* in [0, 1] */
  const float*   reward;           /* [k][n]    */
  const uint8_t* terminated;       /* [k][n]    */
  const uint8_t* truncated;        /* [k][n]    */
  const uint8_t* valid;            /* [k][n], required: non-zero = this step is a transition of this lane */
  const float*   obs;              /* [k][n][D] policy inputs, or NULL (with obs_moments) = no observation moments */
  float*   carry_return;           /* [n] in / out */
  int32_t* carry_length;           /* [n] in / out */
  float*   carry_disc;             /* [n] in / out */
  float*   ep_return_out;          /* [k][n] or NULL */
  int32_t* ep_length_out;          /* [k][n] or NULL */
  double*  summary;                /* [8] out */
  double*  ret_moments;            /* [3] in / out, or NULL */
  double*  obs_moments;            /* [1 + 2 D] in / out, or NULL */
} pf_traj_stats_masked_args;
size_t pf_sizeof_traj_stats_masked(void);
int pf_traj_stats_masked(pf_ctx* ctx, const pf_traj_stats_masked_args* a, int k_steps, void* stream);

/* The clipped PPO objective of a diagonal-Gaussian policy over M rows of a batch, its statistics, and its gradients with respect to
 * the actor's means, the critic's values and log_std: everything between the outputs of the caller's two networks and their
 * output-gradients, in one call. Any context, with an env task or without: it serves the error string and owns the partial sums.
 * rows = M >= 1 is any number of rows (a whole pf_gae batch flattened, or a gathered minibatch); width = A in 1..8. (Added without
 * a new PF_ABI_VERSION: a new function, pf_params and pf_buffers as they were.) Below, c = the number of valid rows, w = 1 / c.
 *   - ADVANTAGE. With normalize_advantage: mu = sum A / c and sigma = sqrt(sum (A - mu)^2 / c) over the valid rows (the population
 *     form), both accumulated in double; a_i = (A_i - mu32) * inv32 with mu32, inv32 the float32 roundings of mu and of
 *     1 / max(sigma, 1e-8). Without it a_i = A_i. No gradient flows through mu or sigma.
 *   - LOG-PROBABILITY. Exactly pf_gae's: logp_i = sum over c, ascending from 0, of -1/2 z_c^2 - log_std_c - 1/2 log(2 pi) with
 *     z_c = (actions_c - mean_c) * exp(-log_std_c).
 *   - SURROGATE. r = exp(logp - logp_old); u = r * a; v = clamp(r, 1 - clip, 1 + clip) * a. The row contributes -w min(u, v) to
 *     policy_loss. The gradient branch is live where u <= v: there d loss / d logp = -w a r; elsewhere it is 0.
 *   - VALUE. value_loss = 1/2 sum w (value - returns)^2; grad_value_i = vf_coef w (value_i - returns_i). No value clipping.
 *   - ENTROPY. H = sum_c (log_std_c + 1/2 (1 + log 2 pi)): state-independent.
 *   - LOSS. loss = policy_loss + vf_coef * value_loss - ent_coef * H.
 *   - GRADIENTS. grad_mean_ic = (d loss / d logp_i) z_ic exp(-log_std_c);
 *     grad_log_std_c = sum_i (d loss / d logp_i) (z_ic^2 - 1) - ent_coef.
 *   - STATS. stats[16], overwritten: 0 c; 1 loss; 2 policy_loss; 3 value_loss; 4 H; 5 approx_kl = sum w ((r - 1) - (logp - logp_old));
 *     6 clip_fraction = sum w [|r - 1| > clip]; 7 mu; 8 sigma (computed whether or not they are applied); 9 explained variance
 *     1 - Var(returns - value) / Var(returns) over the valid rows; 10 min r; 11 max r; 12-15 0.
 *   - INVALID ROWS (valid_i = 0; valid NULL = every row is valid). Their grad_mean row and grad_value entry are exactly 0 and they
 *     enter no sum. Every such choice is a selection, not a multiplication by a mask: a NaN anywhere in an invalid row reaches no
 *     output. With c = 0 every gradient is 0 except grad_log_std = -ent_coef; slots 1-3 and 5-8 are 0 apart from the entropy term
 *     of slot 1; slot 9 is NaN; slots 10 / 11 are +inf / -inf.
 *   - ARITHMETIC. Per row one fixed float32 sequence (w enters it as the float32 rounding of 1 / c). All sums are double, in an
 *     order that (rows, width) alone decide; no atomics: the same call on the same inputs gives the same bits whatever the stream,
 *     and whether the four-wide rows are 16-byte aligned or not.
 *   - ERRORS. PF_ERR_ARG, pf_last_error naming the argument: rows < 1; width outside 1..8; any NULL pointer other than valid;
 *     clip not finite or <= 0; vf_coef or ent_coef negative or not finite; normalize_advantage other than 0 / 1.
 *   - Enqueued on `stream`: four launches, no host synchronisation, no allocation, no copy -- capturable in a HIP graph. The partial
 *     sums between the launches live in a fixed-size block the context allocates at pf_ctx_create (the grid is capped at 1024
 *     blocks, so its size does not depend on rows): calls on one context must not overlap on different streams. */
typedef struct pf_ppo_loss_args {
  float clip;                      /* > 0 */
  float vf_coef, ent_coef;         /* >= 0 */
  int32_t normalize_advantage;     /* 0 / 1 */
  const float*   mean;             /* [M][A] the new policy's means */
  const float*   log_std;          /* [A] */
  const float*   actions;          /* [M][A] */
  const float*   logp_old;         /* [M] */
  const float*   advantages;       /* [M] */
  const float*   returns;          /* [M] */
  const float*   value;            /* [M] the new critic's output */
  const uint8_t* valid;            /* [M] or NULL(= all 1) */
  float*  grad_mean;               /* [M][A] */
  float*  grad_value;              /* [M] */
  float*  grad_log_std;            /* [A] */
  double* stats;                   /* [16] */
} pf_ppo_loss_args;
size_t pf_sizeof_ppo_loss(void);
int pf_ppo_loss(pf_ctx* ctx, const pf_ppo_loss_args* a, size_t rows, int width, void* stream);

/* The two networks of a PPO epoch without a GEMM library: a small MLP over any number of rows, and from the output-gradients of those
 * rows (pf_ppo_loss's grad_mean / grad_value) the gradients of every weight and bias. With them an epoch is pf_mlp_forward ->
 * pf_ppo_loss -> pf_mlp_backward -> the optimiser's step, and no hidden activation is ever written to memory. The context serves its
 * device and pf_last_error only: any context works, with an env task or without. (Added without a new PF_ABI_VERSION: new functions;
 * pf_policy and every other struct as they were.)
 *   - THE NETWORK is pf_policy_act's family: 2 or 3 affine layers, hidden widths 1..PF_POLICY_MAX_HIDDEN, tanh or ReLU between them,
 *     torch.nn.Linear's [out][in] layout, read at every call; in_dim 1..128, out_dim 1..8 (the critic's 1 included).
 *   - FORWARD. out[r] = MLP(x[r]) for x [rows][in_dim], out [rows][out_dim], with pf_policy_act's arithmetic word for word -- it is
 *     the same kernel, launched with the draw off: every sum starts with the bias, then takes the inputs in ascending index with one
 *     float32 fused multiply-add each; the same float32 tanh. For in_dim = pf_obs_dim(), out_dim = the action width and the same
 *     rows, `out` holds the bits of pf_policy_act's mean_out.
 *   - BACKWARD. grad_w[l][j][i] = sum over the rows r of delta_l[r][j] * in_l[r][i], grad_b[l][j] = sum_r delta_l[r][j], where in_0 = x,
 *     in_l = h_(l-1) = act(layer l - 1), delta_last = grad_out [rows][out_dim], delta_l = (delta_(l+1) W_(l+1)) * act'(h_l),
 *     act' = 1 - h^2 for tanh and (h > 0 ? 1 : 0) for ReLU. The hidden activations are computed again from x: the forward saves
 *     nothing and there is no state between the two calls. No gradient is produced for x.
 *   - ARITHMETIC. float32 on the float32-input matrix instruction. Each 64-row tile's products start from zero and are added to its
 *     workgroup's running float32 sums; a workgroup writes one block of partial sums to `workspace`, and a second launch adds the
 *     workgroups' blocks in ascending order in double and rounds to float32. The grid is a function of `rows` alone and there are
 *     no atomics: the same call on the same inputs gives the same bits on any stream and at every repetition.
 *   - ZERO ROWS. A row whose grad_out is all +0 contributes exact zeros, PROVIDED ITS x IS FINITE: the row's activations are still
 *     computed and multiplied by the zero deltas, so a NaN or an infinity in x poisons the sums even under a zero gradient (0 * NaN).
 *     pf_ppo_loss's zeroed invalid rows are safe: the reset rows of a NEXT_STEP trajectory hold finite terminal observations. Rows
 *     past `rows` are never read: the ragged last tile masks its deltas to zero.
 *   - WORKSPACE. The caller's, at least pf_mlp_backward_workspace_bytes(mlp, rows) bytes (a pure host function of the network's shape
 *     and of rows: it grows with rows up to the grid's cap and is constant from there; 0 for a shape the calls refuse). Its contents
 *     mean nothing before or after the call.
 *   - ERRORS. PF_ERR_ARG, pf_last_error naming the argument: a NULL ctx, mlp, x, out, grad_out, grad_w, grad_b, workspace, layer's w /
 *     b / grad_w / grad_b; rows < 1 (or 2^31 - 64 and more); n_layers not 2 or 3; a width outside 1..64; in_dim outside 1..128;
 *     out_dim outside 1..8; an unknown activation; workspace_bytes too small (refused by size, before any launch); x, grad_out,
 *     workspace or an output overlapping one another (forward: x and out).
 *   - Enqueued on `stream`: one launch (forward), two (backward); no host synchronisation, no allocation, no copy -- capturable in a
 *     HIP graph. Calls on one context may run on different streams as long as their outputs and workspaces are distinct. */
typedef struct pf_mlp {
  int32_t n_layers;      /* 2 or 3 affine layers = 1 or 2 hidden layers */
  int32_t width[2];      /* hidden widths, 1..PF_POLICY_MAX_HIDDEN */
  int32_t activation;    /* pf_activation, on the hidden layers; the output layer is affine */
  int32_t in_dim;        /* 1..128 */
  int32_t out_dim;       /* 1..8 */
  const float* w[3];     /* device, row-major [out][in] = torch.nn.Linear.weight */
  const float* b[3];     /* device, [out] */
} pf_mlp;
size_t pf_sizeof_mlp(void);
int pf_mlp_forward(pf_ctx* ctx, const pf_mlp* mlp, const float* x, int64_t rows, float* out, void* stream);
size_t pf_mlp_backward_workspace_bytes(const pf_mlp* mlp, int64_t rows);
int pf_mlp_backward(pf_ctx* ctx, const pf_mlp* mlp, const float* x, const float* grad_out, int64_t rows, float* const grad_w[3],
                    float* const grad_b[3], void* workspace, size_t workspace_bytes, void* stream);

/* A PPO epoch's parameter gradients from x in one call. By definition the semantics are those of the composition
 * pf_mlp_forward(actor), pf_mlp_forward(critic), pf_ppo_loss, pf_mlp_backward(actor, grad_mean), pf_mlp_backward(critic, grad_value) on
 * the same inputs, rows = M and width = actor->out_dim: every clause of pf_ppo_loss and of pf_mlp_forward / pf_mlp_backward above
 * holds, ZERO ROWS included (an invalid row's x must be finite), and every weight and bias gradient has the bits the composition
 * gives. Any context. (Added without a new PF_ABI_VERSION: new functions, every existing struct as it was.) What differs:
 *   - NO mean, value, grad_mean or grad_value tensor exists: a tile's 64 rows of them live in the workgroup's LDS.
 *   - LAUNCHES. Seven: pf_ppo_loss's two advantage kernels; the backward's tile kernel once per network, with the output layer and
 *     pf_ppo_loss's per-row float32 sequence in the place of its load of grad_out; the backward's reduction once per network;
 *     pf_ppo_loss's finish kernel. Enqueued on `stream`, no host synchronisation, no allocation, no copy -- capturable in a HIP graph.
 *     The advantage block is the context's, shared with pf_ppo_loss: calls of either on one context must not overlap on different
 *     streams.
 *   - WORKSPACE. The caller's, 8-byte aligned, at least pf_ppo_grad_workspace_bytes(actor, critic, rows) bytes (a pure host function
 *     of the two shapes and of rows: it grows with rows up to the grid's cap and is constant from there; 0 for what the call
 *     refuses). It holds both networks' blocks of partial sums and the rows of double partials behind stats and grad_log_std.
 *   - THE DOUBLE SUMS behind stats and grad_log_std take the same per-row terms in another order than pf_ppo_loss's (one row of
 *     partials per workgroup of the tile kernel, at most 256, instead of one per 256-row block, at most 1024): those two outputs
 *     agree with pf_ppo_loss's within the reordering of a double sum; slots 0, 7, 8, 10 and 11 are the same bits. The order is a
 *     function of (rows, the two shapes) alone and there are no atomics: the same call gives the same bits on any stream.
 *   - ERRORS. PF_ERR_ARG, pf_last_error naming the argument: a NULL ctx, argument block, actor, critic, layer's w / b, or any pointer
 *     other than valid; rows < 1 (or 2^31 - 64 and more); a network shape pf_mlp_backward refuses, in its words after "actor: " or
 *     "critic: "; critic->out_dim != 1; critic->in_dim != actor->in_dim; pf_ppo_loss's coefficient checks; workspace_bytes too small
 *     (refused by size, before any launch) or workspace not 8-byte aligned; the workspace or an output overlapping an input or
 *     one another. */
typedef struct pf_ppo_grad_args {
  float clip;                      /* > 0 */
  float vf_coef, ent_coef;         /* >= 0 */
  int32_t normalize_advantage;     /* 0 / 1 */
  const pf_mlp* actor;             /* host pointer; out_dim = A in 1..8 */
  const pf_mlp* critic;            /* host pointer; out_dim = 1, in_dim = actor->in_dim */
  const float*   x;                /* [M][in_dim] */
  const float*   log_std;          /* [A] */
  const float*   actions;          /* [M][A] */
  const float*   logp_old;         /* [M] */
  const float*   advantages;       /* [M] */
  const float*   returns;          /* [M] */
  const uint8_t* valid;            /* [M] or NULL(= all 1) */
  float*  actor_grad_w[3];         /* shaped like the parameters; the first n_layers are used */
  float*  actor_grad_b[3];
  float*  critic_grad_w[3];
  float*  critic_grad_b[3];
  float*  grad_log_std;            /* [A] */
  double* stats;                   /* [16], pf_ppo_loss's slots */
} pf_ppo_grad_args;
size_t pf_sizeof_ppo_grad(void);
size_t pf_ppo_grad_workspace_bytes(const pf_mlp* actor, const pf_mlp* critic, int64_t rows);
int pf_ppo_grad(pf_ctx* ctx, const pf_ppo_grad_args* a, int64_t rows, void* workspace, size_t workspace_bytes, void* stream);

/* The optimiser's step of a PPO epoch: Adam / AdamW with global gradient-norm clipping over a set of 1..PF_ADAM_MAX_TENSORS float32
 * parameter tensors, in two launches. With it an epoch is pf_mlp_forward -> pf_ppo_loss -> pf_mlp_backward -> pf_adam_step and holds
 * nothing but this library's launches. The context serves its device and pf_last_error only: any context works, with an env task or
 * without. (Added without a new PF_ABI_VERSION: new functions; every other struct as it was.)
 *   - NORM. norm = sqrt(sum over every element of every tensor of g^2): each square and every sum in double, in an order that
 *     numel[] alone decides; no atomics.
 *   - CLIP. coef = min(1, max_grad_norm / (norm + 1e-6)), torch.nn.utils.clip_grad_norm_'s form, in double: exactly 1 where clipping
 *     is off (max_grad_norm = +infinity) or not reached. g' = g * coef32 with coef32 the float32 rounding of coef (a multiplication
 *     by 1 where coef is 1: the same bits as no clip). grad[] itself is never written.
 *   - STEP. t = state[0] + 1, and with lr the learning rate of this call (*lr_dev, read on the device at every call, where lr_dev is
 *     given; the argument lr otherwise), torch.optim.Adam's / AdamW's update:
 *         p *= 1 - lr weight_decay                 (only where weight_decay > 0: decoupled, AdamW; 0 = plain Adam)
 *         m  = m + (1 - beta1) (g' - m)
 *         v  = beta2 v + (1 - beta2) g'^2
 *         p -= (lr / (1 - beta1^t)) m / (sqrt(v) / sqrt(1 - beta2^t) + eps)
 *     The hyperparameters are the float32 values of this block: beta2 = 0.999f is 0.99900001287..., and that is the beta2 applied.
 *   - ARITHMETIC. The launch-uniform scalars are computed once in double from those values and rounded to float32: coef32,
 *     decay = 1 - lr weight_decay, omb1 = 1 - beta1, omb2 = 1 - beta2, nstep = -lr / (1 - beta1^t), c2 = sqrt(1 - beta2^t) (the two
 *     powers by double pow). Per element one fixed float32 sequence, every operation correctly rounded:
 *         gc = g * coef32;  p0 = weight_decay > 0 ? p * decay : p;
 *         m = fmaf(omb1, gc - m, m);  v = fmaf(omb2, gc * gc, beta2 * v);
 *         p = fmaf(nstep, m / (sqrtf(v) / c2 + eps), p0)
 *     with a fused multiply-add exactly where fmaf is written and nowhere else.
 *   - STATE. state[8], double, read and then overwritten: 0 t, the steps taken; 1 norm, before clipping; 2 coef; 3 the learning rate
 *     used; 4 the number of skipped calls so far; 5-7 0. A zeroed block with zeroed exp_avg / exp_avg_sq is a fresh optimiser.
 *   - SKIP. With skip_nonfinite = 1 and a norm that is not finite, no parameter, no moment and not t changes; slot 4 is incremented,
 *     slot 1 reports the norm and slot 2 a coef of 0. The decision is taken on the device and is a selection, not a multiplication
 *     by a mask. With skip_nonfinite = 0 the arithmetic runs as written and a NaN spreads as it does in torch (an infinite norm
 *     under a finite max_grad_norm gives coef 0 and 0 * inf = NaN in that element; under max_grad_norm = +infinity coef is NaN).
 *   - DETERMINISM. The grid is a function of numel[] alone: the same call on the same inputs gives the same bits on any stream and
 *     at every repetition. A tensor whose four pointers are 16-byte aligned moves as float4s, any other element by element; the
 *     arithmetic is elementwise and an element belongs to the same thread either way, so the bits do not depend on the alignment.
 *   - WORKSPACE. The caller's, at least pf_adam_workspace_bytes(the total of numel[]) bytes (a pure host function: it grows with
 *     the total up to the grid's cap and is constant from there; 0 for a total below 1 or of 2^31 and more). It holds the partial
 *     sums of the norm and what the first launch read of `state`; its contents mean nothing before or after the call.
 *   - ERRORS. PF_ERR_ARG, pf_last_error naming the argument: a NULL ctx, argument block, state, workspace, or param[i] / grad[i] /
 *     exp_avg[i] / exp_avg_sq[i]; n_tensors outside 1..32; a numel[i] < 1, or a total of 2^31 or more; lr negative or not finite
 *     while lr_dev is NULL; beta1 or beta2 outside [0, 1); eps not > 0 or not finite; weight_decay negative or not finite;
 *     max_grad_norm not > 0 (a NaN included); skip_nonfinite other than 0 / 1; workspace_bytes too small (refused by size, before
 *     any launch); any two of the 4 n tensor ranges, state, workspace and lr_dev overlapping (both are named).
 *   - Enqueued on `stream`: two launches, no host synchronisation, no allocation, no copy -- capturable in a HIP graph. The tensor
 *     pointers travel in the kernel arguments: there is no descriptor table in device memory. The call keeps nothing in the
 *     context, so calls with distinct workspaces, states and tensors may run on different streams. */
#define PF_ADAM_MAX_TENSORS 32
typedef struct pf_adam_args {
  int32_t n_tensors;            /* 1..PF_ADAM_MAX_TENSORS */
  int32_t skip_nonfinite;       /* 0 / 1 */
  float   lr;                   /* used when lr_dev is NULL; finite, >= 0 */
  const float* lr_dev;          /* device, [1], or NULL: read by the kernel at every call */
  float   beta1, beta2;         /* in [0, 1) */
  float   eps;                  /* > 0 */
  float   weight_decay;         /* >= 0, decoupled (AdamW); 0 = plain Adam */
  float   max_grad_norm;        /* > 0; +infinity = no clipping (the norm is still reported) */
  int64_t numel[PF_ADAM_MAX_TENSORS];
  float*       param[PF_ADAM_MAX_TENSORS];
  const float* grad[PF_ADAM_MAX_TENSORS];
  float*       exp_avg[PF_ADAM_MAX_TENSORS];
  float*       exp_avg_sq[PF_ADAM_MAX_TENSORS];
  double* state;                /* device, [8], in / out */
} pf_adam_args;
size_t pf_sizeof_adam(void);
size_t pf_adam_workspace_bytes(int64_t total_numel);
int pf_adam_step(pf_ctx* ctx, const pf_adam_args* a, void* workspace, size_t workspace_bytes, void* stream);

/* PPO's usual options, which nothing around the library can add (the means and values of pf_ppo_grad never exist as tensors):
 * pf_ppo_loss_opt and pf_ppo_grad_opt are pf_ppo_loss and pf_ppo_grad with a clipped value loss and a penalty on means that leave the
 * action box. Same argument blocks, workspaces and number of launches; every clause of those two contracts holds, and what the
 * options add is stated here. (Added without a new PF_ABI_VERSION: new functions and a new block, every existing struct as it was.)
 *   - OPTIONS OFF. With options == NULL, or with values_old == NULL and bounds_coef == 0, the call IS pf_ppo_loss / pf_ppo_grad (the
 *     same kernels are launched): every output has their bits, stats[12..15] = 0. An option that is on leaves the other's outputs
 *     as they are: value clipping alone gives pf_ppo_loss's grad_mean bits, the bounds loss alone its grad_value bits.
 *   - VALUE CLIPPING (values_old given). Per row, V the new value, R the return, kv = vf_coef * w32, all float32:
 *         e = V - V_old;  out = |e| > clip_vf;  vc = e > 0 ? V_old + clip_vf : V_old - clip_vf;
 *         dv = V - R;  dc = vc - R;  use_c = out && dc^2 > dv^2      (decided exactly: it is |dc| > |dv|)
 *     The row adds (use_c ? dc : dv)^2 to the value-loss sum, the square taken in double from the float32 difference:
 *     value_loss = 1/2 sum w (...). grad_value = use_c ? 0 : kv * dv. A row inside the clip range takes pf_ppo_loss's path exactly
 *     (there is no V_old + (V - V_old) round trip). The sums behind slot 9 stay those of V - R. stats[12] = sum w [out] over the
 *     valid rows: a whole-number count times w, exact like slot 6. Every choice is a select: a NaN in an invalid row's values_old
 *     reaches nothing.
 *   - BOUNDS LOSS (bounds_coef > 0). Per row and column c < A, float32: hx = fmaxf(m_c - hi_c, 0), lx = fmaxf(lo_c - m_c, 0); the
 *     row's term is b = sum_c (hx * hx + lx * lx), c ascending from 0. bounds_loss = sum w b over the valid rows, in double,
 *     reported in stats[13]; loss (slot 1) gains bounds_coef * bounds_loss. grad_mean_ic gains ((2 * bounds_coef) * w32) * (hx - lx),
 *     added in float32 to the surrogate's term on every valid row, whether or not its surrogate branch is live; invalid rows stay
 *     exact zeros by selection. grad_log_std has no bounds term. stats[14] and stats[15] stay 0.
 *   - pf_ppo_grad_opt is, by definition, pf_mlp_forward x 2 -> pf_ppo_loss_opt -> pf_mlp_backward x 2 on the same inputs: the network
 *     gradients have the composition's bits; grad_log_std and the summed stats agree within the reordering of a double sum, as for
 *     pf_ppo_grad; slots 0, 7, 8, 10, 11 and 12 are the same bits. The critic's launch reads values_old, one more [M] stream.
 *   - ERRORS, beyond those of pf_ppo_loss / pf_ppo_grad. PF_ERR_ARG, pf_last_error naming the argument: clip_vf not finite or <= 0
 *     while values_old is given; bounds_coef negative or not finite; a NaN bound, or lo > hi, in the first A columns (read only when
 *     bounds_coef > 0); pf_ppo_grad_opt: values_old overlapping an output or the workspace. */
typedef struct pf_ppo_options {
  float clip_vf;             /* finite, > 0; read only when values_old != NULL */
  const float* values_old;   /* [M], the batch's values; NULL = no value clipping */
  float bounds_coef;         /* finite, >= 0; 0 = no bounds loss */
  float bounds_lo[8], bounds_hi[8];  /* the first A are used; lo <= hi; -inf / +inf = open on that side; NaN refused */
} pf_ppo_options;
size_t pf_sizeof_ppo_options(void);
int pf_ppo_loss_opt(pf_ctx* ctx, const pf_ppo_loss_args* a, const pf_ppo_options* options, size_t rows, int width, void* stream);
int pf_ppo_grad_opt(pf_ctx* ctx, const pf_ppo_grad_args* a, const pf_ppo_options* options, int64_t rows, void* workspace, size_t workspace_bytes,
                    void* stream);

/* A minibatch of a PPO epoch without a gathered copy: pf_ppo_grad_opt on the m rows of a batch of rows_total rows that an index list
 * names. By definition the call is pf_ppo_grad_opt(ctx, a', options', m, ...) with t'[j] = t[row_index[j]] for every per-row tensor t:
 * x, actions, logp_old, advantages, returns, valid and options->values_old. No row is moved: the kernels read their rows through the
 * index. Every clause of pf_ppo_grad / pf_ppo_grad_opt holds (options == NULL or off: pf_ppo_grad's kernels' arithmetic); what
 * differs is stated here. (Added without a new PF_ABI_VERSION: a new function, every existing struct as it was.)
 *   - BIT IDENTITY. Every sum order of pf_ppo_grad is a function of (rows, the two shapes) alone, so every output -- all weight and
 *     bias gradients, grad_log_std and all sixteen stats slots -- has the bits of pf_ppo_grad_opt on contiguous gathered copies.
 *   - PER MINIBATCH. c, w = 1 / c, mu and sigma are taken over the m indexed rows: the advantages are normalised per minibatch.
 *   - THE INDEX. row_index: device, [m], int32. Duplicates are allowed (rows are only read). A row of the batch that no index names
 *     is never read (but for row 0 under OUT OF RANGE, where nothing of it is chosen): it may hold NaN, in x too.
 *   - OUT OF RANGE. An index outside [0, rows_total) is never dereferenced. Its slot is an invalid row by selection: zero gradient,
 *     in no sum, not counted in c. In its place row 0 of every per-row tensor is loaded and not chosen; the slot's x is zeros (row 0
 *     of x need not be finite). stats[14] = the number of such slots, 0 where there are none (pf_ppo_grad_opt always writes 0).
 *   - LAUNCHES AND WORKSPACE. The same seven launches, with the row numbers taken through the index; no atomics, no allocation, no
 *     copy, no host synchronisation -- capturable. The workspace is pf_ppo_grad's, of pf_ppo_grad_workspace_bytes(actor, critic, m).
 *   - ERRORS, beyond those of pf_ppo_grad_opt (whose `rows` is m here). PF_ERR_ARG, pf_last_error naming the argument: m < 1 or
 *     m >= 2^31 - 64; rows_total < 1 or rows_total >= 2^31 - 64; row_index NULL (these three first, in this order, before the context
 *     is looked at); row_index overlapping an output or the workspace. The overlap checks on the inputs use their extents of
 *     rows_total rows, not m. */
int pf_ppo_grad_rows(pf_ctx* ctx, const pf_ppo_grad_args* a, const pf_ppo_options* options /* may be NULL */,
                     const int32_t* row_index /* device, [m] */, int64_t m, int64_t rows_total,
                     void* workspace, size_t workspace_bytes, void* stream);

/* SHARDED PPO: the gradient of ONE batch from shards of it that live on several devices, one context (and stream) per device. Adding
 * up the outputs of pf_ppo_grad_rows on the shards is wrong: each call normalises the advantages over its own rows and weights its
 * rows by 1 / (its own valid count). Here c, w = 1 / c, mu and sigma come from ALL shards and the raw sums are combined before the
 * finish formulas run, so the result is the joint batch's. The order of a step:
 *     per shard:  pf_ppo_adv_sums                      -> 4 doubles          (copied to the combining device by the caller)
 *     once:       pf_adv_sums_add                      -> the global block   (copied back to every shard's device)
 *     per shard:  pf_ppo_grad_shard                    -> the shard's share of the gradients, its block of raw totals
 *     once:       pf_ppo_shard_combine                 -> the gradients, grad_log_std and stats of the joint batch
 * The library makes no copy between devices and uses no collective: the caller moves 4 doubles, PF_PPO_SHARD_WORDS doubles and one
 * flat gradient buffer per shard. Any context. Every call is enqueued on `stream`: no host synchronisation, no allocation, no
 * copy, no atomics -- capturable in a HIP graph; the same inputs give the same bits on any stream and at every repetition. (Added
 * without a new PF_ABI_VERSION: new functions and a new block, every existing struct as it was.)
 *   - pf_ppo_adv_sums. sums[4], device, double: 0 the valid count c of the m rows (row_index NULL: rows 0..m-1 of the batch, and
 *     rows_total is ignored) or of the m slots of row_index into a batch of rows_total rows; 1 sum A; 2 sum A^2, each square and every
 *     sum in double about 0; 3 the slots whose index lay outside [0, rows_total) (0 without row_index). These are the totals that
 *     pf_ppo_grad / pf_ppo_grad_rows form from the same rows in the same order before they divide: mu = sums[1] / c,
 *     sigma = sqrt(max(sums[2] / c - mu^2, 0)). Three launches into the context's advantage block: a call must not overlap another
 *     pf_ppo_* call on the same context on a different stream. ERRORS (PF_ERR_ARG, the argument named): m < 1 or m >= 2^31 - 64
 *     (first, before the context is looked at); a NULL ctx, advantages or sums; with row_index, rows_total < 1 or >= 2^31 - 64;
 *     sums overlapping an input.
 *   - pf_adv_sums_add. dst[4] = src[0] + src[1] + ... + src[n_src - 1], element by element, in double, in that order. n_src in
 *     1..PF_PPO_MAX_SHARDS; `src` is a HOST array of device pointers. ERRORS: n_src out of range (first); a NULL ctx, dst, src or
 *     src[g]; dst overlapping a src[g].
 *   - pf_ppo_grad_shard is pf_ppo_grad_opt (row_index NULL: the shard is rows 0..m-1 of a's tensors) or pf_ppo_grad_rows (the shard is
 *     the m slots of row_index) with three differences:
 *       (a) c, w32 = float32(1 / c), mu32 and inv32, which every row's float32 sequence applies, come from adv_sums[0..2] -- the
 *           sums of ALL shards -- by the formulas above. The shard's own advantage pass still runs, to count its valid rows and its
 *           out-of-range slots.
 *       (b) a->stats and a->grad_log_std must be NULL: they are outputs of the joint batch. In their place shard_block
 *           [PF_PPO_SHARD_WORDS], device, double, receives the raw totals the finish formulas read, over this shard's valid rows:
 *               0 sum min(u, v)      1 sum (V - R)^2     2 sum (r - 1) - d    3 rows with |r - 1| > clip
 *               4 sum R              5 sum R^2           6 sum (V - R)        7 min r (+inf: no valid row)   8 max r (-inf)
 *               9..16 the sums behind grad_log_std[0..7], without the -ent_coef (0 from A on)
 *               17 sum of the chosen squared value error (value clipping)   18 rows with |V - V_old| > clip_vf   19 sum b (bounds)
 *               20 this shard's valid count    21 its out-of-range slots    22, 23 0
 *           Words 17-19 are 0 in a call without options (an option that is off leaves a sum nobody reads). Words 0-19 have the bits
 *           of the totals pf_ppo_grad_rows forms on the same rows.
 *       (c) the weight and bias gradients written are this shard's SHARE of the joint gradient: already weighted by the global w32,
 *           to be added to the other shards', not averaged.
 *     The workspace (pf_ppo_grad_workspace_bytes(actor, critic, m)), the overlap checks and the refusals are pf_ppo_grad_rows's, with
 *     row_index allowed to be NULL (rows_total is then not read); in addition: a non-NULL a->stats or a->grad_log_std; a NULL
 *     adv_sums or shard_block; either overlapping anything. Eight launches. A shard without a valid row is fine: zero gradients.
 *   - pf_ppo_shard_combine. blocks[g], grads[g]: shard g's block and ONE flat contiguous buffer of numel floats -- all gradient
 *     tensors of both networks in a layout the caller chooses and gives pf_ppo_grad_shard views into; adv_sums: the global block.
 *       grad_out[i] = float32(grads[0][i] + grads[1][i] + ... in double, g ascending), i < numel.
 *       Every raw total is the sum of the shards' words in ascending shard order, in double; words 7 / 8 the min / max. stats[16]
 *       and grad_log_std[width] are what pf_ppo_grad_rows' finish formulas make of those totals, c, mu and sigma from adv_sums:
 *       slot 0 the global c, slots 7 / 8 mu and sigma, slot 14 the sum of the shards' out-of-range counts. With ONE shard every
 *       output has the bits of pf_ppo_grad_rows (pf_ppo_grad_opt) on that shard's rows.
 *     vclip / bnd: 0 / 1, whether the shards ran with value clipping (slots 3 and 12 then come from words 17 and 18) / with the
 *     bounds loss (slot 13 from word 19, and the loss gains bounds_coef times it).
 *     Two launches. ERRORS: n_shards outside 1..PF_PPO_MAX_SHARDS (first); a NULL ctx, argument block, blocks[g] or grads[g] with
 *     g < n_shards, adv_sums, grad_out, log_std, grad_log_std or stats; numel < 1; width outside 1..8; vf_coef, ent_coef or
 *     bounds_coef negative or not finite (pf_ppo_loss's checks); vclip or bnd other than 0 / 1; an output overlapping an input or
 *     another output.
 *   - pf_moments_merge, for the running normalisers of pf_traj_stats on sharded envs. dst, src[g]: device blocks of 1 + 2 D doubles
 *     (count, mean[D], M2[D]), pf_traj_stats's obs_moments (D = pf_obs_dim) and ret_moments (D = 1). dst = dst merged with src[0],
 *     ..., src[n_src - 1] in that order by the pairwise update pf_traj_stats itself uses (Chan et al.): n = na + nb, d = mean_b -
 *     mean_a, mean = mean_a + d nb / n, M2 = M2_a + M2_b + d^2 na nb / n. A block with count 0 merges as nothing; into an empty
 *     dst a block is copied, bit for bit. One launch. ERRORS: n_src outside 1..PF_PPO_MAX_SHARDS, D outside 1..128 (these first); a
 *     NULL ctx, dst, src or src[g]; dst overlapping a src[g]. */
#define PF_PPO_MAX_SHARDS 16
#define PF_PPO_SHARD_WORDS 24
typedef struct pf_ppo_shard_combine_args {
  int32_t n_shards;                /* 1..PF_PPO_MAX_SHARDS */
  int32_t width;                   /* A, the action width: 1..8 */
  int64_t numel;                   /* floats of a flat gradient buffer, >= 1 */
  float vf_coef, ent_coef;         /* >= 0, the shards' */
  int32_t vclip, bnd;              /* 0 / 1: the shards' options */
  float bounds_coef;               /* >= 0; read with bnd = 1 */
  const double* blocks[PF_PPO_MAX_SHARDS];  /* device, [PF_PPO_SHARD_WORDS] each */
  const double* adv_sums;          /* device, [4]: the sums of all shards */
  const float*  grads[PF_PPO_MAX_SHARDS];   /* device, [numel] each */
  float*  grad_out;                /* [numel] */
  const float*  log_std;           /* [A] */
  float*  grad_log_std;            /* [A] */
  double* stats;                   /* [16], pf_ppo_loss's slots */
} pf_ppo_shard_combine_args;
size_t pf_sizeof_ppo_shard_combine(void);
int pf_ppo_adv_sums(pf_ctx* ctx, const float* advantages, const uint8_t* valid /* NULL = all 1 */, const int32_t* row_index /* NULL = rows 0..m-1 */,
                    int64_t m, int64_t rows_total, double* sums /* device, [4] */, void* stream);
int pf_adv_sums_add(pf_ctx* ctx, double* dst /* device, [4] */, const double* const src[], int n_src, void* stream);
int pf_ppo_grad_shard(pf_ctx* ctx, const pf_ppo_grad_args* a, const pf_ppo_options* options /* may be NULL */,
                      const int32_t* row_index /* device, [m], or NULL */, int64_t m, int64_t rows_total,
                      const double* adv_sums /* device, [4]: the sums of ALL shards */, double* shard_block /* device, [PF_PPO_SHARD_WORDS] */,
                      void* workspace, size_t workspace_bytes, void* stream);
int pf_ppo_shard_combine(pf_ctx* ctx, const pf_ppo_shard_combine_args* a, void* stream);
int pf_moments_merge(pf_ctx* ctx, double* dst /* device, [1 + 2 D] */, const double* const src[], int n_src, int D, void* stream);

/* What a PPO recipe decides from the measured KL, on the device: one launch of one thread behind the loss, no host synchronisation,
 * capturable. Any context. (Added without a new PF_ABI_VERSION: a new function and a new block.)
 *   - kl = stats[5] (approx_kl of pf_ppo_loss / pf_ppo_grad and their _opt forms).
 *   - GATE. *gate = kl <= stop_factor * target_kl ? 1 : 0. A NaN closes it; with stop_factor = +inf no number does.
 *   - LEARNING RATE (adapt = 1). kl > lr_high * target_kl: lr = fmaxf(lr / lr_factor, lr_min); kl < lr_low * target_kl:
 *     lr = fminf(lr * lr_factor, lr_max); otherwise, and for a NaN, lr is unchanged. lr is *lr_dev, read and written in this call;
 *     with adapt = 0 it is not written, and the five lr_ arguments are not read.
 *   - ARITHMETIC. The comparisons are in double on the widened float32 arguments (the product in double); the two lr operations
 *     are float32.
 *   - STATE. state[4], double, read and then overwritten: 0 the kl read; 1 the lr after the call (0 without lr_dev); 2 the gate;
 *     3 the closed gates so far. A zeroed block is a fresh one.
 *   - ERRORS. PF_ERR_ARG, pf_last_error naming the argument: a NULL ctx, argument block, stats, gate or state; target_kl not finite
 *     or <= 0; stop_factor < 1 or NaN; adapt other than 0 / 1; with adapt = 1: a NULL lr_dev, lr_factor not finite or <= 1,
 *     not 0 < lr_low < lr_high < inf, not 0 < lr_min <= lr_max < inf; gate, state, lr_dev and stats overlapping. */
typedef struct pf_kl_control_args {
  const double* stats;     /* a pf_ppo_loss / pf_ppo_grad stats block; slot 5 is read */
  float target_kl;         /* finite, > 0 */
  float stop_factor;       /* >= 1, +inf = the gate never closes on a number */
  int32_t adapt;           /* 0 / 1: change *lr_dev in this call */
  float lr_factor;         /* > 1 */
  float lr_low, lr_high;   /* 0 < lr_low < lr_high, multiples of target_kl */
  float lr_min, lr_max;    /* 0 < lr_min <= lr_max, finite */
  float* lr_dev;           /* [1] in/out; required when adapt = 1 */
  uint32_t* gate;          /* [1] out: 1 = take the step */
  double* state;           /* [4] in/out */
} pf_kl_control_args;
size_t pf_sizeof_kl_control(void);
int pf_kl_control(pf_ctx* ctx, const pf_kl_control_args* a, void* stream);

/* pf_adam_step with one more device word: *gate (pf_kl_control's), read by the update kernel. Same block, workspace and launches.
 *   - *gate != 0: parameters, moments and state[0..4] have pf_adam_step's bits.
 *   - *gate == 0: SKIP's rule: no parameter, no moment and not t changes; slot 1 reports the norm, slot 2 a coef of 0.
 *   - state[5] counts the calls a closed gate skipped (kept, not zeroed, by this function; pf_adam_step writes 0 there). Slot 4 stays
 *     the count of calls skipped for a norm that is not finite, whatever the gate.
 *   - The gate is read on the device and applied as a selection; nothing waits for the host. Once a step has pushed the KL over the
 *     limit, later epochs on the same batch see unchanged parameters, hence the same KL, and are skipped too: early stopping
 *     without a latch.
 *   - ERRORS. pf_adam_step's, and PF_ERR_ARG for a NULL gate or one that overlaps a tensor, state, workspace or lr_dev. */
int pf_adam_step_gated(pf_ctx* ctx, const pf_adam_args* a, const uint32_t* gate, void* workspace, size_t workspace_bytes, void* stream);

/* The world-level auto-reset of the multi-agent envs (PF_TASK_DOGFIGHT, PF_TASK_MA_HOVER), which exist with auto-reset OFF only: run
 * between two env steps, it tells which lanes of the step just taken were real transitions, blanks the rows of the agents that had
 * finished before it, keeps the per-lane latch "this agent's episode has ended and its world has not been reset yet", and names
 * the worlds to reset -- NEXT_STEP's contract one level up, where the unit that is reset is the world and not the lane. (Added
 * without a new PF_ABI_VERSION: a new function, every existing struct as it was.) Worlds are groups of A = agents_per_world adjacent
 * lanes, lane = world * A + agent. Below, for lane i of world w:
 *   - was = done[i] != 0; waiting = every lane of w has done != 0 -- both as the latch was when the call began.
 *   - VALID. valid_out[i] = !was && !(exclude && exclude[i]): a lane whose agent had finished flies on with zero commands and is no
 *     transition; `exclude` takes lanes out for good (an opponent's, whose actions come from a policy that is not being trained).
 *   - ROWS. Where was: reward[i] = +0.0f, terminated[i] = truncated[i] = 0; every other lane's entries stay as pf_env_step wrote them.
 *   - LATCH. ended = !was && (terminated[i] | truncated[i]); done[i] = waiting ? 0 : (was | ended).
 *   - RESET MASK. reset_out[i] = waiting: whole worlds, every lane of them.
 *   - SELECTS. Every `?` and `where` above is a selection: a NaN in the reward of a latched lane reaches nothing.
 *   - CONSEQUENCE. A world whose every agent had finished before this step spends the step as its reset step: all its lanes are
 *     invalid, the mask names the world, its latch is cleared. The caller then runs pf_env_reset(mask = reset_out) with b->obs
 *     pointing at THIS step's observation row: the reset observation replaces what the wasted step wrote, the terminal observation
 *     of the last agent to finish stays in the previous row, and a truncated agent bootstraps from that row under pf_gae's OFF rule
 *     (nv[s] = values[s + 1]). One closed-loop step is four launches and one copy: pf_policy_act, pf_env_step, pf_world_sync with its
 *     n-byte device copy, pf_env_reset.
 *   - THE LATCH IS READ BY THE WHOLE WORLD AND REWRITTEN, and two lanes of a world may run in different workgroups (A need not
 *     divide the workgroup). The kernel therefore writes the new latch to a staging buffer of n bytes that the context owns, never
 *     to the latch it reads, and the call copies the staging buffer over `done` behind the kernel on the same stream (a
 *     device-to-device copy node). The caller sees one latch, in and out. Calls on one context share that buffer: they must be
 *     ordered (one stream, or events between streams).
 *   - ANY CONTEXT: it supplies n, the device and the error string; vehicle, task and auto-reset mode are not looked at.
 *   - ERRORS. PF_ERR_ARG, pf_last_error naming the argument: a NULL ctx or argument block; a NULL terminated, truncated, reward,
 *     done, valid_out or reset_out; agents_per_world outside 1..64; n not a multiple of agents_per_world.
 *   - Enqueued on `stream`: one launch and one n-byte device copy, no host synchronisation, no allocation -- capturable in a HIP graph.
 *     One thread per lane; each reads the A latch bytes of its world itself, with plain loads. */
typedef struct pf_world_sync_args {
  uint8_t* terminated;      /* [n] this step's row, read and rewritten */
  uint8_t* truncated;       /* [n] this step's row, read and rewritten */
  float*   reward;          /* [n] this step's row, read and rewritten */
  uint8_t* done;            /* [n] the latch, read and rewritten: 1 = this lane's episode has ended and its world has not been reset yet */
  const uint8_t* exclude;   /* [n] or NULL: lanes that are never valid (an opponent's) */
  uint8_t* valid_out;       /* [n] */
  uint8_t* reset_out;       /* [n] the mask to hand to pf_env_reset */
} pf_world_sync_args;
size_t pf_sizeof_world_sync(void);
int pf_world_sync(pf_ctx* ctx, const pf_world_sync_args* a, int agents_per_world, void* stream);

/* Why episodes end, and who wins a world: the reference reports `collision`, `out_of_bounds`, `env_complete` and
 * `num_targets_reached` (the dogfight: `team_win`, `dead`, `received_hits`) on every step(); inside a closed loop the words behind
 * them are overwritten by the next reset. This call reads them where an episode ends and counts them on the device, per group of
 * lanes. Any context with an env task. (Added without a new PF_ABI_VERSION: a new function and a new block, every existing struct as
 * it was.) Two forms: the TRAJECTORY form (agents_per_world == 1, any k_steps, `info` given -- SAME_STEP's final_info rows, or a block
 * of the caller's) and the STEP form (k_steps == 1, `info` NULL or given), which is also the WORLD form for agents_per_world > 1.
 *   - ENDED. Lane i ends an episode at step s if and only if terminated[s][i] | truncated[s][i]. Nothing else is asked: under
 *     NEXT_STEP the reset step writes zero flags; pf_world_sync blanks the rows of latched lanes and of the reset step; an excluded
 *     opponent lane keeps its real flags (and `valid` takes it out of the agent-level slots).
 *   - WORDS. (word0, word1) of lane i at step s: info[s][i][0..1] as stored, in final_info's layout; with info == NULL (k_steps == 1)
 *     the words of `state` as it stands after the env step and before any reset. PF_TASK_HOVER / WAYPOINTS / ROCKET_LANDING /
 *     MA_HOVER: word0 = the flags word (pf_flag_bits), word1 = the targets left. PF_TASK_DOGFIGHT: word0 = the dogfight's bits word,
 *     word1 = received_hits. The words of a lane that did not end are loaded and not selected: they reach nothing.
 *   - BYTE of an ended episode: PF_OC_ENDED; PF_OC_TERMINATED if terminated (terminated wins over truncated, as in pf_traj_stats);
 *     PF_OC_COLLISION / PF_OC_OOB / PF_OC_COMPLETE / PF_OC_NONFINITE from word0's PF_F_INFO_COLLISION / PF_F_INFO_OOB /
 *     PF_F_INFO_COMPLETE / PF_F_NONFINITE; on the dogfight PF_OC_COLLISION / PF_OC_OOB / PF_OC_COMPLETE / PF_OC_DEAD from its
 *     collision / out_of_bounds / team_win / dead bits, and never PF_OC_NONFINITE. outcome_out[s][i] = the byte where the lane
 *     ended, 0 elsewhere -- for invalid lanes and for lanes whose group is out of range as well.
 *   - AGENT-LEVEL SLOTS, counted where ended && valid[s][i] (valid NULL = 1), into counts[group[i]] (group NULL = 0):
 *       0 episodes   1 terminated   2 truncated   3 collision   4 out of bounds   5 complete / team_win   6 dead   7 nonfinite
 *       8 the sum of num_targets - word1 on PF_TASK_WAYPOINTS, of received_hits (word1) on the dogfight, 0 on the other tasks
 *       9 ended with none of the bits 4..64: ran to the limit cleanly
 *     Bits may co-occur; each slot counts on its own.
 *   - WORLD-LEVEL SLOTS, agents_per_world = A > 1 (worlds of A adjacent lanes, lane = world * A + agent, as in pf_world_sync;
 *     k_steps == 1):   10 worlds   11 team 0 wins   12 team 1 wins   13 draws   14-15 zero.
 *     A lane that ends, valid or not, ASSIGNS its byte to world_latch[i]. Where world_reset[i] != 0 on a world's first lane, the
 *     world that finished before this step is tallied into the row of that first lane's group: slot 10 always; on PF_TASK_DOGFIGHT
 *     team 0 = lanes [0, df_team_size) of the world, team 1 the rest, team t won if some lane of t latched PF_OC_COMPLETE and no
 *     lane of the other team did, otherwise the world is a draw; other tasks have no teams and slots 11-13 stay 0. Nothing is ever
 *     cleared: every lane of a world ends, and so rewrites its byte, before pf_world_sync names the world again. A world reset from
 *     outside (pf_env_reset with a mask of the caller's) is not tallied.
 *   - NO LANE READS A LATCH BYTE THAT ANOTHER LANE WRITES IN THE SAME LAUNCH. The lanes that write belong to worlds that are not
 *     being reset (a lane stores only where world_reset[i] == 0; under pf_world_sync's protocol a lane of a world that is being reset
 *     has blank flags anyway), the bytes that are read belong to worlds that are (world_reset on the first lane), and the mask is
 *     the same on every lane of a world. This holds for every A, 6 included, and wherever a world straddles a wavefront or a
 *     workgroup: the argument never looks at where a world begins. So there is no staging buffer and no copy.
 *   - GROUPS. group[i] is not range-checked on the host (that would read device memory): the kernel takes a lane whose group is
 *     outside 0..n_groups-1 out of every count, and does not tally a world whose first lane is such a lane.
 *   - ARITHMETIC. Integer sums, ADDED to counts in place (a zeroed block = empty): per-workgroup partial sums, then vector atomics
 *     on the int64 block. The counts do not depend on launch shape, stream or order.
 *   - ERRORS. PF_ERR_ARG, pf_last_error naming the argument, before any launch: a NULL ctx, argument block, terminated, truncated or
 *     counts; k_steps < 1; info == NULL with k_steps != 1 or with state == NULL; n_groups outside 1..PF_OUTCOME_MAX_GROUPS;
 *     agents_per_world outside 1..64 or not dividing n; agents_per_world > 1 with k_steps != 1 or without world_reset or
 *     world_latch; agents_per_world == 1 with world_reset given. PF_ERR_UNSUPPORTED: a context without an env task.
 *   - Enqueued on `stream`: one launch, no host synchronisation, no allocation, no copy -- capturable in a HIP graph. One thread per
 *     lane; in the trajectory form the loads of a window of steps are issued before their first use. The call keeps nothing in the
 *     context: calls with distinct outputs may run on different streams. */
#define PF_OUTCOME_SLOTS 16
#define PF_OUTCOME_MAX_GROUPS 16
enum pf_outcome_bit { PF_OC_ENDED = 1, PF_OC_TERMINATED = 2, PF_OC_COLLISION = 4, PF_OC_OOB = 8,
                      PF_OC_COMPLETE = 16 /* env_complete; dogfight: team_win */, PF_OC_DEAD = 32 /* dogfight only */,
                      PF_OC_NONFINITE = 64 };
typedef struct pf_outcome_args {
  const uint8_t* terminated;   /* [k][n] */
  const uint8_t* truncated;    /* [k][n] */
  const uint8_t* valid;        /* [k][n] or NULL (= all 1): whose ended episodes enter the agent-level slots */
  const int32_t* info;         /* [k][n][2] (word0, word1) in final_info's layout, or NULL = read the live state */
  const float*   state;        /* the context's state tensor; required when info == NULL */
  const int32_t* group;        /* [n] in 0..n_groups-1, or NULL (= 0) */
  int32_t        n_groups;     /* 1..PF_OUTCOME_MAX_GROUPS */
  const uint8_t* world_reset;  /* [n]: pf_world_sync's reset_out of this step; required iff agents_per_world > 1 */
  uint8_t*       world_latch;  /* [n] in/out, the caller's; required iff agents_per_world > 1 */
  uint8_t*       outcome_out;  /* [k][n] or NULL */
  int64_t*       counts;       /* [n_groups][PF_OUTCOME_SLOTS], ADDED to in place (zeroed block = empty) */
} pf_outcome_args;
size_t pf_sizeof_outcome(void);
int pf_episode_outcomes(pf_ctx* ctx, const pf_outcome_args* a, int k_steps, int agents_per_world, void* stream);

/* pf_policy_act for a POOL of policies in one launch: every row is evaluated once, by the policy that row_policy names for it -- a
 * learner and a league's past snapshots on their own lanes of one dogfight batch, or G checkpoints side by side in one batch of a
 * single-agent env. (Added without a new PF_ABI_VERSION: three new functions; pf_policy and every other struct are as they were.)
 *   - row_policy: device, [n] int32, n = pf_n_lanes(ctx): the policy of every row, 0 .. n_policies - 1. Any other value (-1 by
 *     convention) means "no policy": that row of actions_out and of mean_out is not written, not one byte.
 *   - THE PLAN. pf_policy_pool_plan turns row_policy into the caller's `plan` buffer (device, opaque, plan_bytes =
 *     pf_policy_pool_plan_bytes(n, n_policies)): per policy the list of its rows, padded to whole tiles of 64 rows, and the policy
 *     every tile runs. ceil(n / 64) + n_policies tiles always suffice, so the size is a function of (n, n_policies) alone and
 *     nothing reads a count back. pf_policy_pool_plan_bytes is a pure host function; it returns 0 for what the calls refuse (n < 1,
 *     n_policies outside 1..PF_POLICY_POOL_MAX). The plan is built once per assignment of rows to policies, not once per step: one
 *     workgroup sorts the rows, so it is not fast (about 0.2 ms at 65 536 rows and 17 policies). A policy without rows is fine. The
 *     plan's bytes are a function of row_policy alone (a policy's rows stand in ascending order); and no bit that
 *     pf_policy_act_pool writes depends on the order in which a plan lists a policy's rows.
 *   - pf_policy_act_pool: `policies` is a HOST array of n_policies pf_policy blocks, passed to the kernel as arguments.
 *     policies[0].obs0 is the call's [n][D] input and policies[0].mean_out its [n][A] mean output or NULL; those two fields of the
 *     other entries are ignored. The entries may differ in n_layers, widths, activation and in whether log_std is NULL; D and A are
 *     the context's (pf_policy_act: ARGUMENTS).
 *   - THE RESULT. For every row i with p = row_policy[i] in range, actions_out[i] and mean_out[i] hold the bits that
 *     pf_policy_act(ctx, &policies[p], ..., step_index) writes for row i on the same observation: the same bias-first ascending fmaf
 *     chain on the float32-input matrix instruction, the same float32 tanh, the same expf(log_std), the same Philox call keyed by
 *     (seed, global lane, step_index, 0) on stream constant 4 -- wherever the row lands in a tile.
 *   - A STALE PLAN (one made for another row_policy, n or n_policies, or bytes that no pf_policy_pool_plan wrote) may give wrong
 *     actions but never an access outside the caller's tensors: the kernel checks every row index and every policy index it reads
 *     from the plan before it addresses anything with them.
 *   - ERRORS: PF_ERR_ARG, the argument named, before any launch, for a NULL ctx / row_policy / policies / plan / actions_out /
 *     policies[0].obs0 or a layer's w / b, n_policies outside 1..PF_POLICY_POOL_MAX, plan_bytes different from
 *     pf_policy_pool_plan_bytes(n, n_policies), and per entry pf_policy_act's checks with "policies[p]: " in front; PF_ERR_UNSUPPORTED
 *     for a context without an env task or a hidden width over PF_POLICY_MAX_HIDDEN.
 *   - Both calls are enqueued on `stream`: no host synchronisation, no allocation, no copy -- capturable in a HIP graph;
 *     pf_policy_act_pool is ONE launch. The weights are read at every call; neither call keeps anything in the context. obs0 and
 *     the outputs must not overlap; the plan must not be rewritten while a pf_policy_act_pool that reads it is in flight. */
#define PF_POLICY_POOL_MAX 17   /* a learner and PF_OUTCOME_MAX_GROUPS opponents */
size_t pf_policy_pool_plan_bytes(int n_rows, int n_policies);
int pf_policy_pool_plan(pf_ctx* ctx, const int32_t* row_policy, int n_policies, void* plan, size_t plan_bytes, void* stream);
int pf_policy_act_pool(pf_ctx* ctx, const pf_policy* policies, int n_policies, const void* plan, size_t plan_bytes,
                       float* actions_out, uint32_t step_index, void* stream);

/* The reference's LOWER boundary for one drone: applyExternalForce / applyExternalTorque on the base link in
 * LINK_FRAME followed by stepSimulation (core/drones/quadx.py:502-510, core/aviary.py:516), n_ticks times with
 * the wrench b->wrench held: the free-body tick alone (collision detection, gyroscopic term, +-max_coord_vel
 * clamp, exponential-map attitude update), no motors / drag / controller. Exists so that the integrator's
 * analytic known-answer tests (free fall, constant torque, torque-free spin, clamp) run against the device
 * code directly. Fills b->out_state / out_contact. */
int pf_body_tick(pf_ctx* ctx, const pf_buffers* b, int n_ticks, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PYFLYT_AMD_H */
