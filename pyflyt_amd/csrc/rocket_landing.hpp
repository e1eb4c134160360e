// rocket_landing.hpp -- PyFlyt/Rocket-Landing-v4 on the GPU: gym_envs/rocket_envs/rocket_landing_env.py with
// rocket_base_env.py:20-400, one lane per env, as the PF_TASK_ROCKET_LANDING instantiation of the generic env kernel
// (env_kernel<Rocket, PF_TASK_ROCKET_LANDING, kRuntimeMode>, an explicit specialisation: the generic body is QuadX / Fixedwing
// shaped -- four-wide actions, six setpoints -- and stays exactly as it is for them).
//
// The landing pad (models/landing_pad.urdf at basePosition (0, 0, 0.1), useFixedBase): a static upright cylinder, the world's
// second collider next to the ground slab (pf_params.pad_*). Everything here is compiled into this instantiation only: the
// Aviary-level kernels run Rocket::tick<NoPad>, i.e. Body::tick_var as before.
//   * detection, per tick at the pre-integration pose: the slab's 15-axis verdict as before (Body::detect_contact) and the pad's
//     vertex rule -- a collider vertex (every box corner, the 16 rim points of a cylinder) whose horizontal distance from the pad
//     axis is <= pad_radius and whose height lies in [pad bottom, pad top + reach], reach = the report distance, or the breaking
//     distance for a body that held contact points after the previous tick;
//   * response: the pad's top face (normal +z) is one more contact plane of the same projected Gauss-Seidel solve -- a vertex
//     over the pad disc and within reach of its top face is a contact with the pad (depth below that face), any other vertex is
//     tested against the slab as before. The rim and the side wall are not modelled.
#pragma once
#include "rocket.hpp"
#include "env_generic.hpp"  // env_kernel, which this header specialises; SideBlock, kWave, kMaxObs

namespace pf {

// The collider vertices of the airframe at pose (p, R) in collider / vertex order: f(off) with `off` the world offset from the base
// origin. reduce: the manifold reduction of the box colliders (pf_params.contact_manifold_points = 4: the face that looks down the
// most, the first axis on a tie), as the slab's solve has it.
template <class F>
PF_DEV void pad_collider_vertices(const pf_params_kptr P, const bool reduce, const v3 p, const m3& R, F&& f) {
  (void)p;
  for (int k = 0; k < P->n_boxes; ++k) {
    const float bc0 = P->boxes[k].c[0], bc1 = P->boxes[k].c[1], bc2 = P->boxes[k].c[2];
    const float bh0 = P->boxes[k].h[0], bh1 = P->boxes[k].h[1], bh2 = P->boxes[k].h[2];
    const int kind = P->boxes[k].kind;
    const float yaw = P->boxes[k].yaw;
    float sy = 0.0f, cy = 1.0f;
    if (yaw != 0.0f) sincosf(yaw, &sy, &cy);  // (wave-uniform)
    const v3 cwk = mul(R, v3{bc0, bc1, bc2});
    if (kind == 1) {  // cylinder: 8 rim points per end disc, -z then +z, at 45 degree steps from the link x axis
#pragma unroll 1
      for (int i = 0; i < 16; ++i) {
        const int j = i & 7;
        const float c45 = (j == 0) ? 1.0f : ((j == 4) ? -1.0f : ((j == 2 || j == 6) ? 0.0f : ((j == 1 || j == 7) ? 0.70710678f : -0.70710678f)));
        const int js = (j + 6) & 7;
        const float s45 = (js == 0) ? 1.0f : ((js == 4) ? -1.0f : ((js == 2 || js == 6) ? 0.0f : ((js == 1 || js == 7) ? 0.70710678f : -0.70710678f)));
        const float l0 = bh0 * c45, l1 = bh0 * s45, l2 = (i >> 3) ? bh2 : -bh2;
        f(cwk + mul(R, v3{cy * l0 - sy * l1, sy * l0 + cy * l1, l2}));
      }
      continue;
    }
    // box: the link axes in the world frame scaled by the half extents (the link frame is the base frame yawed about z)
    const v3 ex{bh0 * fmaf(R.m00, cy, R.m01 * sy), bh0 * fmaf(R.m10, cy, R.m11 * sy), bh0 * fmaf(R.m20, cy, R.m21 * sy)};
    const v3 ey{bh1 * fmaf(R.m01, cy, -(R.m00 * sy)), bh1 * fmaf(R.m11, cy, -(R.m10 * sy)), bh1 * fmaf(R.m21, cy, -(R.m20 * sy))};
    const v3 ez{bh2 * R.m02, bh2 * R.m12, bh2 * R.m22};
    uint32_t keep = 0xffu;
    if (reduce) {
      const float zx = fmaf(R.m20, cy, R.m21 * sy), zy = fmaf(R.m21, cy, -(R.m20 * sy)), zz = R.m22;
      const float ax = __builtin_fabsf(zx), ay = __builtin_fabsf(zy), az = __builtin_fabsf(zz);
      const bool use_y = ay > ax, use_z = az > __builtin_fmaxf(ax, ay);
      const uint32_t lo = use_z ? 0x0fu : (use_y ? 0x33u : 0x55u);
      const float zsel = use_z ? zz : (use_y ? zy : zx);
      keep = zsel < 0.0f ? (lo ^ 0xffu) : lo;
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {  // vertex i: x sign bit 0, y sign bit 1, z sign bit 2
      if (((keep >> i) & 1u) == 0u) continue;
      const float sx = (i & 1) ? 1.0f : -1.0f, syv = (i & 2) ? 1.0f : -1.0f, sz = (i & 4) ? 1.0f : -1.0f;
      f(v3{fmaf(sx, ex.x, fmaf(syv, ey.x, fmaf(sz, ez.x, cwk.x))), fmaf(sx, ex.y, fmaf(syv, ey.y, fmaf(sz, ez.y, cwk.y))),
           fmaf(sx, ex.z, fmaf(syv, ey.z, fmaf(sz, ez.z, cwk.z)))});
    }
  }
}

// The pad's constants as the solve and the detection read them.
struct PadGeom {
  float cx, cy, r2, bottom, top;
  PF_DEV explicit PadGeom(const pf_params_kptr P) {
    cx = P->pad_pos[0]; cy = P->pad_pos[1];
    r2 = P->pad_radius * P->pad_radius;
    bottom = P->pad_pos[2] - P->pad_half_height; top = P->pad_pos[2] + P->pad_half_height;
  }
  PF_DEV bool over(const v3 x) const {
    const float dx = x.x - cx, dy = x.y - cy;
    return fmaf(dx, dx, dy * dy) <= r2;
  }
  // a vertex at world position x touches the pad within `reach` of its top face
  PF_DEV bool touches(const v3 x, const float reach) const { return over(x) && x.z >= bottom && x.z <= top + reach; }
};

// The solve's world with the pad: ParamContactSrc (the slab, the contact model's constants) with the pad's top face as a second
// contact plane. for_each hands contact_solve_impl the vertex's height above ITS plane (the solve's depth is its negation).
struct PadContactSrc : ParamContactSrc {
  PadGeom pad;
  PF_DEV explicit PadContactSrc(pf_params_kptr p) : ParamContactSrc(p), pad(p) {}
  template <class F> PF_DEV void for_each(const v3 p, const m3& R, const float reach, F&& f) const {
    pad_collider_vertices(P, !all8_, p, R, [&](const v3 off) {
      const v3 x = p + off;
      if (pad.touches(x, reach)) f(off, x.z - pad.top);
      else if (x.z <= reach && x.z >= -hz2_ && __builtin_fabsf(x.x) <= hxy_ && __builtin_fabsf(x.y) <= hxy_) f(off, x.z);
    });
  }
};

// The world of one Rocket-Landing lane: Rocket::tick<PadWorld> ends in tick_var below instead of Body::tick_var.
struct PadWorld {
  const pf_params* pdev;
  bool pad_step;  // the body touched the pad in some tick of the current Aviary step (contact_array[rocket, pad])
  // Can any vertex be within `reach` of the pad at all? (a bound-sphere test first: most lanes are far above it)
  PF_DEV bool pad_in_reach(const Body& b, const pf_params& P, const float reach) const {
    const float rb = P.bound_radius;
    const float top = P.pad_pos[2] + P.pad_half_height, bottom = P.pad_pos[2] - P.pad_half_height;
    const float dx = b.p.x - P.pad_pos[0], dy = b.p.y - P.pad_pos[1], rr = P.pad_radius + rb;
    return (b.p.z - rb <= top + reach) && (b.p.z + rb >= bottom) && (fmaf(dx, dx, dy * dy) <= rr * rr);
  }
  PF_DEV bool detect_pad(const Body& b, const pf_params& P, const float reach) const {
    if (!pad_in_reach(b, P, reach)) return false;
    const pf_params_kptr K = uniform_params(pdev);
    const PadGeom pad(K);
    bool hit = false;
    pad_collider_vertices(K, false, b.p, b.R, [&](const v3 off) { hit = hit || pad.touches(b.p + off, reach); });
    return hit;
  }
  // Body::contact_may_act for two planes: the slab's top face (z = 0) and the pad's (z = top, over the disc)
  PF_DEV bool may_act(const Body& b, const pf_params& P) const {
    const float reach = b.persisted ? P.contact_break_distance : P.contact_margin;
    const float vlow = b.v.z - __builtin_sqrtf(dot(b.w, b.w)) * P.bound_radius;
    auto acts = [&](const float low) { return low <= reach && ((low + P.contact_slop + P.dt * vlow < 0.0f) || (low < -P.contact_slop)); };
    const float low = b.p.z - P.bound_radius;
    const bool slab = b.slab_in_reach(P, reach) && acts(low);
    const bool pad = pad_in_reach(b, P, reach) && acts(low - (P.pad_pos[2] + P.pad_half_height));
    return slab || pad;
  }
  // Body::tick_var with the pad: detection against both colliders, dynamics, the two-plane contact solve, integration.
  PF_DEV void tick_var(Body& b, const pf_params& P, v3 F, v3 tau, float inv_mass, v3 com, const float H[6], const float Iinv[6]) {
    b.persisted = b.contact_now;
    const float rd = b.persisted ? P.contact_break_distance : P.contact_report_distance;
    const bool floor = b.detect_contact(P, rd);
    const bool pad = detect_pad(b, P, rd);
    b.contact_now = floor || pad;
    tau = tau - cross(com, F);
    v3 h = symmul(H, b.wb);
    v3 wdot_b = symmul(Iinv, tau - cross(b.wb, h));
    v3 wdot = mul(b.R, wdot_b);
    v3 a = inv_mass * mul(b.R, F);
    a.z += P.gravity_z;
    v3 cw = mul(b.R, com);
    a = a - cross(wdot, cw) - cross(b.w, cross(b.w, cw));
    const float dt = P.dt, vm = P.max_coord_vel;
    b.w = v3{clampf(fmaf(wdot.x, dt, b.w.x), -vm, vm), clampf(fmaf(wdot.y, dt, b.w.y), -vm, vm), clampf(fmaf(wdot.z, dt, b.w.z), -vm, vm)};
    b.v = v3{clampf(fmaf(a.x, dt, b.v.x), -vm, vm), clampf(fmaf(a.y, dt, b.v.y), -vm, vm), clampf(fmaf(a.z, dt, b.v.z), -vm, vm)};
    float lift = 0.0f;
    const bool need = P.contact_response && may_act(b, P);
    if (__any(need)) {
      const int need_cap = need_cap_of(need, b.ccap, b.persisted);
      const int cap_floats = __reduce_max_cap(need_cap);
      const ContactOut o = contact_solve_impl(PadContactSrc(uniform_params(pdev)), b.cws, cap_floats, need, need && b.persisted, b.p, b.R, b.v, b.w,
                                              inv_mass, com, Iinv[0], Iinv[1], Iinv[2], Iinv[3], Iinv[4], Iinv[5]);
      b.v = o.v; b.w = o.w;
      lift = P.contact_erp * o.deepest;
    }
    b.p = v3{fmaf(dt, b.v.x, b.p.x), fmaf(dt, b.v.y, b.p.y), fmaf(dt, b.v.z, b.p.z) + lift};
    b.q = quat_integrate(b.q, b.w, 0.5f * dt);
    b.derive();
    b.contact_step |= floor;  // (contact_step: every contact that is not the rocket's with the pad -- the base env's fatal_collision)
    pad_step |= pad;
  }
};

// ------------------------------------------------------------------ the env kernel
// State: the Rocket's groups 0-6 (rocket.hpp) + group 7 the last action [0..3], group 8 the last action [4..6] and a zero.
// The flags word carries PF_F_PAD_CONTACT: landing_pad_contact as the last pad check left it (what the next compute_state shows).
constexpr int kRlGroups = Rocket::GROUPS + 2;
constexpr int kRlActionDim = 7;
// the action box (rocket_base_env.py:95-119): low (-1, -1, -1, 0, 0, -1, -1), high 1 -- seven wide, so not pf_params.action_low / high
constexpr float kRlActionLow[kRlActionDim] = {-1.0f, -1.0f, -1.0f, 0.0f, 0.0f, -1.0f, -1.0f};
constexpr float kRlActionHigh[kRlActionDim] = {1.0f, 1.0f, 1.0f, 1.0f, 1.0f, 1.0f, 1.0f};

template <>
__global__ void __launch_bounds__(kWave) env_kernel<Rocket, PF_TASK_ROCKET_LANDING, kRuntimeMode>(
    const pf_params P, const pf_buffers B, const int n, const uint64_t lane0, const int op, const uint8_t* mask,
    const float4* __restrict__ tmpl, const pf_params* __restrict__ Pdev, const int roll_steps, const uint32_t step0) {
  (void)tmpl;
  __shared__ __attribute__((aligned(16))) float tile[kWave * kMaxObs];
  const int tid = threadIdx.x;
  const int wave_base = blockIdx.x * kWave;
  const int lane = wave_base + tid;
  const bool valid = lane < n;
  const size_t li = valid ? lane : n - 1;
  const size_t N = (size_t)n;
  const float4* Sin = reinterpret_cast<const float4*>(B.state);
  float4* Sout = reinterpret_cast<float4*>(B.state);

  Rocket V;
  bind_contact(V, P, Pdev, tile, kWave * kMaxObs);  // (the tile is idle during the physics ticks)
  PadWorld W;
  W.pdev = Pdev;
  W.pad_step = false;
  float nd_;
  int4 ints;
  V.load(Sin, N, li, 0, nd_, ints);
  float act[kRlActionDim];
  {
    const float4 g7 = Sin[(size_t)(Rocket::GROUPS + 0) * N + li], g8 = Sin[(size_t)(Rocket::GROUPS + 1) * N + li];
    act[0] = g7.x; act[1] = g7.y; act[2] = g7.z; act[3] = g7.w; act[4] = g8.x; act[5] = g8.y; act[6] = g8.z;
  }
  int step_count = ints.x, flags = ints.y;
  uint32_t rng_ctr = (uint32_t)ints.z;
  bool term = (flags & PF_F_TERMINATED) != 0, trunc = (flags & PF_F_TRUNCATED) != 0;
  float pad_contact = (flags & PF_F_PAD_CONTACT) ? 1.0f : 0.0f;  // self.landing_pad_contact
  float obs_pad = pad_contact;                                   // ... as the last compute_state saw it

  Noise nz;
  nz.init(P, n, li, lane0);

  bool active = false, do_reset = false, wave_all = false;
  float sp[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  float reward = 0.0f;
  bool rpy_valid = false;
  const int D = (P.angle_repr ? 13 : 12) + kRlActionDim + Rocket::AUX + 1;

  // rocket_base_env.py:162-214 (begin_reset) + rocket_landing_env.py:86-104: spawn pose and velocity by the reset options, fuel at
  // starting_fuel_ratio (pf_params.rocket), the pad bit cleared; the settle steps run in the loop below
  auto begin_reset = [&]() {
    float pose[7] = {P.start_pos[0], P.start_pos[1], P.start_pos[2], P.start_quat[0], P.start_quat[1], P.start_quat[2], P.start_quat[3]};
    nz.begin_event(rng_ctr, 1u, B.xi_reset);
    if (P.rl_reset_options & PF_RL_RANDOMIZE_DROP) {  // rocket_base_env.py:184-189
      float u[6];
      const bool inj = P.noise_mode == PF_NOISE_INJECT && B.u_targets != nullptr;
      const float s = 0.1f * P.max_displacement;
#pragma unroll
      for (int j = 0; j < 6; ++j) {
        const float lo = j < 2 ? -s : (j == 2 ? 0.8f * P.ceiling : -0.3f), hi = j < 2 ? s : (j == 2 ? 0.9f * P.ceiling : 0.3f);
        u[j] = inj ? B.u_targets[(size_t)j * N + li] : fmaf(hi - lo, nz.uniform(j, 2u), lo);
      }
      const quat q = quat_from_euler(v3{u[3], u[4], u[5]});
      pose[0] = u[0]; pose[1] = u[1]; pose[2] = u[2]; pose[3] = q.x; pose[4] = q.y; pose[5] = q.z; pose[6] = q.w;
    }
    // (the reference's random start velocities sit behind the misspelt key "randoimize_drop", rocket_base_env.py:205: never taken)
    const float rest[3] = {0.0f, 0.0f, 0.0f};
    V.reset(P, pose, sp, rest);
    // accelerate_drop: resetBaseVelocity AFTER the Aviary's reset (rocket_base_env.py:206-211), so the first tick's aerodynamics still
    // see the spawn's zero velocity (the fins and the body drag read the velocities of the last update_state): v is set, vb / wb are not
    if (P.rl_reset_options & PF_RL_ACCELERATE_DROP) V.b.v.z = -100.0f;
    rpy_valid = false;
    step_count = 0; term = false; trunc = false; flags = 0;
    pad_contact = 0.0f; obs_pad = 0.0f;
#pragma unroll
    for (int k = 0; k < kRlActionDim; ++k) act[k] = 0.0f;
  };
  // rocket_landing_env.py:141-169: what the observation's ground_lin_vel is -- R(quat(euler(q))) lin_vel_body, the z row
  auto ground_vz = [&]() {
    const m3 Re = rot_from_quat(canon_quat(V.b.q));
    return fmaf(Re.m20, V.b.vb.x, fmaf(Re.m21, V.b.vb.y, Re.m22 * V.b.vb.z));
  };
  // one Aviary.step with the pad in the world (Rocket::aviary_step with tick<PadWorld>)
  auto aviary_step = [&](int flat_base) {
    V.b.contact_step = false;
    W.pad_step = false;
    V.template control<0>(P, sp);
    for (int t = 0; t < P.ticks_per_control; ++t) V.template tick<PadWorld>(P, nz.get(flat_base + t), nullptr, &W);
    V.b.rpy = euler_from_quat_fast(V.b.q);
    rpy_valid = true;
  };
  // rocket_base_env.py:268-301 (compute_base_term_trunc_reward) + rocket_landing_env.py:171-234; `prev_*`: the state before
  // this Aviary step (what compute_state moved into previous_*)
  auto term_trunc_reward = [&](const v3 prev_p, const float prev_w2, const float prev_v2, const float prev_gvz) {
    if (step_count > P.max_steps) trunc = true;
    const v3 p = V.b.p;
    if (V.b.contact_step || p.z < 0.0f) { flags |= PF_F_INFO_COLLISION; term = true; }
    const float lat = sqrtf(fmaf(p.x, p.x, p.y * p.y));
    if (lat > P.max_displacement || p.z > P.ceiling) { flags |= PF_F_INFO_OOB; term = true; }
    const float gvz = ground_vz();
    if (!P.sparse_reward) {
      const float lateral_progress = sqrtf(fmaf(prev_p.x, prev_p.x, prev_p.y * prev_p.y)) - lat;
      const float vertical_progress = prev_p.z - p.z;
      const float lateral_distance = lat + 0.1f;
      const float decel = (gvz - prev_gvz + 1.0f) / expf(p.z) * (gvz < 0.0f ? 1.0f : -1.0f);
      reward += -0.3f + 0.3f / lateral_distance + 10.0f * lateral_progress + 0.2f * vertical_progress + 4.0f * decel -
                __builtin_fabsf(V.b.wb.z) - sqrtf(fmaf(V.b.rpy.x, V.b.rpy.x, V.b.rpy.y * V.b.rpy.y));
    }
    if (!W.pad_step) { pad_contact = 0.0f; return; }
    pad_contact = 1.0f;
    reward += 5.0f - 0.3f * __builtin_fabsf(gvz);
    if (prev_w2 > 0.35f * 0.35f || prev_v2 > 1.0f) { term = true; flags |= PF_F_INFO_COLLISION; return; }
    if (prev_w2 < 0.02f * 0.02f && prev_v2 < 0.02f * 0.02f && fmaf(V.b.rpy.x, V.b.rpy.x, V.b.rpy.y * V.b.rpy.y) < 0.1f * 0.1f) {
      trunc = true; flags |= PF_F_INFO_COMPLETE; reward += 3.0f;
    }
  };
  // the Aviary steps of an env step (settling = false: rocket_base_env.py:317-325) or of a reset's settle phase; wave-uniform loop
  // (inlined at both call sites: called out of line it took the lane's whole state through scratch memory, 2.7 KB per lane)
  auto run = [&](int my_its, const bool settling) __attribute__((always_inline)) {
    int it = 0;
    while (__any(my_its > 0)) {
      if (my_its > 0) {
        const v3 prev_p = V.b.p;
        const float prev_w2 = dot(V.b.w, V.b.w), prev_v2 = dot(V.b.v, V.b.v);
        const float prev_gvz = settling ? 0.0f : ground_vz();
        aviary_step(it * P.ticks_per_control);
        my_its -= 1;
        if (!settling) {
          obs_pad = pad_contact;  // compute_state runs before the pad check
          term_trunc_reward(prev_p, prev_w2, prev_v2, prev_gvz);
          if (term || trunc) my_its = 0;
        }
      }
      it += 1;
    }
  };
  auto write_obs_row = [&]() {
    if (!rpy_valid) { V.b.rpy = euler_from_quat_fast(V.b.q); rpy_valid = true; }
    float* row = tile + tid * D;
    int k = 0;
    row[k++] = V.b.wb.x; row[k++] = V.b.wb.y; row[k++] = V.b.wb.z;
    if (P.angle_repr) { const quat qe = canon_quat(V.b.q); row[k++] = qe.x; row[k++] = qe.y; row[k++] = qe.z; row[k++] = qe.w; }
    else { row[k++] = V.b.rpy.x; row[k++] = V.b.rpy.y; row[k++] = V.b.rpy.z; }
    row[k++] = V.b.vb.x; row[k++] = V.b.vb.y; row[k++] = V.b.vb.z;
    row[k++] = V.b.p.x; row[k++] = V.b.p.y; row[k++] = V.b.p.z;
#pragma unroll
    for (int a = 0; a < kRlActionDim; ++a) row[k++] = act[a];
    float aux[Rocket::AUX];
    V.aux(aux);
#pragma unroll
    for (int a = 0; a < Rocket::AUX; ++a) row[k++] = aux[a];
    row[k++] = obs_pad;
  };

  const int n_env_steps = roll_steps > 0 ? roll_steps : 1;
  for (int ks = 0; ks < n_env_steps; ++ks) {
    const size_t toff = (size_t)ks * N;
    if (ks > 0) {  // what the next launch would start from (Rocket::load on the stored groups)
      V.b.contact_now = (flags & PF_F_CONTACT) != 0;
      V.b.contact_step = false;
      V.b.derive();
      rpy_valid = false;
      reward = 0.0f;
    }
    if (op == OP_RESET) {
      do_reset = (mask == nullptr) || (mask[li] != 0);
      active = do_reset;
    } else {
      do_reset = (P.autoreset == PF_AUTORESET_NEXT_STEP) && (term || trunc);
      active = true;
    }
    active = active && valid;
    do_reset = do_reset && active;
    wave_all = __all(active || !valid);

    float a[kRlActionDim] = {0, 0, 0, 0, 0, 0, 0};
    if (roll_steps > 0 && B.actions == nullptr) {  // pf_sample_actions' draw for (lane, step0 + ks)
      sampled_action7<true>((uint32_t)P.seed, (uint32_t)(P.seed >> 32), (uint32_t)(lane0 + li), step0 + (uint32_t)ks, kRlActionLow, kRlActionHigh, a);
      if (B.actions_out != nullptr && valid)
#pragma unroll
        for (int j = 0; j < kRlActionDim; ++j) B.actions_out[(toff + li) * kRlActionDim + j] = a[j];
    } else if (active && !do_reset) {
#pragma unroll
      for (int j = 0; j < kRlActionDim; ++j) a[j] = B.actions[(toff + li) * kRlActionDim + j];
    }
    bool settling = false;
    int my_its = 0;
    if (do_reset) {
      begin_reset();
      settling = true;
      my_its = P.settle_steps;
    } else if (active) {  // rocket_base_env.py:310-326
#pragma unroll
      for (int j = 0; j < kRlActionDim; ++j) { act[j] = a[j]; sp[j] = a[j]; }
      reward = 0.0f;
      my_its = (term || trunc) ? 0 : P.env_step_ratio;
      nz.begin_event(rng_ctr, 0u, B.xi);
    }
    run(my_its, settling);
    const bool stepped = active && !settling && op == OP_STEP;
    const float out_reward = stepped ? reward : 0.0f;
    const bool out_term = stepped && term, out_trunc = stepped && trunc;
    if (stepped) {
      step_count += 1; rng_ctr += 1;  // rocket_base_env.py:327
      if (V.b.nonfinite()) flags |= PF_F_NONFINITE;  // (the base state words; NaN / Inf guard as in the other env kernels)
    }
    auto flags_word = [&]() {
      return done_flags(flags & ~PF_F_PAD_CONTACT, term, trunc, V.b.contact_now) | (pad_contact != 0.0f ? PF_F_PAD_CONTACT : 0);
    };
    // SAME_STEP auto-reset (rare path): terminal observation and info, then the reset with its settle steps in this launch
    if (P.autoreset == PF_AUTORESET_SAME_STEP) {
      const bool same = stepped && (term || trunc);
      if (__any(same)) {
        if (B.final_obs != nullptr) {
          if (active) write_obs_row();
          flush_obs_tile(tile, B.final_obs + toff * D, D, kWave, n, wave_base, tid, wave_all, active);
        }
        if (B.final_info != nullptr && same) {
          B.final_info[2 * (toff + li) + 0] = flags_word();
          B.final_info[2 * (toff + li) + 1] = 0;
        }
        if (same) {
          begin_reset();
          settling = true;
        }
        run(same ? P.settle_steps : 0, true);
      }
    }
    if (active && settling) rng_ctr += 1;  // end_reset's compute_state (rocket_base_env.py:216-223)

    if (active) write_obs_row();
    flush_obs_tile(tile, B.obs + toff * D, D, kWave, n, wave_base, tid, wave_all, active);
    if (active) {
      flags = flags_word();
      if (ks == n_env_steps - 1) {  // the state goes back to HBM once per launch
        V.store(Sout, N, li, 0, 0.0f, int4{step_count, flags, (int)rng_ctr, 0});
        Sout[(size_t)(Rocket::GROUPS + 0) * N + li] = float4{act[0], act[1], act[2], act[3]};
        Sout[(size_t)(Rocket::GROUPS + 1) * N + li] = float4{act[4], act[5], act[6], 0.0f};
      }
      step_outputs(B, op, toff, li, out_reward, out_term, out_trunc);
    }
  }
}

// pf_sample_actions for the seven-wide action box (rocket_base_env.py:95-119): the same Philox keys as env_kernel's rollout draws
__global__ void __launch_bounds__(256) sample_actions7_kernel(const pf_params P, float* actions, const int n, const uint64_t lane0,
                                                              const uint32_t step_index) {
  const int lane = blockIdx.x * 256 + threadIdx.x;
  if (lane >= n) return;
  float a[kRlActionDim];
  sampled_action7<true>((uint32_t)P.seed, (uint32_t)(P.seed >> 32), (uint32_t)(lane0 + lane), step_index, kRlActionLow, kRlActionHigh, a);
#pragma unroll
  for (int j = 0; j < kRlActionDim; ++j) actions[(size_t)lane * kRlActionDim + j] = a[j];
}

}  // namespace pf
