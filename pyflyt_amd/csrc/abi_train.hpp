// abi_train.hpp -- the C ABI's training side: pf_policy_act, pf_gae, pf_traj_stats / pf_traj_stats_masked, pf_ppo_loss, pf_mlp_forward / pf_mlp_backward, pf_ppo_grad (and pf_ppo_grad_rows),
// the sharded calls (pf_ppo_adv_sums, pf_ppo_grad_shard, pf_ppo_shard_combine, pf_adv_sums_add, pf_moments_merge), pf_adam_step, pf_world_sync and pf_episode_outcomes, each behind the checks and launches it shares with another. Host code.
#pragma once
#include <cmath>
#include <type_traits>

#include "abi_ctx.hpp"  // (with the HIP runtime)
#include "rocket_landing.hpp"  // kRlActionDim
#include "gae.hpp"
#include "traj_stats.hpp"
#include "ppo_loss.hpp"
#include "policy_act.hpp"
#include "mlp.hpp"
#include "ppo_grad.hpp"
#include "ppo_shard.hpp"
#include "adam.hpp"
#include "kl_control.hpp"
#include "world_sync.hpp"
#include "outcomes.hpp"

// the env's action width: what pf_policy_act writes per row and pf_gae's log-probabilities sum over
static int env_action_dim(const pf_params& P) { return P.task == PF_TASK_ROCKET_LANDING ? pf::kRlActionDim : (P.task == PF_TASK_DOGFIGHT && P.df_action_dim == 6) ? 6 : 4; }
static_assert(pf::kRlActionDim <= pf::kActMaxA, "the output layer's block holds the widest action");
// policy_act_kernel's one launch site: workgroups stride over the 64-row tiles, two per CU at the most (all resident), so the weight staging is paid once per workgroup
static int launch_policy_act(pf_ctx* ctx, const pf::ActK& AK, int64_t rows, void* stream) {
  const int64_t tiles = (rows + pf::kActRows - 1) / pf::kActRows;
  const int grid = tiles < (int64_t)ctx->act_grid_cap ? (int)tiles : ctx->act_grid_cap;
  hipLaunchKernelGGL(pf::policy_act_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, AK);
  return launched(ctx);
}
// What pf_ppo_loss and pf_ppo_grad launch first: the advantages' moments, into `fin`; vbytes / vmask: how the kernels behind it read `valid`.
struct ppo_adv {
  const uint8_t* vbytes;
  uint32_t vmask;
  double* fin;
};
// pf_ppo_grad_rows' index list: the slots' row numbers into a batch of rows_total rows; index null = a contiguous call, every row its own slot
struct ppo_rows {
  const int32_t* index;
  int64_t rows_total;
};
constexpr ppo_rows kNoIndex{nullptr, 0};
// pf_ppo_grad_shard's two additions: the advantage sums of ALL shards, and the shard's block of raw totals; adv_sums null = any other call
struct ppo_shard {
  const double* adv_sums;
  double* block;
};
constexpr ppo_shard kNoShard{nullptr, nullptr};
// the advantage pass over `rows` rows, or over the `rows` slots of the index list ix: its rows of partials in the context's block, nothing finished
static ppo_adv launch_ppo_adv_part(pf_ctx* ctx, const float* advantages, const uint8_t* valid, size_t rows, const ppo_rows& ix, hipStream_t s) {
  double* adv_part = ctx->ppo_scratch + pf::kPpoAdvOffset;
  // (no valid: the byte loads read the advantages' first M bytes and the mask drops them)
  const ppo_adv r{valid ? valid : reinterpret_cast<const uint8_t*>(advantages), valid ? 0xFFu : 0u, ctx->ppo_scratch + pf::kPpoFinOffset};
  const unsigned grid = pf::ppo_grid(rows);
  if (ix.index)
    hipLaunchKernelGGL(pf::ppo_adv_rows_kernel, dim3(grid), dim3(pf::kPpoBlock), 0, s, advantages, r.vbytes, r.vmask, ix.index, rows, (uint32_t)ix.rows_total, adv_part);
  else
    hipLaunchKernelGGL(pf::ppo_adv_kernel, dim3(grid), dim3(pf::kPpoBlock), 0, s, advantages, r.vbytes, r.vmask, rows, adv_part);
  return r;
}
// the moments over `rows` rows, or over the `rows` slots of the index list ix
static ppo_adv launch_ppo_adv(pf_ctx* ctx, const float* advantages, const uint8_t* valid, size_t rows, const ppo_rows& ix, hipStream_t s) {
  const ppo_adv r = launch_ppo_adv_part(ctx, advantages, valid, rows, ix, s);
  hipLaunchKernelGGL(pf::ppo_adv_finish_kernel, dim3(1), dim3(pf::kPpoBlock), 0, s, (const double*)(ctx->ppo_scratch + pf::kPpoAdvOffset), (int)pf::ppo_grid(rows), r.fin);
  return r;
}
// What pf_ppo_loss and pf_ppo_grad launch last: `kernel`, one of the finish kernels, over n_blocks rows of partials. `a`: either call's
// argument block; `more`: what ppo_finish_opt_kernel and ppo_finish_rows_kernel take behind the arguments all of them have.
template <class KERNEL, class ARGS, class... MORE>
static void launch_ppo_finish(KERNEL kernel, hipStream_t s, const double* partials, int n_blocks, const ppo_adv& adv, const ARGS* a, int width, MORE... more) {
  hipLaunchKernelGGL(kernel, dim3(1), dim3(pf::kPpoBlock), 0, s, partials, n_blocks, (const double*)adv.fin, a->log_std, width, a->vf_coef, a->ent_coef, a->stats,
                     a->grad_log_std, more...);
}
// ppo_main_kernel's instantiation for a row width and a path; KT: PpoK, or PpoOptMainK for the call with the options
template <class KT>
static auto ppo_main_pick(int width, bool vec) -> void (*)(KT, size_t, const double*, double*) {
  using pf::ppo_main_kernel;
  void (*const by_width[pf::kPpoMaxA])(KT, size_t, const double*, double*) = {
      ppo_main_kernel<1, false, KT>, ppo_main_kernel<2, false, KT>, ppo_main_kernel<3, false, KT>, ppo_main_kernel<4, false, KT>,
      ppo_main_kernel<5, false, KT>, ppo_main_kernel<6, false, KT>, ppo_main_kernel<7, false, KT>, ppo_main_kernel<8, false, KT>};
  return vec ? ppo_main_kernel<4, true, KT> : by_width[width - 1];
}
// pf_ppo_loss' launches behind the advantage pass: the main kernel of K's type and the finish kernel that goes with it
template <class KT>
static void launch_ppo_loss(pf_ctx* ctx, const KT& K, const pf_ppo_loss_args* a, size_t rows, int width, const ppo_adv& adv, hipStream_t s) {
  double* main_part = ctx->ppo_scratch + pf::kPpoMainOffset;
  const unsigned grid = pf::ppo_grid(rows);
  // (one float4 per row where the rows are four wide and the caller's pointers allow it; the same arithmetic either way)
  const bool vec = width == 4 && (((uintptr_t)a->actions | (uintptr_t)a->mean | (uintptr_t)a->grad_mean) & 15) == 0;
  hipLaunchKernelGGL(ppo_main_pick<KT>(width, vec), dim3(grid), dim3(pf::kPpoBlock), 0, s, K, rows, (const double*)adv.fin, main_part);
  if constexpr (KT::kOpt)
    launch_ppo_finish(pf::ppo_finish_opt_kernel, s, main_part, (int)grid, adv, a, width, K.o.vclip, K.o.bnd, K.o.bounds_coef);
  else
    launch_ppo_finish(pf::ppo_finish_kernel, s, main_part, (int)grid, adv, a, width);
}
// A head's tile launch on one network. Its block is MlpK, what pf_ppo_grad_args gives both heads, the call's advantage block and rows of
// partials; OPT adds the options KO, IDX the index list. The block's type is the one each call has always named.
template <int HEAD, bool OPT, bool IDX>
static void launch_ppo_grad_head(const pf_ppo_grad_args* a, const pf_mlp* net, float* part, int64_t rows, const ppo_adv& adv, double* stat_part,
                                 const pf::PpoOptK& KO, const ppo_rows& ix, int grid, hipStream_t s) {
  typedef std::conditional_t<IDX, pf::PpoGradRowsK<HEAD, OPT>, std::conditional_t<OPT, pf::PpoGradOptK<HEAD>, pf::PpoGradK<HEAD>>> KT;
  KT K;
  static_cast<pf::MlpK&>(K) = pf::MlpK{*net, a->x, nullptr, part, (int)rows};
  K.clip = a->clip, K.vf_coef = a->vf_coef, K.normalize = a->normalize_advantage;
  K.log_std = a->log_std, K.actions = a->actions, K.logp_old = a->logp_old, K.advantages = a->advantages, K.returns = a->returns;
  K.vbytes = adv.vbytes, K.vmask = adv.vmask, K.fin = adv.fin, K.stat_part = stat_part;
  if constexpr (OPT) K.o = KO;
  if constexpr (IDX) K.row_index = ix.index, K.rows_total = (uint32_t)ix.rows_total;
  hipLaunchKernelGGL(pf::mlp_backward_kernel<KT>, dim3(grid), dim3(256), 0, s, K);
}
// the workgroups' partial gradients (`part`, one row of the network's parameters per workgroup of the backward launch) summed into gw / gb
static void launch_mlp_reduce(const pf_mlp* q, float* const* gw, float* const* gb, const float* part, int grid, hipStream_t s) {
  pf::MlpOutK O;
  const int P = pf::mlp_param_count(*q, O.end);
  for (int l = 0; l < 3; ++l) {
    O.p[2 * l] = l < q->n_layers ? gw[l] : nullptr;
    O.p[2 * l + 1] = l < q->n_layers ? gb[l] : nullptr;
  }
  hipLaunchKernelGGL(pf::mlp_reduce_kernel, dim3((P + 255) / 256), dim3(256), 0, s, part, grid, P, O);
}
// The seven launches of a gradient call on `rows` rows, or slots of ix: the advantage pass and its finish, the actor's head and the critic's,
// a reduction for each, the finish. OPT: the heads and the finish with the options KO; IDX: all of them through the index list (DESIGN.md
// section 31 has the table). gw / gb: either network's gradient outputs. sh (pf_ppo_grad_shard): the advantage block comes
// from sh.adv_sums behind the shard's own pass, and the last launch leaves the raw totals in sh.block.
template <bool OPT, bool IDX>
static void launch_ppo_grad(pf_ctx* ctx, const pf_ppo_grad_args* a, float* const* const (&gw)[2], float* const* const (&gb)[2], const pf::PpoOptK& KO,
                            const ppo_rows& ix, const ppo_shard& sh, int64_t rows, void* workspace, hipStream_t s) {
  const pf_mlp* nets[2] = {a->actor, a->critic};
  const int grid = pf::mlp_grid(rows), A = a->actor->out_dim;
  double* stat_part = (double*)workspace;
  float* const part0 = (float*)((char*)workspace + pf::ppo_grad_stat_bytes(grid));
  float* const part[2] = {part0, part0 + (size_t)grid * (size_t)pf::mlp_param_count(*a->actor, nullptr)};
  const ppo_adv adv = sh.adv_sums ? launch_ppo_adv_part(ctx, a->advantages, a->valid, (size_t)rows, ix, s) : launch_ppo_adv(ctx, a->advantages, a->valid, (size_t)rows, ix, s);
  if (sh.adv_sums) hipLaunchKernelGGL(pf::ppo_shard_fin_kernel, dim3(1), dim3(64), 0, s, sh.adv_sums, adv.fin);
  launch_ppo_grad_head<pf::kGradActor, OPT, IDX>(a, nets[0], part[0], rows, adv, stat_part, KO, ix, grid, s);
  launch_ppo_grad_head<pf::kGradCritic, OPT, IDX>(a, nets[1], part[1], rows, adv, stat_part, KO, ix, grid, s);
  for (int k = 0; k < 2; ++k) launch_mlp_reduce(nets[k], gw[k], gb[k], part[k], grid, s);
  if (sh.adv_sums)
    hipLaunchKernelGGL(pf::ppo_shard_finish_kernel, dim3(1), dim3(pf::kPpoBlock), 0, s, (const double*)stat_part, grid, OPT ? pf::kPpoStride : pf::kPpoQ,
                       (const double*)(ctx->ppo_scratch + pf::kPpoAdvOffset), (int)pf::ppo_grid((size_t)rows), IDX ? 1 : 0, sh.block);
  else if constexpr (IDX)  // (with the options off, the finish without them: nothing of KO is read)
    launch_ppo_finish(pf::ppo_finish_rows_kernel<OPT>, s, stat_part, grid, adv, a, A, OPT ? KO.vclip : 0, OPT ? KO.bnd : 0, OPT ? KO.bounds_coef : 0.0f,
                      (const double*)(ctx->ppo_scratch + pf::kPpoAdvOffset), (int)pf::ppo_grid((size_t)rows));
  else if constexpr (OPT)
    launch_ppo_finish(pf::ppo_finish_opt_kernel, s, stat_part, grid, adv, a, A, KO.vclip, KO.bnd, KO.bounds_coef);
  else
    launch_ppo_finish(pf::ppo_finish_kernel, s, stat_part, grid, adv, a, A);
}

extern "C" {
int pf_policy_act(pf_ctx* ctx, const pf_policy* q, float* actions_out, uint32_t step_index, void* stream) {
  static const char* who = "pf_policy_act";
  if (!ctx) return arg_fail(ctx, who, "ctx is required");
  if (!q) return arg_fail(ctx, who, "policy is required");
  const pf_params& P = ctx->P;
  if (P.task == PF_TASK_NONE) return who_fail(ctx, PF_ERR_UNSUPPORTED, who, "needs a context with an env task (this one drives the Aviary level only)");
  if (!actions_out) return arg_fail(ctx, who, "actions_out is required");
  if (!q->obs0) return arg_fail(ctx, who, "obs0 (the [n][pf_obs_dim()] input rows) is required");
  if (int rc = policy_net_check(ctx, who, q)) return rc;
  const int D = pf_obs_dim(ctx);
  if (D > pf::kActMaxIn) return who_fail(ctx, PF_ERR_UNSUPPORTED, who, "observation wider than 128");
  if (int rc = ensure_device(ctx)) return rc;
  const pf::ActK AK{*q, actions_out, ctx->n, D, env_action_dim(P), (uint32_t)P.seed, (uint32_t)(P.seed >> 32), step_index, ctx->lane0};
  return launch_policy_act(ctx, AK, ctx->n, stream);
}
// what pf_gae and pf_traj_stats refuse first, in this order (`a`: the call's argument block)
static int traj_call_check(pf_ctx* ctx, const char* who, const void* a, int k_steps) {
  if (!ctx || !a) return arg_fail(ctx, who, "ctx and the argument block are required");
  if (ctx->P.task == PF_TASK_NONE) return who_fail(ctx, PF_ERR_UNSUPPORTED, who, "needs a context with an env task (this one drives the Aviary level only)");
  if (k_steps < 1) return arg_fail(ctx, who, "k_steps must be >= 1");
  return PF_OK;
}
int pf_gae(pf_ctx* ctx, const pf_gae_args* a, int k_steps, void* stream) {
  static const char* who = "pf_gae";
  if (int rc = traj_call_check(ctx, who, a, k_steps)) return rc;
  const pf_params& P = ctx->P;
  const arg_ptr required[] = {{"reward", a->reward}, {"terminated", a->terminated}, {"truncated", a->truncated}, {"values", a->values},
                              {"advantages", a->advantages}, {"returns", a->returns}, {nullptr, nullptr}};
  if (int rc = require_args(ctx, who, required)) return rc;
  if (!(a->gamma >= 0.0f && a->gamma <= 1.0f)) return arg_fail(ctx, who, "gamma must be finite and in [0, 1]");
  if (!(a->lambda >= 0.0f && a->lambda <= 1.0f)) return arg_fail(ctx, who, "lambda must be finite and in [0, 1]");
  if (P.autoreset == PF_AUTORESET_SAME_STEP && !a->final_values)
    return arg_fail(ctx, who, "final_values is required under SAME_STEP (the value of the terminal observation in final_obs)");
  if (P.autoreset != PF_AUTORESET_SAME_STEP && a->final_values)
    return arg_fail(ctx, who, "final_values must be NULL outside SAME_STEP (there is no final_obs)");
  if (P.autoreset != PF_AUTORESET_NEXT_STEP && a->episode_start)
    return arg_fail(ctx, who, "episode_start must be NULL outside NEXT_STEP (no other mode has reset steps)");
  const int n_logp = (a->actions != nullptr) + (a->mean != nullptr) + (a->log_std != nullptr) + (a->logp_out != nullptr);
  if (n_logp != 0 && n_logp != 4) return arg_fail(ctx, who, "actions, mean, log_std and logp_out come together or are all NULL");
  if (int rc = ensure_device(ctx)) return rc;
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
  return launched(ctx);
}
// pf_traj_stats and pf_traj_stats_masked behind traj_call_check: `masked` = validity is the [k][n] bytes of `valid` (and a->episode_start is NULL)
static int traj_stats_launch(pf_ctx* ctx, const char* who, const pf_traj_stats_args* a, bool masked, const uint8_t* valid, int k_steps, void* stream) {
  const pf_params& P = ctx->P;
  const arg_ptr required[] = {{"reward", a->reward}, {"terminated", a->terminated}, {"truncated", a->truncated}, {"summary", a->summary},
                              {"carry_return", a->carry_return}, {"carry_length", a->carry_length}, {"carry_disc", a->carry_disc}, {nullptr, nullptr}};
  if (int rc = require_args(ctx, who, required)) return rc;
  if (masked && !valid) return arg_fail(ctx, who, "valid (the [k][n] mask of the steps that are transitions) is required");
  if (!(a->gamma >= 0.0f && a->gamma <= 1.0f)) return arg_fail(ctx, who, "gamma must be finite and in [0, 1]");
  if (P.autoreset != PF_AUTORESET_NEXT_STEP && a->episode_start)
    return arg_fail(ctx, who, "episode_start must be NULL outside NEXT_STEP (no other mode has reset steps)");
  if (a->obs && !a->obs_moments) return arg_fail(ctx, who, "obs comes with obs_moments (the block its moments are merged into)");
  if (!a->obs && a->obs_moments) return arg_fail(ctx, who, "obs_moments comes with obs");
  const int D = pf_obs_dim(ctx);
  if (a->obs && D > pf::kTsMaxD) return who_fail(ctx, PF_ERR_UNSUPPORTED, who, "observation rows wider than 128 have no moments kernel");
  if (int rc = ensure_device(ctx)) return rc;
  hipStream_t s = (hipStream_t)stream;
  const bool next = P.autoreset == PF_AUTORESET_NEXT_STEP;
  const int waves = (ctx->n + 63) / 64;
  double* scan_part = ctx->ts_scratch;
  double* obs_part = ctx->ts_scratch + pf::ts_scan_words(ctx->n);
  const uint8_t* bytes = masked ? valid : a->episode_start;  // (the kernels' one slot for either: traj_stats.hpp)
  const pf::TsK K{a->gamma, a->reward, a->terminated, a->truncated, bytes, a->carry_return, a->carry_length, a->carry_disc,
                  a->ep_return_out, a->ep_length_out, a->ret_moments};
  using pf::kTsAll, pf::kTsMask, pf::kTsNext;
  hipLaunchKernelGGL(masked ? pf::ts_scan_kernel<kTsMask> : next ? pf::ts_scan_kernel<kTsNext> : pf::ts_scan_kernel<kTsAll>, dim3(waves), dim3(64), 0, s, K,
                     ctx->n, k_steps, scan_part);
  unsigned grid = 0;
  if (a->obs) {
    const size_t rows = (size_t)k_steps * (size_t)ctx->n;
    grid = pf::ts_obs_grid(rows * (size_t)D);
    hipLaunchKernelGGL(masked ? pf::ts_obs_kernel<kTsMask> : next ? pf::ts_obs_kernel<kTsNext> : pf::ts_obs_kernel<kTsAll>, dim3(grid), dim3(pf::kTsObsBlock),
                       0, s, a->obs, a->terminated, a->truncated, bytes, a->obs_moments, obs_part, rows, ctx->n, D);
  }
  hipLaunchKernelGGL(pf::ts_finish_kernel, dim3(1), dim3(pf::kTsFinishBlock), 0, s, scan_part, waves, a->obs ? obs_part : nullptr, (int)grid, D,
                     a->summary, a->ret_moments, a->obs_moments);
  return launched(ctx);
}
int pf_traj_stats(pf_ctx* ctx, const pf_traj_stats_args* a, int k_steps, void* stream) {
  static const char* who = "pf_traj_stats";
  if (int rc = traj_call_check(ctx, who, a, k_steps)) return rc;
  return traj_stats_launch(ctx, who, a, false, nullptr, k_steps, stream);
}
int pf_traj_stats_masked(pf_ctx* ctx, const pf_traj_stats_masked_args* a, int k_steps, void* stream) {
  static const char* who = "pf_traj_stats_masked";
  if (int rc = traj_call_check(ctx, who, a, k_steps)) return rc;
  // (the block is pf_traj_stats_args with `valid` where episode_start stood; there is no episode_start here)
  const pf_traj_stats_args u{a->gamma, a->reward, a->terminated, a->truncated, nullptr, a->obs, a->carry_return, a->carry_length, a->carry_disc,
                             a->ep_return_out, a->ep_length_out, a->summary, a->ret_moments, a->obs_moments};
  return traj_stats_launch(ctx, who, &u, true, a->valid, k_steps, stream);
}
// what pf_ppo_loss and pf_ppo_grad check of the loss's coefficients
static int ppo_coef_check(pf_ctx* ctx, const char* who, float clip, float vf_coef, float ent_coef, int32_t normalize_advantage) {
  if (!(clip > 0.0f && clip < INFINITY)) return arg_fail(ctx, who, "clip must be finite and > 0");
  if (!(vf_coef >= 0.0f && vf_coef < INFINITY)) return arg_fail(ctx, who, "vf_coef must be finite and >= 0");
  if (!(ent_coef >= 0.0f && ent_coef < INFINITY)) return arg_fail(ctx, who, "ent_coef must be finite and >= 0");
  if (normalize_advantage != 0 && normalize_advantage != 1) return arg_fail(ctx, who, "normalize_advantage must be 0 or 1");
  return PF_OK;
}
// What pf_ppo_loss_opt and pf_ppo_grad_opt check of their options, A = the action width. *on = an option is on (off: the call is the
// one without options); K: the kernels' block, an option that is off filled so that nothing of it is chosen (`readable`: M floats)
static int ppo_options_check(pf_ctx* ctx, const char* who, const pf_ppo_options* o, int A, const float* readable, pf::PpoOptK* K, bool* on) {
  *on = false;
  if (!o) return PF_OK;
  if (o->values_old && !(o->clip_vf > 0.0f && o->clip_vf < INFINITY)) return arg_fail(ctx, who, "clip_vf must be finite and > 0 (values_old is given)");
  if (!(o->bounds_coef >= 0.0f && o->bounds_coef < INFINITY)) return arg_fail(ctx, who, "bounds_coef must be finite and >= 0");
  const bool bnd = o->bounds_coef > 0.0f;
  for (int c = 0; bnd && c < A; ++c) {
    if (o->bounds_lo[c] != o->bounds_lo[c]) return arg_fail(ctx, who, "bounds_lo must not hold a NaN (-infinity: open below)");
    if (o->bounds_hi[c] != o->bounds_hi[c]) return arg_fail(ctx, who, "bounds_hi must not hold a NaN (+infinity: open above)");
    if (o->bounds_lo[c] > o->bounds_hi[c]) return arg_fail(ctx, who, "bounds_lo must be <= bounds_hi in every column");
  }
  K->values_old = o->values_old ? o->values_old : readable;
  K->vclip = o->values_old ? 1 : 0;
  K->bnd = bnd ? 1 : 0;
  K->clip_vf = o->values_old ? o->clip_vf : 1.0f;
  K->bounds_coef = o->bounds_coef;
  for (int c = 0; c < pf::kPpoMaxA; ++c) {
    K->lo[c] = bnd && c < A ? o->bounds_lo[c] : -INFINITY;
    K->hi[c] = bnd && c < A ? o->bounds_hi[c] : INFINITY;
  }
  *on = K->vclip || K->bnd;
  return PF_OK;
}
// pf_ppo_loss (o = NULL) and pf_ppo_loss_opt
static int ppo_loss_call(pf_ctx* ctx, const char* who, const pf_ppo_loss_args* a, const pf_ppo_options* o, size_t rows, int width, void* stream) {
  if (!ctx || !a) return arg_fail(ctx, who, "ctx and the argument block are required");
  if (rows < 1) return arg_fail(ctx, who, "rows must be >= 1");
  if (width < 1 || width > pf::kPpoMaxA) return arg_fail(ctx, who, "width must be in 1..8");
  const arg_ptr required[] = {{"mean", a->mean}, {"log_std", a->log_std}, {"actions", a->actions}, {"logp_old", a->logp_old},
                              {"advantages", a->advantages}, {"returns", a->returns}, {"value", a->value}, {"grad_mean", a->grad_mean},
                              {"grad_value", a->grad_value}, {"grad_log_std", a->grad_log_std}, {"stats", a->stats}, {nullptr, nullptr}};
  if (int rc = require_args(ctx, who, required)) return rc;
  if (int rc = ppo_coef_check(ctx, who, a->clip, a->vf_coef, a->ent_coef, a->normalize_advantage)) return rc;
  pf::PpoOptMainK K;  // (the call without options passes the PpoK in it)
  bool opt = false;
  if (int rc = ppo_options_check(ctx, who, o, width, a->returns, &K.o, &opt)) return rc;
  if (int rc = ensure_device(ctx)) return rc;
  hipStream_t s = (hipStream_t)stream;
  const ppo_adv adv = launch_ppo_adv(ctx, a->advantages, a->valid, rows, kNoIndex, s);
  static_cast<pf::PpoK&>(K) = pf::PpoK{a->clip, a->vf_coef, a->normalize_advantage, a->mean, a->log_std, a->actions, a->logp_old, a->advantages, a->returns, a->value,
                                      adv.vbytes, adv.vmask, a->grad_mean, a->grad_value};
  if (opt)
    launch_ppo_loss<pf::PpoOptMainK>(ctx, K, a, rows, width, adv, s);
  else
    launch_ppo_loss<pf::PpoK>(ctx, K, a, rows, width, adv, s);
  return launched(ctx);
}
int pf_ppo_loss(pf_ctx* ctx, const pf_ppo_loss_args* a, size_t rows, int width, void* stream) {
  return ppo_loss_call(ctx, "pf_ppo_loss", a, nullptr, rows, width, stream);
}
size_t pf_sizeof_ppo_options(void) { return sizeof(pf_ppo_options); }
int pf_ppo_loss_opt(pf_ctx* ctx, const pf_ppo_loss_args* a, const pf_ppo_options* options, size_t rows, int width, void* stream) {
  return ppo_loss_call(ctx, "pf_ppo_loss_opt", a, options, rows, width, stream);
}
// ---- pf_mlp_forward, pf_mlp_backward and pf_ppo_grad: what they check of a network and of `rows`, and the pieces of their launches
static const char* mlp_shape_error(const pf_mlp* q) {
  if (q->n_layers != 2 && q->n_layers != 3) return "n_layers must be 2 or 3";
  for (int l = 0; l + 1 < q->n_layers; ++l)
    if (q->width[l] < 1 || q->width[l] > PF_POLICY_MAX_HIDDEN) return "width: hidden widths must be in 1..PF_POLICY_MAX_HIDDEN (64)";
  if (q->activation != PF_ACT_TANH && q->activation != PF_ACT_RELU) return "activation must be PF_ACT_TANH or PF_ACT_RELU";
  if (q->in_dim < 1 || q->in_dim > pf::kActMaxIn) return "in_dim must be in 1..128";
  if (q->out_dim < 1 || q->out_dim > pf::kActMaxA) return "out_dim must be in 1..8";
  return nullptr;
}
static bool mlp_has_params(const pf_mlp* q) {
  for (int l = 0; l < q->n_layers; ++l)
    if (!q->w[l] || !q->b[l]) return false;
  return true;
}
// a count of rows under the name the call gives it: 1 or more, and below what the tile loops reach in 32 bits (`why`: the call's reason for that)
static int rows_check(pf_ctx* ctx, const char* who, int64_t rows, const char* name, const char* why) {
  if (rows >= 1 && rows <= (int64_t)INT32_MAX - pf::kActRows) return PF_OK;
  char what[128];
  if (rows < 1)
    snprintf(what, sizeof(what), "%s must be >= 1", name);
  else
    snprintf(what, sizeof(what), "%s must be below 2^31 - 64 (%s)", name, why);
  return arg_fail(ctx, who, what);
}
// pf_mlp_forward / pf_mlp_backward: what both check first, the context included; `who` is the call's name
static int mlp_check(pf_ctx* ctx, const char* who, const pf_mlp* q, int64_t rows) {
  if (!ctx) return arg_fail(ctx, who, "ctx is required");
  if (!q) return arg_fail(ctx, who, "mlp is required");
  if (const char* e = mlp_shape_error(q)) return arg_fail(ctx, who, e);
  if (!mlp_has_params(q)) return arg_fail(ctx, who, "w / b: every layer needs w and b");
  return rows_check(ctx, who, rows, "rows", "the kernels index rows with 32 bits");
}
// a network's gradient outputs as spans, layer l's under the names wn[l] and bn[l]; returns the new count
static int append_grad_spans(arg_span* spans, int ns, const pf_mlp* q, const char* const* wn, const char* const* bn, float* const* gw, float* const* gb) {
  for (int l = 0; l < q->n_layers; ++l) {
    const size_t n_in = l == 0 ? q->in_dim : q->width[l - 1], n_out = l + 1 == q->n_layers ? q->out_dim : q->width[l];
    spans[ns++] = {wn[l], gw[l], sizeof(float) * n_in * n_out};
    spans[ns++] = {bn[l], gb[l], sizeof(float) * n_out};
  }
  return ns;
}
int pf_mlp_forward(pf_ctx* ctx, const pf_mlp* q, const float* x, int64_t rows, float* out, void* stream) {
  static const char* who = "pf_mlp_forward";
  if (int rc = mlp_check(ctx, who, q, rows)) return rc;
  if (!x) return arg_fail(ctx, who, "x is required");
  if (!out) return arg_fail(ctx, who, "out is required");
  char buf[128];
  const arg_span spans[2] = {{"x", x, sizeof(float) * (size_t)rows * q->in_dim}, {"out", out, sizeof(float) * (size_t)rows * q->out_dim}};
  if (const char* e = spans_overlap(spans, 2, buf, sizeof(buf))) return arg_fail(ctx, who, e);
  if (int rc = ensure_device(ctx)) return rc;
  // policy_act_kernel itself, the draw off (no log_std), the caller's rows as its observations and out_dim as its action width
  pf_policy P{};  // (log_std, mean_out and the layers the network does not have: null)
  P.n_layers = q->n_layers;
  P.width[0] = q->width[0];
  P.width[1] = q->width[1];
  P.activation = q->activation;
  for (int l = 0; l < q->n_layers; ++l) P.w[l] = q->w[l], P.b[l] = q->b[l];
  P.obs0 = x;
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
  if (int rc = mlp_check(ctx, who, q, rows)) return rc;
  const arg_ptr required[] = {{"x", x}, {"grad_out", grad_out}, {"grad_w", grad_w}, {"grad_b", grad_b}, {nullptr, nullptr}};
  if (int rc = require_args(ctx, who, required)) return rc;
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
  ns = append_grad_spans(spans, ns, q, wn, bn, grad_w, grad_b);
  char buf[128];
  if (const char* e = spans_overlap(spans, ns, buf, sizeof(buf))) return arg_fail(ctx, who, e);
  if (int rc = ensure_device(ctx)) return rc;
  hipStream_t s = (hipStream_t)stream;
  const int grid = pf::mlp_grid(rows);
  const pf::MlpK K{*q, x, grad_out, (float*)workspace, (int)rows};
  hipLaunchKernelGGL(pf::mlp_backward_kernel<pf::MlpK>, dim3(grid), dim3(256), 0, s, K);
  launch_mlp_reduce(q, grad_w, grad_b, (const float*)workspace, grid, s);
  return launched(ctx);
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
// pf_ppo_grad (o = NULL), pf_ppo_grad_opt, pf_ppo_grad_rows (ix.index: rows = m slots of it into a batch of ix.rows_total rows) and
// pf_ppo_grad_shard (`shard`: sh holds its two blocks, which stand where grad_log_std and stats stand in the other calls)
static int ppo_grad_call(pf_ctx* ctx, const char* who, const pf_ppo_grad_args* a, const pf_ppo_options* o, int64_t rows, const ppo_rows& ix, void* workspace,
                         size_t workspace_bytes, void* stream, bool shard = false, const ppo_shard& sh = kNoShard) {
  if (!ctx) return arg_fail(ctx, who, "ctx is required");
  if (!a) return arg_fail(ctx, who, "the argument block is required");
  if (!a->actor) return arg_fail(ctx, who, "actor is required");
  if (!a->critic) return arg_fail(ctx, who, "critic is required");
  char buf[160];
  if (const char* e = ppo_grad_shape_error(a->actor, a->critic, buf, sizeof(buf))) return arg_fail(ctx, who, e);
  const pf_mlp* nets[2] = {a->actor, a->critic};
  if (!mlp_has_params(a->actor)) return arg_fail(ctx, who, "actor: w / b: every layer needs w and b");
  if (!mlp_has_params(a->critic)) return arg_fail(ctx, who, "critic: w / b: every layer needs w and b");
  if (!ix.index)  // (pf_ppo_grad_rows has refused a bad m, under that name, before anything else)
    if (int rc = rows_check(ctx, who, rows, "rows", "the kernels index rows with 32 bits")) return rc;
  if (shard && a->grad_log_std) return arg_fail(ctx, who, "grad_log_std must be NULL (an output of the joint batch: pf_ppo_shard_combine writes it)");
  if (shard && a->stats) return arg_fail(ctx, who, "stats must be NULL (an output of the joint batch: pf_ppo_shard_combine writes it)");
  const arg_ptr required[] = {{"x", a->x}, {"log_std", a->log_std}, {"actions", a->actions}, {"logp_old", a->logp_old}, {"advantages", a->advantages},
                              {"returns", a->returns}, {shard ? "adv_sums" : "grad_log_std", shard ? (const void*)sh.adv_sums : a->grad_log_std},
                              {shard ? "shard_block" : "stats", shard ? (const void*)sh.block : a->stats}, {"workspace", workspace}, {nullptr, nullptr}};
  if (int rc = require_args(ctx, who, required)) return rc;
  static const char* const gn[2][2][3] = {{{"actor_grad_w[0]", "actor_grad_w[1]", "actor_grad_w[2]"}, {"actor_grad_b[0]", "actor_grad_b[1]", "actor_grad_b[2]"}},
                                          {{"critic_grad_w[0]", "critic_grad_w[1]", "critic_grad_w[2]"}, {"critic_grad_b[0]", "critic_grad_b[1]", "critic_grad_b[2]"}}};
  float* const* const gw[2] = {a->actor_grad_w, a->critic_grad_w};
  float* const* const gb[2] = {a->actor_grad_b, a->critic_grad_b};
  for (int k = 0; k < 2; ++k)
    for (int l = 0; l < nets[k]->n_layers; ++l) {
      const arg_ptr outs[] = {{gn[k][0][l], gw[k][l]}, {gn[k][1][l], gb[k][l]}, {nullptr, nullptr}};
      if (int rc = require_args(ctx, who, outs)) return rc;
    }
  if (int rc = ppo_coef_check(ctx, who, a->clip, a->vf_coef, a->ent_coef, a->normalize_advantage)) return rc;
  const size_t need = pf_ppo_grad_workspace_bytes(a->actor, a->critic, rows);
  if (workspace_bytes < need) return arg_fail(ctx, who, "workspace_bytes is below pf_ppo_grad_workspace_bytes(actor, critic, rows)");
  if (((uintptr_t)workspace & 7) != 0) return arg_fail(ctx, who, "workspace must be 8-byte aligned (it holds rows of double partial sums)");
  // M: the rows the inputs hold (an indexed call reads anywhere in the batch); the kernels work on `rows` of them
  const size_t M = (size_t)(ix.index ? ix.rows_total : rows), A = (size_t)a->actor->out_dim;
  pf::PpoOptK KO;
  bool opt = false;
  if (int rc = ppo_options_check(ctx, who, o, (int)A, a->returns, &KO, &opt)) return rc;
  arg_span spans[10 + 15];
  int ns = 0;
  if (ix.index) spans[ns++] = {"row_index", ix.index, sizeof(int32_t) * (size_t)rows};
  spans[ns++] = {"x", a->x, sizeof(float) * M * a->actor->in_dim};
  spans[ns++] = {"log_std", a->log_std, sizeof(float) * A};
  spans[ns++] = {"actions", a->actions, sizeof(float) * M * A};
  spans[ns++] = {"logp_old", a->logp_old, sizeof(float) * M};
  spans[ns++] = {"advantages", a->advantages, sizeof(float) * M};
  spans[ns++] = {"returns", a->returns, sizeof(float) * M};
  if (a->valid) spans[ns++] = {"valid", a->valid, M};
  if (o && o->values_old) spans[ns++] = {"values_old", o->values_old, sizeof(float) * M};
  if (shard) spans[ns++] = {"adv_sums", sh.adv_sums, sizeof(double) * 4};
  const int n_read = ns;
  spans[ns++] = {"workspace", workspace, need};
  if (shard) {
    spans[ns++] = {"shard_block", sh.block, sizeof(double) * PF_PPO_SHARD_WORDS};
  } else {
    spans[ns++] = {"grad_log_std", a->grad_log_std, sizeof(float) * A};
    spans[ns++] = {"stats", a->stats, sizeof(double) * 16};
  }
  for (int k = 0; k < 2; ++k) ns = append_grad_spans(spans, ns, nets[k], gn[k][0], gn[k][1], gw[k], gb[k]);
  if (const char* e = spans_overlap(spans, ns, buf, sizeof(buf), n_read)) return arg_fail(ctx, who, e);
  if (int rc = ensure_device(ctx)) return rc;
  const auto launches = ix.index ? (opt ? launch_ppo_grad<true, true> : launch_ppo_grad<false, true>) : (opt ? launch_ppo_grad<true, false> : launch_ppo_grad<false, false>);
  launches(ctx, a, gw, gb, KO, ix, sh, rows, workspace, (hipStream_t)stream);
  return launched(ctx);
}
int pf_ppo_grad(pf_ctx* ctx, const pf_ppo_grad_args* a, int64_t rows, void* workspace, size_t workspace_bytes, void* stream) {
  return ppo_grad_call(ctx, "pf_ppo_grad", a, nullptr, rows, kNoIndex, workspace, workspace_bytes, stream);
}
int pf_ppo_grad_opt(pf_ctx* ctx, const pf_ppo_grad_args* a, const pf_ppo_options* options, int64_t rows, void* workspace, size_t workspace_bytes, void* stream) {
  return ppo_grad_call(ctx, "pf_ppo_grad_opt", a, options, rows, kNoIndex, workspace, workspace_bytes, stream);
}
int pf_ppo_grad_rows(pf_ctx* ctx, const pf_ppo_grad_args* a, const pf_ppo_options* options, const int32_t* row_index, int64_t m, int64_t rows_total, void* workspace,
                     size_t workspace_bytes, void* stream) {
  static const char* who = "pf_ppo_grad_rows";
  // (what the call adds comes first and needs nothing else: m and rows_total decide every extent below)
  if (int rc = rows_check(ctx, who, m, "m", "the kernels index slots with 32 bits")) return rc;
  if (int rc = rows_check(ctx, who, rows_total, "rows_total", "row_index holds 32-bit row numbers")) return rc;
  if (!row_index) return arg_fail(ctx, who, "row_index is required");
  return ppo_grad_call(ctx, who, a, options, m, ppo_rows{row_index, rows_total}, workspace, workspace_bytes, stream);
}
// ---- the sharded calls (include/pyflyt_amd.h: SHARDED PPO)
size_t pf_sizeof_ppo_shard_combine(void) { return sizeof(pf_ppo_shard_combine_args); }
int pf_ppo_adv_sums(pf_ctx* ctx, const float* advantages, const uint8_t* valid, const int32_t* row_index, int64_t m, int64_t rows_total, double* sums, void* stream) {
  static const char* who = "pf_ppo_adv_sums";
  if (int rc = rows_check(ctx, who, m, "m", "the kernels index slots with 32 bits")) return rc;
  if (!ctx) return arg_fail(ctx, who, "ctx is required");
  const arg_ptr required[] = {{"advantages", advantages}, {"sums", sums}, {nullptr, nullptr}};
  if (int rc = require_args(ctx, who, required)) return rc;
  if (row_index)
    if (int rc = rows_check(ctx, who, rows_total, "rows_total", "row_index holds 32-bit row numbers")) return rc;
  const size_t M = (size_t)(row_index ? rows_total : m);
  arg_span spans[4];
  int ns = 0;
  if (row_index) spans[ns++] = {"row_index", row_index, sizeof(int32_t) * (size_t)m};
  spans[ns++] = {"advantages", advantages, sizeof(float) * M};
  if (valid) spans[ns++] = {"valid", valid, M};
  const int n_read = ns;
  spans[ns++] = {"sums", sums, sizeof(double) * 4};
  char buf[128];
  if (const char* e = spans_overlap(spans, ns, buf, sizeof(buf), n_read)) return arg_fail(ctx, who, e);
  if (int rc = ensure_device(ctx)) return rc;
  hipStream_t s = (hipStream_t)stream;
  launch_ppo_adv_part(ctx, advantages, valid, (size_t)m, row_index ? ppo_rows{row_index, rows_total} : kNoIndex, s);
  hipLaunchKernelGGL(pf::ppo_adv_sums_kernel, dim3(1), dim3(pf::kPpoBlock), 0, s, (const double*)(ctx->ppo_scratch + pf::kPpoAdvOffset), (int)pf::ppo_grid((size_t)m),
                     row_index ? 1 : 0, sums);
  return launched(ctx);
}
// what pf_adv_sums_add and pf_moments_merge check of their list of blocks of `words` doubles, and the kernels' copy of it
static int shard_src_check(pf_ctx* ctx, const char* who, const double* dst, const double* const src[], int n_src, size_t words, pf::ShardSrcK* K) {
  if (!ctx) return arg_fail(ctx, who, "ctx is required");
  const arg_ptr required[] = {{"dst", dst}, {"src", src}, {nullptr, nullptr}};
  if (int rc = require_args(ctx, who, required)) return rc;
  char buf[128];
  K->n_src = n_src;
  for (int g = 0; g < PF_PPO_MAX_SHARDS; ++g) {
    K->src[g] = g < n_src ? src[g] : nullptr;
    if (g >= n_src) continue;
    snprintf(buf, sizeof(buf), "src[%d]", g);
    if (!src[g]) {
      char what[64];
      snprintf(what, sizeof(what), "%s is required", buf);
      return arg_fail(ctx, who, what);
    }
    const arg_span spans[2] = {{buf, src[g], sizeof(double) * words}, {"dst", dst, sizeof(double) * words}};
    char msg[128];
    if (const char* e = spans_overlap(spans, 2, msg, sizeof(msg))) return arg_fail(ctx, who, e);
  }
  return PF_OK;
}
int pf_adv_sums_add(pf_ctx* ctx, double* dst, const double* const src[], int n_src, void* stream) {
  static const char* who = "pf_adv_sums_add";
  if (n_src < 1 || n_src > PF_PPO_MAX_SHARDS) return arg_fail(ctx, who, "n_src must be in 1..PF_PPO_MAX_SHARDS (16)");
  pf::ShardSrcK K;
  if (int rc = shard_src_check(ctx, who, dst, src, n_src, 4, &K)) return rc;
  if (int rc = ensure_device(ctx)) return rc;
  hipLaunchKernelGGL(pf::adv_sums_add_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, K, dst);
  return launched(ctx);
}
int pf_moments_merge(pf_ctx* ctx, double* dst, const double* const src[], int n_src, int D, void* stream) {
  static const char* who = "pf_moments_merge";
  if (n_src < 1 || n_src > PF_PPO_MAX_SHARDS) return arg_fail(ctx, who, "n_src must be in 1..PF_PPO_MAX_SHARDS (16)");
  if (D < 1 || D > pf::kTsMaxD) return arg_fail(ctx, who, "D must be in 1..128");
  pf::ShardSrcK K;
  if (int rc = shard_src_check(ctx, who, dst, src, n_src, 1 + 2 * (size_t)D, &K)) return rc;
  if (int rc = ensure_device(ctx)) return rc;
  hipLaunchKernelGGL(pf::moments_merge_kernel, dim3(1), dim3(pf::kTsMaxD), 0, (hipStream_t)stream, K, dst, D);
  return launched(ctx);
}
int pf_ppo_grad_shard(pf_ctx* ctx, const pf_ppo_grad_args* a, const pf_ppo_options* options, const int32_t* row_index, int64_t m, int64_t rows_total,
                      const double* adv_sums, double* shard_block, void* workspace, size_t workspace_bytes, void* stream) {
  static const char* who = "pf_ppo_grad_shard";
  if (int rc = rows_check(ctx, who, m, "m", "the kernels index slots with 32 bits")) return rc;
  if (row_index)
    if (int rc = rows_check(ctx, who, rows_total, "rows_total", "row_index holds 32-bit row numbers")) return rc;
  return ppo_grad_call(ctx, who, a, options, m, row_index ? ppo_rows{row_index, rows_total} : kNoIndex, workspace, workspace_bytes, stream, true,
                       ppo_shard{adv_sums, shard_block});
}
int pf_ppo_shard_combine(pf_ctx* ctx, const pf_ppo_shard_combine_args* a, void* stream) {
  static const char* who = "pf_ppo_shard_combine";
  if (a && (a->n_shards < 1 || a->n_shards > PF_PPO_MAX_SHARDS)) return arg_fail(ctx, who, "n_shards must be in 1..PF_PPO_MAX_SHARDS (16)");
  if (!ctx) return arg_fail(ctx, who, "ctx is required");
  if (!a) return arg_fail(ctx, who, "the argument block is required");
  if (a->numel < 1) return arg_fail(ctx, who, "numel must be >= 1");
  if (a->width < 1 || a->width > pf::kPpoMaxA) return arg_fail(ctx, who, "width must be in 1..8");
  // (clip and normalize_advantage are the shards' business: what the rows made of them is in the totals)
  if (int rc = ppo_coef_check(ctx, who, 1.0f, a->vf_coef, a->ent_coef, 0)) return rc;
  if (!(a->bounds_coef >= 0.0f && a->bounds_coef < INFINITY)) return arg_fail(ctx, who, "bounds_coef must be finite and >= 0");
  if ((a->vclip != 0 && a->vclip != 1) || (a->bnd != 0 && a->bnd != 1)) return arg_fail(ctx, who, "vclip and bnd must be 0 or 1");
  const size_t A = (size_t)a->width, G = (size_t)a->n_shards;
  arg_span spans[2 * PF_PPO_MAX_SHARDS + 5];
  char names[2 * PF_PPO_MAX_SHARDS][16];
  int ns = 0;
  for (size_t g = 0; g < G; ++g) {
    const void* const ptrs[2] = {a->blocks[g], a->grads[g]};
    for (int k = 0; k < 2; ++k) {
      snprintf(names[ns], sizeof(names[ns]), "%s[%d]", k ? "grads" : "blocks", (int)g);
      const arg_ptr one[] = {{names[ns], ptrs[k]}, {nullptr, nullptr}};
      if (int rc = require_args(ctx, who, one)) return rc;
      spans[ns] = {names[ns], ptrs[k], k ? sizeof(float) * (size_t)a->numel : sizeof(double) * PF_PPO_SHARD_WORDS};
      ++ns;
    }
  }
  const arg_ptr required[] = {{"adv_sums", a->adv_sums}, {"grad_out", a->grad_out}, {"log_std", a->log_std}, {"grad_log_std", a->grad_log_std},
                              {"stats", a->stats}, {nullptr, nullptr}};
  if (int rc = require_args(ctx, who, required)) return rc;
  spans[ns++] = {"adv_sums", a->adv_sums, sizeof(double) * 4};
  spans[ns++] = {"log_std", a->log_std, sizeof(float) * A};
  const int n_read = ns;
  spans[ns++] = {"grad_out", a->grad_out, sizeof(float) * (size_t)a->numel};
  spans[ns++] = {"grad_log_std", a->grad_log_std, sizeof(float) * A};
  spans[ns++] = {"stats", a->stats, sizeof(double) * 16};
  char buf[128];
  if (const char* e = spans_overlap(spans, ns, buf, sizeof(buf), n_read)) return arg_fail(ctx, who, e);
  if (int rc = ensure_device(ctx)) return rc;
  hipStream_t s = (hipStream_t)stream;
  pf::ShardSumK S;
  pf::ShardCombineK K;
  S.n_shards = K.n_shards = a->n_shards;
  for (size_t g = 0; g < PF_PPO_MAX_SHARDS; ++g) {
    S.grads[g] = g < G ? a->grads[g] : nullptr;
    K.blocks[g] = g < G ? a->blocks[g] : nullptr;
  }
  S.out = a->grad_out;
  K.width = a->width, K.vclip = a->vclip, K.bnd = a->bnd;
  K.vf_coef = a->vf_coef, K.ent_coef = a->ent_coef, K.bounds_coef = a->bounds_coef;
  K.adv_sums = a->adv_sums, K.log_std = a->log_std, K.grad_log_std = a->grad_log_std, K.stats = a->stats;
  const size_t blocks = ((size_t)a->numel + pf::kShardSumBlock - 1) / pf::kShardSumBlock;
  const unsigned grid = (unsigned)(blocks < (size_t)pf::kShardSumMaxGrid ? blocks : (size_t)pf::kShardSumMaxGrid);
  hipLaunchKernelGGL(pf::ppo_shard_sum_kernel, dim3(grid), dim3(pf::kShardSumBlock), 0, s, S, (size_t)a->numel);
  hipLaunchKernelGGL(pf::ppo_shard_combine_kernel, dim3(1), dim3(pf::kPpoBlock), 0, s, K);
  return launched(ctx);
}
size_t pf_adam_workspace_bytes(int64_t total_numel) {
  if (total_numel < 1 || total_numel > (int64_t)INT32_MAX) return 0;
  return sizeof(double) * (pf::adam_grid_bound(total_numel) + pf::kAdamHeader);
}
// what pf_adam_step refuses, or null; `buf` holds a composed message
static const char* adam_error(const pf_adam_args* a, const void* workspace, size_t workspace_bytes, char* buf, size_t len, bool gated = false,
                              const uint32_t* gate = nullptr) {
  if (!a) return "the argument block is required";
  if (gated && !gate) return "gate is required";
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
  arg_span spans[4 * PF_ADAM_MAX_TENSORS + 4];
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
  if (gated) spans[ns++] = {"gate", gate, sizeof(uint32_t)};
  return spans_overlap(spans, ns, buf, len);
}
// pf_adam_step (gated = false) and pf_adam_step_gated
static int adam_call(pf_ctx* ctx, const char* who, const pf_adam_args* a, bool gated, const uint32_t* gate, void* workspace, size_t workspace_bytes, void* stream) {
  if (!ctx) return arg_fail(ctx, who, "ctx is required");
  char buf[128];
  if (const char* e = adam_error(a, workspace, workspace_bytes, buf, sizeof(buf), gated, gate)) return arg_fail(ctx, who, e);
  if (int rc = ensure_device(ctx)) return rc;
  pf::AdamGatedK K;  // (the plain call passes the AdamK in it)
  K.gate = gate;
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
  const pf::AdamK& plain = K;
  hipLaunchKernelGGL(pf::adam_norm_kernel, dim3(grid), dim3(pf::kAdamBlock), 0, s, plain);
  if (gated)
    hipLaunchKernelGGL(pf::adam_update_kernel<pf::AdamGatedK>, dim3(grid), dim3(pf::kAdamBlock), 0, s, K);
  else
    hipLaunchKernelGGL(pf::adam_update_kernel<pf::AdamK>, dim3(grid), dim3(pf::kAdamBlock), 0, s, plain);
  return launched(ctx);
}
int pf_adam_step(pf_ctx* ctx, const pf_adam_args* a, void* workspace, size_t workspace_bytes, void* stream) {
  return adam_call(ctx, "pf_adam_step", a, false, nullptr, workspace, workspace_bytes, stream);
}
int pf_adam_step_gated(pf_ctx* ctx, const pf_adam_args* a, const uint32_t* gate, void* workspace, size_t workspace_bytes, void* stream) {
  return adam_call(ctx, "pf_adam_step_gated", a, true, gate, workspace, workspace_bytes, stream);
}
size_t pf_sizeof_kl_control(void) { return sizeof(pf_kl_control_args); }
int pf_kl_control(pf_ctx* ctx, const pf_kl_control_args* a, void* stream) {
  static const char* who = "pf_kl_control";
  if (!ctx) return arg_fail(ctx, who, "ctx is required");
  if (!a) return arg_fail(ctx, who, "the argument block is required");
  const arg_ptr required[] = {{"stats", a->stats}, {"gate", a->gate}, {"state", a->state}, {nullptr, nullptr}};
  if (int rc = require_args(ctx, who, required)) return rc;
  if (!(a->target_kl > 0.0f && a->target_kl < INFINITY)) return arg_fail(ctx, who, "target_kl must be finite and > 0");
  if (!(a->stop_factor >= 1.0f)) return arg_fail(ctx, who, "stop_factor must be >= 1 (+infinity: the gate never closes on a number)");
  if (a->adapt != 0 && a->adapt != 1) return arg_fail(ctx, who, "adapt must be 0 or 1");
  if (a->adapt) {
    if (!a->lr_dev) return arg_fail(ctx, who, "lr_dev is required with adapt = 1");
    if (!(a->lr_factor > 1.0f && a->lr_factor < INFINITY)) return arg_fail(ctx, who, "lr_factor must be finite and > 1");
    if (!(a->lr_low > 0.0f && a->lr_low < a->lr_high && a->lr_high < INFINITY)) return arg_fail(ctx, who, "lr_low and lr_high must be finite with 0 < lr_low < lr_high");
    if (!(a->lr_min > 0.0f && a->lr_min <= a->lr_max && a->lr_max < INFINITY)) return arg_fail(ctx, who, "lr_min and lr_max must be finite with 0 < lr_min <= lr_max");
  }
  arg_span spans[4];
  int ns = 0;
  spans[ns++] = {"stats", a->stats, sizeof(double) * 16};
  spans[ns++] = {"gate", a->gate, sizeof(uint32_t)};
  spans[ns++] = {"state", a->state, sizeof(double) * 4};
  if (a->lr_dev) spans[ns++] = {"lr_dev", a->lr_dev, sizeof(float)};
  char buf[128];
  if (const char* e = spans_overlap(spans, ns, buf, sizeof(buf))) return arg_fail(ctx, who, e);
  if (int rc = ensure_device(ctx)) return rc;
  const pf::KlControlK K{a->stats, a->target_kl, a->stop_factor, a->adapt, a->lr_factor, a->lr_low, a->lr_high, a->lr_min, a->lr_max, a->lr_dev, a->gate, a->state};
  hipLaunchKernelGGL(pf::kl_control_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, K);
  return launched(ctx);
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
  if (int rc = ensure_device(ctx)) return rc;
  hipStream_t s = (hipStream_t)stream;
  // (the new latch goes to the context's staging buffer and is copied over the caller's behind the kernel: world_sync.hpp)
  const pf::WorldSyncK K{a->terminated, a->truncated, a->reward, a->done, a->exclude, a->valid_out, a->reset_out, ctx->sync_latch};
  hipLaunchKernelGGL(pf::world_sync_kernel, dim3((ctx->n + pf::kWorldSyncBlock - 1) / pf::kWorldSyncBlock), dim3(pf::kWorldSyncBlock), 0, s, K, ctx->n,
                     agents_per_world);
  PF_HIP(ctx, hipGetLastError());
  PF_HIP(ctx, hipMemcpyAsync(a->done, ctx->sync_latch, (size_t)ctx->n, hipMemcpyDeviceToDevice, s));
  return PF_OK;
}
int pf_episode_outcomes(pf_ctx* ctx, const pf_outcome_args* a, int k_steps, int agents_per_world, void* stream) {
  static const char* who = "pf_episode_outcomes";
  if (int rc = traj_call_check(ctx, who, a, k_steps)) return rc;
  const arg_ptr required[] = {{"terminated", a->terminated}, {"truncated", a->truncated}, {"counts", a->counts}, {nullptr, nullptr}};
  if (int rc = require_args(ctx, who, required)) return rc;
  if (!a->info && k_steps != 1) return arg_fail(ctx, who, "info is required for k_steps > 1 (the live state holds the words of one step)");
  if (!a->info && !a->state) return arg_fail(ctx, who, "state (the context's state tensor) is required when info is NULL");
  if (a->n_groups < 1 || a->n_groups > PF_OUTCOME_MAX_GROUPS) return arg_fail(ctx, who, "n_groups must be in 1..PF_OUTCOME_MAX_GROUPS (16)");
  const int A = agents_per_world;
  if (A < 1 || A > pf::kWorldSyncMaxA) return arg_fail(ctx, who, "agents_per_world must be in 1..64");
  if (ctx->n % A != 0) return arg_fail(ctx, who, "agents_per_world must divide the context's lane count n");
  if (A > 1 && k_steps != 1) return arg_fail(ctx, who, "k_steps must be 1 with agents_per_world > 1 (the world form runs once per step)");
  if (A > 1 && !a->world_reset) return arg_fail(ctx, who, "world_reset (pf_world_sync's reset_out of this step) is required with agents_per_world > 1");
  if (A > 1 && !a->world_latch) return arg_fail(ctx, who, "world_latch is required with agents_per_world > 1");
  if (A == 1 && a->world_reset) return arg_fail(ctx, who, "world_reset must be NULL with agents_per_world == 1 (there are no worlds to tally)");
  if (int rc = ensure_device(ctx)) return rc;
  const pf_params& P = ctx->P;
  const bool dogfight = P.task == PF_TASK_DOGFIGHT;
  // the live words: the dogfight's side group 6 (bits word 3, received_hits word 2); elsewhere the int group (flags word 1, targets left word 3)
  const int g = dogfight ? 6 : (P.vehicle == PF_FIXEDWING ? 5 : 6), w0 = dogfight ? 3 : 1, w1 = dogfight ? 2 : 3;
  const int32_t* words = a->info ? nullptr : reinterpret_cast<const int32_t*>(a->state) + (size_t)g * (size_t)ctx->n * 4;
  const pf::OutcomeK K{a->terminated, a->truncated, a->valid, a->info, words ? words + w0 : nullptr, words ? words + w1 : nullptr, a->group,
                       a->world_reset, a->world_latch, a->outcome_out, reinterpret_cast<unsigned long long*>(a->counts), a->n_groups, dogfight ? 1 : 0,
                       P.task == PF_TASK_WAYPOINTS ? P.num_targets : 0, dogfight ? P.df_team_size : A};
  hipLaunchKernelGGL(pf::outcomes_kernel, dim3((ctx->n + pf::kOcBlock - 1) / pf::kOcBlock), dim3(pf::kOcBlock), 0, (hipStream_t)stream, K, ctx->n, k_steps, A);
  return launched(ctx);
}
}  // extern "C"
