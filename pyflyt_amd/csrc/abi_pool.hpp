// abi_pool.hpp -- pf_policy_pool_plan_bytes, pf_policy_pool_plan and pf_policy_act_pool: pf_policy_act for a pool of policies in one
// launch (policy_act_pool.hpp has the plan's layout and the kernels). Host code.
#pragma once
#include "abi_ctx.hpp"  // (with the HIP runtime)
#include "abi_train.hpp"  // env_action_dim
#include "policy_act_pool.hpp"

// what both calls refuse first, in this order
static int policy_pool_check(pf_ctx* ctx, const char* who, int n_policies, const void* plan, size_t plan_bytes) {
  if (ctx->P.task == PF_TASK_NONE) return who_fail(ctx, PF_ERR_UNSUPPORTED, who, "needs a context with an env task (this one drives the Aviary level only)");
  if (ctx->n > pf::kPoolMaxRows) return who_fail(ctx, PF_ERR_UNSUPPORTED, who, "more rows than a plan's 32-bit slot indices admit");
  if (n_policies < 1 || n_policies > PF_POLICY_POOL_MAX) return arg_fail(ctx, who, "n_policies must be in 1..PF_POLICY_POOL_MAX (17)");
  if (!plan) return arg_fail(ctx, who, "plan is required");
  if (plan_bytes != pf_policy_pool_plan_bytes(ctx->n, n_policies)) return arg_fail(ctx, who, "plan_bytes must be pf_policy_pool_plan_bytes(pf_n_lanes(ctx), n_policies)");
  return PF_OK;
}

extern "C" {
size_t pf_policy_pool_plan_bytes(int n_rows, int n_policies) {
  if (n_rows < 1 || n_policies < 1 || n_policies > PF_POLICY_POOL_MAX) return 0;
  return (size_t)pf::pool_plan_tiles(n_rows, n_policies) * (size_t)(pf::kActRows + 1) * sizeof(int32_t);
}
int pf_policy_pool_plan(pf_ctx* ctx, const int32_t* row_policy, int n_policies, void* plan, size_t plan_bytes, void* stream) {
  static const char* who = "pf_policy_pool_plan";
  if (!ctx) return arg_fail(ctx, who, "ctx is required");
  if (!row_policy) return arg_fail(ctx, who, "row_policy is required");
  if (int rc = policy_pool_check(ctx, who, n_policies, plan, plan_bytes)) return rc;
  if (int rc = ensure_device(ctx)) return rc;
  hipLaunchKernelGGL(pf::policy_pool_plan_kernel, dim3(1), dim3(64 * pf::kPoolPlanWaves), 0, (hipStream_t)stream, row_policy, ctx->n, n_policies,
                     (int32_t*)plan, pf::pool_plan_tiles(ctx->n, n_policies));
  return launched(ctx);
}
int pf_policy_act_pool(pf_ctx* ctx, const pf_policy* policies, int n_policies, const void* plan, size_t plan_bytes, float* actions_out,
                       uint32_t step_index, void* stream) {
  static const char* who = "pf_policy_act_pool";
  if (!ctx) return arg_fail(ctx, who, "ctx is required");
  if (!policies) return arg_fail(ctx, who, "policies is required");
  if (int rc = policy_pool_check(ctx, who, n_policies, plan, plan_bytes)) return rc;
  const pf_params& P = ctx->P;
  if (!actions_out) return arg_fail(ctx, who, "actions_out is required");
  if (!policies[0].obs0) return arg_fail(ctx, who, "policies[0].obs0 (the [n][pf_obs_dim()] input rows) is required");
  for (int p = 0; p < n_policies; ++p) {
    char entry[48];
    snprintf(entry, sizeof(entry), "%s: policies[%d]", who, p);
    if (int rc = policy_net_check(ctx, entry, &policies[p])) return rc;
  }
  const int D = pf_obs_dim(ctx);
  if (D > pf::kActMaxIn) return who_fail(ctx, PF_ERR_UNSUPPORTED, who, "observation wider than 128");
  if (int rc = ensure_device(ctx)) return rc;
  pf::ActPoolK AK;
  for (int p = 0; p < pf::kPoolMax; ++p) AK.Q[p] = policies[p < n_policies ? p : 0];
  AK.obs = policies[0].obs0, AK.mean_out = policies[0].mean_out, AK.actions_out = actions_out, AK.plan = (const int32_t*)plan;
  AK.n = ctx->n, AK.D = D, AK.A = env_action_dim(P), AK.P = n_policies, AK.T = pf::pool_plan_tiles(ctx->n, n_policies);
  AK.seed_lo = (uint32_t)P.seed, AK.seed_hi = (uint32_t)(P.seed >> 32), AK.step = step_index, AK.lane0 = ctx->lane0;
  // a contiguous range of tiles per workgroup, two workgroups per CU at the most (pf_policy_act's cap: the same registers and LDS)
  const int grid = AK.T < ctx->act_grid_cap ? AK.T : ctx->act_grid_cap;
  hipLaunchKernelGGL(pf::policy_act_pool_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, AK);
  return launched(ctx);
}
}
