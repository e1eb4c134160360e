// pyflyt_amd.hip -- kernels + C ABI (include/pyflyt_amd.h) of the MI355X-native batched UAV step.
//
// The library's one translation unit: the build takes the device assembly of this file, and all of its code is in the headers next
// to it ("The files of csrc/"). Kernels have a header per family, the ABI's host code has three:
//   uav_device.hpp, uav_vehicles.hpp, quadx_control_d.hpp, shared_world.hpp, rocket.hpp   math, vehicles, the body tick, contacts
//   env_generic.hpp (its head: the execution model), quadx_fast.hpp, fixedwing_fast.hpp, dogfight.hpp, rocket_landing.hpp   the env kernels
//   aviary_kernels.hpp                                         pf_aviary_*, pf_body_tick, pf_sample_actions
//   policy_mlp.hpp, mlp_tile.hpp, policy_act.hpp, mlp.hpp      the policy network: inside a rollout, as a launch, its backward pass
//   policy_act_pool.hpp                                        the same launch for a pool of policies, rows sorted by policy
//   gae.hpp, traj_stats.hpp, ppo_loss.hpp, ppo_grad.hpp, ppo_shard.hpp, adam.hpp, world_sync.hpp, outcomes.hpp   the training operations
//   abi_ctx.hpp     pf_ctx, the refusals, the argument tables, the current device, the per-lane launch
//   abi_env.hpp     the choice of the env kernel and its launch, pf_ctx_create / destroy and the queries, pf_env_*, pf_aviary_*, pf_rollout*
//   abi_train.hpp   pf_policy_act, pf_gae, pf_traj_stats, pf_traj_stats_masked, pf_ppo_loss, pf_mlp_*, pf_ppo_grad, the sharded PPO calls, pf_adam_step, pf_world_sync, pf_episode_outcomes
//   abi_pool.hpp    pf_policy_pool_plan_bytes, pf_policy_pool_plan, pf_policy_act_pool
// Every header includes what it uses, so the order below is only the order of reading.
#include "abi_ctx.hpp"
#include "abi_env.hpp"
#include "abi_train.hpp"
#include "abi_pool.hpp"
