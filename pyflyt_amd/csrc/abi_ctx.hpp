// abi_ctx.hpp -- the C ABI's context (pf_ctx) and what the entry points in abi_env.hpp and abi_train.hpp share: refusals, argument
// tables, the current device, the launch with one lane per drone. Host code, part of the one translation unit pyflyt_amd.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>
#include <cstdio>

#include "../../include/pyflyt_amd.h"
#include "quadx_fast.hpp"      // QuadK
#include "fixedwing_fast.hpp"  // FwK, FwTable
#include "env_generic.hpp"     // kWave

// The env kernel a context runs, chosen once at pf_ctx_create (abi_env.hpp: select_env_kernel).
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

// Created value-initialised (every pointer null), freed by pf_ctx_destroy alone: a new device buffer is a member here and a line in each.
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

// a refusal with the text "<who>: <what>"; arg_fail: the usual code
static int who_fail(pf_ctx* ctx, int code, const char* who, const char* what) {
  char buf[256];
  snprintf(buf, sizeof(buf), "%s: %s", who, what);
  return fail(ctx, code, buf);
}
static int arg_fail(pf_ctx* ctx, const char* who, const char* what) { return who_fail(ctx, PF_ERR_ARG, who, what); }
// a call's required pointers, a table that ends with a null name: the first missing one is refused as "<who>: <name> is required"
struct arg_ptr { const char* name; const void* p; };
static int require_args(pf_ctx* ctx, const char* who, const arg_ptr* args) {
  for (; args->name; ++args)
    if (!args->p) {
      char what[64];
      snprintf(what, sizeof(what), "%s is required", args->name);
      return arg_fail(ctx, who, what);
    }
  return PF_OK;
}
struct arg_span { const char* name; const void* p; size_t bytes; };
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

// pf_ctx_create's allocations: `device` is current inside the scope, the caller's own device again behind it.
struct device_scope {
  int saved = -1;
  explicit device_scope(int device) { (void)hipGetDevice(&saved), (void)hipSetDevice(device); }
  ~device_scope() { if (saved >= 0) (void)hipSetDevice(saved); }
};
// Every other entry point: the context's device is made current and stays current.
static int ensure_device(pf_ctx* ctx) {
  int cur = -1;
  PF_HIP(ctx, hipGetDevice(&cur));
  if (cur != ctx->device) PF_HIP(ctx, hipSetDevice(ctx->device));
  return PF_OK;
}

// behind a call's launches: the error of the first that failed, if any
static int launched(pf_ctx* ctx) {
  PF_HIP(ctx, hipGetLastError());
  return PF_OK;
}
// The instantiation of a per-vehicle kernel for the context's vehicle. Each call passes those of the vehicles it admits (none for
// the Rocket where the call or pf_ctx_create refuses it).
template <class KERNEL>
static KERNEL vehicle_kernel(const pf_ctx* ctx, KERNEL quadx, KERNEL fixedwing, KERNEL rocket = nullptr) {
  return ctx->P.vehicle == PF_QUADX ? quadx : (ctx->P.vehicle == PF_ROCKET && rocket) ? rocket : fixedwing;
}
// One launch with a lane per drone (aviary_kernels.hpp), a wavefront per workgroup: kernel(ctx->P, *b, ctx->n, rest...) on the caller's stream.
template <class KERNEL, class... REST>
static int launch_per_lane(pf_ctx* ctx, const pf_buffers* b, void* stream, KERNEL kernel, REST... rest) {
  if (int rc = ensure_device(ctx)) return rc;
  hipLaunchKernelGGL(kernel, dim3((ctx->n + pf::kWave - 1) / pf::kWave), dim3(pf::kWave), 0, (hipStream_t)stream, ctx->P, *b, ctx->n, rest...);
  return launched(ctx);
}
