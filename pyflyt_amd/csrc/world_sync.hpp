// pf_world_sync: the world-level auto-reset of the multi-agent envs, between two env steps (include/pyflyt_amd.h states the rules).
// One thread per lane; a world is A adjacent lanes, lane = world * A + agent, and A need not divide the wavefront or the workgroup
// (a 3 v 3 dogfight has worlds of six: at 256 threads per workgroup every 128th world straddles two of them). So every thread reads
// the A latch bytes of its world itself, with plain byte loads -- no ballot, no LDS, nothing that assumes where a world begins.
//
// The latch is read by the whole world and rewritten, and nothing orders the workgroups of a launch: a lane that stored its new latch
// byte in place could be read, as the OLD one, by a lane of its world in a workgroup that runs later. The kernel therefore never
// writes the latch it reads. It writes the new bytes to `done_next`, a staging buffer of n bytes that the context owns
// (pf_ctx.sync_latch), and pf_world_sync copies the staging buffer over the caller's latch behind the kernel, on the same stream:
// one latch in and out for the caller, read-then-write across workgroups by construction. The rows (terminated, truncated, reward)
// are another matter: lane i's entries are read and written by lane i's thread alone, in that order.
//
// Selections are selects: the reward of a latched lane is loaded and not chosen, so a NaN in it reaches nothing.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace pf {

constexpr int kWorldSyncBlock = 256;
constexpr int kWorldSyncMaxA = 64;

struct WorldSyncK {
  uint8_t* terminated;
  uint8_t* truncated;
  float* reward;
  const uint8_t* done;     // the caller's latch: read only
  const uint8_t* exclude;  // or null
  uint8_t* valid_out;
  uint8_t* reset_out;
  uint8_t* done_next;      // the context's staging buffer: the new latch
};

__global__ __launch_bounds__(kWorldSyncBlock) void world_sync_kernel(const WorldSyncK a, const int n, const int A) {
  const int i = blockIdx.x * kWorldSyncBlock + threadIdx.x;
  if (i >= n) return;
  const int base = (i / A) * A;  // (n % A == 0, checked by the caller: base + A <= n)
  uint32_t waiting = 1u;
  for (int j = 0; j < A; ++j) waiting &= a.done[base + j] != 0 ? 1u : 0u;
  const bool was = a.done[i] != 0;
  const uint32_t te = a.terminated[i], tr = a.truncated[i];
  const float r = a.reward[i];
  const bool excluded = a.exclude != nullptr && a.exclude[i] != 0;
  const bool ended = !was && (te | tr) != 0;
  a.valid_out[i] = (!was && !excluded) ? 1 : 0;
  a.reward[i] = was ? 0.0f : r;
  a.terminated[i] = was ? 0 : (uint8_t)te;
  a.truncated[i] = was ? 0 : (uint8_t)tr;
  a.done_next[i] = waiting ? 0 : ((was || ended) ? 1 : 0);
  a.reset_out[i] = (uint8_t)waiting;
}

}  // namespace pf
