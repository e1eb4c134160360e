// pf_episode_outcomes: why episodes end, counted per group, and who wins a world (include/pyflyt_amd.h states the contract).
// One thread per lane, 256 per workgroup. A lane walks its k steps with the loads of a window of steps issued before the window's
// first use (traj_stats.hpp: ts_scan_kernel), keeps its ten agent-level counts in registers, and adds what is not zero to the
// workgroup's block of PF_OUTCOME_MAX_GROUPS x PF_OUTCOME_SLOTS 64-bit sums in LDS; behind one barrier thread t adds entry t of that
// block to the caller's counts with one vector atomic, where it is not zero. Integer sums: the counts depend on no order.
//
// A non-ended lane's words are loaded and not selected: whatever they hold reaches nothing.
//
// The world form (A > 1, one step per call) and its latch. A lane that ends stores its byte in world_latch[i]; the first lane of a
// world whose reset mask is set reads the A latch bytes of its world and tallies the world. The two sets of lanes never share a byte
// within one launch: a lane stores only where world_reset[i] == 0, a first lane reads only the lanes of a world where
// world_reset[first] != 0, and pf_world_sync's mask is the same on every lane of a world (whole worlds). So nothing has to order the
// workgroups of a launch, whatever A is and wherever a world straddles a wavefront or a workgroup -- and no staging buffer is needed,
// unlike pf_world_sync's latch, which the whole world reads AND rewrites. (Under the protocol the guard never fires: every lane of a
// world that is being reset was latched before the step, and pf_world_sync blanked its flags.)
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/pyflyt_amd.h"
#include "dogfight.hpp"  // DF_INFO_*

namespace pf {

constexpr int kOcBlock = 256;
constexpr int kOcWin = 8;  // steps per window: four loads a step
static_assert(kOcBlock == PF_OUTCOME_MAX_GROUPS * PF_OUTCOME_SLOTS, "thread t flushes entry t of the workgroup's block");

struct OutcomeK {
  const uint8_t* terminated;
  const uint8_t* truncated;
  const uint8_t* valid;      // or null
  const int32_t* info;       // [k][n][2], or null = the live words
  const int32_t* live0;      // info == null: lane i's word0 at live0[4 i], its word1 at live1[4 i] (words of one state group)
  const int32_t* live1;
  const int32_t* group;      // or null
  const uint8_t* world_reset;  // A > 1
  uint8_t* world_latch;        // A > 1
  uint8_t* outcome_out;      // or null
  unsigned long long* counts;
  int32_t n_groups;
  int32_t dogfight;     // the words are the dogfight's (bits, received_hits)
  int32_t num_targets;  // waypoint tasks: slot 8 adds num_targets - word1; 0 = slot 8 adds nothing (dogfight: word1 itself)
  int32_t team_size;    // dogfight: lanes [0, team_size) of a world are team 0
};

// the byte of an episode that ended with `w0` as its first word
__device__ __forceinline__ uint32_t oc_byte(uint32_t w0, bool term, bool dogfight) {
  const uint32_t cause = dogfight ? (((w0 & DF_INFO_COLLISION) ? PF_OC_COLLISION : 0u) | ((w0 & DF_INFO_OOB) ? PF_OC_OOB : 0u) |
                                     ((w0 & DF_INFO_TEAM_WIN) ? PF_OC_COMPLETE : 0u) | ((w0 & DF_INFO_DEAD) ? PF_OC_DEAD : 0u))
                                  : (((w0 & PF_F_INFO_COLLISION) ? PF_OC_COLLISION : 0u) | ((w0 & PF_F_INFO_OOB) ? PF_OC_OOB : 0u) |
                                     ((w0 & PF_F_INFO_COMPLETE) ? PF_OC_COMPLETE : 0u) | ((w0 & PF_F_NONFINITE) ? PF_OC_NONFINITE : 0u));
  return PF_OC_ENDED | (term ? PF_OC_TERMINATED : 0u) | cause;
}

__global__ __launch_bounds__(kOcBlock) void outcomes_kernel(const OutcomeK a, const int n_lanes, const int k, const int A) {
  __shared__ unsigned long long part[kOcBlock];
  part[threadIdx.x] = 0ull;
  __syncthreads();
  const size_t n = (size_t)n_lanes;
  const size_t lane = (size_t)blockIdx.x * kOcBlock + threadIdx.x;
  const bool live = lane < n;
  const size_t i = live ? lane : n - 1;  // (the threads past n read lane n - 1 and select nothing: they stay for the barrier)
  const int32_t g = a.group ? a.group[i] : 0;
  const bool grouped = live && g >= 0 && g < a.n_groups;  // (a lane whose group is out of range enters no count)
  const bool dogfight = a.dogfight != 0;
  // (no valid: the byte loads read `terminated` again and vall makes every step count -- one load either way, as in ppo_loss.hpp)
  const uint8_t* vbytes = a.valid ? a.valid : a.terminated;
  const uint32_t vall = a.valid ? 0u : 1u;
  const bool has_info = a.info != nullptr;
  uint32_t c[10] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
  long long sum8 = 0;
  uint32_t last = 0u;  // the byte of the last step: what the world form latches (k == 1 there)
  for (int s0 = 0; s0 < k; s0 += kOcWin) {  // (nothing of a window is carried round the loop)
    uint32_t te[kOcWin], tr[kOcWin], vb[kOcWin];
    int32_t w0[kOcWin], w1[kOcWin];
#pragma unroll
    for (int j = 0; j < kOcWin; ++j) {  // every load of the window; the slots past step k - 1 read row k - 1 again and are skipped below
      const int s = s0 + j < k ? s0 + j : k - 1;
      const size_t o = (size_t)s * n + i;
      te[j] = a.terminated[o];
      tr[j] = a.truncated[o];
      vb[j] = vbytes[o] | vall;
      w0[j] = *(has_info ? a.info + 2 * o : a.live0 + 4 * i);  // (the address is selected, the load is one: no branch inside the window)
      w1[j] = *(has_info ? a.info + 2 * o + 1 : a.live1 + 4 * i);
    }
#pragma unroll
    for (int j = 0; j < kOcWin; ++j) {
      if (s0 + j < k) {  // (uniform)
        const bool term = te[j] != 0;
        const bool ended = term || tr[j] != 0;
        const uint32_t b = ended ? oc_byte((uint32_t)w0[j], term, dogfight) : 0u;
        if (live && a.outcome_out) a.outcome_out[(size_t)(s0 + j) * n + i] = (uint8_t)b;
        last = b;
        const uint32_t m = (grouped && vb[j] != 0) ? b : 0u;  // the byte where it counts, 0 elsewhere
        c[0] += m & PF_OC_ENDED;
        c[1] += (m >> 1) & 1u;
        c[2] += (m & PF_OC_ENDED) & ~(m >> 1);
        c[3] += (m >> 2) & 1u;
        c[4] += (m >> 3) & 1u;
        c[5] += (m >> 4) & 1u;
        c[6] += (m >> 5) & 1u;
        c[7] += (m >> 6) & 1u;
        c[9] += (m != 0u && (m & (PF_OC_COLLISION | PF_OC_OOB | PF_OC_COMPLETE | PF_OC_DEAD | PF_OC_NONFINITE)) == 0u) ? 1u : 0u;
        const int32_t second = dogfight ? w1[j] : (a.num_targets > 0 ? a.num_targets - w1[j] : 0);
        sum8 += m != 0u ? (long long)second : 0ll;
      }
    }
  }
  if (c[0] != 0u) {  // (every count is zero where no counted episode ended)
    unsigned long long* row = part + g * PF_OUTCOME_SLOTS;
#pragma unroll
    for (int q = 0; q < 10; ++q) {
      const unsigned long long v = q == 8 ? (unsigned long long)sum8 : (unsigned long long)c[q];
      if (v != 0ull) atomicAdd(row + q, v);
    }
  }
  if (A > 1 && live) {
    const bool resetting = a.world_reset[i] != 0;
    if (last != 0u && !resetting) a.world_latch[i] = (uint8_t)last;
    if (resetting && lane % (size_t)A == 0 && grouped) {  // the world that finished before this step (n % A == 0: i + A <= n)
      uint32_t won0 = 0u, won1 = 0u;
      for (int j = 0; j < A; ++j) {
        const uint32_t complete = (a.world_latch[i + j] & PF_OC_COMPLETE) ? 1u : 0u;
        won0 |= j < a.team_size ? complete : 0u;
        won1 |= j < a.team_size ? 0u : complete;
      }
      unsigned long long* row = part + g * PF_OUTCOME_SLOTS;
      atomicAdd(row + 10, 1ull);
      if (dogfight) atomicAdd(row + (won0 != won1 ? (won0 ? 11 : 12) : 13), 1ull);
    }
  }
  __syncthreads();
  const unsigned long long v = part[threadIdx.x];
  if (v != 0ull && (int)threadIdx.x < a.n_groups * PF_OUTCOME_SLOTS) atomicAdd(a.counts + threadIdx.x, v);
}

}  // namespace pf
