// pf_ppo_grad: the parameter gradients of a PPO epoch from x, without a mean, value, grad_mean or grad_value tensor (include/pyflyt_amd.h
// states the semantics: those of pf_mlp_forward x 2 -> pf_ppo_loss -> pf_mlp_backward x 2). Seven launches in one call:
//
//   ppo_adv_kernel, ppo_adv_finish_kernel   ppo_loss.hpp's, as they are, into the context's block: c, mu, sigma depend on no network output.
//   mlp_backward_kernel<PpoGradK<ACTOR>>    mlp.hpp's tile loop with its step 2 (load the rows of grad_out into G) replaced by a head:
//   mlp_backward_kernel<PpoGradK<CRITIC>>     2'. with h_last in LDS, the output layer by policy_act_kernel's code (mlp_tile.hpp: tile_out_pair; lane = row,
//                                                 wave w the outputs 2 w and 2 w + 1) -> G holds the tile's means (the critic: its values in column 0);
//                                                 wave 0, lane = row, runs ppo_main_kernel's float32 sequence for its row (ppo_loss.hpp: ppo_actor_row /
//                                                 ppo_critic_row) on G's row and the row's data, and writes grad_mean's row (the critic: grad_value in
//                                                 column 0) over it, columns from out_dim on as zeros; invalid rows and rows past `rows` are zeros by selection.
//                                               The row data (the actor: actions, logp_old, advantage, validity byte; the critic: return, validity byte) is
//                                               loaded a tile ahead like x and goes through LDS. Steps 3 - 6, the running sums and the block of partials are
//                                               the one text of mlp.hpp. The terms of `stats` and grad_log_std stay in wave 0's lanes in double over the
//                                               workgroup's tiles; at the end one butterfly over the wave (traj_stats.hpp) and one row of kPpoStride doubles per
//                                               workgroup: the actor's launch writes the columns ppo_main_kernel fills from the means, the critic's the other four.
//   mlp_reduce_kernel x 2                   mlp.hpp's, one per network.
//   ppo_finish_kernel                       ppo_loss.hpp's, over the mlp_grid(rows) rows of partials.
//
// pf_ppo_grad_rows is the same seven launches on the m rows an index list names: ppo_adv_rows_kernel, ppo_adv_finish_kernel as it is,
// mlp_backward_kernel<PpoGradRowsK<head, options>> (mlp.hpp: how the indices travel a tile ahead of the rows), the two reductions and
// ppo_finish_rows_kernel. A slot is the same lane of the same tile of the same workgroup as the row of a contiguous call, so every sum
// has that call's bits.
//
// So the order of the double sums behind stats and grad_log_std differs from pf_ppo_loss's (a lane's rows are 64 apart in a tile and the
// workgroup's tiles gridDim apart; at most 256 rows of partials instead of 1024) and nothing else does. LDS: the backward's 120 576 bytes
// plus 3 200 for the head, under gfx950's 160 KB with one network staged: a launch per network. No atomics; the grid is mlp_grid(rows).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <type_traits>

#include "../../include/pyflyt_amd.h"
#include "uav_device.hpp"
#include "mlp_tile.hpp"
#include "ppo_loss.hpp"  // the per-row terms of the loss
#include "mlp.hpp"  // mlp_backward_kernel, which these heads instantiate

namespace pf {

constexpr int kGradActor = 1, kGradCritic = 2;
// a head's LDS in floats: the tile's actions [64][kMlpGS], three per-row words [3][64], then what a call fixes: the output bias [8],
// log_std [8], exp(-log_std) [8] (0 and 1 from A on), and w32, mu32, inv32 as ppo_main_kernel takes them from the advantage block
constexpr int kGradLdsAct = 0, kGradLdsRow = kActRows * kMlpGS, kGradLdsBias = kGradLdsRow + 3 * kActRows, kGradLdsStd = kGradLdsBias + kActMaxA;
constexpr int kGradLdsInv = kGradLdsStd + kPpoMaxA, kGradLdsFin = kGradLdsInv + kPpoMaxA, kGradLdsFloats = kGradLdsFin + 8;

struct PpoGradRows {
  float a[2];     // the actor: two elements of the tile's actions, as load_g takes grad_out's
  float p, q;     // the actor: logp_old and the advantage of row `lane`; the critic: p = the return
  uint32_t b;     // the row's validity byte
};
struct PpoGradSums {
  double s[4] = {0.0, 0.0, 0.0, 0.0};  // the actor: sum min(u, v), sum (r - 1) - d; the critic: sum (V - R)^2, sum R, sum R^2, sum (V - R)
  double gls[kPpoMaxA] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  uint32_t n_clip = 0;
  float r_lo = INFINITY, r_hi = -INFINITY;
};

// the options' sums (pf_ppo_grad_opt): the critic: o[0] the sum of the chosen squared value error, n_out the rows outside the clip
// range; the actor: o[0] = sum b
struct PpoGradOptSums : PpoGradSums {
  double o[1] = {0.0};
  uint32_t n_out = 0;
};
template <bool OPT>
struct PpoGradOpt {};  // (an empty base: a head without options has the arguments it always had)
template <>
struct PpoGradOpt<true> {
  PpoOptK o;
};

// what a head of pf_ppo_grad_rows adds: the index list [n] and the rows of the batch it points into
template <bool IDX>
struct PpoGradIdx {};
template <>
struct PpoGradIdx<true> {
  const int32_t* row_index;
  uint32_t rows_total;
};
constexpr uint32_t kGradBadSlot = 0x100u;  // set in a slot's validity word (a byte otherwise) where its index lay outside the batch

// OPT: the heads of pf_ppo_grad_opt, instantiations of their own (PpoGradOptK below); PpoGradK is the head without.
// IDX: the heads of pf_ppo_grad_rows (PpoGradRowsK below): slot j of the n is row row_index[j] of every per-row tensor
template <int HEAD, bool OPT, bool IDX = false>
struct PpoGradHead : MlpK, PpoGradOpt<OPT>, PpoGradIdx<IDX> {
  static constexpr int kHead = HEAD;
  static constexpr bool kIndexed = IDX;
  static constexpr int kLdsFloats = kGradLdsFloats;
  typedef PpoGradRows Rows;
  typedef std::conditional_t<OPT, PpoGradOptSums, PpoGradSums> Sums;
  float clip, vf_coef;
  int32_t normalize;
  const float* log_std;
  const float* actions;
  const float* logp_old;
  const float* advantages;
  const float* returns;
  const uint8_t* vbytes;  // `valid`, or any M readable bytes with vmask 0 where the caller gave none
  uint32_t vmask;
  const double* fin;      // ppo_adv_finish_kernel's block
  double* stat_part;      // [grid][kPpoStride]

  // what the call fixes, once per workgroup
  PF_DEV void stage_head(const int t, float* HS) const {
    const float* bo = Q.b[Q.n_layers - 1];
    if (t < kActMaxA) {
      HS[kGradLdsBias + t] = t < Q.out_dim ? bo[t] : 0.0f;
      if constexpr (HEAD == kGradActor) {
        const float l = t < Q.out_dim ? log_std[t] : 0.0f;
        HS[kGradLdsStd + t] = l;
        HS[kGradLdsInv + t] = expf(-l);
      }
    }
    if (t == 64) {
      const double cnt = fin[0];
      HS[kGradLdsFin] = cnt > 0.0 ? (float)(1.0 / cnt) : 0.0f;
      HS[kGradLdsFin + 1] = (float)fin[3];
      HS[kGradLdsFin + 2] = (float)fin[4];
    }
  }
  // a tile's row data: the rows past n re-read row n - 1 and are selected away; the actions past n and past A are zeros, never read
  PF_DEV void load_rows(const int tile, const int t, Rows& r) const {
    const int A = Q.out_dim;
    if constexpr (HEAD == kGradActor) {
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int idx = t + 256 * u, row = idx / kActMaxA, c = idx % kActMaxA;
        const int gr = tile * kActRows + row;
        r.a[u] = (gr < n && c < A) ? actions[(size_t)gr * A + c] : 0.0f;
      }
    }
    if (t < kActRows) {
      const size_t g = (size_t)min(tile * kActRows + t, n - 1);
      if constexpr (HEAD == kGradActor) {
        r.p = logp_old[g];
        r.q = advantages[g];
      } else {
        r.p = returns[g];
        if constexpr (OPT) r.q = this->o.values_old[g];  // (the critic's free word of the row block)
      }
      r.b = vbytes[g];
    }
  }
  // the index list's number of slot `lane` of a tile as it stands in memory (slots past n: slot n - 1's), and what the kernel makes of
  // it once it has arrived: the row, or -1 for a number outside [0, rows_total)
  PF_DEV int load_index(const int tile, const int lane) const { return this->row_index[min(tile * kActRows + lane, n - 1)]; }
  PF_DEV int row_of(const int raw) const { return (uint32_t)raw < this->rows_total ? raw : -1; }
  // load_rows through the index: `s` = row_of() of the tile's 64 slots, lane = slot, in every wave. A slot outside the batch loads row 0
  // and carries kGradBadSlot in its validity word: nothing of it is chosen (make_g)
  PF_DEV void load_rows(const int tile, const int t, const int s, Rows& r) const {
    const int A = Q.out_dim;
    if constexpr (HEAD == kGradActor) {
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int idx = t + 256 * u, row = idx / kActMaxA, c = idx % kActMaxA;
        const int g = __shfl(s, row);
        r.a[u] = (tile * kActRows + row < n && g >= 0 && c < A) ? actions[(size_t)g * A + c] : 0.0f;
      }
    }
    if (t < kActRows) {
      const size_t g = (size_t)max(s, 0);
      if constexpr (HEAD == kGradActor) {
        r.p = logp_old[g];
        r.q = advantages[g];
      } else {
        r.p = returns[g];
        if constexpr (OPT) r.q = this->o.values_old[g];
      }
      r.b = (uint32_t)vbytes[g] | (s < 0 ? kGradBadSlot : 0u);
    }
  }
  PF_DEV void stage_rows(const int t, const Rows& r, float* HS) const {
    if constexpr (HEAD == kGradActor) {
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int idx = t + 256 * u;
        HS[kGradLdsAct + (idx / kActMaxA) * kMlpGS + idx % kActMaxA] = r.a[u];
      }
    }
    if (t < kActRows) {
      HS[kGradLdsRow + t] = r.p;
      if constexpr (HEAD == kGradActor || OPT) HS[kGradLdsRow + kActRows + t] = r.q;
      HS[kGradLdsRow + 2 * kActRows + t] = __uint_as_float(r.b);
    }
  }
  // step 2' of a tile; every thread of the workgroup arrives with h_last complete in TL and leaves with G complete
  PF_DEV void make_g(const int tile, const int t, const float* TL, const float* WOs, const float* HS, float* G, Sums& S) const {
    const int lane = t & 63, wv = t >> 6, A = Q.out_dim, ca = 2 * wv;
    if (ca < A) {
      float m0 = HS[kGradLdsBias + ca], m1 = HS[kGradLdsBias + ca + 1];
      tile_out_pair(WOs, TL + lane * kActTS, ca, m0, m1);
      G[lane * kMlpGS + ca] = m0;
      G[lane * kMlpGS + ca + 1] = m1;
    }
    if (A > 2) act_barrier();  // (up to two outputs are wave 0's own: each of its lanes reads back what it wrote)
    if (wv == 0) {
      const float w32 = HS[kGradLdsFin];
      const uint32_t all = vmask == 0u ? 1u : 0u;
      bool live = tile * kActRows + lane < n && ((__float_as_uint(HS[kGradLdsRow + 2 * kActRows + lane]) & vmask) | all) != 0u;
      if constexpr (IDX) live = live && (__float_as_uint(HS[kGradLdsRow + 2 * kActRows + lane]) & kGradBadSlot) == 0u;
      float* g = G + lane * kMlpGS;
      if constexpr (HEAD == kGradActor) {
        const float cf[5] = {1.0f - clip, 1.0f + clip, w32, HS[kGradLdsFin + 1], HS[kGradLdsFin + 2]};
        float m[kPpoMaxA], x[kPpoMaxA], ls[kPpoMaxA], inv[kPpoMaxA], gm[kPpoMaxA], gt[kPpoMaxA], surr, r, d;
#pragma unroll
        for (int c = 0; c < kPpoMaxA; ++c) {
          m[c] = g[c];
          x[c] = HS[kGradLdsAct + lane * kMlpGS + c];
          ls[c] = HS[kGradLdsStd + c];
          inv[c] = HS[kGradLdsInv + c];
        }
        ppo_actor_row<kPpoMaxA>(m, x, ls, inv, A, HS[kGradLdsRow + lane], HS[kGradLdsRow + kActRows + lane], live, normalize != 0, cf, gm, gt, surr, r, d);
        if constexpr (OPT) {
          const PpoOptK& o = this->o;
          S.o[0] = S.o[0] + (double)ppo_bounds_row<kPpoMaxA>(m, A, live && o.bnd != 0, (2.0f * o.bounds_coef) * w32, o.lo, o.hi, gm);
        }
#pragma unroll
        for (int c = 0; c < kPpoMaxA; ++c) {
          g[c] = gm[c];
          S.gls[c] = S.gls[c] + (double)gt[c];
        }
        ppo_actor_terms(live, surr, r, d, clip, S.s[0], S.s[1], S.n_clip, S.r_lo, S.r_hi);
      } else {
        float gv = ppo_critic_row(g[0], HS[kGradLdsRow + lane], vf_coef * w32, live, S.s[0], S.s[1], S.s[2], S.s[3]);
        if constexpr (OPT) {
          const PpoOptK& o = this->o;
          gv = ppo_vclip_row(gv, g[0], HS[kGradLdsRow + lane], HS[kGradLdsRow + kActRows + lane], o.clip_vf, live && o.vclip != 0, S.o[0], S.n_out);
        }
        g[0] = gv;
#pragma unroll
        for (int c = 1; c < kActMaxA; ++c) g[c] = 0.0f;
      }
    }
    act_barrier();
  }
  // wave 0's sums over its 64 lanes -> this head's columns of the workgroup's row of partials (lane j writes column j)
  PF_DEV void write_sums(const int t, const Sums& S) const {
    if (t >= 64) return;
    constexpr int QN = OPT ? kPpoStride : kPpoQ;
    double q[QN];
#pragma unroll
    for (int j = 0; j < QN; ++j) q[j] = 0.0;
    bool mine;
    if constexpr (HEAD == kGradActor) {
      q[0] = ts_wave_sum(S.s[0]);
      q[2] = ts_wave_sum(S.s[1]);
      q[3] = ts_wave_sum((double)S.n_clip);
      q[kPpoSums] = ts_wave_min((double)S.r_lo);
      q[kPpoSums + 1] = ts_wave_max((double)S.r_hi);
#pragma unroll
      for (int c = 0; c < kPpoMaxA; ++c) q[kPpoSums + 2 + c] = ts_wave_sum(S.gls[c]);
      mine = t == 0 || t == 2 || t == 3 || (t >= kPpoSums && t < kPpoQ);
      if constexpr (OPT) {
        q[kPpoColBnd] = ts_wave_sum(S.o[0]);
        mine = mine || t == kPpoColBnd;
      }
    } else {
      q[1] = ts_wave_sum(S.s[0]);
      q[4] = ts_wave_sum(S.s[1]);
      q[5] = ts_wave_sum(S.s[2]);
      q[6] = ts_wave_sum(S.s[3]);
      mine = t == 1 || t == 4 || t == 5 || t == 6;
      if constexpr (OPT) {
        q[kPpoColVc] = ts_wave_sum(S.o[0]);
        q[kPpoColOut] = ts_wave_sum((double)S.n_out);
        mine = mine || t == kPpoColVc || t == kPpoColOut;
      }
    }
    double v = q[0];
#pragma unroll
    for (int j = 1; j < QN; ++j) v = t == j ? q[j] : v;
    if (mine) stat_part[(size_t)blockIdx.x * kPpoStride + t] = v;
  }
};
template <int HEAD>
struct PpoGradK : PpoGradHead<HEAD, false> {};
template <int HEAD>
struct PpoGradOptK : PpoGradHead<HEAD, true> {};
template <int HEAD, bool OPT>
struct PpoGradRowsK : PpoGradHead<HEAD, OPT, true> {};

// the workspace, in this order: the rows of double partials, the actor's blocks of float partials, the critic's
inline size_t ppo_grad_stat_bytes(int grid) { return sizeof(double) * (size_t)grid * kPpoStride; }

}  // namespace pf
