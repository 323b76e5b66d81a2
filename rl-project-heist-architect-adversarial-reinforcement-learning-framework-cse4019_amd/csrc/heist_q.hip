// heist_q.hip -- heist_plan_q (include/heist.h): the five exact action values of every visited
// state, from a planner's per-tick value table and visibility rows.
//
// Q_k(x, a) = rew(x, a, k) + gamma V_{k+1}(move(x, a)) is heist_plan_value's own candidate, so the
// launch restates that kernel's lines on caller-chosen states instead of every cell: no ray is
// cast, no env is touched, no LDS array per cell (every grid up to 64 x 64 is served).  An aligned
// group of 8 lanes serves one state, state s = k N + e: lanes 0 .. 4 take one action each (lanes
// 5 .. 7 repeat action 0 and store nothing), so a wave holds 8 neighbouring envs of one tick and a
// lane carries one gather chain instead of five (30 VGPRs).  The work is a gather, so a lane's
// loads are issued in three batches, each complete before its first use:
//   1. the env's scalars, the state's cell and its taken action (one address per group);
//   2. the grid bytes of the cell and of the lane's neighbour (address clamped into the grid);
//   3. for the lane's cell y = move(x, a): V_{k+1}[y] and the word of vis row k that holds y.
// The five values then reach every lane of the group through width-8 shuffles; maximum, first
// argmax, equality mask and gap are computed from them in every lane alike, lanes 0 .. 4 store
// q[a] (40 contiguous bytes per group) and lane 0 the rest.  Measured against one lane per state
// with the five gathers in flight (same outputs bit for bit): equal on the C2 batch's play states,
// 3-8 % faster the more states are live.
// A state that is not live (past the env's steps, off the grid, a wall cell) keeps every address
// inside the arrays by reading cell 0 and stores the fill; so do the groups past the last state,
// which store nothing.  Plain vector loads and stores only, no atomics, nothing shared between
// workgroups; the launch reads the handle (EnvScalars, grid) and the caller's tables and writes the
// caller's arrays alone.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "heist_device.h"

#pragma clang fp contract(off)

namespace heist {

namespace {

__device__ __forceinline__ int q_iabs(int x) { return x < 0 ? -x : x; }

struct QOut {
  double* q;
  double* value;
  int8_t* best;
  uint8_t* optimal;
  double* gap;
};

constexpr int kQBlock = 256;

__global__ __launch_bounds__(kQBlock) void plan_q_kernel(EnvParams p, int H, int K, double gamma,
                                                         const double* __restrict__ value_table,
                                                         const uint32_t* __restrict__ vis,
                                                         const int32_t* __restrict__ tick0,
                                                         const int32_t* __restrict__ pos,
                                                         const int64_t* __restrict__ taken, QOut o) {
  const int R = p.R, C = p.C, RC = p.RC, N = p.n_envs;
  const long long gt = (long long)blockIdx.x * kQBlock + threadIdx.x;
  const long long total = (long long)K * N;
  const long long s_raw = gt >> 3;
  const bool in_range = s_raw < total;
  const long long s = in_range ? s_raw : total - 1;  // whole groups stay converged for the shuffles
  const int a = (int)(gt & 7) < 5 ? (int)(gt & 7) : 0;
  const int k = (int)(s / N), e = (int)(s - (long long)k * N);
  const int nvis = (RC + 31) >> 5, WR = (nvis + 4) & ~3;  // the record's words (obs_record_words)

  // 1. the env's scalars, the cell, the taken action
  const EnvScalars sc = p.scal[e];
  const int t0_arg = tick0 ? tick0[e] : 0;
  const int xr_raw = pos[2 * s], xc_raw = pos[2 * s + 1];
  const long long tk_raw = taken ? taken[s] : 0;

  const int t0 = tick0 ? t0_arg : (sc.done ? -1 : sc.tick);
  int HK = p.max_steps - t0;
  HK = HK < H ? HK : H;
  if (t0 < 0 || HK < 0) HK = 0;
  const bool inside = xr_raw >= 0 && xr_raw < R && xc_raw >= 0 && xc_raw < C;
  const int xr = inside ? xr_raw : 0, xc = inside ? xc_raw : 0;
  const int x = xr * C + xc;

  // 2. move(x, a): the grid bytes of the cell and of the lane's neighbour; a blocked move is a stay
  const int dr = a == 1 ? -1 : (a == 2 ? 1 : 0), dc = a == 3 ? -1 : (a == 4 ? 1 : 0);
  const int nr = xr + dr, nc = xc + dc;
  const bool in_a = nr >= 0 && nr < R && nc >= 0 && nc < C;
  const uint8_t* g = p.grid + (size_t)e * RC;
  const uint8_t g0 = g[x];
  const uint8_t ga = g[in_a ? nr * C + nc : x];
  const bool live = k < HK && inside && g0 != kWall;
  const bool ok = in_a && ga != kWall;
  const int yr = ok ? nr : xr, yc = ok ? nc : xc, y = yr * C + yc;

  // 3. V_{k+1}[y] and y's word of vis row k
  const uint32_t word = vis[((size_t)k * N + e) * WR + (y >> 5)];
  double nxt = 0.0;
  if (k + 1 < H) nxt = value_table[((size_t)(k + 1) * N + e) * RC + y];

  const int vr = p.vr, vc = p.vc, vcell = vr * C + vc;
  const int D0 = sc.initial_dist;
  const bool bonus = D0 > 3;
  const bool last = t0 + k + 1 >= p.max_steps;
  const int dx = q_iabs(xr - vr) + q_iabs(xc - vc);
  const int curr = q_iabs(yr - vr) + q_iabs(yc - vc);
  // heist_plan_value's candidate, line for line, each line one IEEE double operation
  double rew = p.r_step;
  rew += (double)(dx - curr) * 0.1;
  if (curr <= 3 && bonus) rew += 0.05 * (double)(3 - curr);
  const bool seen = ((word >> (y & 31)) & 1u) != 0u;
  if (seen) rew += p.r_detect;
  if (y == vcell) rew += p.r_vault;
  if (last) {
    double frac = 1.0 - (double)curr / (double)(D0 > 1 ? D0 : 1);
    if (frac < 0.0) frac = 0.0;
    rew += frac * 2.0;
  }
  const double on = rew + gamma * nxt;
  const double qa = live ? ((seen || y == vcell || last) ? rew : on) : 0.0;

  const double q0 = __shfl(qa, 0, 8), q1 = __shfl(qa, 1, 8), q2 = __shfl(qa, 2, 8), q3 = __shfl(qa, 3, 8),
               q4 = __shfl(qa, 4, 8);
  double best = 0.0, gap = 0.0;
  int act = -1;
  uint32_t opt = 0u;
  if (live) {
    best = q0;
    act = 0;
    if (q1 > best) best = q1, act = 1;
    if (q2 > best) best = q2, act = 2;
    if (q3 > best) best = q3, act = 3;
    if (q4 > best) best = q4, act = 4;
    opt = (q0 == best ? 1u : 0u) | (q1 == best ? 2u : 0u) | (q2 == best ? 4u : 0u) | (q3 == best ? 8u : 0u) |
          (q4 == best ? 16u : 0u);
    const int ta = (tk_raw < 0 || tk_raw > 4) ? 0 : (int)tk_raw;
    const double qt = ta == 0 ? q0 : (ta == 1 ? q1 : (ta == 2 ? q2 : (ta == 3 ? q3 : q4)));
    gap = best - qt;
  }
  if (!in_range) return;
  const int l = (int)(gt & 7);
  if (o.q && l < 5) o.q[5 * (size_t)s + l] = qa;
  if (l == 0) {
    if (o.value) o.value[s] = best;
    if (o.best) o.best[s] = (int8_t)act;
    if (o.optimal) o.optimal[s] = (uint8_t)opt;
    if (o.gap) o.gap[s] = gap;
  }
}

}  // namespace

hipError_t launch_plan_q(const EnvParams& p, int horizon, int K, double gamma, const double* value_table,
                         const uint32_t* vis, const int32_t* tick0, const int32_t* pos, const int64_t* taken,
                         double* q_out, double* value_out, int8_t* best_out, uint8_t* optimal_out, double* gap_out,
                         hipStream_t st) {
  if (p.R < 1 || p.C < 1 || p.R > kMaxDim || p.C > kMaxDim || K < 1 || K > horizon || p.n_envs < 1)
    return hipErrorInvalidValue;
  const long long states = (long long)K * p.n_envs;
  const long long blocks = (states * 8 + kQBlock - 1) / kQBlock;  // 8 lanes per state
  if (blocks > 0x7FFFFFFFll) return hipErrorInvalidValue;
  QOut o{q_out, value_out, best_out, optimal_out, gap_out};
  hipLaunchKernelGGL(plan_q_kernel, dim3((unsigned)blocks), dim3(kQBlock), 0, st, p, horizon, K, gamma, value_table,
                     vis, tick0, pos, taken, o);
  return hipGetLastError();
}

}  // namespace heist
