// heist_play.hip -- heist_plan_play (include/heist.h): episodes played from a planner's per-tick
// tables, with no ray cast and no env touched.
//
// The emitters do not depend on the Solver, so an episode is a function of the visibility rows a
// planner launch left (heist_plan_field / heist_plan_value's vis_out), the env's grid, the start
// cell and an action rule: the table's action, or a uniform one on a counter-hashed share of the
// steps.  One wave plays one env; every quantity of the play is wave-uniform (formed through
// readfirstlane, so every branch below is a scalar one) and lane 0 stores the step's outputs:
//   * the env's grid is staged once, R C bytes of LDS;
//   * the dependent chain of a step is table byte -> move -> grid byte (LDS) and visibility bit
//     (a readlane of the row the wave holds) -> reward; the next step's table byte and value are
//     requested as soon as the cell is known, BEFORE the step's reward and stores: vmcnt counts
//     loads and stores in issue order, so a load issued behind the stores would wait for them;
//   * the wave holds visibility row k as one uint4 per lane (W / 4 <= 33 quads at 64 x 64), row
//     k + 1 is requested under step k, and the record of step k is that row with the position
//     word set: 16-byte loads and stores;
//   * the rows after the play's end are filled by the whole wave, 64 rows per pass.
// Plain vector loads and stores only, no atomics, nothing shared between workgroups; the launch
// reads the handle (EnvScalars, grid) and writes the caller's arrays alone.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "heist_device.h"

#pragma clang fp contract(off)

namespace heist {

namespace {

__device__ __forceinline__ int ufirst(int x) { return __builtin_amdgcn_readfirstlane(x); }

__device__ __forceinline__ uint64_t play_mix64(uint64_t z) {  // splitmix64 finaliser (heist_solver_head's)
  z ^= z >> 30;
  z *= 0xBF58476D1CE4E5B9ull;
  z ^= z >> 27;
  z *= 0x94D049BB133111EBull;
  z ^= z >> 31;
  return z;
}

__device__ __forceinline__ int iabs(int x) { return x < 0 ? -x : x; }

struct PlayOut {
  int64_t* actions;
  int8_t* expert;
  double* value;
  uint4* records;
  double* reward64;
  uint8_t* done;
  int8_t* status;
  int32_t* len;
};

__global__ __launch_bounds__(64) void plan_play_kernel(EnvParams p, int H, const int8_t* __restrict__ action_table,
                                                       const uint4* __restrict__ vis4,
                                                       const double* __restrict__ value_table,
                                                       const int32_t* __restrict__ pos0, uint32_t noise_q24,
                                                       uint64_t seed, PlayOut o) {
  __shared__ uint8_t grid[kMaxDim * kMaxDim];
  const int e = blockIdx.x, lane = threadIdx.x;
  const int R = p.R, C = p.C, RC = p.RC, N = p.n_envs;
  const int nvis = (RC + 31) >> 5, W4 = ((nvis + 4) & ~3) >> 2;  // the record's words (obs_record_words) / 4
  {
    const uint8_t* g = p.grid + (size_t)e * RC;
    for (int i = lane; i < RC; i += 64) grid[i] = g[i];
  }
  const EnvScalars s = p.scal[e];
  const int tick0 = ufirst(s.tick), D0 = ufirst(s.initial_dist);
  int HK = p.max_steps - tick0;
  HK = HK < H ? HK : H;
  if (ufirst(s.done) || HK < 0) HK = 0;
  int xr = ufirst(s.pos_r), xc = ufirst(s.pos_c);
  if (pos0) {
    xr = ufirst(pos0[2 * (size_t)e]);
    xc = ufirst(pos0[2 * (size_t)e + 1]);
  }
  const bool off_grid = xr < 0 || xr >= R || xc < 0 || xc >= C;
  if (off_grid) HK = 0;
  __syncthreads();  // the grid

  const int vr = p.vr, vc = p.vc;
  const double r_step = p.r_step, r_detect = p.r_detect, r_vault = p.r_vault;
  const bool bonus = D0 > 3;
  const uint64_t ekey = (uint64_t)e * 0x9E3779B97F4A7C15ull;
  const int pw = nvis >> 2, pcomp = nvis & 3;  // the position word's quad and component
  auto load_row = [&](int k) {
    return lane < W4 ? vis4[((size_t)k * N + e) * W4 + lane] : make_uint4(0u, 0u, 0u, 0u);
  };

  int len = 0;
  if (HK > 0) {
    size_t cell = (size_t)e * RC + (size_t)(xr * C + xc);  // row 0
    int t_raw = action_table[cell];
    double v = value_table ? value_table[cell] : 0.0;
    uint4 row = load_row(0);
    for (int k = 0; k < HK; ++k) {
      const int t = ufirst(t_raw);
      const int ex = (t < 0 || t > 4) ? -1 : t;
      const double vk = v;
      const uint64_t z = play_mix64(seed ^ ((uint64_t)(uint32_t)(tick0 + k) * 0xD1B54A32D192ED03ull) ^ ekey);
      const bool noisy = (uint32_t)(z >> 40) < noise_q24;
      int a = ex < 0 ? 0 : ex;
      if (noisy) a = (int)(((z & 0xFFFFFFFFull) * 5ull) >> 32);
      // move(x, a): a blocked move is a stay
      const int nr = xr + (a == 1 ? -1 : (a == 2 ? 1 : 0)), nc = xc + (a == 3 ? -1 : (a == 4 ? 1 : 0));
      int yr = xr, yc = xc;
      if (nr >= 0 && nr < R && nc >= 0 && nc < C && ufirst(grid[nr * C + nc]) != kWall) yr = nr, yc = nc;
      const int y = yr * C + yc;
      const int wi = y >> 5, comp = wi & 3;
      const uint32_t sel = comp == 0 ? row.x : (comp == 1 ? row.y : (comp == 2 ? row.z : row.w));
      const uint32_t word = __builtin_amdgcn_readlane(sel, ufirst(wi >> 2));
      const bool seen = ((word >> (y & 31)) & 1u) != 0u;
      const bool at_vault = yr == vr && yc == vc;
      const bool last = tick0 + k + 1 >= p.max_steps;
      const bool done = seen || at_vault || last;
      const uint4 rec_row = row;
      // the next step's loads, ahead of this step's stores
      if (!done && k + 1 < HK) {
        cell = ((size_t)(k + 1) * N + e) * RC + (size_t)y;
        t_raw = action_table[cell];
        if (value_table) v = value_table[cell];
        row = load_row(k + 1);
      }
      // the step's reward: heist_plan_value's rew, one IEEE double operation per line
      const int dx = iabs(xr - vr) + iabs(xc - vc), curr = iabs(yr - vr) + iabs(yc - vc);
      double rew = r_step;
      rew += (double)(dx - curr) * 0.1;
      if (curr <= 3 && bonus) rew += 0.05 * (double)(3 - curr);
      if (seen) rew += r_detect;
      if (at_vault) rew += r_vault;
      if (last) {
        double frac = 1.0 - (double)curr / (double)(D0 > 1 ? D0 : 1);
        if (frac < 0.0) frac = 0.0;
        rew += frac * 2.0;
      }
      int status = kRunning;
      if (seen) status = kDetected;
      if (at_vault) status = kVaultReached;
      if (last) status = kTimeout;
      const size_t out = (size_t)k * N + e;
      if (lane == 0) {
        o.actions[out] = (int64_t)a;
        if (o.expert) o.expert[out] = (int8_t)ex;
        if (o.value) o.value[out] = vk;
        if (o.reward64) o.reward64[out] = rew;
        o.done[out] = done ? 1 : 0;
        o.status[out] = (int8_t)status;
      }
      if (o.records && lane < W4) {
        uint4 rec = rec_row;
        if (lane == pw) {
          const uint32_t pos = (uint32_t)pack_rc(yr, yc);
          if (pcomp == 0) rec.x = pos;
          else if (pcomp == 1) rec.y = pos;
          else if (pcomp == 2) rec.z = pos;
          else rec.w = pos;
        }
        o.records[out * W4 + lane] = rec;
      }
      xr = yr;
      xc = yc;
      len = k + 1;
      if (done) break;
    }
  }

  // the rows after the end (every row of an env with nothing to play)
  for (int k = len + lane; k < H; k += 64) {
    const size_t out = (size_t)k * N + e;
    o.actions[out] = 0;
    if (o.expert) o.expert[out] = (int8_t)-1;
    if (o.value) o.value[out] = 0.0;
    if (o.reward64) o.reward64[out] = 0.0;
    o.done[out] = 1;
    o.status[out] = (int8_t)kAlreadyDone;
  }
  if (o.records) {
    const uint4 z4 = make_uint4(0u, 0u, 0u, 0u);
    for (int i = lane; i < (H - len) * W4; i += 64) {
      const int r = len + i / W4, q = i - (i / W4) * W4;
      o.records[((size_t)r * N + e) * W4 + q] = z4;
    }
  }
  if (o.len && lane == 0) o.len[e] = off_grid ? -1 : len;
}

}  // namespace

hipError_t launch_plan_play(const EnvParams& p, int horizon, const int8_t* action_table, const uint32_t* vis,
                            const double* value_table, const int32_t* pos0, uint32_t noise_q24, uint64_t seed,
                            int64_t* actions_out, int8_t* expert_out, double* value_out, uint32_t* records_out,
                            double* reward64_out, uint8_t* done_out, int8_t* status_out, int32_t* len_out,
                            hipStream_t st) {
  if (p.R < 1 || p.C < 1 || p.R > kMaxDim || p.C > kMaxDim) return hipErrorInvalidValue;
  PlayOut o{actions_out, expert_out, value_out, reinterpret_cast<uint4*>(records_out), reward64_out, done_out,
            status_out, len_out};
  hipLaunchKernelGGL(plan_play_kernel, dim3(p.n_envs), dim3(64), 0, st, p, horizon, action_table,
                     reinterpret_cast<const uint4*>(vis), value_table, pos0, noise_q24, seed, o);
  return hipGetLastError();
}

}  // namespace heist
