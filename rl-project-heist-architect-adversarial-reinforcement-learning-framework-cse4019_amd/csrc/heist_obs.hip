// heist_obs.hip -- compact observation records (include/heist.h: heist_obs_pack / heist_obs_expand).
//
// An observation [3][R][C] float32 (get_state_tensor, environment.py:347-374) is a function of the
// layout's grid (channel 0), one visibility bit per cell (channel 1) and the solver's cell (channel
// 2, with the vault position a constant of the handle).  obs_pack_kernel keeps the bits and the cell
// as a record of W uint32 words; obs_expand_kernel rebuilds any gathered subset of records, bit for
// bit, from the records and a snapshot of the grids.  Both run one wavefront per observation.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "heist_device.h"

#pragma clang fp contract(off)

namespace heist {

int obs_record_words(int R, int C) {
  const int nvis = (R * C + 31) >> 5;
  return (nvis + 1 + 3) & ~3;  // visibility words + the position word, padded to 16 bytes
}

namespace {

constexpr int kObsBlock = 256;  // 4 waves, one observation each
constexpr int kObsWaves = kObsBlock / 64;
constexpr int kDivShift = 19;   // cell / C == (cell * ceil(2^19 / C)) >> 19 for cell < 4096, C <= 64

// float32(tile) / 5 (environment.py:319), folded at compile time; tiles are 0..5
__device__ const float kTileLut[8] = {0.0f / 5.0f, 1.0f / 5.0f, 2.0f / 5.0f, 3.0f / 5.0f, 4.0f / 5.0f, 5.0f / 5.0f,
                                      0.0f, 0.0f};

// kVec: R * C is a multiple of 4 and the rows are 16-byte aligned, so a lane takes 4 cells per
// 16-byte load; otherwise a lane takes one cell and a ballot is two record words.
template <bool kVec>
__global__ __launch_bounds__(kObsBlock) void obs_pack_kernel(const float* __restrict__ obs, int64_t n, int RC, int C,
                                                             uint32_t div_c, uint32_t vault_pos,
                                                             uint32_t* __restrict__ rec) {
  const int lane = threadIdx.x & 63;
  const int nvis = (RC + 31) >> 5;
  const int W = (nvis + 1 + 3) & ~3;
  for (int64_t row = (int64_t)blockIdx.x * kObsWaves + (threadIdx.x >> 6); row < n;
       row += (int64_t)gridDim.x * kObsWaves) {
    const float* vis = obs + row * 3 * RC + RC;
    const float* pch = vis + RC;
    uint32_t* out = rec + row * W;
    int cell = -1;  // the one cell of channel 2 above 0.5: the solver's, unless it stands on the vault
    if (kVec) {
      const int nq = RC >> 2;
      for (int q0 = 0; q0 < nq; q0 += 64) {
        const int q = q0 + lane;
        float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f), p = v;
        if (q < nq) {
          v = reinterpret_cast<const float4*>(vis)[q];
          p = reinterpret_cast<const float4*>(pch)[q];
        }
        const uint32_t nib = (v.x != 0.0f ? 1u : 0u) | (v.y != 0.0f ? 2u : 0u) | (v.z != 0.0f ? 4u : 0u) |
                             (v.w != 0.0f ? 8u : 0u);
        uint32_t w = nib << ((lane & 7) * 4);  // 8 lanes x 4 cells = one record word
        w |= __shfl_xor(w, 1);
        w |= __shfl_xor(w, 2);
        w |= __shfl_xor(w, 4);
        const int wi = (q0 >> 3) + (lane >> 3);
        if ((lane & 7) == 0 && wi < nvis) out[wi] = w;
        if (p.x > 0.5f) cell = 4 * q;
        if (p.y > 0.5f) cell = 4 * q + 1;
        if (p.z > 0.5f) cell = 4 * q + 2;
        if (p.w > 0.5f) cell = 4 * q + 3;
      }
    } else {
      for (int c0 = 0; c0 < RC; c0 += 64) {
        const int i = c0 + lane;
        const float v = i < RC ? vis[i] : 0.0f;
        const float p = i < RC ? pch[i] : 0.0f;
        const unsigned long long b = __ballot(v != 0.0f);
        const int wi = c0 >> 5;
        if (lane == 0) out[wi] = (uint32_t)b;
        if (lane == 1 && wi + 1 < nvis) out[wi + 1] = (uint32_t)(b >> 32);
        if (p > 0.5f) cell = i;
      }
    }
    const unsigned long long found = __ballot(cell >= 0);
    uint32_t pos = vault_pos;
    if (found) {
      const uint32_t c = (uint32_t)__shfl(cell, __ffsll((long long)found) - 1);
      const uint32_t r = (c * div_c) >> kDivShift;
      pos = r | ((c - r * (uint32_t)C) << 8);
    }
    if (lane < W - nvis) out[nvis + lane] = lane == 0 ? pos : 0u;
  }
}

// Position channel of one cell: base + fl32(-0.3 * (d / (R + C))) with the second term from the
// block's table (gtab[d]), one f32 add (environment.py:357-367 under NEP 50).
__device__ __forceinline__ float pos_value(int cell, int C, uint32_t div_c, int vr, int vc, int vault_cell,
                                           int solver_cell, const float* gtab) {
  const int r = (int)(((uint32_t)cell * div_c) >> kDivShift);
  const int c = cell - r * C;
  const int d = abs(r - vr) + abs(c - vc);
  const float base = cell == vault_cell ? -1.0f : (cell == solver_cell ? 1.0f : 0.0f);
  return base + gtab[d];
}

template <bool kVec>
__global__ __launch_bounds__(kObsBlock) void obs_expand_kernel(const uint32_t* __restrict__ rec, int64_t n_rec,
                                                               const int32_t* __restrict__ rec_env,
                                                               const int64_t* __restrict__ index, int64_t m,
                                                               const int8_t* __restrict__ grid, int n_envs, int R, int C,
                                                               int vr, int vc, uint32_t div_c, float* __restrict__ out) {
  __shared__ float s_g[128];  // d <= R + C - 2 <= 126
  __shared__ float s_lut[8];
  if (threadIdx.x < 128)  // the oracle's arithmetic: f64 divide, f64 multiply, cast, each rounded
    s_g[threadIdx.x] = (float)(-0.3 * ((double)(int)threadIdx.x / (double)(R + C)));
  if (threadIdx.x < 8) s_lut[threadIdx.x] = kTileLut[threadIdx.x];
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int RC = R * C;
  const int nvis = (RC + 31) >> 5;
  const int W = (nvis + 1 + 3) & ~3;
  const int vault_cell = vr * C + vc;
  for (int64_t s = (int64_t)blockIdx.x * kObsWaves + (threadIdx.x >> 6); s < m; s += (int64_t)gridDim.x * kObsWaves) {
    float* o = out + s * 3 * RC;
    const int64_t j = index ? index[s] : s;
    int env = -1;
    if (j >= 0 && j < n_rec) env = rec_env[j];
    if (env < 0 || env >= n_envs) {  // wave-uniform: a bad index or env gives a sample of NaNs, never a stray read
      for (int i = lane; i < 3 * RC; i += 64) o[i] = __int_as_float(0x7FC00000);
      continue;
    }
    const uint32_t* r = rec + j * W;
    const int8_t* g = grid + (int64_t)env * RC;
    const uint32_t pos = r[nvis];
    const int solver_cell = (int)(pos & 0xFF) * C + (int)((pos >> 8) & 0xFF);
    if (kVec) {
      const int nq = RC >> 2;
      for (int q = lane; q < nq; q += 64) {
        const int cell = 4 * q;
        const uint32_t g4 = reinterpret_cast<const uint32_t*>(g)[q];
        const uint32_t bits = r[cell >> 5] >> (cell & 31);
        float4 a, b, p;
        a.x = s_lut[g4 & 7];
        a.y = s_lut[(g4 >> 8) & 7];
        a.z = s_lut[(g4 >> 16) & 7];
        a.w = s_lut[(g4 >> 24) & 7];
        b.x = (bits & 1) ? 1.0f : 0.0f;
        b.y = (bits & 2) ? 1.0f : 0.0f;
        b.z = (bits & 4) ? 1.0f : 0.0f;
        b.w = (bits & 8) ? 1.0f : 0.0f;
        p.x = pos_value(cell, C, div_c, vr, vc, vault_cell, solver_cell, s_g);
        p.y = pos_value(cell + 1, C, div_c, vr, vc, vault_cell, solver_cell, s_g);
        p.z = pos_value(cell + 2, C, div_c, vr, vc, vault_cell, solver_cell, s_g);
        p.w = pos_value(cell + 3, C, div_c, vr, vc, vault_cell, solver_cell, s_g);
        reinterpret_cast<float4*>(o)[q] = a;
        reinterpret_cast<float4*>(o + RC)[q] = b;
        reinterpret_cast<float4*>(o + 2 * RC)[q] = p;
      }
    } else {
      for (int cell = lane; cell < RC; cell += 64) {
        o[cell] = s_lut[(uint32_t)g[cell] & 7];
        o[RC + cell] = ((r[cell >> 5] >> (cell & 31)) & 1) ? 1.0f : 0.0f;
        o[2 * RC + cell] = pos_value(cell, C, div_c, vr, vc, vault_cell, solver_cell, s_g);
      }
    }
  }
}

uint32_t div_magic(int C) { return (uint32_t)(((1 << kDivShift) + C - 1) / C); }

int obs_blocks(int64_t n) {
  const int64_t b = (n + kObsWaves - 1) / kObsWaves;
  return (int)(b < 8192 ? b : 8192);  // the kernels stride over the rest
}

}  // namespace

hipError_t launch_obs_pack(const float* obs, int64_t n, int R, int C, int vr, int vc, uint32_t* rec, hipStream_t st) {
  const int RC = R * C;
  const bool vec = RC % 4 == 0 && ((uintptr_t)obs & 15) == 0;
  auto k = vec ? obs_pack_kernel<true> : obs_pack_kernel<false>;
  hipLaunchKernelGGL(k, dim3(obs_blocks(n)), dim3(kObsBlock), 0, st, obs, n, RC, C, div_magic(C),
                     (uint32_t)pack_rc(vr, vc), rec);
  return hipGetLastError();
}

hipError_t launch_obs_expand(const uint32_t* rec, int64_t n_rec, const int32_t* rec_env, const int64_t* index, int64_t m,
                             const int8_t* grid, int n_envs, int R, int C, int vr, int vc, float* out, hipStream_t st) {
  const bool vec = (R * C) % 4 == 0 && ((uintptr_t)out & 15) == 0 && ((uintptr_t)grid & 3) == 0;
  auto k = vec ? obs_expand_kernel<true> : obs_expand_kernel<false>;
  hipLaunchKernelGGL(k, dim3(obs_blocks(m)), dim3(kObsBlock), 0, st, rec, n_rec, rec_env, index, m, grid, n_envs, R, C, vr,
                     vc, div_magic(C), out);
  return hipGetLastError();
}

}  // namespace heist
