// heist_state.hip -- env state blobs: heist_state_save / heist_state_load (include/heist.h).
//
// A blob restates one env as the kernels keep it in HBM between launches (heist_device.h), so an
// env loaded from it continues bit for bit.  Layout (StateLayout, every section 16-byte aligned):
//   header   64 B   16 uint32: magic, format version, rows, cols, max_cams, max_guards, max_path,
//                   guard_cones, max_steps, start r, c, vault r, c, 0, 0, 0
//   scalars  48 B   EnvScalars
//   cams     32 B x max_cams    Cam records (heading = the camera's current heading)
//   guards   32 B x max_guards  Guard records (idx, pos, heading, hslot, nslot: the current pose)
//   paths    2 B x max_guards x max_path, padded to 16
//   grid     rows x cols bytes, padded to 16
//   stop     stop_bytes: the bit-packed padded stop map (a function of the grid; 128 B at 20 x 20)
// The guard cone cache (8 KB per guard) is not in the blob: the load rebuilds it with the kernel
// heist_set_layout uses (guard_cone_kernel), which needs the guards as set_layout leaves them --
// patrol point 0, heading 0, no slots.  So a load is three launches: state_load_kernel writes
// everything and the guards in that form, guard_cone_kernel fills the cones of the loaded envs,
// state_guards_kernel puts the guards' saved pose back.  Loads and stores are plain vector ones.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "heist_device.h"

namespace heist {

constexpr uint32_t kStateMagic = 0x54534548u;  // "HEST"
constexpr uint32_t kStateVersion = 1;
constexpr int kStateHeaderWords = 16;

struct StateLayout {
  int scal, cams, guards, paths, grid, stop, bytes;  // byte offsets of the sections, total size
  int path_bytes, grid_bytes;                        // unpadded sizes of the two byte-copied sections
};

static __host__ __device__ inline int state_align16(int x) { return (x + 15) & ~15; }

__host__ __device__ inline StateLayout state_layout(const EnvParams& p) {
  StateLayout L;
  L.scal = 4 * kStateHeaderWords;
  L.cams = L.scal + (int)sizeof(EnvScalars);
  L.guards = L.cams + (int)sizeof(Cam) * p.max_cams;
  L.paths = L.guards + (int)sizeof(Guard) * p.max_guards;
  L.path_bytes = 2 * p.max_guards * p.max_path;
  L.grid = L.paths + state_align16(L.path_bytes);
  L.grid_bytes = p.RC;
  L.stop = L.grid + state_align16(L.grid_bytes);
  L.bytes = L.stop + p.stop_bytes;
  return L;
}

int64_t state_blob_bytes(const EnvParams& p) { return state_layout(p).bytes; }

__device__ __forceinline__ uint32_t state_header_word(const EnvParams& p, int k) {
  switch (k) {
    case 0: return kStateMagic;
    case 1: return kStateVersion;
    case 2: return (uint32_t)p.R;
    case 3: return (uint32_t)p.C;
    case 4: return (uint32_t)p.max_cams;
    case 5: return (uint32_t)p.max_guards;
    case 6: return (uint32_t)p.max_path;
    case 7: return (uint32_t)p.guard_cones;
    case 8: return (uint32_t)p.max_steps;
    case 9: return (uint32_t)p.sr;
    case 10: return (uint32_t)p.sc;
    case 11: return (uint32_t)p.vr;
    case 12: return (uint32_t)p.vc;
    default: return 0u;
  }
}

// n16 16-byte words src -> dst (both 16-byte aligned), by threads lane, lane + 64, ...
__device__ __forceinline__ void copy16(void* dst, const void* src, int n16, int lane) {
  uint4* d = reinterpret_cast<uint4*>(dst);
  const uint4* s = reinterpret_cast<const uint4*>(src);
  for (int i = lane; i < n16; i += 64) d[i] = s[i];
}

// n bytes src -> dst, then zeros up to pad bytes (pad >= n), any alignment
__device__ __forceinline__ void copy_bytes(uint8_t* dst, const uint8_t* src, int n, int pad, int lane) {
  for (int i = lane; i < pad; i += 64) dst[i] = i < n ? src[i] : (uint8_t)0;
}

// One wave per blob: env env_ids[i] (NULL: i) -> blob i.  An env id outside [0, n_envs) gives a
// blob of zeros (no magic: a load rejects it).
__global__ __launch_bounds__(64) void state_save_kernel(EnvParams p, const int32_t* __restrict__ env_ids,
                                                         uint8_t* __restrict__ blobs) {
  const int i = blockIdx.x, lane = threadIdx.x;
  const StateLayout L = state_layout(p);
  uint8_t* b = blobs + (size_t)i * L.bytes;
  const int e = env_ids ? env_ids[i] : i;
  if ((unsigned)e >= (unsigned)p.n_envs) {
    const uint4 z = make_uint4(0u, 0u, 0u, 0u);
    for (int k = lane; k < L.bytes / 16; k += 64) reinterpret_cast<uint4*>(b)[k] = z;
    return;
  }
  if (lane < kStateHeaderWords) reinterpret_cast<uint32_t*>(b)[lane] = state_header_word(p, lane);
  copy16(b + L.scal, p.scal + e, (int)sizeof(EnvScalars) / 16, lane);
  copy16(b + L.cams, p.cams + (size_t)e * p.max_cams, 2 * p.max_cams, lane);
  copy16(b + L.guards, p.guards + (size_t)e * p.max_guards, 2 * p.max_guards, lane);
  copy_bytes(b + L.paths, reinterpret_cast<const uint8_t*>(p.paths + (size_t)e * p.max_guards * p.max_path),
             L.path_bytes, L.grid - L.paths, lane);
  copy_bytes(b + L.grid, p.grid + (size_t)e * p.RC, L.grid_bytes, L.stop - L.grid, lane);
  copy16(b + L.stop, p.stop + (size_t)e * p.stop_bytes, p.stop_bytes / 16, lane);
}

// The blob's records keep the env inside what the step kernels index: counts within the handle's
// capacities, the solver on the grid, every live guard's patrol index and step inside its path,
// its cone slots inside the table.  (Checked by every lane on the same words: uniform.)
__device__ bool state_blob_sane(const EnvParams& p, const StateLayout& L, const uint8_t* b) {
  const EnvScalars s = *reinterpret_cast<const EnvScalars*>(b + L.scal);
  if ((unsigned)s.n_cams > (unsigned)p.max_cams || (unsigned)s.n_guards > (unsigned)p.max_guards) return false;
  if ((unsigned)s.pos_r >= (unsigned)p.R || (unsigned)s.pos_c >= (unsigned)p.C) return false;
  const Cam* cams = reinterpret_cast<const Cam*>(b + L.cams);
  for (int c = 0; c < s.n_cams; ++c)
    if ((unsigned)cams[c].row >= (unsigned)p.R || (unsigned)cams[c].col >= (unsigned)p.C) return false;
  const Guard* gs = reinterpret_cast<const Guard*>(b + L.guards);
  const uint16_t* paths = reinterpret_cast<const uint16_t*>(b + L.paths);
  for (int g = 0; g < s.n_guards; ++g) {
    const Guard gd = gs[g];
    if (gd.len < 1 || gd.len > p.max_path || gd.idx < 0 || gd.idx >= gd.len || gd.step < 0 || gd.step >= gd.len)
      return false;
    if ((gd.hslot != kUncached && gd.hslot >= kConeSlots) || (gd.nslot != kUncached && gd.nslot >= kConeSlots))
      return false;
    if (gd.hslot != kUncached && (gd.len > kConePath || gd.nslot == kUncached)) return false;
    for (int k = 0; k < gd.len; ++k) {
      const uint16_t v = paths[g * p.max_path + k];
      if ((v & 0xff) >= p.R || (v >> 8) >= p.C) return false;
    }
  }
  return true;
}

// One wave per item: env env_ids[i] (NULL: i) <- blob blob_index[i] (NULL: i).  An item is
// rejected -- status 0, nothing written to the env -- when its env or blob index is out of range,
// when another item names the same env (every such item is rejected, so no env has two writers),
// or when the blob's header differs from the handle's or its records fail state_blob_sane.
// An accepted item writes the env's scalars, cameras, paths, grid and stop map, and its guards as
// heist_set_layout leaves them (guard_cone_kernel's input); loaded[e] = 1 and src[e] = the blob
// for the two launches that follow.
__global__ __launch_bounds__(64) void state_load_kernel(EnvParams p, const int32_t* __restrict__ env_ids, int m,
                                                         const uint8_t* __restrict__ blobs, int n_blobs,
                                                         const int32_t* __restrict__ blob_index,
                                                         uint8_t* __restrict__ status_out,
                                                         uint8_t* __restrict__ loaded, int32_t* __restrict__ src) {
  const int i = blockIdx.x, lane = threadIdx.x;
  const StateLayout L = state_layout(p);
  const int e = env_ids ? env_ids[i] : i;
  const int bi = blob_index ? blob_index[i] : i;
  bool ok = (unsigned)e < (unsigned)p.n_envs && (unsigned)bi < (unsigned)n_blobs;
  if (ok && env_ids) {
    bool dup = false;
    for (int j = lane; j < m; j += 64) dup |= (j != i && env_ids[j] == e);
    ok = !__any(dup);
  }
  const uint8_t* b = blobs + (size_t)(ok ? bi : 0) * L.bytes;
  if (ok) {
    const bool bad = lane < kStateHeaderWords && reinterpret_cast<const uint32_t*>(b)[lane] != state_header_word(p, lane);
    ok = !__any(bad);
  }
  if (ok) ok = state_blob_sane(p, L, b);
  if (status_out && lane == 0) status_out[i] = ok ? 1 : 0;
  if (!ok) return;
  copy16(p.scal + e, b + L.scal, (int)sizeof(EnvScalars) / 16, lane);
  copy16(p.cams + (size_t)e * p.max_cams, b + L.cams, 2 * p.max_cams, lane);
  if (lane < p.max_guards) {
    Guard gd = reinterpret_cast<const Guard*>(b + L.guards)[lane];
    gd.heading = 0.0;
    gd.idx = 0;
    gd.pos = gd.pos0;
    gd.hslot = kUncached;
    gd.nslot = kUncached;
    p.guards[(size_t)e * p.max_guards + lane] = gd;
  }
  copy_bytes(reinterpret_cast<uint8_t*>(p.paths + (size_t)e * p.max_guards * p.max_path), b + L.paths, L.path_bytes,
             L.path_bytes, lane);
  copy_bytes(p.grid + (size_t)e * p.RC, b + L.grid, L.grid_bytes, L.grid_bytes, lane);
  copy16(p.stop + (size_t)e * p.stop_bytes, b + L.stop, p.stop_bytes / 16, lane);
  if (lane == 0) {
    loaded[e] = 1;
    src[e] = bi;
  }
}

// After guard_cone_kernel: the guards of every loaded env as the blob holds them (one thread per
// (env, guard)).  On a handle whose cone cache is off the guards stay uncached, whatever the
// blob's source had (heist_set_guard_cones may have changed after its layouts were set).
__global__ __launch_bounds__(256) void state_guards_kernel(EnvParams p, const uint8_t* __restrict__ blobs,
                                                            const uint8_t* __restrict__ loaded,
                                                            const int32_t* __restrict__ src) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= p.n_envs * p.max_guards) return;
  const int e = t / p.max_guards, g = t - e * p.max_guards;
  if (!loaded[e]) return;
  const StateLayout L = state_layout(p);
  Guard gd = reinterpret_cast<const Guard*>(blobs + (size_t)src[e] * L.bytes + L.guards)[g];
  if (!p.guard_cones) {
    gd.hslot = kUncached;
    gd.nslot = kUncached;
  }
  p.guards[(size_t)e * p.max_guards + g] = gd;
}

hipError_t launch_state_save(const EnvParams& p, const int32_t* env_ids, int m, void* blobs, hipStream_t st) {
  if (m == 0) return hipSuccess;
  hipLaunchKernelGGL(state_save_kernel, dim3(m), dim3(64), 0, st, p, env_ids, (uint8_t*)blobs);
  return hipGetLastError();
}

// loaded [n_envs] uint8 and src [n_envs] int32: the handle's scratch (heist_state_load clears
// `loaded` on the stream first)
hipError_t launch_state_load(const EnvParams& p, const int32_t* env_ids, int m, const void* blobs, int n_blobs,
                             const int32_t* blob_index, uint8_t* status_out, uint8_t* loaded, int32_t* src,
                             hipStream_t st) {
  hipLaunchKernelGGL(state_load_kernel, dim3(m), dim3(64), 0, st, p, env_ids, m, (const uint8_t*)blobs, n_blobs,
                     blob_index, status_out, loaded, src);
  return hipGetLastError();
}

hipError_t launch_state_guards(const EnvParams& p, const void* blobs, const uint8_t* loaded, const int32_t* src,
                               hipStream_t st) {
  if (p.max_guards == 0) return hipSuccess;
  const int n = p.n_envs * p.max_guards;
  hipLaunchKernelGGL(state_guards_kernel, dim3((n + 255) / 256), dim3(256), 0, st, p, (const uint8_t*)blobs, loaded,
                     src);
  return hipGetLastError();
}

}  // namespace heist
