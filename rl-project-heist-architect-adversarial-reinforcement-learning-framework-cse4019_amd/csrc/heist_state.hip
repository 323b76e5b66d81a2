// heist_state.hip -- env state blobs: heist_state_save / heist_state_load, and the blob-free
// fork inside a handle: heist_state_fork (include/heist.h).
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
//
// heist_state_fork (state_fork_kernel) copies env to env inside one handle without a blob: the
// same records, and the cone blocks themselves instead of a rebuild.  It relies on, and keeps,
// this invariant: the cone block of a live guard with hslot != kUncached is always
// guard_cone_kernel's output for the env's current grid, that guard's static fields (fov, step,
// len, range, num_rays, pos0) and its path.  heist_set_layout and heist_state_load rebuild the
// block whenever those change; a fork either copies the block along with them or, where the
// destination already holds equal ones under a cached guard, leaves the equal block in place.
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

// lane's share of "n bytes at a and b differ" (any alignment; 16-byte words where both pointers
// and n allow -- a wave-uniform choice)
__device__ __forceinline__ bool bytes_differ(const uint8_t* a, const uint8_t* b, int n, int lane) {
  bool diff = false;
  if ((((uintptr_t)a | (uintptr_t)b | (uintptr_t)n) & 15) == 0) {
    const uint4* x = reinterpret_cast<const uint4*>(a);
    const uint4* y = reinterpret_cast<const uint4*>(b);
    for (int i = lane; i < n / 16; i += 64) {
      const uint4 u = x[i], v = y[i];
      diff |= u.x != v.x || u.y != v.y || u.z != v.z || u.w != v.w;
    }
  } else {
    for (int i = lane; i < n; i += 64) diff |= a[i] != b[i];
  }
  return diff;
}

// copy16 for the cone blocks: four loads in flight per lane before the first store
__device__ __forceinline__ void copy16x4(uint16_t* dst, const uint16_t* src, int n16, int lane) {
  uint4* d = reinterpret_cast<uint4*>(dst);
  const uint4* s = reinterpret_cast<const uint4*>(src);
  for (int i = lane; i < n16; i += 256) {
    uint4 v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (i + 64 * k < n16) v[k] = s[i + 64 * k];
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (i + 64 * k < n16) d[i + 64 * k] = v[k];
  }
}

// One wave per item: env dst_ids[i] <- env src_ids[i] of the same handle, no blob in between.
// An item is rejected -- status 0, nothing written -- when an id is outside [0, n_envs), when
// src == dst, when another item names its dst as dst (every such item is rejected) or when any
// item names its dst as src: sources are only read during the launch and every destination has
// one writer.  No address is formed from an id before that check.
// An accepted item copies what a blob holds (scalars, cameras, guards as they stand, paths, grid,
// stop map) and, per live guard g the source has cached (g < n_guards, hslot != kUncached), the
// patrol-index rows [0, len) of its cone block -- every entry a tick, reset or plan can read (idx
// < len) -- unless dst's block is kept.
// The invariant the keep rule rests on: a live cached guard's cone block is guard_cone_kernel's
// output for the env's current grid, that guard's static fields and its path (heist_set_layout
// and heist_state_load rebuild it whenever those change; a fork copies it with them).  So the
// block is kept exactly when, before the item wrote anything, dst's guard g was live and cached
// and dst's grid bytes, the guard's fov, step, len, range, num_rays and pos0 and its first len
// path points equalled src's.  (A record past dst's n_guards is a leftover of an earlier layout
// whose cones another grid may have shaped: never kept.)  The comparisons read dst first; the
// stores follow the ballots.
// status: 1 every cached guard's cones copied (or none cached), 2 every one kept, 3 some of each.
__global__ __launch_bounds__(64) void state_fork_kernel(EnvParams p, const int32_t* __restrict__ src_ids,
                                                         const int32_t* __restrict__ dst_ids, int m,
                                                         uint8_t* __restrict__ status_out) {
  const int i = blockIdx.x, lane = threadIdx.x;
  const int s = src_ids[i], d = dst_ids[i];
  bool ok = (unsigned)s < (unsigned)p.n_envs && (unsigned)d < (unsigned)p.n_envs && s != d;
  if (ok) {
    bool clash = false;
    for (int j = lane; j < m; j += 64) clash |= (j != i && dst_ids[j] == d) || src_ids[j] == d;
    ok = !__any(clash);
  }
  if (!ok) {
    if (status_out && lane == 0) status_out[i] = 0;
    return;
  }
  const int mg = p.max_guards, mp = p.max_path;  // mg <= kMaxEmitters = 64: one lane per guard
  const Guard* sg = p.guards + (size_t)s * mg;
  Guard* dg = p.guards + (size_t)d * mg;
  const uint16_t* sp = p.paths + (size_t)s * mg * mp;
  uint16_t* dp = p.paths + (size_t)d * mg * mp;
  const uint8_t* sgrid = p.grid + (size_t)s * p.RC;
  uint8_t* dgrid = p.grid + (size_t)d * p.RC;
  const int sng = min(p.scal[s].n_guards, mg), dng = min(p.scal[d].n_guards, mg);
  bool cached = false, keep = false;
  if (lane < sng) {
    const Guard a = sg[lane];
    cached = a.hslot != kUncached;
    if (cached && lane < dng) {
      const Guard b = dg[lane];
      keep = b.hslot != kUncached && __builtin_bit_cast(uint64_t, a.fov) == __builtin_bit_cast(uint64_t, b.fov) &&
             a.step == b.step && a.len == b.len && a.range == b.range && a.num_rays == b.num_rays && a.pos0 == b.pos0;
      const int len = min((int)a.len, mp);
      for (int k = 0; keep && k < len; ++k) keep = sp[lane * mp + k] == dp[lane * mp + k];
    }
  }
  const uint64_t cmask = __ballot(cached);
  uint64_t kmask = __ballot(keep);
  if (kmask && __any(bytes_differ(sgrid, dgrid, p.RC, lane))) kmask = 0;
  const uint64_t copy = cmask & ~kmask;
  if (status_out && lane == 0) status_out[i] = copy == 0 && cmask != 0 ? 2 : (kmask == 0 ? 1 : 3);

  copy16(p.scal + d, p.scal + s, (int)sizeof(EnvScalars) / 16, lane);
  copy16(p.cams + (size_t)d * p.max_cams, p.cams + (size_t)s * p.max_cams, 2 * p.max_cams, lane);
  copy16(dg, sg, 2 * mg, lane);
  const int path_bytes = 2 * mg * mp;
  copy_bytes(reinterpret_cast<uint8_t*>(dp), reinterpret_cast<const uint8_t*>(sp), path_bytes, path_bytes, lane);
  if ((((uintptr_t)sgrid | (uintptr_t)dgrid | (uintptr_t)p.RC) & 15) == 0)
    copy16(dgrid, sgrid, p.RC / 16, lane);
  else
    copy_bytes(dgrid, sgrid, p.RC, p.RC, lane);
  copy16(p.stop + (size_t)d * p.stop_bytes, p.stop + (size_t)s * p.stop_bytes, p.stop_bytes / 16, lane);
  constexpr int kBlock = kConePath * kConeSlots * kConeEntry;  // u16 per guard
  constexpr int kRow16 = kConeSlots * kConeEntry * 2 / 16;     // 16-byte words per patrol index
  for (uint64_t rest = copy; rest; rest &= rest - 1) {
    const int g = __builtin_ctzll(rest);
    const int rows = min(max((int)sg[g].len, 0), kConePath);
    copy16x4(p.cones + ((size_t)d * mg + g) * kBlock, p.cones + ((size_t)s * mg + g) * kBlock, rows * kRow16, lane);
  }
}

hipError_t launch_state_fork(const EnvParams& p, const int32_t* src_ids, const int32_t* dst_ids, int m,
                             uint8_t* status_out, hipStream_t st) {
  hipLaunchKernelGGL(state_fork_kernel, dim3(m), dim3(64), 0, st, p, src_ids, dst_ids, m, status_out);
  return hipGetLastError();
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
