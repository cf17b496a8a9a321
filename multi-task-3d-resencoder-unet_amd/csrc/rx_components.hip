// rx_components.hip -- exact 3-D connected-component labelling, component sizes and size filtering of uint8 volumes (host side
// postprocess/components.py, whose label_numpy, component_sizes_numpy and filter_numpy are the statements).  Volumes are contiguous
// (Z, Y, X) blocks packed back to back, `nvol` of them per call.  Everything is integer.  The label of a foreground voxel is
// 1 + the smallest linear index z*Y*X + y*X + x of its component, so the result does not depend on the order anything ran in.
//
// The label volume doubles as the union-find forest: label = parent + 1, 0 = background, a root points at itself.  The find /
// union / tile-merge logic is rx_components_core.h (shared with the host check); this file holds the memory accessors, the kernels
// and the entry points.
//
//   cc_tile_kernel     a workgroup owns one 8 x 8 x 64 tile; a wave owns a tile row at a time, a lane one voxel.  The bytes are read
//                      once; the ballot of `value > level` is the row's mask and gives every lane its run start, which seeds the
//                      tile's forest in LDS (16 KiB + 64 masks).  After a barrier every foreground voxel joins its run to the runs of
//                      the preceding rows (LDS atomics only), and after another one every voxel writes the GLOBAL index of its local
//                      root + 1.  HBM: one byte read, one word written per voxel.
//   cc_seam_kernel     one launch per axis: a lane owns a voxel on the low face of a tile and joins it to its (up to nine) neighbours
//                      one step down that axis -- across faces, edges and corners as the connectivity allows.  Parents are read with
//                      relaxed agent-scope loads and changed only by atomicMin, on any XCD.
//   cc_flatten_kernel  label = root + 1 for every foreground voxel.
//   cc_sizes_kernel    sizes[root] += voxels.  A wave walks 16 chunks of 64 consecutive voxels; the first lane of a run of equal
//                      labels adds the run's length, and keeps adding into a register while the next chunk continues the run, so
//                      a component that fills whole rows costs one atomic per 1024 voxels.
//   cc_filter_kernel   out = values where sizes[label - 1] >= min_voxels, else 0; four voxels per lane where the pointers allow.
#include "rx_common.h"
#include "rx_components_core.h"

#define RX_CC_BLOCK 256
#define RX_CC_WAVES (RX_CC_BLOCK / 64)
#define RX_CC_SIZE_CHUNKS 16
#define RX_CC_MAX_VOLUMES 65535
static_assert(RX_CC_TX == 64, "a tile row is one wave: its mask is one ballot");

// ---- the two forests ----------------------------------------------------------------------------------------------------------------
struct cc_lds_forest {      // a tile's: LDS words hold the local parent, -1 on background (never walked)
  int* p;
  __device__ __forceinline__ int parent(int i) { return __hip_atomic_load(p + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
  __device__ __forceinline__ int parent_min(int i, int v) { return atomicMin(p + i, v); }
};

struct cc_vol_forest {      // a volume's: the label words themselves.  Other workgroups, on other XCDs, change them while they are
  int* l;                   // read: every load is a relaxed agent-scope atomic load (served past this CU's L1), every change an atomic
  __device__ __forceinline__ int label(int i) { return __hip_atomic_load(l + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
  __device__ __forceinline__ int parent(int i) { return label(i) - 1; }
  __device__ __forceinline__ int parent_min(int i, int v) { return atomicMin(l + i, v + 1) - 1; }
  __device__ __forceinline__ void set_parent(int i, int v) { __hip_atomic_store(l + i, v + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
};

// ---- pass 1: a tile -------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(RX_CC_BLOCK) void cc_tile_kernel(const unsigned char* __restrict__ values, int level, int Z, int Y, int X,
                                                              int ntx, int nty, int max_steps, int* __restrict__ labels) {
  __shared__ int s_p[RX_CC_TILE];
  __shared__ uint64_t s_mask[RX_CC_ROWS];
  const long V = (long)Z * Y * X, XY = (long)Y * X;
  // tile blockIdx.x of ntx * nty * ntz, volume blockIdx.y of nvol: every index below is base + [0, V)
  const int b = (int)blockIdx.x, tix = b % ntx, tiy = (b / ntx) % nty, tiz = b / (ntx * nty);
  const int x0 = tix * RX_CC_TX, y0 = tiy * RX_CC_TY, z0 = tiz * RX_CC_TZ;
  const unsigned char* __restrict__ v = values + (long)blockIdx.y * V;
  int* __restrict__ out = labels + (long)blockIdx.y * V;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, x = x0 + lane;
  cc_lds_forest lds{s_p};

  for (int row = wave; row < RX_CC_ROWS; row += RX_CC_WAVES) {      // the whole wave takes every step: the ballot sees 64 lanes
    const int z = z0 + row / RX_CC_TY, y = y0 + row % RX_CC_TY;
    const bool inside = z < Z && y < Y && x < X;      // z0, y0, x0 are inside by the grid; only then is the byte read
    const bool fg = inside && (int)v[z * XY + (long)y * X + x] > level;
    const unsigned long long mask = __ballot(fg);
    if (lane == 0) s_mask[row] = mask;
    s_p[row * RX_CC_TX + lane] = fg ? row * RX_CC_TX + cc_run_start(mask, lane) : -1;
  }
  __syncthreads();
  for (int row = wave; row < RX_CC_ROWS; row += RX_CC_WAVES)
    if ((s_mask[row] >> lane) & 1ull) cc_tile_voxel(lds, s_mask, row / RX_CC_TY, row % RX_CC_TY, lane, max_steps);
  __syncthreads();      // the forest is final: from here on LDS is only read
  for (int row = wave; row < RX_CC_ROWS; row += RX_CC_WAVES) {
    const int z = z0 + row / RX_CC_TY, y = y0 + row % RX_CC_TY;
    if (!(z < Z && y < Y && x < X)) continue;
    int label = 0;
    if ((s_mask[row] >> lane) & 1ull) {
      // the local root lies in the tile and is foreground, so inside the volume: its global index is < V <= 2^31 - 2
      const int r = cc_find(lds, row * RX_CC_TX + lane), rrow = r / RX_CC_TX;
      label = (int)((z0 + rrow / RX_CC_TY) * XY + (long)(y0 + rrow % RX_CC_TY) * X + x0 + r % RX_CC_TX) + 1;
    }
    out[z * XY + (long)y * X + x] = label;
  }
}

// ---- pass 2: the faces between tiles, one axis per launch ---------------------------------------------------------------------------------
__global__ __launch_bounds__(RX_CC_BLOCK) void cc_seam_kernel(int* labels, int axis, int Z, int Y, int X, int faces, long count,
                                                              int max_steps) {
  const long i = (long)blockIdx.x * RX_CC_BLOCK + threadIdx.x;
  if (i >= count) return;      // count = faces * (the plane of the other two extents)
  int z, y, x;
  if (axis == 0) {            // (face, y, x)
    const long XY = (long)Y * X, r = i % XY;
    z = ((int)(i / XY) + 1) * RX_CC_TZ, y = (int)(r / X), x = (int)(r % X);
  } else if (axis == 1) {     // (z, face, x): a wave reads along x
    const long r = i / X;
    x = (int)(i % X), y = ((int)(r % faces) + 1) * RX_CC_TY, z = (int)(r / faces);
  } else {                    // (z, y, face)
    const long r = i / faces;
    x = ((int)(i % faces) + 1) * RX_CC_TX, y = (int)(r % Y), z = (int)(r / Y);
  }
  // faces = ceil(extent / tile) - 1, so the face coordinate is <= extent - 1; the other two are remainders of their extents:
  // (z, y, x) is inside the volume, and cc_seam_voxel forms no neighbour outside it
  cc_vol_forest vol{labels + (long)blockIdx.y * ((long)Z * Y * X)};
  cc_seam_voxel(vol, axis, z, y, x, Z, Y, X, max_steps);
}

// ---- pass 3: roots ----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(RX_CC_BLOCK) void cc_flatten_kernel(int* labels, long V) {
  const long i = (long)blockIdx.x * RX_CC_BLOCK + threadIdx.x;
  if (i >= V) return;
  cc_vol_forest vol{labels + (long)blockIdx.y * V};
  cc_flatten_voxel(vol, (int)i);
}

// ---- sizes --------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(RX_CC_BLOCK) void cc_sizes_kernel(const int* __restrict__ labels, long total, long voxels, int* __restrict__ sizes) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long w0 = ((long)blockIdx.x * RX_CC_WAVES + wave) * (64L * RX_CC_SIZE_CHUNKS);
  long held = -1;      // the sizes word this lane is collecting for, and what it has collected
  int held_n = 0;
  for (int k = 0; k < RX_CC_SIZE_CHUNKS; ++k) {      // wave-uniform trip count: the shuffles and ballots see 64 lanes
    const long i = w0 + k * 64 + lane;
    const int l = i < total ? labels[i] : 0;
    // the word of this voxel's root: its volume's block of `sizes` + (label - 1) < voxels.  Different volumes, different words.
    const long t = l > 0 && l <= voxels ? i - i % voxels + (l - 1) : -1;      // any other label is background
    const long prev = __shfl_up(t, 1, 64);
    const bool cont = lane > 0 && t == prev;      // continues the run of the lane before
    const unsigned long long stops = ~__ballot(cont);
    if (t >= 0 && !cont) {
      const unsigned long long above = lane == 63 ? 0ull : stops >> (lane + 1);
      const int n = above ? __ffsll((long long)above) : 64 - lane;      // lanes up to the next run start, or to the wave's end
      if (t == held) {
        held_n += n;
      } else {
        if (held >= 0) atomicAdd(sizes + held, held_n);
        held = t, held_n = n;
      }
    }
  }
  if (held >= 0) atomicAdd(sizes + held, held_n);
}

// ---- filter -------------------------------------------------------------------------------------------------------------------------------
// a label outside 1 .. voxels, which rx_cc_label never writes, is background: no word outside the volume's block of `sizes` is read
__device__ __forceinline__ unsigned char cc_keep(unsigned char v, int l, const int* __restrict__ sizes, long j, long voxels, int min_voxels) {
  return l > 0 && l <= voxels && sizes[j - j % voxels + (l - 1)] >= min_voxels ? v : (unsigned char)0;
}

// values and out may be the same buffer: a lane reads its own four bytes before it writes them and touches nobody else's
__global__ __launch_bounds__(RX_CC_BLOCK) void cc_filter_kernel(const unsigned char* values, const int* __restrict__ labels,
                                                                const int* __restrict__ sizes, int min_voxels, long total, long voxels,
                                                                unsigned char* out, int vec) {
  const long i = ((long)blockIdx.x * RX_CC_BLOCK + threadIdx.x) * 4;
  if (i >= total) return;
  if (vec && i + 4 <= total) {      // all three pointers are 16 / 4 / 4-byte aligned and i is a multiple of 4
    const uchar4 v = *(const uchar4*)(values + i);
    const int4 l = *(const int4*)(labels + i);
    uchar4 o;
    o.x = cc_keep(v.x, l.x, sizes, i, voxels, min_voxels);
    o.y = cc_keep(v.y, l.y, sizes, i + 1, voxels, min_voxels);
    o.z = cc_keep(v.z, l.z, sizes, i + 2, voxels, min_voxels);
    o.w = cc_keep(v.w, l.w, sizes, i + 3, voxels, min_voxels);
    *(uchar4*)(out + i) = o;
  } else {
    for (long j = i; j < i + 4 && j < total; ++j) out[j] = cc_keep(values[j], labels[j], sizes, j, voxels, min_voxels);
  }
}

// ---- host side ----------------------------------------------------------------------------------------------------------------------------
extern "C" int rx_cc_label(const uint8_t* values, int level, int nvol, int z, int y, int x, int connectivity, int32_t* labels, void* stream) {
  if (!values) RX_FAIL(RX_EINVAL, "rx_cc_label: null input pointer");
  if (!labels) RX_FAIL(RX_EINVAL, "rx_cc_label: null output pointer");
  if (nvol <= 0 || z <= 0 || y <= 0 || x <= 0) RX_FAIL(RX_EINVAL, "rx_cc_label: sizes must be positive (got nvol=%d z=%d y=%d x=%d)", nvol, z, y, x);
  if (nvol > RX_CC_MAX_VOLUMES) RX_FAIL(RX_EINVAL, "rx_cc_label: at most %d volumes in a call (got %d)", RX_CC_MAX_VOLUMES, nvol);
  const int max_steps = cc_max_steps(connectivity);
  if (!max_steps) RX_FAIL(RX_EINVAL, "rx_cc_label: connectivity %d (6, 18 or 26)", connectivity);
  if (level < 0 || level > 254) RX_FAIL(RX_EINVAL, "rx_cc_label: level %d (0 .. 254: the mask is value > level)", level);
  const long v = (long)z * y * x;
  if (v > RX_CC_MAX_VOXELS) RX_FAIL(RX_EINVAL, "rx_cc_label: %ld voxels in a volume (at most 2^31 - 2: a label is an index + 1 in int32)", v);
  if (((uintptr_t)labels & 3) != 0) RX_FAIL(RX_EINVAL, "rx_cc_label: labels must be 4-byte aligned");
  if ((const void*)values == (const void*)labels) RX_FAIL(RX_EINVAL, "rx_cc_label: values and labels must be different buffers");
  const int ntx = (x + RX_CC_TX - 1) / RX_CC_TX, nty = (y + RX_CC_TY - 1) / RX_CC_TY, ntz = (z + RX_CC_TZ - 1) / RX_CC_TZ;
  const long tiles = (long)ntx * nty * ntz;      // <= v
  hipStream_t st = (hipStream_t)stream;
  const dim3 block(RX_CC_BLOCK);
  hipLaunchKernelGGL(cc_tile_kernel, dim3((unsigned)tiles, (unsigned)nvol), block, 0, st, values, level, z, y, x, ntx, nty, max_steps, labels);
  RX_CHECK_LAUNCH("rx_cc_label");
  const int faces[3] = {ntz - 1, nty - 1, ntx - 1};
  const long plane[3] = {(long)y * x, (long)z * x, (long)z * y};
  for (int axis = 0; axis < 3; ++axis) {
    const long count = faces[axis] * plane[axis];      // < v
    if (count == 0) continue;
    hipLaunchKernelGGL(cc_seam_kernel, dim3((unsigned)((count + RX_CC_BLOCK - 1) / RX_CC_BLOCK), (unsigned)nvol), block, 0, st, labels, axis, z,
                       y, x, faces[axis], count, max_steps);
    RX_CHECK_LAUNCH("rx_cc_label");
  }
  if (tiles > 1) {      // one tile: the tile pass already wrote roots
    hipLaunchKernelGGL(cc_flatten_kernel, dim3((unsigned)((v + RX_CC_BLOCK - 1) / RX_CC_BLOCK), (unsigned)nvol), block, 0, st, labels, v);
    RX_CHECK_LAUNCH("rx_cc_label");
  }
  return RX_OK;
}

static inline int cc_total_ok(const char* fn, int nvol, long voxels) {
  if (nvol <= 0 || voxels <= 0) RX_FAIL(RX_EINVAL, "%s: sizes must be positive (got nvol=%d voxels=%ld)", fn, nvol, voxels);
  if (voxels > RX_CC_MAX_VOXELS) RX_FAIL(RX_EINVAL, "%s: %ld voxels in a volume (at most 2^31 - 2)", fn, voxels);
  if (nvol > RX_CC_MAX_VOLUMES) RX_FAIL(RX_EINVAL, "%s: at most %d volumes in a call (got %d)", fn, RX_CC_MAX_VOLUMES, nvol);
  return RX_OK;
}

extern "C" int rx_cc_sizes(const int32_t* labels, int nvol, long voxels, int32_t* sizes, void* stream) {
  if (!labels) RX_FAIL(RX_EINVAL, "rx_cc_sizes: null input pointer");
  if (!sizes) RX_FAIL(RX_EINVAL, "rx_cc_sizes: null output pointer");
  if (int rc = cc_total_ok("rx_cc_sizes", nvol, voxels)) return rc;
  if ((((uintptr_t)labels | (uintptr_t)sizes) & 3) != 0) RX_FAIL(RX_EINVAL, "rx_cc_sizes: labels and sizes must be 4-byte aligned");
  if ((const void*)labels == (const void*)sizes) RX_FAIL(RX_EINVAL, "rx_cc_sizes: labels and sizes must be different buffers");
  const long total = (long)nvol * voxels, per_block = 64L * RX_CC_SIZE_CHUNKS * RX_CC_WAVES;
  const long grid = (total + per_block - 1) / per_block;
  if (grid > 0x7fffffffL) RX_FAIL(RX_EINVAL, "rx_cc_sizes: %ld voxels are more than one call's grid covers", total);
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(sizes, 0, (size_t)total * sizeof(int32_t), st) != hipSuccess) RX_FAIL(RX_ELAUNCH, "rx_cc_sizes: hipMemsetAsync failed");
  hipLaunchKernelGGL(cc_sizes_kernel, dim3((unsigned)grid), dim3(RX_CC_BLOCK), 0, st, labels, total, voxels, sizes);
  RX_CHECK_LAUNCH("rx_cc_sizes");
  return RX_OK;
}

extern "C" int rx_cc_filter(const uint8_t* values, const int32_t* labels, const int32_t* sizes, int min_voxels, int nvol, long voxels,
                            uint8_t* out, void* stream) {
  if (!values || !labels || !sizes) RX_FAIL(RX_EINVAL, "rx_cc_filter: null input pointer");
  if (!out) RX_FAIL(RX_EINVAL, "rx_cc_filter: null output pointer");
  if (int rc = cc_total_ok("rx_cc_filter", nvol, voxels)) return rc;
  if ((((uintptr_t)labels | (uintptr_t)sizes) & 3) != 0) RX_FAIL(RX_EINVAL, "rx_cc_filter: labels and sizes must be 4-byte aligned");
  const long total = (long)nvol * voxels;
  const long grid = (total + 4L * RX_CC_BLOCK - 1) / (4L * RX_CC_BLOCK);
  if (grid > 0x7fffffffL) RX_FAIL(RX_EINVAL, "rx_cc_filter: %ld voxels are more than one call's grid covers", total);
  const int vec = (((uintptr_t)values | (uintptr_t)out) & 3) == 0 && ((uintptr_t)labels & 15) == 0;
  hipLaunchKernelGGL(cc_filter_kernel, dim3((unsigned)grid), dim3(RX_CC_BLOCK), 0, (hipStream_t)stream, values, labels, sizes, min_voxels, total,
                     voxels, out, vec);
  RX_CHECK_LAUNCH("rx_cc_filter");
  return RX_OK;
}
