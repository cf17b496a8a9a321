// rx_surface.hip -- the device half of the surface-distance validation metrics (host side training/metrics/surface.py, whose
// edges_numpy, edt_sq_numpy and surface_hist_numpy are the statements): the edge voxels of a thresholded volume, the exact squared
// Euclidean distance transform, and the histogram of one edge set's distances to the other.  Volumes are contiguous (Z, Y, X)
// blocks packed back to back, `n` of them per call (n = samples * channels).  Everything here is integer: there is no
// floating-point arithmetic in this file beyond the one comparison `value > threshold`.
//
//   mask_edges_kernel<T>   a lane owns one voxel: on = value > threshold (float32 compare, a NaN is off); an on voxel is an edge unless
//                          it is interior AND its six face neighbours are on.  The neighbours come from L1 / L2 (HBM sees one read of
//                          the values and one write of the bytes), and are read only for on voxels that are interior to their volume.
//   edt_x_kernel           pass 1, along x: a workgroup stages a run of whole rows (contiguous bytes) as g0 = 0 on a feature,
//                          RX_EDT_NONE elsewhere, and every lane takes min_j (g0[j] + (i - j)^2) over its own row from LDS.
//   edt_line_kernel        passes 2 (y) and 3 (z), in place: the volume is (outer, L, inner) with the line axis `inner` apart; a
//                          workgroup owns the L x XT tile of XT neighbouring lines (all of y for one z and a run of x; all of z for a
//                          run of the flattened y*x), reads it completely into LDS -- every global access is XT contiguous words --
//                          and, after the barrier, writes min_j (g[j] + (i - j)^2) back over it.  A lane keeps 4 outputs of one line
//                          in registers per LDS word it reads.  The brute-force minimum: L min-adds per voxel, no data-dependent
//                          control flow.  Every minimum starts from RX_EDT_NONE, which is the clamp; with extents <= 1024 the largest intermediate,
//                          RX_EDT_NONE + 1026^2, fits int32.
//   surface_hist_kernel    per edge voxel one count: `unmatched` if its distance is RX_EDT_NONE, else hist[min(d, bins - 1)].  The
//                          first RX_SF_LOW bins of a workgroup live in LDS (near surfaces put most voxels into a handful of bins),
//                          the rest are global 64-bit atomics; integer adds only, so the result does not depend on arrival order.
#include "rx_common.h"

#define RX_SF_BLOCK 256
#define RX_SF_WAVES (RX_SF_BLOCK / 64)
#define RX_EDT_ROW_WORDS 4096        // LDS words of the x pass: at least 4 whole rows (16 KiB)
#define RX_EDT_TILE_WORDS 16384      // LDS words of a line pass: 16 lines of 1024 (64 KiB, the most a launch gets without opting in)
#define RX_EDT_PER_LANE 4            // outputs of one line a lane holds
#define RX_SF_LOW 256                // histogram bins kept in LDS
#define RX_SF_CHUNK (RX_SF_BLOCK * 16)
static_assert(RX_SF_LOW == RX_SF_BLOCK, "surface_hist_kernel: lane t owns LDS bin t");

// ---- edges ---------------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(RX_SF_BLOCK) void mask_edges_kernel(const T* __restrict__ values, float thr, int Z, int Y, int X,
                                                                 unsigned char* __restrict__ edges) {
  const int V = Z * Y * X;      // < 2^31 (extents <= 1024: <= 2^30, so i below cannot wrap either)
  const int i = (int)blockIdx.x * RX_SF_BLOCK + (int)threadIdx.x;
  if (i >= V) return;
  // volume blockIdx.y of gridDim.y = n: every index below is p[0 .. V), the lane's own volume.  A neighbour is i +- 1, +- X,
  // +- X*Y and is read only when `inner` says that x, y and z all have both neighbours -- the z neighbour of a volume's last slice
  // would be the next volume's first slice (or past the buffer), so it is never formed into a load.
  const T* __restrict__ p = values + (long)blockIdx.y * V;
  const int r = i / X, x = i - r * X, z = r / Y, y = r - z * Y, XY = X * Y;
  auto on = [&](int k) { return Elem<T>::to_f(p[k]) > thr; };      // IEEE: a NaN is off
  bool e = false;
  if (on(i)) {
    const bool inner = x > 0 && x + 1 < X && y > 0 && y + 1 < Y && z > 0 && z + 1 < Z;
    e = !(inner && on(i - 1) && on(i + 1) && on(i - X) && on(i + X) && on(i - XY) && on(i + XY));
  }
  edges[(long)blockIdx.y * V + i] = e ? 1 : 0;
}

// ---- squared distance, pass 1: along x --------------------------------------------------------------------------------------------
__global__ __launch_bounds__(RX_SF_BLOCK) void edt_x_kernel(const unsigned char* __restrict__ feature, int* __restrict__ dist, long rows,
                                                            int X, int rows_per_block) {
  extern __shared__ int s_g[];      // [rows_per_block][X] <= RX_EDT_ROW_WORDS
  const long r0 = (long)blockIdx.x * rows_per_block;      // < rows: the grid is ceil(rows / rows_per_block)
  const long left = rows - r0;
  const int nrows = left < rows_per_block ? (int)left : rows_per_block;
  const int E = nrows * X;
  // rows r0 .. r0 + nrows are contiguous: elements f0 .. f0 + E, and f0 + E = (r0 + nrows) * X <= rows * X, the buffer
  const long f0 = r0 * X;
  for (int e = threadIdx.x; e < E; e += RX_SF_BLOCK) s_g[e] = feature[f0 + e] ? 0 : RX_EDT_NONE;
  __syncthreads();
  for (int e = threadIdx.x; e < E; e += RX_SF_BLOCK) {
    const int r = e / X, i = e - r * X;
    const int* __restrict__ row = s_g + r * X;      // row[0 .. X) lies inside s_g[0 .. E)
    int m = RX_EDT_NONE;
#pragma unroll 4
    for (int j = 0; j < X; ++j) {
      const int d = i - j;
      m = min(m, row[j] + __mul24(d, d));      // |d| < 2^23: the 24-bit multiply is exact (and full rate)
    }
    dist[f0 + e] = m;      // already <= RX_EDT_NONE
  }
}

// ---- squared distance, passes 2 and 3: along an axis whose elements are `inner` apart, in place -----------------------------------
__global__ __launch_bounds__(RX_SF_BLOCK) void edt_line_kernel(int* __restrict__ g, int L, long inner, int tiles, int xt_log2) {
  extern __shared__ int s_g[];      // [L][XT]
  const int XT = 1 << xt_log2;
  const long o = (long)(blockIdx.x / (unsigned)tiles);      // < outer: the grid is outer * tiles
  const long c0 = (long)(blockIdx.x - (unsigned)o * (unsigned)tiles) * XT;      // < inner: tiles = ceil(inner / XT)
  // element (j, xl) of the tile is g[base + j * inner + xl] with j < L and, where it is touched at all, c0 + xl < inner: at most
  // o * L * inner + (L - 1) * inner + inner - 1 < outer * L * inner, the buffer.  Columns at or past `inner` are neither loaded
  // nor stored; their LDS words hold RX_EDT_NONE so the arithmetic below stays in range.
  int* __restrict__ base = g + o * L * inner + c0;
  const int words = L << xt_log2;
  for (int e = threadIdx.x; e < words; e += RX_SF_BLOCK) {
    const int j = e >> xt_log2, xl = e & (XT - 1);
    s_g[e] = c0 + xl < inner ? base[(long)j * inner + xl] : RX_EDT_NONE;
  }
  __syncthreads();      // the whole tile is read: from here on global memory is only written
  const int xl = threadIdx.x & (XT - 1), ig = threadIdx.x >> xt_log2, groups = RX_SF_BLOCK >> xt_log2;
  const bool live = c0 + xl < inner;
  for (int i0 = ig * RX_EDT_PER_LANE; i0 < L; i0 += groups * RX_EDT_PER_LANE) {
    int m[RX_EDT_PER_LANE];
#pragma unroll
    for (int k = 0; k < RX_EDT_PER_LANE; ++k) m[k] = RX_EDT_NONE;
#pragma unroll 4
    for (int j = 0; j < L; ++j) {
      const int v = s_g[(j << xt_log2) + xl];      // the lanes of a wave read XT consecutive words, each shared by 64 / XT lanes
#pragma unroll
      for (int k = 0; k < RX_EDT_PER_LANE; ++k) {
        const int d = i0 + k - j;      // |d| <= L + 2
        m[k] = min(m[k], v + __mul24(d, d));
      }
    }
#pragma unroll
    for (int k = 0; k < RX_EDT_PER_LANE; ++k)
      if (live && i0 + k < L) base[(long)(i0 + k) * inner + xl] = m[k];
  }
}

// ---- histogram ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(RX_SF_BLOCK) void surface_hist_kernel(const unsigned char* __restrict__ edges, const int* __restrict__ dist,
                                                                   long total, long bins, unsigned long long* __restrict__ hist,
                                                                   unsigned long long* __restrict__ count,
                                                                   unsigned long long* __restrict__ unmatched) {
  __shared__ unsigned s_low[RX_SF_LOW];
  __shared__ unsigned s_red[RX_SF_WAVES][2];
  s_low[threadIdx.x] = 0u;
  __syncthreads();
  const long b0 = (long)blockIdx.x * RX_SF_CHUNK;      // < total: the grid is ceil(total / RX_SF_CHUNK)
  const long b1 = b0 + RX_SF_CHUNK < total ? b0 + RX_SF_CHUNK : total;
  unsigned c[2] = {0u, 0u};      // edge voxels, of them unmatched
  for (long i = b0 + threadIdx.x; i < b1; i += RX_SF_BLOCK)      // i < total: edges[i] and dist[i] are inside their buffers
    if (edges[i]) {
      c[0] += 1u;
      const unsigned d = (unsigned)dist[i];      // a negative word, which rx_edt_sq never writes, is unmatched too
      if (d >= (unsigned)RX_EDT_NONE) {
        c[1] += 1u;
      } else {
        const long k = (long)d < bins ? (long)d : bins - 1;      // 0 <= k < bins: inside hist
        if (k < RX_SF_LOW) atomicAdd(&s_low[k], 1u);
        else atomicAdd(hist + k, 1ull);
      }
    }
  __syncthreads();
  if (s_low[threadIdx.x]) atomicAdd(hist + threadIdx.x, (unsigned long long)s_low[threadIdx.x]);      // non-zero only for a k < bins
#pragma unroll
  for (int w = 0; w < 2; ++w)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c[w] += __shfl_xor(c[w], o, 64);
  if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6][0] = c[0], s_red[threadIdx.x >> 6][1] = c[1];
  __syncthreads();
  if (threadIdx.x < 2) {
    unsigned long long s = 0ull;
#pragma unroll
    for (int k = 0; k < RX_SF_WAVES; ++k) s += s_red[k][threadIdx.x];
    if (s) atomicAdd(threadIdx.x == 0 ? count : unmatched, s);
  }
}

// ---- host side -------------------------------------------------------------------------------------------------------------------
static inline int surface_sizes_ok(const char* fn, int n, int z, int y, int x) {
  if (n <= 0 || z <= 0 || y <= 0 || x <= 0) RX_FAIL(RX_EINVAL, "%s: sizes must be positive (got n=%d z=%d y=%d x=%d)", fn, n, z, y, x);
  if (z > RX_EDT_MAX_EXTENT || y > RX_EDT_MAX_EXTENT || x > RX_EDT_MAX_EXTENT)
    RX_FAIL(RX_EINVAL, "%s: an extent above %d (got z=%d y=%d x=%d)", fn, RX_EDT_MAX_EXTENT, z, y, x);
  return RX_OK;
}

extern "C" int rx_mask_edges(const void* values, int dtype, float threshold, int n, int z, int y, int x, uint8_t* edges, void* stream) {
  if (!values) RX_FAIL(RX_EINVAL, "rx_mask_edges: null input pointer");
  if (!edges) RX_FAIL(RX_EINVAL, "rx_mask_edges: null output pointer");
  if (int rc = surface_sizes_ok("rx_mask_edges", n, z, y, x)) return rc;
  if (n > 65535) RX_FAIL(RX_EINVAL, "rx_mask_edges: at most 65535 volumes in a call (got %d)", n);
  if (dtype != RX_F32 && dtype != RX_BF16 && dtype != RX_F16) RX_FAIL(RX_EINVAL, "rx_mask_edges: unknown dtype %d (RX_F32, RX_BF16 or RX_F16)", dtype);
  if (((uintptr_t)values & (uintptr_t)(rx_dtype_size(dtype) - 1)) != 0)
    RX_FAIL(RX_EINVAL, "rx_mask_edges: the values must be aligned to their %zu-byte element", rx_dtype_size(dtype));
  if (threshold != threshold) RX_FAIL(RX_EINVAL, "rx_mask_edges: the threshold is NaN");
  const long v = (long)z * y * x;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)((v + RX_SF_BLOCK - 1) / RX_SF_BLOCK), (unsigned)n), block(RX_SF_BLOCK);
  RX_DISPATCH_DTYPE(dtype, T, hipLaunchKernelGGL(mask_edges_kernel<T>, grid, block, 0, st, (const T*)values, threshold, z, y, x, edges));
  RX_CHECK_LAUNCH("rx_mask_edges");
  return RX_OK;
}

// XT = lines per tile of a line pass: a power of two, at most a wave wide, within the LDS budget, no wider than `inner` needs
static inline int edt_xt_log2(int L, long inner) {
  int lg = 6;
  while (lg > 0 && ((long)L << lg) > RX_EDT_TILE_WORDS) --lg;      // L <= 1024: stops at 16 lines or more
  while (lg > 0 && (1L << (lg - 1)) >= inner) --lg;
  return lg;
}

extern "C" int rx_edt_sq(const uint8_t* feature, int n, int z, int y, int x, int32_t* dist, void* stream) {
  if (!feature) RX_FAIL(RX_EINVAL, "rx_edt_sq: null input pointer");
  if (!dist) RX_FAIL(RX_EINVAL, "rx_edt_sq: null output pointer");
  if (int rc = surface_sizes_ok("rx_edt_sq", n, z, y, x)) return rc;
  if (((uintptr_t)dist & 3) != 0) RX_FAIL(RX_EINVAL, "rx_edt_sq: dist must be 4-byte aligned");
  if ((const void*)feature == (const void*)dist) RX_FAIL(RX_EINVAL, "rx_edt_sq: feature and dist must be different buffers");
  hipStream_t st = (hipStream_t)stream;
  const dim3 block(RX_SF_BLOCK);
  // the three grids, all checked before the first launch
  const long rows = (long)n * z * y;
  const int rpb = RX_EDT_ROW_WORDS / x;      // >= 4
  const long grid_x = (rows + rpb - 1) / rpb;
  const int lg_y = edt_xt_log2(y, x), lg_z = edt_xt_log2(z, (long)y * x);
  const long tiles_y = ((long)x + (1L << lg_y) - 1) >> lg_y, tiles_z = ((long)y * x + (1L << lg_z) - 1) >> lg_z;
  const long grid_y = (long)n * z * tiles_y, grid_z = (long)n * tiles_z;
  if (grid_x > 0x7fffffffL || grid_y > 0x7fffffffL || grid_z > 0x7fffffffL)
    RX_FAIL(RX_EINVAL, "rx_edt_sq: %d volumes of %d x %d x %d are more than one call's grid covers", n, z, y, x);
  hipLaunchKernelGGL(edt_x_kernel, dim3((unsigned)grid_x), block, (size_t)rpb * x * sizeof(int), st, feature, dist, rows, x, rpb);
  RX_CHECK_LAUNCH("rx_edt_sq");
  hipLaunchKernelGGL(edt_line_kernel, dim3((unsigned)grid_y), block, ((size_t)y << lg_y) * sizeof(int), st, dist, y, (long)x, (int)tiles_y,
                     lg_y);
  RX_CHECK_LAUNCH("rx_edt_sq");
  hipLaunchKernelGGL(edt_line_kernel, dim3((unsigned)grid_z), block, ((size_t)z << lg_z) * sizeof(int), st, dist, z, (long)y * x,
                     (int)tiles_z, lg_z);
  RX_CHECK_LAUNCH("rx_edt_sq");
  return RX_OK;
}

extern "C" int rx_surface_hist(const uint8_t* edges, const int32_t* dist, long total, long bins, int64_t* hist, int64_t* count,
                               int64_t* unmatched, void* stream) {
  if (!edges || !dist) RX_FAIL(RX_EINVAL, "rx_surface_hist: null input pointer");
  if (!hist || !count || !unmatched) RX_FAIL(RX_EINVAL, "rx_surface_hist: null output pointer");
  if (total <= 0 || bins <= 0) RX_FAIL(RX_EINVAL, "rx_surface_hist: sizes must be positive (got total=%ld bins=%ld)", total, bins);
  if (((uintptr_t)dist & 3) != 0 || ((uintptr_t)hist & 7) != 0 || ((uintptr_t)count & 7) != 0 || ((uintptr_t)unmatched & 7) != 0)
    RX_FAIL(RX_EINVAL, "rx_surface_hist: dist must be 4-byte, hist, count and unmatched 8-byte aligned");
  const long grid = (total + RX_SF_CHUNK - 1) / RX_SF_CHUNK;
  if (grid > 0x7fffffffL) RX_FAIL(RX_EINVAL, "rx_surface_hist: %ld voxels are more than one call's grid covers", total);
  hipLaunchKernelGGL(surface_hist_kernel, dim3((unsigned)grid), dim3(RX_SF_BLOCK), 0, (hipStream_t)stream, edges, dist, total, bins,
                     (unsigned long long*)hist, (unsigned long long*)count, (unsigned long long*)unmatched);
  RX_CHECK_LAUNCH("rx_surface_hist");
  return RX_OK;
}
