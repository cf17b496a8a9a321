// rx_patchsearch.hip -- box statistics for the valid-patch search (reference helpers.py: _check_patch_chunk asks of every
// candidate patch np.count_nonzero(patch) and the bounding box of np.argwhere(patch > 0); find_label_bounding_box asks the same of
// the whole label).  Per box of a contiguous (Z, Y, X) volume of uint8, uint16 or float32:
//   count = the voxels != 0;   ext = (minz, maxz, miny, maxy, minx, maxx) of the voxels > 0, box-local, (dz, -1, dy, -1, dx, -1) if none.
// The host statement is dataloading/patch_search_device.py: box_stats_numpy.  Integers only: the float32 predicates are taken on
// the bit pattern u (v != 0  <=>  u & 0x7fffffff;  v > 0  <=>  1 <= u <= 0x7f800000: sign clear, not zero, not a NaN).
//
// Two launches behind one copy of the box table:
//   box_stats_init_kernel   count = 0 and the empty record, one lane per box.
//   box_stats_kernel<T>     a box is dz * dy x-rows in (z, y) order, cut into chunks of R rows (R is launch-wide: a box deeper
//                           than a chunk spans several workgroups, a plane wider than a chunk is cut along y too); workgroup
//                           b works on chunk b % bpb of box b / bpb and leaves at once if that box has no such chunk.  A row is
//                           a scalar head up to the first 16-byte boundary, 16-byte vectors, a scalar tail: `units` of work, and
//                           L = 2^k lanes (launch-wide, from the widest box) share a row, 256 / L rows in flight per workgroup,
//                           so 128-voxel rows and 33000-voxel rows both keep the lanes busy.  Nothing outside a box is read.
//                           Reduction: lane, wave (xor shuffles), workgroup (LDS), then ONE atomic per workgroup and output word
//                           -- 64-bit add, 32-bit min / max: order-free, so a launch is bit-reproducible.
// Every voxel offset is 64-bit; a box's row count is 64-bit too (one 64-bit division per lane, then (z, y) advance by a fixed step).
#include "rx_common.h"

#define RX_BOX_BLOCK 256
#define RX_BOX_WAVES (RX_BOX_BLOCK / 64)
#define RX_BOX_MIN_BYTES 4096       // a chunk holds at least this much of the widest box (small calls stay a handful of workgroups)
#define RX_BOX_TARGET_BLOCKS 8192   // ... and large calls are cut into about this many chunks (32 per CU)

template <typename T>
struct BoxElem;
template <>
struct BoxElem<uint8_t> {
  __device__ static inline bool nz(uint8_t v) { return v != 0; }
  __device__ static inline bool pos(uint8_t v) { return v != 0; }
  // 16 voxels: the nonzero count; lo / hi take the first / last element index that is > 0
  __device__ static inline int vec(const u32x4& v, int& lo, int& hi) {
    int c = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const uint32_t w = v[j], t = (w | ((w & 0x7f7f7f7fu) + 0x7f7f7f7fu)) & 0x80808080u;      // bit 7 of every nonzero byte
      if (t) {
        c += __popc(t);
        lo = min(lo, j * 4 + ((__ffs((int)t) - 1) >> 3));
        hi = max(hi, j * 4 + ((31 - __clz((int)t)) >> 3));
      }
    }
    return c;
  }
};
template <>
struct BoxElem<uint16_t> {
  __device__ static inline bool nz(uint16_t v) { return v != 0; }
  __device__ static inline bool pos(uint16_t v) { return v != 0; }
  __device__ static inline int vec(const u32x4& v, int& lo, int& hi) {
    int c = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const uint32_t w = v[j], t = (w | ((w & 0x7fff7fffu) + 0x7fff7fffu)) & 0x80008000u;      // bit 15 of every nonzero half
      if (t) {
        c += __popc(t);
        lo = min(lo, j * 2 + ((__ffs((int)t) - 1) >> 4));
        hi = max(hi, j * 2 + ((31 - __clz((int)t)) >> 4));
      }
    }
    return c;
  }
};
template <>
struct BoxElem<uint32_t> {      // float32 by its bits
  __device__ static inline bool nz(uint32_t u) { return (u & 0x7fffffffu) != 0; }
  __device__ static inline bool pos(uint32_t u) { return u - 1u < 0x7f800000u; }
  __device__ static inline int vec(const u32x4& v, int& lo, int& hi) {
    int c = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      c += nz(v[j]) ? 1 : 0;
      if (pos(v[j])) lo = min(lo, j), hi = max(hi, j);
    }
    return c;
  }
};

__global__ __launch_bounds__(RX_BOX_BLOCK) void box_stats_init_kernel(const int32_t* __restrict__ boxes, int n,
                                                                      unsigned long long* __restrict__ count, int32_t* __restrict__ ext) {
  const long i = (long)blockIdx.x * RX_BOX_BLOCK + threadIdx.x;
  if (i >= n) return;
  count[i] = 0ull;
  const int32_t* b = boxes + i * 6;
  int32_t* e = ext + i * 6;
  e[0] = b[3], e[1] = -1, e[2] = b[4], e[3] = -1, e[4] = b[5], e[5] = -1;
}

template <typename T>
__global__ __launch_bounds__(RX_BOX_BLOCK) void box_stats_kernel(const T* __restrict__ vol, long Y, long X, const int32_t* __restrict__ boxes,
                                                                 int bpb, long R, int lshift, unsigned long long* __restrict__ count,
                                                                 int32_t* __restrict__ ext) {
  constexpr int P = 16 / (int)sizeof(T);      // voxels per 16-byte vector
  __shared__ unsigned long long s_cnt[RX_BOX_WAVES];
  __shared__ int s_ext[RX_BOX_WAVES][6];
  const int box = (int)(blockIdx.x / (unsigned)bpb), chunk = (int)(blockIdx.x - (unsigned)box * (unsigned)bpb);
  const int32_t* __restrict__ b = boxes + (long)box * 6;
  const int z0 = b[0], y0 = b[1], x0 = b[2], dz = b[3], dy = b[4], dx = b[5];
  const long rows = (long)dz * dy, r0 = (long)chunk * R;
  if (r0 >= rows) return;      // the whole workgroup: this box has fewer chunks than the largest of the call
  const long r1 = r0 + R < rows ? r0 + R : rows;
  const int sub = threadIdx.x & ((1 << lshift) - 1), lanes = 1 << lshift, step = RX_BOX_BLOCK >> lshift;
  long r = r0 + (threadIdx.x >> lshift);
  int z = (int)(r / dy), y = (int)(r - (long)z * dy);
  const int step_z = step / dy, step_y = step - step_z * dy;
  unsigned long long cnt = 0;
  int minz = dz, maxz = -1, miny = dy, maxy = -1, minx = dx, maxx = -1;
  for (; r < r1; r += step) {
    const T* __restrict__ row = vol + ((long)(z0 + z) * Y + (y0 + y)) * X + x0;
    int h = (int)(((16u - (unsigned)((uintptr_t)row & 15u)) & 15u) / (unsigned)sizeof(T));      // voxels before the first 16-byte boundary
    h = h < dx ? h : dx;
    const int nvec = (dx - h) / P;
    int lo = dx, hi = -1, c = 0;
    for (int u = sub; u < nvec + 2; u += lanes) {      // unit 0: the head, 1 .. nvec: the vectors, nvec + 1: the tail
      if (u >= 1 && u <= nvec) {
        const int xb = h + (u - 1) * P;
        const u32x4 v = *reinterpret_cast<const u32x4*>(row + xb);
        int l = P, g = -1;
        c += BoxElem<T>::vec(v, l, g);
        if (g >= 0) lo = min(lo, xb + l), hi = max(hi, xb + g);
      } else {
        const int k0 = u == 0 ? 0 : h + nvec * P, k1 = u == 0 ? h : dx;
        for (int k = k0; k < k1; ++k) {
          const T v = row[k];
          c += BoxElem<T>::nz(v) ? 1 : 0;
          if (BoxElem<T>::pos(v)) lo = min(lo, k), hi = max(hi, k);
        }
      }
    }
    cnt += (unsigned)c;
    if (hi >= 0) {
      minx = min(minx, lo), maxx = max(maxx, hi);
      miny = min(miny, y), maxy = max(maxy, y);
      minz = min(minz, z), maxz = max(maxz, z);
    }
    z += step_z, y += step_y;
    if (y >= dy) y -= dy, ++z;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    cnt += __shfl_xor(cnt, o, 64);
    minz = min(minz, __shfl_xor(minz, o, 64)), maxz = max(maxz, __shfl_xor(maxz, o, 64));
    miny = min(miny, __shfl_xor(miny, o, 64)), maxy = max(maxy, __shfl_xor(maxy, o, 64));
    minx = min(minx, __shfl_xor(minx, o, 64)), maxx = max(maxx, __shfl_xor(maxx, o, 64));
  }
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    s_cnt[wave] = cnt;
    s_ext[wave][0] = minz, s_ext[wave][1] = maxz, s_ext[wave][2] = miny, s_ext[wave][3] = maxy, s_ext[wave][4] = minx, s_ext[wave][5] = maxx;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 1; w < RX_BOX_WAVES; ++w) {
      cnt += s_cnt[w];
      minz = min(minz, s_ext[w][0]), maxz = max(maxz, s_ext[w][1]);
      miny = min(miny, s_ext[w][2]), maxy = max(maxy, s_ext[w][3]);
      minx = min(minx, s_ext[w][4]), maxx = max(maxx, s_ext[w][5]);
    }
    if (cnt) atomicAdd(count + box, cnt);
    if (maxz >= 0) {
      int32_t* e = ext + (long)box * 6;
      atomicMin(e + 0, minz), atomicMax(e + 1, maxz);
      atomicMin(e + 2, miny), atomicMax(e + 3, maxy);
      atomicMin(e + 4, minx), atomicMax(e + 5, maxx);
    }
  }
}

// ---- host side -----------------------------------------------------------------------------------------------------------------
extern "C" size_t rx_box_stats_workspace(int n_boxes) {
  if (n_boxes <= 0) return 0;
  return rx_align_up((size_t)n_boxes * 6 * sizeof(int32_t), 16);
}

extern "C" int rx_box_stats(const void* vol, int dtype, int z, int y, int x, const int32_t* host_boxes, int n_boxes, void* workspace,
                            size_t workspace_bytes, uint64_t* count, int32_t* ext, void* stream) {
  if (!vol) RX_FAIL(RX_EINVAL, "rx_box_stats: null volume pointer");
  if (!host_boxes) RX_FAIL(RX_EINVAL, "rx_box_stats: null box table");
  if (!workspace) RX_FAIL(RX_EINVAL, "rx_box_stats: null workspace pointer");
  if (!count || !ext) RX_FAIL(RX_EINVAL, "rx_box_stats: null output pointer");
  if (dtype != RX_SW_U8 && dtype != RX_SW_U16 && dtype != RX_SW_F32)
    RX_FAIL(RX_EINVAL, "rx_box_stats: unknown dtype %d (RX_SW_U8, RX_SW_U16 or RX_SW_F32)", dtype);
  if (z <= 0 || y <= 0 || x <= 0) RX_FAIL(RX_EINVAL, "rx_box_stats: sizes must be positive (got %d x %d x %d)", z, y, x);
  if (n_boxes <= 0) RX_FAIL(RX_EINVAL, "rx_box_stats: n_boxes must be positive (got %d)", n_boxes);
  const int esize = dtype == RX_SW_U8 ? 1 : dtype == RX_SW_U16 ? 2 : 4;
  if (((uintptr_t)vol & (uintptr_t)(esize - 1)) != 0) RX_FAIL(RX_EINVAL, "rx_box_stats: the volume must be aligned to its %d-byte element", esize);
  if (((uintptr_t)workspace & 15) != 0) RX_FAIL(RX_EINVAL, "rx_box_stats: workspace must be 16-byte aligned");
  if (((uintptr_t)count & 7) != 0 || ((uintptr_t)ext & 3) != 0)
    RX_FAIL(RX_EINVAL, "rx_box_stats: count must be 8-byte and ext 4-byte aligned");
  long rows_max = 0, rows_total = 0;
  int dx_max = 0;
  for (long i = 0; i < n_boxes; ++i) {
    const int32_t* b = host_boxes + i * 6;
    if (b[3] <= 0 || b[4] <= 0 || b[5] <= 0)
      RX_FAIL(RX_EINVAL, "rx_box_stats: box %ld has a non-positive extent (%d x %d x %d)", i, b[3], b[4], b[5]);
    if (b[0] < 0 || b[1] < 0 || b[2] < 0 || (long)b[0] + b[3] > z || (long)b[1] + b[4] > y || (long)b[2] + b[5] > x)
      RX_FAIL(RX_EINVAL, "rx_box_stats: box %ld (%d, %d, %d) + (%d, %d, %d) leaves the %d x %d x %d volume", i, b[0], b[1], b[2], b[3],
              b[4], b[5], z, y, x);
    const long rows = (long)b[3] * b[4];
    rows_max = rows > rows_max ? rows : rows_max;
    rows_total += rows;
    dx_max = b[5] > dx_max ? b[5] : dx_max;
  }
  if (workspace_bytes < rx_box_stats_workspace(n_boxes))
    RX_FAIL(RX_EWORKSPACE, "rx_box_stats: workspace of %zu bytes, rx_box_stats_workspace says %zu", workspace_bytes,
            rx_box_stats_workspace(n_boxes));
  // rows per chunk: about RX_BOX_TARGET_BLOCKS chunks in all, none below RX_BOX_MIN_BYTES of the widest box, the grid below 2^31
  long R = (rows_total + RX_BOX_TARGET_BLOCKS - 1) / RX_BOX_TARGET_BLOCKS;
  const long r_min = (RX_BOX_MIN_BYTES + (long)dx_max * esize - 1) / ((long)dx_max * esize);
  R = R > r_min ? R : r_min;
  while ((rows_max + R - 1) / R * n_boxes > 0x7fffffffL) R *= 2;
  const int bpb = (int)((rows_max + R - 1) / R);
  const int units = dx_max / (16 / esize) + 2;
  int lshift = 0;
  while ((1 << lshift) < units && (1 << lshift) < RX_BOX_BLOCK) ++lshift;
  hipStream_t st = (hipStream_t)stream;
  int32_t* table = (int32_t*)workspace;
  const hipError_t e = hipMemcpyAsync(table, host_boxes, (size_t)n_boxes * 6 * sizeof(int32_t), hipMemcpyHostToDevice, st);
  if (e != hipSuccess) RX_FAIL(RX_ELAUNCH, "rx_box_stats: copying the box table: %s", hipGetErrorString(e));
  unsigned long long* cnt = (unsigned long long*)count;
  hipLaunchKernelGGL(box_stats_init_kernel, dim3((unsigned)((n_boxes + RX_BOX_BLOCK - 1) / RX_BOX_BLOCK)), dim3(RX_BOX_BLOCK), 0, st,
                     (const int32_t*)table, n_boxes, cnt, ext);
  RX_CHECK_LAUNCH("rx_box_stats");
  const dim3 grid((unsigned)((long)n_boxes * bpb)), block(RX_BOX_BLOCK);
  if (dtype == RX_SW_U8)
    hipLaunchKernelGGL(box_stats_kernel<uint8_t>, grid, block, 0, st, (const uint8_t*)vol, (long)y, (long)x, (const int32_t*)table, bpb, R,
                       lshift, cnt, ext);
  else if (dtype == RX_SW_U16)
    hipLaunchKernelGGL(box_stats_kernel<uint16_t>, grid, block, 0, st, (const uint16_t*)vol, (long)y, (long)x, (const int32_t*)table, bpb, R,
                       lshift, cnt, ext);
  else
    hipLaunchKernelGGL(box_stats_kernel<uint32_t>, grid, block, 0, st, (const uint32_t*)vol, (long)y, (long)x, (const int32_t*)table, bpb, R,
                       lshift, cnt, ext);
  RX_CHECK_LAUNCH("rx_box_stats");
  return RX_OK;
}
