// rx_meshrefine.hip -- refinement of an indexed triangle mesh on the device: a canonical vertex adjacency, Taubin smoothing passes
// and area-weighted vertex normals (host side postprocess/refine.py, whose adjacency_numpy, smooth_numpy and vertex_normals_numpy
// are the statements).  The per-corner, per-vertex and per-face work is rx_meshrefine_core.h (shared with the host check); this
// file holds the kernels and the entry points.  Contraction is off and denormals are kept, so a position or a normal is the
// statement's float32, bit for bit.  There is no float atomic anywhere.
//
//   mesh_count_kernel      a thread per triangle: an id outside [0, V) raises the flag and drops the triangle; else one integer
//                          atomic add per corner into its vertex's count.
//   mesh_scan_*            exclusive prefix sums of an int32 column in int64, n + 1 results (the last is the total): 1024 values per
//                          workgroup on their own, the workgroup totals by one workgroup (each base lands in its group's first
//                          word), the base added to the rest.  Integers only.
//   mesh_fill_kernel       a thread per triangle: each corner takes the next slot of its vertex (an integer atomic on the vertex's
//                          cursor) and stores its triangle and its two edge partners there.  Arrival order chooses the slot.
//   mesh_canonical_kernel  a thread per vertex: heap sort of its triangle list and of its partner list in place, boundary flag from
//                          the multiplicities, duplicates and the vertex itself removed (mr_canonical).  Any degree: a list lives
//                          in global memory, not in registers or LDS.  After it nothing of the arrival order is left.
//   mesh_compact_kernel    a thread per vertex copies its distinct neighbours to the compact CSR at the second scan's offsets.
//   mesh_smooth_kernel     a thread per vertex, one launch per pass: gathers the neighbours' positions in list order from the
//                          pass's input buffer, writes the output buffer (mr_smooth_vertex).
//   mesh_face_kernel       a thread per triangle: its face vector, stored.
//   mesh_normal_kernel     a thread per vertex: gathers the stored face vectors over its sorted triangle list (mr_vertex_normal).
#include "rx_common.h"
#include "rx_meshrefine_core.h"
#include "rx_mesh_host.h"

#pragma clang fp contract(off)

#define RX_MR_SCAN_PER 4
#define RX_MR_SCAN_GROUP (RX_MESH_BLOCK * RX_MR_SCAN_PER)      // values scanned by one workgroup
#define RX_MR_SCAN_TOP 1024                                    // threads of the workgroup that scans the group totals

// ---- adjacency ------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(RX_MESH_BLOCK) void mesh_count_kernel(const long long* __restrict__ tri, long long T, long long V,
                                                                 int* __restrict__ counts, int* __restrict__ flag) {
  const long long t = (long long)blockIdx.x * RX_MESH_BLOCK + threadIdx.x;
  if (t >= T) return;
  const int64_t id[3] = {tri[3 * t], tri[3 * t + 1], tri[3 * t + 2]};
  if (!mr_triangle_ok(id, V)) {
    atomicOr(flag, 1);
    return;
  }
  for (int k = 0; k < 3; ++k) atomicAdd(&counts[id[k]], 1);
}

// exclusive scan of one value per thread over a workgroup of NW waves; `total` gets the workgroup's sum
template <int NW>
__device__ __forceinline__ long long mr_block_scan(long long x, long long* s_w, long long* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  long long inc = x;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const long long v = __shfl_up(inc, o, 64);
    if (lane >= o) inc += v;
  }
  __syncthreads();      // s_w may still be read from the call before
  if (lane == 63) s_w[wave] = inc;
  __syncthreads();
  long long base = 0, sum = 0;
#pragma unroll
  for (int w = 0; w < NW; ++w) {
    if (w < wave) base += s_w[w];
    sum += s_w[w];
  }
  *total = sum;
  return base + inc - x;
}

__global__ __launch_bounds__(RX_MESH_BLOCK) void mesh_scan_local_kernel(const int* __restrict__ counts, long long n, long long* __restrict__ offs) {
  __shared__ long long s_w[RX_MESH_BLOCK / 64];
  const long long r0 = (long long)blockIdx.x * RX_MR_SCAN_GROUP + (long long)threadIdx.x * RX_MR_SCAN_PER;
  long long c[RX_MR_SCAN_PER], sum = 0, total;
#pragma unroll
  for (int e = 0; e < RX_MR_SCAN_PER; ++e) {
    c[e] = r0 + e < n ? (long long)counts[r0 + e] : 0;
    sum += c[e];
  }
  long long at = mr_block_scan<RX_MESH_BLOCK / 64>(sum, s_w, &total);
#pragma unroll
  for (int e = 0; e < RX_MR_SCAN_PER; ++e) {
    if (r0 + e < n) offs[r0 + e] = at;
    at += c[e];
  }
}

// one workgroup: group g's total is its last value's local offset + count; its base goes into its first word (local offset 0)
__global__ __launch_bounds__(RX_MR_SCAN_TOP) void mesh_scan_groups_kernel(const int* __restrict__ counts, long long n, long long groups,
                                                                          long long* offs) {
  __shared__ long long s_w[RX_MR_SCAN_TOP / 64];
  long long carry = 0;
  for (long long g0 = 0; g0 < groups; g0 += RX_MR_SCAN_TOP) {      // uniform trip count
    const long long g = g0 + threadIdx.x;
    long long t = 0, total;
    if (g < groups) {
      const long long last = (g + 1) * RX_MR_SCAN_GROUP < n ? (g + 1) * RX_MR_SCAN_GROUP - 1 : n - 1;
      t = offs[last] + counts[last];
    }
    const long long at = mr_block_scan<RX_MR_SCAN_TOP / 64>(t, s_w, &total);
    if (g < groups) offs[g * RX_MR_SCAN_GROUP] = carry + at;      // read above by this thread alone
    carry += total;
  }
  if (threadIdx.x == 0) offs[n] = carry;
}

__global__ __launch_bounds__(RX_MESH_BLOCK) void mesh_scan_add_kernel(long long n, long long* offs) {
  const long long r = (long long)blockIdx.x * RX_MESH_BLOCK + threadIdx.x;
  if (r >= n || r % RX_MR_SCAN_GROUP == 0) return;      // a group's first word holds the base and is only read here
  offs[r] += offs[r - r % RX_MR_SCAN_GROUP];
}

__global__ __launch_bounds__(RX_MESH_BLOCK) void mesh_fill_kernel(const long long* __restrict__ tri, long long T, long long V,
                                                                const long long* __restrict__ foff, int* __restrict__ cursor,
                                                                long long capacity, int* __restrict__ faces, int* __restrict__ raw) {
  const long long t = (long long)blockIdx.x * RX_MESH_BLOCK + threadIdx.x;
  if (t >= T) return;
  const int64_t id[3] = {tri[3 * t], tri[3 * t + 1], tri[3 * t + 2]};
  if (!mr_triangle_ok(id, V)) return;      // as the count pass: it has no slots
  for (int k = 0; k < 3; ++k) {
    const long long b = foff[id[k]], e = foff[id[k] + 1];
    const long long at = b + atomicAdd(&cursor[id[k]], 1);
    if (at < e) mr_fill_corner(id, k, t, at, capacity, faces, raw);      // at >= e: more corners than were counted -- not this mesh's scan
  }
}

__global__ __launch_bounds__(RX_MESH_BLOCK) void mesh_canonical_kernel(long long V, const long long* __restrict__ foff, long long capacity, int* faces,
                                                                     int* raw, int* __restrict__ degrees, unsigned char* __restrict__ boundary) {
  const long long v = (long long)blockIdx.x * RX_MESH_BLOCK + threadIdx.x;
  if (v >= V) return;
  long long b = foff[v], e = foff[v + 1];
  if (b < 0 || e > capacity || e < b) b = e = 0;      // not a scan of this mesh: the vertex gets nothing
  uint8_t open = 0;
  degrees[v] = mr_canonical((int32_t)v, faces + b, raw + 2 * b, e - b, &open);
  boundary[v] = open;
}

__global__ __launch_bounds__(RX_MESH_BLOCK) void mesh_compact_kernel(long long V, const long long* __restrict__ foff, const int* __restrict__ raw,
                                                                   long long raw_capacity, const long long* __restrict__ offs, long long capacity,
                                                                   int* __restrict__ nbr) {
  const long long v = (long long)blockIdx.x * RX_MESH_BLOCK + threadIdx.x;
  if (v >= V) return;
  const long long src = 2 * foff[v], dst = offs[v], n = offs[v + 1] - dst;
  if (src < 0 || dst < 0 || n < 0 || src + n > 2 * raw_capacity || dst + n > capacity) return;
  for (long long r = 0; r < n; ++r) nbr[dst + r] = raw[src + r];
}

// ---- smoothing and normals ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(RX_MESH_BLOCK) void mesh_check_kernel(const float* __restrict__ x, long long n, int* __restrict__ flag) {
  const long long i = (long long)blockIdx.x * RX_MESH_BLOCK + threadIdx.x;
  if (i < n && !(fabsf(x[i]) <= 3.402823466e38f)) atomicOr(flag, 1);      // a NaN compares false
}

__global__ __launch_bounds__(RX_MESH_BLOCK) void mesh_smooth_kernel(const float* __restrict__ pos, const float* __restrict__ p0, long long V,
                                                                  const long long* __restrict__ offs, const int* __restrict__ nbr, long long E,
                                                                  const unsigned char* __restrict__ boundary, float f, float c,
                                                                  float* __restrict__ out) {
  const long long v = (long long)blockIdx.x * RX_MESH_BLOCK + threadIdx.x;
  if (v >= V) return;
  float q[3];
  mr_smooth_vertex(v, pos, p0, V, (const int64_t*)offs, nbr, E, boundary && boundary[v], f, c, q);
  out[3 * v] = q[0], out[3 * v + 1] = q[1], out[3 * v + 2] = q[2];
}

__global__ __launch_bounds__(RX_MESH_BLOCK) void mesh_face_kernel(const float* __restrict__ pos, long long V, const long long* __restrict__ tri,
                                                                long long T, float* __restrict__ fvec) {
  const long long t = (long long)blockIdx.x * RX_MESH_BLOCK + threadIdx.x;
  if (t >= T) return;
  const int64_t id[3] = {tri[3 * t], tri[3 * t + 1], tri[3 * t + 2]};
  float n[3] = {0.0f, 0.0f, 0.0f};
  if (mr_triangle_ok(id, V)) mr_face_vector(pos + 3 * id[0], pos + 3 * id[1], pos + 3 * id[2], n);
  fvec[3 * t] = n[0], fvec[3 * t + 1] = n[1], fvec[3 * t + 2] = n[2];
}

__global__ __launch_bounds__(RX_MESH_BLOCK) void mesh_normal_kernel(long long V, const long long* __restrict__ foff, const int* __restrict__ faces,
                                                                  long long capacity, const float* __restrict__ fvec, long long T,
                                                                  float* __restrict__ normals) {
  const long long v = (long long)blockIdx.x * RX_MESH_BLOCK + threadIdx.x;
  if (v >= V) return;
  float n[3];
  mr_vertex_normal(v, (const int64_t*)foff, faces, capacity, fvec, T, n);
  normals[3 * v] = n[0], normals[3 * v + 1] = n[1], normals[3 * v + 2] = n[2];
}

// ---- host side ----------------------------------------------------------------------------------------------------------------------------------
extern "C" int rx_mesh_count(const int64_t* triangles, int64_t n_triangles, int64_t n_vertices, int32_t* counts, int32_t* flag, void* stream) {
  if (n_triangles > 0 && !triangles) RX_FAIL(RX_EINVAL, "rx_mesh_count: null input pointer");
  if (!counts || !flag) RX_FAIL(RX_EINVAL, "rx_mesh_count: null output pointer");
  if (int rc = rx_mesh_sizes_ok("rx_mesh_count", n_vertices, n_triangles)) return rc;
  if (!RX_MESH_ALIGNED(triangles, 8) || !RX_MESH_ALIGNED(counts, 4) || !RX_MESH_ALIGNED(flag, 4)) RX_FAIL(RX_EINVAL, "rx_mesh_count: misaligned pointer");
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(counts, 0, (size_t)n_vertices * 4, st) != hipSuccess) RX_FAIL(RX_ELAUNCH, "rx_mesh_count: clearing the counts failed");
  if (n_triangles == 0) return RX_OK;
  RX_MESH_LAUNCH("rx_mesh_count", mesh_count_kernel, n_triangles, st, (const long long*)triangles, (long long)n_triangles,
                     (long long)n_vertices, counts, flag);
  return RX_OK;
}

extern "C" int rx_mesh_scan(const int32_t* counts, int64_t n, int64_t* offsets, void* stream) {
  if (!counts) RX_FAIL(RX_EINVAL, "rx_mesh_scan: null input pointer");
  if (!offsets) RX_FAIL(RX_EINVAL, "rx_mesh_scan: null output pointer");
  if (n <= 0 || n > RX_MESH_MAX_VERTICES) RX_FAIL(RX_EINVAL, "rx_mesh_scan: %lld values (1 .. 2^31 - 2)", (long long)n);
  if (!RX_MESH_ALIGNED(counts, 4) || !RX_MESH_ALIGNED(offsets, 8)) RX_FAIL(RX_EINVAL, "rx_mesh_scan: misaligned pointer");
  hipStream_t st = (hipStream_t)stream;
  const long long groups = (n + RX_MR_SCAN_GROUP - 1) / RX_MR_SCAN_GROUP;
  hipLaunchKernelGGL(mesh_scan_local_kernel, dim3((unsigned)groups), dim3(RX_MESH_BLOCK), 0, st, counts, (long long)n, (long long*)offsets);
  RX_CHECK_LAUNCH("rx_mesh_scan");
  hipLaunchKernelGGL(mesh_scan_groups_kernel, dim3(1), dim3(RX_MR_SCAN_TOP), 0, st, counts, (long long)n, groups, (long long*)offsets);
  RX_CHECK_LAUNCH("rx_mesh_scan");
  if (groups > 1) {
    RX_MESH_LAUNCH("rx_mesh_scan", mesh_scan_add_kernel, n, st, (long long)n, (long long*)offsets);
  }
  return RX_OK;
}

extern "C" int rx_mesh_fill(const int64_t* triangles, int64_t n_triangles, int64_t n_vertices, const int64_t* face_offsets, int32_t* cursor,
                            int64_t capacity, int32_t* faces, int32_t* raw, void* stream) {
  if ((n_triangles > 0 && !triangles) || !face_offsets) RX_FAIL(RX_EINVAL, "rx_mesh_fill: null input pointer");
  if (!cursor || (capacity > 0 && (!faces || !raw))) RX_FAIL(RX_EINVAL, "rx_mesh_fill: null output pointer");
  if (int rc = rx_mesh_sizes_ok("rx_mesh_fill", n_vertices, n_triangles)) return rc;
  if (capacity < 0 || capacity > 3 * RX_MESH_MAX_TRIANGLES) RX_FAIL(RX_EINVAL, "rx_mesh_fill: capacity %lld (0 .. 2^31 - 2 corner slots)", (long long)capacity);
  if (!RX_MESH_ALIGNED(triangles, 8) || !RX_MESH_ALIGNED(face_offsets, 8) || !RX_MESH_ALIGNED(cursor, 4) || !RX_MESH_ALIGNED(faces, 4) || !RX_MESH_ALIGNED(raw, 4))
    RX_FAIL(RX_EINVAL, "rx_mesh_fill: misaligned pointer");
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(cursor, 0, (size_t)n_vertices * 4, st) != hipSuccess) RX_FAIL(RX_ELAUNCH, "rx_mesh_fill: clearing the cursors failed");
  if (n_triangles == 0) return RX_OK;
  RX_MESH_LAUNCH("rx_mesh_fill", mesh_fill_kernel, n_triangles, st, (const long long*)triangles, (long long)n_triangles,
                     (long long)n_vertices, (const long long*)face_offsets, cursor, (long long)capacity, faces, raw);
  return RX_OK;
}

extern "C" int rx_mesh_canonical(int64_t n_vertices, const int64_t* face_offsets, int64_t capacity, int32_t* faces, int32_t* raw, int32_t* degrees,
                                 uint8_t* boundary, void* stream) {
  if (!face_offsets) RX_FAIL(RX_EINVAL, "rx_mesh_canonical: null input pointer");
  if (!degrees || !boundary || (capacity > 0 && (!faces || !raw))) RX_FAIL(RX_EINVAL, "rx_mesh_canonical: null output pointer");
  if (int rc = rx_mesh_sizes_ok("rx_mesh_canonical", n_vertices, 0)) return rc;
  if (capacity < 0 || capacity > 3 * RX_MESH_MAX_TRIANGLES)
    RX_FAIL(RX_EINVAL, "rx_mesh_canonical: capacity %lld (0 .. 2^31 - 2 corner slots)", (long long)capacity);
  if (!RX_MESH_ALIGNED(face_offsets, 8) || !RX_MESH_ALIGNED(faces, 4) || !RX_MESH_ALIGNED(raw, 4) || !RX_MESH_ALIGNED(degrees, 4))
    RX_FAIL(RX_EINVAL, "rx_mesh_canonical: misaligned pointer");
  RX_MESH_LAUNCH("rx_mesh_canonical", mesh_canonical_kernel, n_vertices, stream, (long long)n_vertices,
                     (const long long*)face_offsets, (long long)capacity, faces, raw, degrees, boundary);
  return RX_OK;
}

extern "C" int rx_mesh_compact(int64_t n_vertices, const int64_t* face_offsets, const int32_t* raw, int64_t raw_capacity, const int64_t* offsets,
                               int64_t capacity, int32_t* neighbours, void* stream) {
  if (!face_offsets || !offsets || (raw_capacity > 0 && !raw)) RX_FAIL(RX_EINVAL, "rx_mesh_compact: null input pointer");
  if (capacity > 0 && !neighbours) RX_FAIL(RX_EINVAL, "rx_mesh_compact: null output pointer");
  if (int rc = rx_mesh_sizes_ok("rx_mesh_compact", n_vertices, 0)) return rc;
  if (capacity < 0 || raw_capacity < 0 || raw_capacity > 3 * RX_MESH_MAX_TRIANGLES) RX_FAIL(RX_EINVAL, "rx_mesh_compact: negative or oversized capacity");
  if (!RX_MESH_ALIGNED(face_offsets, 8) || !RX_MESH_ALIGNED(offsets, 8) || !RX_MESH_ALIGNED(raw, 4) || !RX_MESH_ALIGNED(neighbours, 4))
    RX_FAIL(RX_EINVAL, "rx_mesh_compact: misaligned pointer");
  if (capacity == 0) return RX_OK;      // nothing to write
  RX_MESH_LAUNCH("rx_mesh_compact", mesh_compact_kernel, n_vertices, stream, (long long)n_vertices,
                     (const long long*)face_offsets, raw, (long long)raw_capacity, (const long long*)offsets, (long long)capacity, neighbours);
  return RX_OK;
}

extern "C" int rx_mesh_check_vertices(const float* vertices, int64_t n_vertices, int32_t* flag, void* stream) {
  if (!vertices) RX_FAIL(RX_EINVAL, "rx_mesh_check_vertices: null input pointer");
  if (!flag) RX_FAIL(RX_EINVAL, "rx_mesh_check_vertices: null output pointer");
  if (int rc = rx_mesh_sizes_ok("rx_mesh_check_vertices", n_vertices, 0)) return rc;
  if (!RX_MESH_ALIGNED(vertices, 4) || !RX_MESH_ALIGNED(flag, 4)) RX_FAIL(RX_EINVAL, "rx_mesh_check_vertices: misaligned pointer");
  RX_MESH_LAUNCH("rx_mesh_check_vertices", mesh_check_kernel, 3 * n_vertices, stream, vertices, (long long)(3 * n_vertices),
                     flag);
  return RX_OK;
}

extern "C" int rx_mesh_smooth_pass(const float* positions, const float* origin, int64_t n_vertices, const int64_t* offsets, const int32_t* neighbours,
                                   int64_t n_neighbours, const uint8_t* boundary, float factor, float clamp, float* out, void* stream) {
  if (!positions || !offsets || (n_neighbours > 0 && !neighbours)) RX_FAIL(RX_EINVAL, "rx_mesh_smooth_pass: null input pointer");
  if (!out) RX_FAIL(RX_EINVAL, "rx_mesh_smooth_pass: null output pointer");
  if (out == positions) RX_FAIL(RX_EINVAL, "rx_mesh_smooth_pass: out must be another buffer than positions (a pass reads the positions before it)");
  if (int rc = rx_mesh_sizes_ok("rx_mesh_smooth_pass", n_vertices, 0)) return rc;
  if (n_neighbours < 0) RX_FAIL(RX_EINVAL, "rx_mesh_smooth_pass: negative n_neighbours");
  if (!(fabsf(factor) <= 3.402823466e38f)) RX_FAIL(RX_EINVAL, "rx_mesh_smooth_pass: factor is not finite");
  if (origin && !(clamp >= 0.0f && clamp <= 3.402823466e38f)) RX_FAIL(RX_EINVAL, "rx_mesh_smooth_pass: clamp must be finite and >= 0");
  if (!RX_MESH_ALIGNED(positions, 4) || !RX_MESH_ALIGNED(origin, 4) || !RX_MESH_ALIGNED(out, 4) || !RX_MESH_ALIGNED(offsets, 8) || !RX_MESH_ALIGNED(neighbours, 4))
    RX_FAIL(RX_EINVAL, "rx_mesh_smooth_pass: misaligned pointer");
  RX_MESH_LAUNCH("rx_mesh_smooth_pass", mesh_smooth_kernel, n_vertices, stream, positions, origin, (long long)n_vertices,
                     (const long long*)offsets, neighbours, (long long)n_neighbours, boundary, factor, clamp, out);
  return RX_OK;
}

extern "C" int rx_mesh_face_vectors(const float* vertices, int64_t n_vertices, const int64_t* triangles, int64_t n_triangles, float* face_vectors,
                                    void* stream) {
  if (!vertices || (n_triangles > 0 && !triangles)) RX_FAIL(RX_EINVAL, "rx_mesh_face_vectors: null input pointer");
  if (n_triangles > 0 && !face_vectors) RX_FAIL(RX_EINVAL, "rx_mesh_face_vectors: null output pointer");
  if (int rc = rx_mesh_sizes_ok("rx_mesh_face_vectors", n_vertices, n_triangles)) return rc;
  if (!RX_MESH_ALIGNED(vertices, 4) || !RX_MESH_ALIGNED(triangles, 8) || !RX_MESH_ALIGNED(face_vectors, 4)) RX_FAIL(RX_EINVAL, "rx_mesh_face_vectors: misaligned pointer");
  if (n_triangles == 0) return RX_OK;
  RX_MESH_LAUNCH("rx_mesh_face_vectors", mesh_face_kernel, n_triangles, stream, vertices, (long long)n_vertices,
                     (const long long*)triangles, (long long)n_triangles, face_vectors);
  return RX_OK;
}

extern "C" int rx_mesh_vertex_normals(int64_t n_vertices, const int64_t* face_offsets, const int32_t* faces, int64_t capacity, const float* face_vectors,
                                      int64_t n_triangles, float* normals, void* stream) {
  if (!face_offsets || (capacity > 0 && !faces) || (n_triangles > 0 && !face_vectors)) RX_FAIL(RX_EINVAL, "rx_mesh_vertex_normals: null input pointer");
  if (!normals) RX_FAIL(RX_EINVAL, "rx_mesh_vertex_normals: null output pointer");
  if (int rc = rx_mesh_sizes_ok("rx_mesh_vertex_normals", n_vertices, n_triangles)) return rc;
  if (capacity < 0) RX_FAIL(RX_EINVAL, "rx_mesh_vertex_normals: negative capacity");
  if (!RX_MESH_ALIGNED(face_offsets, 8) || !RX_MESH_ALIGNED(faces, 4) || !RX_MESH_ALIGNED(face_vectors, 4) || !RX_MESH_ALIGNED(normals, 4))
    RX_FAIL(RX_EINVAL, "rx_mesh_vertex_normals: misaligned pointer");
  RX_MESH_LAUNCH("rx_mesh_vertex_normals", mesh_normal_kernel, n_vertices, stream, (long long)n_vertices,
                     (const long long*)face_offsets, faces, (long long)capacity, face_vectors, (long long)n_triangles, normals);
  return RX_OK;
}
