// rx_meshsample.hip -- orientation of an indexed triangle mesh against a sampled vector field, on the device (host side
// postprocess/orient.py, whose sample_points_numpy, unit_numpy, face_cos_numpy and side_numpy are the statements).  The per-vertex
// and per-triangle work is rx_meshsample_core.h (shared with the host check); this file holds the kernels and the entry points.
// Contraction is off and denormals are kept, so every value is the statement's float32, bit for bit.  There is no atomic here: a
// thread writes its own vertex or triangle, and `used` receives plain stores of the constant 1.  The prefix sums and the emit pass
// that follow are rx_mesh_scan (rx_meshrefine.hip) and rx_mesh_cluster_emit (rx_meshdecimate.hip) under the identity map.
//
//   msp_sample_kernel     a thread per vertex, all C channels: the clamped indices once, per channel the four x-pairs, the decode
//                        and the seven lerps; with `unit` the three values are normalised before the store.  A vertex whose two
//                        z planes are not both in the slab is left alone, so successive slab launches fill one (V, C) buffer.
//                        These are gathers: the mesher numbers vertices in ascending cell index, so the threads of a wave read
//                        neighbouring lines; per vertex 12 bytes in, 4 C out and 8 C values of the volume, mostly from cache.
//   msp_face_cos_kernel   a thread per triangle: cos, side, the keep flag (side == want, or every triangle where want is 0), and
//                        used[v] = 1 for the corners of a kept triangle.
//   msp_mark_kernel       a thread per triangle: used[v] = 1 for the corners of a triangle whose keep flag is set.
#include "rx_common.h"
#include "rx_meshsample_core.h"
#include "rx_mesh_host.h"

#pragma clang fp contract(off)

template <int RULE, typename T>
__global__ __launch_bounds__(RX_MESH_BLOCK) void msp_sample_kernel(const T* __restrict__ vol, int C, int z_base, int z_depth, int z_total, int Y, int X,
                                                                const float* __restrict__ points, long long V, int unit, float* __restrict__ out) {
  RX_MESH_THREAD(v, V);
  const float p[3] = {points[3 * v], points[3 * v + 1], points[3 * v + 2]};
  msp_sample_point<RULE, T>(vol, C, z_base, z_depth, z_total, Y, X, p, unit != 0, out + v * C);
}

__global__ __launch_bounds__(RX_MESH_BLOCK) void msp_face_cos_kernel(const float* __restrict__ pos, const float* __restrict__ vec, long long V,
                                                                  const long long* __restrict__ tri, long long T, float min_cos, int want,
                                                                  float* __restrict__ cos_out, signed char* __restrict__ side_out,
                                                                  int* __restrict__ keep, int* __restrict__ used, int* __restrict__ flag) {
  RX_MESH_THREAD(t, T);
  const int64_t id[3] = {tri[3 * t], tri[3 * t + 1], tri[3 * t + 2]};
  if (!mr_triangle_ok(id, V)) {      // never followed: the triangle is rim, and the caller refuses the mesh
    atomicOr(flag, 4);
    cos_out[t] = nanf(""), side_out[t] = 0, keep[t] = 0;
    return;
  }
  const float c = msp_face_cos(pos + 3 * id[0], pos + 3 * id[1], pos + 3 * id[2], vec + 3 * id[0], vec + 3 * id[1], vec + 3 * id[2]);
  const int s = msp_side(c, min_cos);
  const int k = want == 0 || s == want;
  cos_out[t] = c, side_out[t] = (signed char)s, keep[t] = k;
  if (k) used[id[0]] = 1, used[id[1]] = 1, used[id[2]] = 1;      // every writer stores the same value
}

__global__ __launch_bounds__(RX_MESH_BLOCK) void msp_mark_kernel(const long long* __restrict__ tri, long long T, long long V, const int* __restrict__ keep,
                                                              int* __restrict__ used, int* __restrict__ flag) {
  RX_MESH_THREAD(t, T);
  if (!keep[t]) return;
  const int64_t id[3] = {tri[3 * t], tri[3 * t + 1], tri[3 * t + 2]};
  if (!mr_triangle_ok(id, V)) {
    atomicOr(flag, 4);
    return;
  }
  used[id[0]] = 1, used[id[1]] = 1, used[id[2]] = 1;
}

// ---- host side --------------------------------------------------------------------------------------------------------------------------------
extern "C" int rx_mesh_sample(const void* volume, int rule, int channels, int z_base, int z_depth, int z_total, int y, int x, const float* points,
                              int64_t n_points, int unit, float* out, void* stream) {
  const char* fn = "rx_mesh_sample";
  if (!volume || !points) RX_FAIL(RX_EINVAL, "%s: null input pointer", fn);
  if (!out) RX_FAIL(RX_EINVAL, "%s: null output pointer", fn);
  if (rule < RX_MSP_COPY || rule > RX_MSP_NORMAL_U16) RX_FAIL(RX_EINVAL, "%s: rule %d (0 copy, 1 u8, 2 u16, 3 normal_u16)", fn, rule);
  if (channels < 1 || channels > RX_MSP_MAX_CHANNELS) RX_FAIL(RX_EINVAL, "%s: %d channels (1 .. %d)", fn, channels, RX_MSP_MAX_CHANNELS);
  if (unit != 0 && channels != 3) RX_FAIL(RX_EINVAL, "%s: unit needs 3 channels, got %d", fn, channels);
  if (y < 1 || x < 1 || z_total < 1 || y > RX_MSP_MAX_EXTENT || x > RX_MSP_MAX_EXTENT || z_total > RX_MSP_MAX_EXTENT)
    RX_FAIL(RX_EINVAL, "%s: extents %d x %d x %d (1 .. 2^24 - 2 each)", fn, z_total, y, x);
  if (z_base < 0 || z_depth < 1 || z_depth > z_total - z_base)
    RX_FAIL(RX_EINVAL, "%s: slab planes %d .. %d + %d do not lie inside the %d planes of the volume", fn, z_base, z_base, z_depth, z_total);
  if (int rc = rx_mesh_range_ok(fn, n_points, 1, RX_MESH_MAX_VERTICES, "points (1 .. 2^31 - 2)")) return rc;
  const int width = rule == RX_MSP_COPY ? 4 : (rule == RX_MSP_U8 ? 1 : 2);
  if (!RX_MESH_ALIGNED(volume, width) || !RX_MESH_ALIGNED(points, 4) || !RX_MESH_ALIGNED(out, 4)) RX_FAIL(RX_EINVAL, "%s: misaligned pointer", fn);
#define MSP_SAMPLE(RULE, T)                                                                                                                  \
  RX_MESH_LAUNCH(fn, (msp_sample_kernel<RULE, T>), n_points, stream, (const T*)volume, channels, z_base, z_depth, z_total, y, x, points, \
            (long long)n_points, unit, out)
  switch (rule) {
    case RX_MSP_COPY: MSP_SAMPLE(RX_MSP_COPY, float); break;
    case RX_MSP_U8: MSP_SAMPLE(RX_MSP_U8, uint8_t); break;
    case RX_MSP_U16: MSP_SAMPLE(RX_MSP_U16, uint16_t); break;
    default: MSP_SAMPLE(RX_MSP_NORMAL_U16, uint16_t); break;
  }
#undef MSP_SAMPLE
  return RX_OK;
}

extern "C" int rx_mesh_face_cos(const float* vertices, const float* vectors, int64_t n_vertices, const int64_t* triangles, int64_t n_triangles,
                                float min_cos, int want, float* cos, int8_t* side, int32_t* keep, int32_t* used, int32_t* flag, void* stream) {
  const char* fn = "rx_mesh_face_cos";
  if (!vertices || !vectors || !triangles) RX_FAIL(RX_EINVAL, "%s: null input pointer", fn);
  if (!cos || !side || !keep || !used || !flag) RX_FAIL(RX_EINVAL, "%s: null output pointer", fn);
  if (int rc = rx_mesh_range_ok(fn, n_vertices, 1, RX_MESH_MAX_VERTICES, "vertices (1 .. 2^31 - 2)")) return rc;
  if (int rc = rx_mesh_range_ok(fn, n_triangles, 1, RX_MESH_MAX_TRIANGLES, "triangles (1 .. (2^31 - 2) / 3)")) return rc;
  if (!(min_cos >= 0.0f && min_cos < 1.0f)) RX_FAIL(RX_EINVAL, "%s: min_cos must lie in [0, 1)", fn);
  if (want < -1 || want > 1) RX_FAIL(RX_EINVAL, "%s: want %d (1 front, -1 back, 0 every triangle)", fn, want);
  if (!RX_MESH_ALIGNED(vertices, 4) || !RX_MESH_ALIGNED(vectors, 4) || !RX_MESH_ALIGNED(triangles, 8) || !RX_MESH_ALIGNED(cos, 4) || !RX_MESH_ALIGNED(keep, 4) ||
      !RX_MESH_ALIGNED(used, 4) || !RX_MESH_ALIGNED(flag, 4))
    RX_FAIL(RX_EINVAL, "%s: misaligned pointer", fn);
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(used, 0, (size_t)n_vertices * 4, st) != hipSuccess) RX_FAIL(RX_ELAUNCH, "%s: clearing the used flags failed", fn);
  RX_MESH_LAUNCH(fn, msp_face_cos_kernel, n_triangles, st, vertices, vectors, (long long)n_vertices, (const long long*)triangles, (long long)n_triangles,
            min_cos, want, cos, (signed char*)side, keep, used, flag);
  return RX_OK;
}

extern "C" int rx_mesh_select_mark(const int64_t* triangles, int64_t n_triangles, int64_t n_vertices, const int32_t* keep, int32_t* used, int32_t* flag,
                                   void* stream) {
  const char* fn = "rx_mesh_select_mark";
  if (!triangles || !keep) RX_FAIL(RX_EINVAL, "%s: null input pointer", fn);
  if (!used || !flag) RX_FAIL(RX_EINVAL, "%s: null output pointer", fn);
  if (int rc = rx_mesh_range_ok(fn, n_vertices, 1, RX_MESH_MAX_VERTICES, "vertices (1 .. 2^31 - 2)")) return rc;
  if (int rc = rx_mesh_range_ok(fn, n_triangles, 1, RX_MESH_MAX_TRIANGLES, "triangles (1 .. (2^31 - 2) / 3)")) return rc;
  if (!RX_MESH_ALIGNED(triangles, 8) || !RX_MESH_ALIGNED(keep, 4) || !RX_MESH_ALIGNED(used, 4) || !RX_MESH_ALIGNED(flag, 4)) RX_FAIL(RX_EINVAL, "%s: misaligned pointer", fn);
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(used, 0, (size_t)n_vertices * 4, st) != hipSuccess) RX_FAIL(RX_ELAUNCH, "%s: clearing the used flags failed", fn);
  RX_MESH_LAUNCH(fn, msp_mark_kernel, n_triangles, st, (const long long*)triangles, (long long)n_triangles, (long long)n_vertices, keep, used, flag);
  return RX_OK;
}
