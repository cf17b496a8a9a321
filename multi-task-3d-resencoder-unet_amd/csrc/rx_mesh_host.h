// rx_mesh_host.h -- the one launch path of the mesh post-processing files (rx_meshrefine.hip, rx_meshdecimate.hip, rx_meshsample.hip):
// a thread per vertex, per triangle or per cluster in workgroups of RX_MESH_BLOCK, the pointer alignment test, the launch with its
// error check, and the count checks of the entry points.  The scan kernels of rx_meshrefine.hip keep a geometry of their own.
#pragma once
#include "rx_common.h"

#define RX_MESH_BLOCK 256

static inline unsigned rx_mesh_blocks(long long n) { return (unsigned)((n + RX_MESH_BLOCK - 1) / RX_MESH_BLOCK); }      // n <= 2^31 - 2

// first statement of a kernel launched by RX_MESH_LAUNCH over n items: this thread's item i, or nothing to do
#define RX_MESH_THREAD(i, n)                                                     \
  const long long i = (long long)blockIdx.x * RX_MESH_BLOCK + threadIdx.x;       \
  if (i >= (n)) return

#define RX_MESH_ALIGNED(p, a) ((((uintptr_t)(p)) & ((a) - 1)) == 0)

// one thread per item of n, RX_MESH_BLOCK threads per workgroup, no LDS, on stream st; a failed launch returns RX_ELAUNCH from fn
#define RX_MESH_LAUNCH(fn, kernel, n, st, ...)                                                                   \
  do {                                                                                                           \
    hipLaunchKernelGGL(kernel, dim3(rx_mesh_blocks(n)), dim3(RX_MESH_BLOCK), 0, (hipStream_t)(st), __VA_ARGS__); \
    RX_CHECK_LAUNCH(fn);                                                                                         \
  } while (0)

// ---- count checks -------------------------------------------------------------------------------------------------------------------------------
// n in [lo, hi], refused as "<fn>: <n> <what>", where `what` names the items and states the range
static inline int rx_mesh_range_ok(const char* fn, int64_t n, int64_t lo, int64_t hi, const char* what) {
  if (n < lo || n > hi) RX_FAIL(RX_EINVAL, "%s: %lld %s", fn, (long long)n, what);
  return RX_OK;
}

// the refinement's: at least one vertex, any number of triangles
static inline int rx_mesh_sizes_ok(const char* fn, int64_t V, int64_t T) {
  if (int rc = rx_mesh_range_ok(fn, V, 1, RX_MESH_MAX_VERTICES, "vertices (1 .. 2^31 - 2: ids are int32)")) return rc;
  return rx_mesh_range_ok(fn, T, 0, RX_MESH_MAX_TRIANGLES, "triangles (0 .. (2^31 - 2) / 3: a vertex's corners are counted in int32)");
}

// the decimation's: the range in numbers, since a cluster count is bounded by the vertex count of the call
static inline int rx_mesh_count_ok(const char* fn, const char* what, int64_t n, int64_t lo, int64_t hi) {
  if (n < lo || n > hi) RX_FAIL(RX_EINVAL, "%s: %lld %s (%lld .. %lld)", fn, (long long)n, what, (long long)lo, (long long)hi);
  return RX_OK;
}
#define RX_MESH_VERTICES(fn, V) if (int rc = rx_mesh_count_ok(fn, "vertices", V, 1, RX_MESH_MAX_VERTICES)) return rc
#define RX_MESH_CLUSTERS(fn, C, V) if (int rc = rx_mesh_count_ok(fn, "clusters", C, 1, V)) return rc
#define RX_MESH_TRIANGLES(fn, T) if (int rc = rx_mesh_count_ok(fn, "triangles", T, 1, RX_MESH_MAX_TRIANGLES)) return rc
