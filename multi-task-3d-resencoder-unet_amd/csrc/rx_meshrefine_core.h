// rx_meshrefine_core.h -- the per-corner, per-vertex and per-face work of the mesh refinement passes (rx_meshrefine.hip), written so
// that it compiles for the host as well: csrc/tools/meshrefine_host_check.cpp runs exactly these functions serially against a direct
// restatement, under the address and undefined-behaviour sanitizers.  postprocess/refine.py (adjacency_numpy, smooth_numpy,
// vertex_normals_numpy) is the statement; every float32 operation here is one rounding (contraction is off, denormals are kept,
// / and sqrtf are correctly rounded: IEEE on the host, hipcc's default on the device).
//
// Storage: a vertex's triangle corners own consecutive SLOTS [face_offsets[v], face_offsets[v + 1]); slot s holds the corner's
// triangle in faces[s] and its two edge partners in raw[2 s], raw[2 s + 1].  Which corner gets which slot is decided by arrival;
// mr_canonical sorts both lists of a vertex, after which nothing of that order is left.  Ids are int32: at most
// RX_MESH_MAX_VERTICES vertices, and at most RX_MESH_MAX_TRIANGLES triangles so that a vertex's corner count fits as well.
#ifndef RX_MESHREFINE_CORE_H
#define RX_MESHREFINE_CORE_H
#include <math.h>
#include <stdint.h>

#pragma clang fp contract(off)

#if defined(__HIPCC__)
#define RX_MR_HD __host__ __device__ __forceinline__
#else
#define RX_MR_HD inline
#endif

#ifndef RX_MESH_MAX_VERTICES
#define RX_MESH_MAX_VERTICES 2147483646L      // 2^31 - 2 (include/rxunet.h says the same)
#define RX_MESH_MAX_TRIANGLES 715827882L      // (2^31 - 2) / 3: the corners of one vertex are counted in int32
#endif

// a triangle takes part only when all three ids name a vertex
RX_MR_HD bool mr_triangle_ok(const int64_t t[3], int64_t V) {
  return (uint64_t)t[0] < (uint64_t)V && (uint64_t)t[1] < (uint64_t)V && (uint64_t)t[2] < (uint64_t)V;
}

// corner k of triangle `tri` = (t[0], t[1], t[2]) takes slot `at` of its vertex; nothing is stored outside [0, capacity)
RX_MR_HD void mr_fill_corner(const int64_t t[3], int k, int64_t tri, int64_t at, int64_t capacity, int32_t* faces, int32_t* raw) {
  if (at < 0 || at >= capacity) return;
  faces[at] = (int32_t)tri;
  raw[2 * at] = (int32_t)t[(k + 1) % 3];
  raw[2 * at + 1] = (int32_t)t[(k + 2) % 3];
}

RX_MR_HD void mr_sift(int32_t* a, int64_t root, int64_t n) {
  const int32_t x = a[root];
  int64_t i = root;
  for (;;) {
    int64_t c = 2 * i + 1;
    if (c >= n) break;
    if (c + 1 < n && a[c + 1] > a[c]) ++c;
    if (a[c] <= x) break;
    a[i] = a[c];
    i = c;
  }
  a[i] = x;
}

// ascending, in place, any length: O(n log n) reads and writes of a[0 .. n)
RX_MR_HD void mr_heapsort(int32_t* a, int64_t n) {
  for (int64_t r = n / 2 - 1; r >= 0; --r) mr_sift(a, r, n);
  for (int64_t m = n - 1; m > 0; --m) {
    const int32_t top = a[0];
    a[0] = a[m];
    a[m] = top;
    mr_sift(a, 0, m);
  }
}

// Vertex v with n corner slots: faces[0 .. n) and raw[0 .. 2n) are its own.  Sorts both ascending; the distinct partners other than
// v itself move to raw[0 .. degree); *boundary = some partner appears exactly once (an edge at v used by exactly one triangle edge).
RX_MR_HD int32_t mr_canonical(int32_t v, int32_t* faces, int32_t* raw, int64_t n, uint8_t* boundary) {
  mr_heapsort(faces, n);
  mr_heapsort(raw, 2 * n);
  int64_t w = 0;
  uint8_t open = 0;
  for (int64_t i = 0; i < 2 * n;) {
    const int32_t u = raw[i];
    int64_t j = i + 1;
    while (j < 2 * n && raw[j] == u) ++j;
    if (u != v) {
      if (j - i == 1) open = 1;
      raw[w++] = u;      // w <= i: a slot already read
    }
    i = j;
  }
  *boundary = open;
  return (int32_t)w;      // at most V - 1
}

// One Jacobi pass at vertex v: q = p + f * (mean of the neighbours - p), clamped to p0 +- c where p0 is given.  offsets / nbr: the
// compact adjacency with E entries; `pinned`: the vertex keeps its position.  An entry outside [0, V) is skipped, never followed.
RX_MR_HD void mr_smooth_vertex(int64_t v, const float* pos, const float* p0, int64_t V, const int64_t* offsets, const int32_t* nbr, int64_t E,
                               bool pinned, float f, float c, float q[3]) {
  const float p[3] = {pos[3 * v], pos[3 * v + 1], pos[3 * v + 2]};
  int64_t b = offsets[v], e = offsets[v + 1];
  if (b < 0) b = 0;
  if (e > E) e = E;
  q[0] = p[0], q[1] = p[1], q[2] = p[2];
  if (e <= b || pinned) return;
  float s[3] = {0.0f, 0.0f, 0.0f};
  for (int64_t i = b; i < e; ++i) {
    const int64_t n = nbr[i];
    if ((uint64_t)n >= (uint64_t)V) continue;
    s[0] = s[0] + pos[3 * n], s[1] = s[1] + pos[3 * n + 1], s[2] = s[2] + pos[3 * n + 2];
  }
  const float d = (float)(e - b);
  for (int k = 0; k < 3; ++k) {
    const float m = s[k] / d;
    const float step = f * (m - p[k]);
    float r = p[k] + step;
    if (p0) {
      const float lo = p0[3 * v + k] - c, hi = p0[3 * v + k] + c;
      r = r < lo ? lo : r;
      r = r > hi ? hi : r;
    }
    q[k] = r;
  }
}

// cross(pb - pa, pc - pa): two products and one difference per component
RX_MR_HD void mr_face_vector(const float* pa, const float* pb, const float* pc, float out[3]) {
  const float ux = pb[0] - pa[0], uy = pb[1] - pa[1], uz = pb[2] - pa[2];
  const float wx = pc[0] - pa[0], wy = pc[1] - pa[1], wz = pc[2] - pa[2];
  out[0] = uy * wz - uz * wy;
  out[1] = uz * wx - ux * wz;
  out[2] = ux * wy - uy * wx;
}

// the normal of vertex v: its corners' face vectors summed in slot order (ascending triangle after mr_canonical), normalised
RX_MR_HD void mr_vertex_normal(int64_t v, const int64_t* face_offsets, const int32_t* faces, int64_t capacity, const float* fvec, int64_t T,
                               float out[3]) {
  int64_t b = face_offsets[v], e = face_offsets[v + 1];
  if (b < 0) b = 0;
  if (e > capacity) e = capacity;
  float a[3] = {0.0f, 0.0f, 0.0f};
  for (int64_t i = b; i < e; ++i) {
    const int64_t t = faces[i];
    if ((uint64_t)t >= (uint64_t)T) continue;
    a[0] = a[0] + fvec[3 * t], a[1] = a[1] + fvec[3 * t + 1], a[2] = a[2] + fvec[3 * t + 2];
  }
  const float len = sqrtf(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);
  if (len == 0.0f) out[0] = 0.0f, out[1] = 0.0f, out[2] = 0.0f;
  else out[0] = a[0] / len, out[1] = a[1] / len, out[2] = a[2] / len;
}
#endif
