// rx_meshslice.hip -- mesh targets on the device: triangle meshes sliced by every z-plane of a slab into the normals / label /
// mask volumes the network trains on (host side tasks/normals/mesh_targets.py, whose slice_normals_numpy and slice_labels_numpy are
// the statements; the arithmetic is rx_meshslice_core.h, shared with the host check).
//
// The reference paints a slice serially, triangle after triangle, so a pixel keeps its last writer.  Writers are ordered by
// (triangle, pair, step, sample): the last writer is the LARGEST such tuple, and a maximum does not depend on the order in which
// the writers arrive.  So the pass is a scatter of order keys with an integer atomic maximum, then a resolve that recomputes each
// pixel's value from its winning key alone:
//
//   mesh_keys_normals_kernel / mesh_keys_labels_kernel   one lane per triangle.  The triangle visits only the slices of the slab
//     inside its own [min z, max z] (each compared in float32 / float64 exactly as the statement compares it), cuts itself, walks
//     its segments and issues one atomicMax per painted pixel that lies in the window: 64-bit keys for normals, 32-bit (triangle + 1)
//     for labels.  Normal lines are closed-form in `step`; label lines accumulate x_f += x_inc serially as the reference's DDA does.
//     Integer atomics: the result is bit-identical run to run.
//   mesh_resolve_normals_kernel   one lane per key: triangle, pair and step from the key, the cut and the interpolated normal
//     recomputed, the uint16 code (and the optional viz / mask bytes) staged in LDS and stored by the workgroup as whole dwords.
//   mesh_resolve_labels_kernel    one lane per key: the label of the winning triangle, the optional 0 / 255 mask.
//
// The output covers slices [z0, z0 + nz) and the window (y0, x0, wh, ww) of the full w x h image; endpoint and pixel tests use the
// full image, only window pixels are stored, so a slab or window result equals the full result cropped.  Every vertex index is
// clamped, every loop has a bound that does not depend on device data alone, every offset is 64-bit.
#include "rx_common.h"
#include "rx_meshslice_core.h"

#pragma clang fp contract(off)

#define RX_MS_BLOCK 256
#define RX_MS_LABEL_MAX_STEPS (1 << 26)      // |coordinate| < 2^24 (checked by the caller) keeps a label segment below this

__device__ inline long ms_clampl(long i, long hi) { return i < 0 ? 0 : (i > hi ? hi : i); }

// the three vertices (and normals) of triangle t, indices clamped into the vertex array
__device__ inline void ms_load_tri(const float* __restrict__ vertices, const float* __restrict__ normals, const int32_t* __restrict__ triangles,
                                   long n_vertices, long t, float v[3][3], float n[3][3]) {
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const long i = ms_clampl((long)triangles[3 * t + c], n_vertices - 1);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      v[c][k] = vertices[3 * i + k];
      if (normals) n[c][k] = normals[3 * i + k];
    }
  }
}

// the slices of [z0, z0 + nz) inside [lo, hi]: a superset by one on either side at most, each re-tested by the core
__device__ inline void ms_slice_range(const float v[3][3], int z0, int nz, int* za, int* zb) {
  float lo = fminf(fminf(v[0][2], v[1][2]), v[2][2]), hi = fmaxf(fmaxf(v[0][2], v[1][2]), v[2][2]);
  lo = fminf(fmaxf(lo, -RX_MS_INT_GUARD), RX_MS_INT_GUARD);
  hi = fminf(fmaxf(hi, -RX_MS_INT_GUARD), RX_MS_INT_GUARD);
  const long a = (long)floorf(lo) - 1, b = (long)ceilf(hi) + 1;
  const long s = a > (long)z0 ? a : (long)z0, e = b < (long)z0 + nz - 1 ? b : (long)z0 + nz - 1;
  *za = (int)s, *zb = (int)e;      // empty when zb < za (NaN bounds give lo = hi = -2^30: empty as well for any slab the host accepts)
}

struct MsGeom {
  int w, h, z0, nz, y0, x0, wh, ww;
};

__global__ __launch_bounds__(RX_MS_BLOCK) void mesh_keys_normals_kernel(const float* __restrict__ vertices, long n_vertices,
                                                                         const int32_t* __restrict__ triangles, long n_triangles,
                                                                         const float* __restrict__ normals, MsGeom g, double eff, int n_exp,
                                                                         unsigned long long* __restrict__ keys) {
  const long t = (long)blockIdx.x * RX_MS_BLOCK + threadIdx.x;
  if (t >= n_triangles) return;
  float v[3][3], n[3][3];
  ms_load_tri(vertices, normals, triangles, n_vertices, t, v, n);
  int za, zb;
  ms_slice_range(v, g.z0, g.nz, &za, &zb);
  float off[RX_MS_MAX_SAMPLES];
#pragma unroll
  for (int e = 0; e < RX_MS_MAX_SAMPLES; ++e) off[e] = e < n_exp ? rx_ms_exp_offset(e, n_exp, eff) : 0.0f;
  for (int z = za; z <= zb; ++z) {
    RxMsPoint pts[3];
    const int np = rx_ms_tri_points_normals(v, n, (float)z, pts);
    const int pairs = rx_ms_num_pairs(np);
    unsigned long long* __restrict__ plane = keys + (long)(z - g.z0) * g.wh * g.ww;
    for (int pair = 0; pair < pairs; ++pair) {
      int i, j, x0, y0, x1, y1;
      rx_ms_pair(pair, &i, &j);
      if (!rx_ms_segment(&pts[i], &pts[j], g.w, g.h, &x0, &y0, &x1, &y1)) continue;
      int steps = rx_ms_steps(x0, y0, x1, y1);
      steps = steps < RX_MS_MAX_STEPS ? steps : RX_MS_MAX_STEPS;      // (the host refuses images in which a segment could get there)
      for (int step = 0; step < steps; ++step) {
        double x, y;
        float nn[3];
        rx_ms_step_state(x0, y0, x1, y1, pts[i].n, pts[j].n, steps, step, &x, &y, nn);
        for (int e = 0; e < n_exp; ++e) {
          const int px = rx_ms_exp_pixel(x, off[e], nn[0]), py = rx_ms_exp_pixel(y, off[e], nn[1]);
          if (px < 0 || px >= g.w || py < 0 || py >= g.h) continue;                         // the full image decides what is painted
          const int wx = px - g.x0, wy = py - g.y0;
          if (wx < 0 || wx >= g.ww || wy < 0 || wy >= g.wh) continue;                       // the window decides what is stored
          atomicMax(plane + (long)wy * g.ww + wx, (unsigned long long)rx_ms_key(t, pair, step, e));
        }
      }
    }
  }
}

__global__ __launch_bounds__(RX_MS_BLOCK) void mesh_keys_labels_kernel(const float* __restrict__ vertices, long n_vertices,
                                                                        const int32_t* __restrict__ triangles, long n_triangles, MsGeom g,
                                                                        unsigned* __restrict__ keys) {
  const long t = (long)blockIdx.x * RX_MS_BLOCK + threadIdx.x;
  if (t >= n_triangles) return;
  float v[3][3];
  ms_load_tri(vertices, nullptr, triangles, n_vertices, t, v, nullptr);
  int za, zb;
  ms_slice_range(v, g.z0, g.nz, &za, &zb);
  const unsigned key = (unsigned)(t + 1);
  for (int z = za; z <= zb; ++z) {
    RxMsPoint pts[3];
    const int np = rx_ms_tri_points_labels(v, z, pts);
    const int pairs = rx_ms_num_pairs(np);
    unsigned* __restrict__ plane = keys + (long)(z - g.z0) * g.wh * g.ww;
    for (int pair = 0; pair < pairs; ++pair) {
      int i, j;
      rx_ms_pair(pair, &i, &j);
      RxMsDda d = rx_ms_dda(pts[i].x, pts[i].y, pts[j].x, pts[j].y);
      const int steps = d.steps < RX_MS_LABEL_MAX_STEPS ? d.steps : RX_MS_LABEL_MAX_STEPS;
      for (int s = 0; s <= steps; ++s) {
        const int px = rx_ms_rint(d.x), py = rx_ms_rint(d.y);
        rx_ms_dda_next(&d);
        if (px < 0 || px >= g.w || py < 0 || py >= g.h) continue;
        const int wx = px - g.x0, wy = py - g.y0;
        if (wx < 0 || wx >= g.ww || wy < 0 || wy >= g.wh) continue;
        atomicMax(plane + (long)wy * g.ww + wx, key);
      }
    }
  }
}

// the workgroup's staged bytes -> out[byte0 ..), whole dwords while they end inside the array, bytes for the last one
__device__ inline void ms_store_stream(const unsigned* s_words, int nwords, uint8_t* __restrict__ out, long byte0, long total_bytes) {
  for (int d = threadIdx.x; d < nwords; d += RX_MS_BLOCK) {
    const long b = byte0 + 4L * d;
    if (b + 4 <= total_bytes) {
      *reinterpret_cast<unsigned*>(out + b) = s_words[d];
    } else {
      const unsigned wv = s_words[d];
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (b + e < total_bytes) out[b + e] = (uint8_t)(wv >> (8 * e));
    }
  }
}

__global__ __launch_bounds__(RX_MS_BLOCK) void mesh_resolve_normals_kernel(const unsigned long long* __restrict__ keys,
                                                                            const float* __restrict__ vertices, long n_vertices,
                                                                            const int32_t* __restrict__ triangles, long n_triangles,
                                                                            const float* __restrict__ normals, MsGeom g, long npix,
                                                                            uint8_t* __restrict__ out, uint8_t* __restrict__ viz,
                                                                            uint8_t* __restrict__ mask) {
  __shared__ unsigned s_code[RX_MS_BLOCK * 6 / 4];      // 256 pixels x 3 uint16
  __shared__ unsigned s_viz[RX_MS_BLOCK * 3 / 4];       // 256 pixels x 3 bytes
  __shared__ unsigned s_mask[RX_MS_BLOCK / 4];
  const int tid = threadIdx.x;
  const long p0 = (long)blockIdx.x * RX_MS_BLOCK, p = p0 + tid;
  uint16_t code[3] = {0, 0, 0};
  if (p < npix) {
    const unsigned long long k = keys[p];
    const long t = rx_ms_key_tri(k);
    if (k != 0ull && t >= 0 && t < n_triangles) {
      const int z = g.z0 + (int)(p / ((long)g.wh * g.ww));
      float v[3][3], n[3][3];
      ms_load_tri(vertices, normals, triangles, n_vertices, t, v, n);
      RxMsPoint pts[3];
      const int np = rx_ms_tri_points_normals(v, n, (float)z, pts);
      const int pair = rx_ms_key_pair(k), step = rx_ms_key_step(k);
      int i, j, x0, y0, x1, y1;
      rx_ms_pair(pair < 3 ? pair : 0, &i, &j);
      if (pair < rx_ms_num_pairs(np) && rx_ms_segment(&pts[i], &pts[j], g.w, g.h, &x0, &y0, &x1, &y1)) {
        const int steps = rx_ms_steps(x0, y0, x1, y1);
        if (step < steps) {
          double x, y;
          float nn[3];
          rx_ms_step_state(x0, y0, x1, y1, pts[i].n, pts[j].n, steps, step, &x, &y, nn);
#pragma unroll
          for (int c = 0; c < 3; ++c) code[c] = rx_ms_code(nn[c]);
        }
      }
    }
  }
  uint16_t* s16 = reinterpret_cast<uint16_t*>(s_code);
  uint8_t* s8 = reinterpret_cast<uint8_t*>(s_viz);
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    s16[3 * tid + c] = code[c];
    s8[3 * tid + c] = rx_ms_viz(code[c]);
  }
  reinterpret_cast<uint8_t*>(s_mask)[tid] = (code[0] | code[1] | code[2]) ? 255 : 0;
  __syncthreads();
  ms_store_stream(s_code, RX_MS_BLOCK * 6 / 4, out, p0 * 6, npix * 6);
  if (viz) ms_store_stream(s_viz, RX_MS_BLOCK * 3 / 4, viz, p0 * 3, npix * 3);
  if (mask) ms_store_stream(s_mask, RX_MS_BLOCK / 4, mask, p0, npix);
}

__global__ __launch_bounds__(RX_MS_BLOCK) void mesh_resolve_labels_kernel(const unsigned* __restrict__ keys, const int32_t* __restrict__ tri_labels,
                                                                           long n_triangles, long npix, uint8_t* __restrict__ out,
                                                                           uint8_t* __restrict__ mask) {
  __shared__ unsigned s_lab[RX_MS_BLOCK * 2 / 4];
  __shared__ unsigned s_mask[RX_MS_BLOCK / 4];
  const int tid = threadIdx.x;
  const long p0 = (long)blockIdx.x * RX_MS_BLOCK, p = p0 + tid;
  uint16_t lab = 0;
  if (p < npix) {
    const unsigned k = keys[p];
    if (k != 0u && (long)k <= n_triangles) lab = (uint16_t)(tri_labels[(long)k - 1] & 0xFFFF);
  }
  reinterpret_cast<uint16_t*>(s_lab)[tid] = lab;
  reinterpret_cast<uint8_t*>(s_mask)[tid] = lab ? 255 : 0;
  __syncthreads();
  ms_store_stream(s_lab, RX_MS_BLOCK * 2 / 4, out, p0 * 2, npix * 2);
  if (mask) ms_store_stream(s_mask, RX_MS_BLOCK / 4, mask, p0, npix);
}

// ---- host side -------------------------------------------------------------------------------------------------------------------
static int ms_check_geom(const char* who, const void* vertices, long n_vertices, const void* triangles, long n_triangles, int w, int h, int z0,
                         int nz, int y0, int x0, int wh, int ww, long* npix) {
  if (!vertices || !triangles) RX_FAIL(RX_EINVAL, "%s: null vertices or triangles", who);
  if (n_vertices < 1 || n_vertices > 0x7fffffffL) RX_FAIL(RX_EINVAL, "%s: n_vertices %ld must lie in [1, 2^31)", who, n_vertices);
  if (n_triangles < 0) RX_FAIL(RX_EINVAL, "%s: n_triangles %ld is negative", who, n_triangles);
  if (w < 1 || h < 1 || nz < 1) RX_FAIL(RX_EINVAL, "%s: w, h and nz must be positive (got w=%d h=%d nz=%d)", who, w, h, nz);
  if (w > (1 << 24) || h > (1 << 24)) RX_FAIL(RX_EINVAL, "%s: image sides above 2^24 are not supported (got w=%d h=%d)", who, w, h);
  if (z0 <= -(1 << 24) || (long)z0 + nz > (1 << 24)) RX_FAIL(RX_EINVAL, "%s: slices must lie inside (-2^24, 2^24) (got z0=%d nz=%d)", who, z0, nz);
  if (y0 < 0 || x0 < 0 || wh < 1 || ww < 1 || (long)y0 + wh > h || (long)x0 + ww > w)
    RX_FAIL(RX_EINVAL, "%s: window (y0=%d x0=%d wh=%d ww=%d) does not lie inside the %d x %d image", who, y0, x0, wh, ww, w, h);
  long a = 0;
  if (__builtin_mul_overflow((long)nz, (long)wh, &a) || __builtin_mul_overflow(a, (long)ww, npix) || *npix > (1L << 40))
    RX_FAIL(RX_EINVAL, "%s: nz * wh * ww is too large", who);
  if ((n_triangles + RX_MS_BLOCK - 1) / RX_MS_BLOCK > 0x7fffffffL || (*npix + RX_MS_BLOCK - 1) / RX_MS_BLOCK > 0x7fffffffL)
    RX_FAIL(RX_EINVAL, "%s: too many workgroups", who);
  return RX_OK;
}

extern "C" int rx_mesh_slice_keys(int labels, const float* vertices, long n_vertices, const int32_t* triangles, long n_triangles,
                                  const float* normals, int w, int h, int z0, int nz, int y0, int x0, int wh, int ww, double exp_factor,
                                  void* keys, void* stream) {
  long npix = 0;
  const int rc = ms_check_geom("rx_mesh_slice_keys", vertices, n_vertices, triangles, n_triangles, w, h, z0, nz, y0, x0, wh, ww, &npix);
  if (rc != RX_OK) return rc;
  if (!keys) RX_FAIL(RX_EINVAL, "rx_mesh_slice_keys: null keys");
  if (((uintptr_t)keys & (labels ? 3u : 7u)) != 0) RX_FAIL(RX_EINVAL, "rx_mesh_slice_keys: keys must be aligned to their %d bytes", labels ? 4 : 8);
  if (n_triangles > (labels ? RX_MS_LABEL_MAX_TRIANGLES : RX_MS_MAX_TRIANGLES))
    RX_FAIL(RX_EINVAL, "rx_mesh_slice_keys: %ld triangles do not fit the order key", n_triangles);
  const MsGeom g{w, h, z0, nz, y0, x0, wh, ww};
  hipStream_t st = (hipStream_t)stream;
  if (n_triangles == 0) return RX_OK;
  const dim3 grid((unsigned)((n_triangles + RX_MS_BLOCK - 1) / RX_MS_BLOCK)), block(RX_MS_BLOCK);
  if (labels) {
    hipLaunchKernelGGL(mesh_keys_labels_kernel, grid, block, 0, st, vertices, n_vertices, triangles, n_triangles, g, (unsigned*)keys);
  } else {
    if (!normals) RX_FAIL(RX_EINVAL, "rx_mesh_slice_keys: null normals");
    const double eff = exp_factor * 1.2;
    if (!(eff >= 0.0) || !(eff < 1e6)) RX_FAIL(RX_EINVAL, "rx_mesh_slice_keys: exp_factor %g must be finite and not negative", exp_factor);
    const int n_exp = (int)(4.0 * eff + 1.0);
    if (n_exp < 2 || n_exp > RX_MS_MAX_SAMPLES)
      RX_FAIL(RX_EINVAL, "rx_mesh_slice_keys: exp_factor %g gives %d expansion samples (2 to %d)", exp_factor, n_exp, RX_MS_MAX_SAMPLES);
    // the longest segment joins two corners of the image: its step count must fit the key's 20 bits
    if (rx_ms_steps(0, 0, w - 1, h - 1) >= RX_MS_MAX_STEPS)
      RX_FAIL(RX_EINVAL, "rx_mesh_slice_keys: a %d x %d image allows segments of 2^20 steps or more, which the key cannot hold", w, h);
    hipLaunchKernelGGL(mesh_keys_normals_kernel, grid, block, 0, st, vertices, n_vertices, triangles, n_triangles, normals, g, eff, n_exp,
                       (unsigned long long*)keys);
  }
  RX_CHECK_LAUNCH("rx_mesh_slice_keys");
  return RX_OK;
}

extern "C" int rx_mesh_resolve_normals(const void* keys, const float* vertices, long n_vertices, const int32_t* triangles, long n_triangles,
                                       const float* normals, int w, int h, int z0, int nz, int y0, int x0, int wh, int ww, uint16_t* out,
                                       uint8_t* viz, uint8_t* mask, void* stream) {
  long npix = 0;
  const int rc = ms_check_geom("rx_mesh_resolve_normals", vertices, n_vertices, triangles, n_triangles, w, h, z0, nz, y0, x0, wh, ww, &npix);
  if (rc != RX_OK) return rc;
  if (!keys || !normals || !out) RX_FAIL(RX_EINVAL, "rx_mesh_resolve_normals: null keys, normals or out");
  if (((uintptr_t)keys & 7u) != 0) RX_FAIL(RX_EINVAL, "rx_mesh_resolve_normals: keys must be 8-byte aligned");
  if ((((uintptr_t)out | (uintptr_t)viz | (uintptr_t)mask) & 3u) != 0)
    RX_FAIL(RX_EINVAL, "rx_mesh_resolve_normals: out, viz and mask must be 4-byte aligned (they are stored as dwords)");
  const MsGeom g{w, h, z0, nz, y0, x0, wh, ww};
  const dim3 grid((unsigned)((npix + RX_MS_BLOCK - 1) / RX_MS_BLOCK)), block(RX_MS_BLOCK);
  hipLaunchKernelGGL(mesh_resolve_normals_kernel, grid, block, 0, (hipStream_t)stream, (const unsigned long long*)keys, vertices, n_vertices,
                     triangles, n_triangles, normals, g, npix, (uint8_t*)out, viz, mask);
  RX_CHECK_LAUNCH("rx_mesh_resolve_normals");
  return RX_OK;
}

extern "C" int rx_mesh_resolve_labels(const void* keys, const int32_t* tri_labels, long n_triangles, long npix, uint16_t* out, uint8_t* mask,
                                      void* stream) {
  if (!keys || !out) RX_FAIL(RX_EINVAL, "rx_mesh_resolve_labels: null keys or out");
  if (n_triangles < 0 || n_triangles > RX_MS_LABEL_MAX_TRIANGLES || (n_triangles > 0 && !tri_labels))
    RX_FAIL(RX_EINVAL, "rx_mesh_resolve_labels: bad n_triangles %ld or null tri_labels", n_triangles);
  if (npix < 1 || npix > (1L << 40)) RX_FAIL(RX_EINVAL, "rx_mesh_resolve_labels: npix %ld out of range", npix);
  if ((((uintptr_t)keys | (uintptr_t)out | (uintptr_t)mask) & 3u) != 0)
    RX_FAIL(RX_EINVAL, "rx_mesh_resolve_labels: keys, out and mask must be 4-byte aligned");
  const dim3 grid((unsigned)((npix + RX_MS_BLOCK - 1) / RX_MS_BLOCK)), block(RX_MS_BLOCK);
  hipLaunchKernelGGL(mesh_resolve_labels_kernel, grid, block, 0, (hipStream_t)stream, (const unsigned*)keys, tri_labels, n_triangles, npix,
                     (uint8_t*)out, mask);
  RX_CHECK_LAUNCH("rx_mesh_resolve_labels");
  return RX_OK;
}
