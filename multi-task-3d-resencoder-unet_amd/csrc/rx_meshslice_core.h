// rx_meshslice_core.h -- the arithmetic of the mesh slicing pass (rx_meshslice.hip), host- and device-callable: the kernels call
// these functions, and a plain C++ program runs the same ones on the CPU (tools/meshslice_host_check.cpp does, under
// AddressSanitizer, against a dump of tasks/normals/mesh_targets.py: slice_normals_numpy and slice_labels_numpy).  The statement is
// that module's docstring; every line below is one operation of it at the width it names (float32 unless a double appears), in
// its order.  NOTHING here may be contracted into an fma; sqrt and / are correctly rounded (IEEE on the host, hipcc's default on
// the device); rintf rounds half to even.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define RX_MS_HD __host__ __device__ inline
#else
#define RX_MS_HD inline
#endif

#pragma clang fp contract(off)

// the order key of a normals pixel: (triangle + 1) << 26 | pair << 24 | step << 4 | e; 0 = never painted
#define RX_MS_KEY_TRI_SHIFT 26
#define RX_MS_KEY_PAIR_SHIFT 24
#define RX_MS_KEY_E_BITS 4
#define RX_MS_MAX_STEPS (1 << 20)
#define RX_MS_MAX_SAMPLES 16
#define RX_MS_MAX_TRIANGLES ((1LL << 38) - 2)
#define RX_MS_LABEL_MAX_TRIANGLES ((1LL << 32) - 2)
#define RX_MS_INT_GUARD 1073741824.0f      // 2^30: a rounded coordinate is forced inside +-2^30 before it becomes an int

struct RxMsPoint {
  float x, y;
  float n[3];      // normals only
};

RX_MS_HD uint64_t rx_ms_key(long tri, int pair, int step, int e) {
  return ((uint64_t)(tri + 1) << RX_MS_KEY_TRI_SHIFT) | ((uint64_t)pair << RX_MS_KEY_PAIR_SHIFT) | ((uint64_t)step << RX_MS_KEY_E_BITS) | (uint64_t)e;
}
RX_MS_HD long rx_ms_key_tri(uint64_t k) { return (long)(k >> RX_MS_KEY_TRI_SHIFT) - 1; }
RX_MS_HD int rx_ms_key_pair(uint64_t k) { return (int)(k >> RX_MS_KEY_PAIR_SHIFT) & 3; }
RX_MS_HD int rx_ms_key_step(uint64_t k) { return (int)(k >> RX_MS_KEY_E_BITS) & (RX_MS_MAX_STEPS - 1); }

// int(round(float32)): half to even; anything beyond +-2^30 lands outside every image either way
RX_MS_HD int rx_ms_rint(float x) {
  float r = rintf(x);
  r = r > RX_MS_INT_GUARD ? RX_MS_INT_GUARD : r;
  r = r < -RX_MS_INT_GUARD ? -RX_MS_INT_GUARD : r;
  return r == r ? (int)r : (int)-RX_MS_INT_GUARD;
}

// pair k of the 2 or 3 points: (0,1), (0,2), (1,2)
RX_MS_HD void rx_ms_pair(int k, int* i, int* j) {
  *i = k == 2 ? 1 : 0;
  *j = k == 0 ? 1 : 2;
}
RX_MS_HD int rx_ms_num_pairs(int npts) { return npts == 3 ? 3 : (npts == 2 ? 1 : 0); }

// v / sqrt((v0^2 + v1^2) + v2^2); a zero vector passes through
RX_MS_HD void rx_ms_normalise(float* v) {
  const float q0 = v[0] * v[0], q1 = v[1] * v[1], q2 = v[2] * v[2];
  const float q01 = q0 + q1;
  const float s = q01 + q2;
  const float norm = sqrtf(s);
  if (norm == 0.0f) return;
  v[0] = v[0] / norm;
  v[1] = v[1] / norm;
  v[2] = v[2] / norm;
}

// ---- normals -------------------------------------------------------------------------------------------------------------------
RX_MS_HD bool rx_ms_edge_normals(const float* s, const float* e, const float* ns, const float* ne, float zf, RxMsPoint* p) {
  if (fabsf(s[2] - zf) <= 1e-8f) {
    p->x = s[0], p->y = s[1], p->n[0] = ns[0], p->n[1] = ns[1], p->n[2] = ns[2];
    return true;
  }
  if (fabsf(e[2] - zf) <= 1e-8f) {
    p->x = e[0], p->y = e[1], p->n[0] = ne[0], p->n[1] = ne[1], p->n[2] = ne[2];
    return true;
  }
  const float dz = e[2] - s[2];
  if (fabsf(dz) <= 1e-8f) return false;
  const float t = (zf - s[2]) / dz;
  if (!(-0.01f <= t && t <= 1.01f)) return false;
  const float ex = e[0] - s[0], ey = e[1] - s[1];
  const float tx = t * ex, ty = t * ey;
  p->x = s[0] + tx;
  p->y = s[1] + ty;
  for (int k = 0; k < 3; ++k) {
    const float d = ne[k] - ns[k];
    const float td = t * d;
    p->n[k] = ns[k] + td;
  }
  rx_ms_normalise(p->n);
  return true;
}

// the 0..3 distinct points in which slice zf cuts the triangle (v: 3 vertices, n: their normals)
RX_MS_HD int rx_ms_tri_points_normals(const float v[3][3], const float n[3][3], float zf, RxMsPoint pts[3]) {
  const float lo = fminf(fminf(v[0][2], v[1][2]), v[2][2]), hi = fmaxf(fmaxf(v[0][2], v[1][2]), v[2][2]);
  if (!(lo <= zf && zf <= hi)) return 0;
  int np = 0;
  for (int a = 0; a < 3; ++a) {
    const int b = a == 2 ? 0 : a + 1;
    RxMsPoint p;
    if (!rx_ms_edge_normals(v[a], v[b], n[a], n[b], zf, &p)) continue;
    bool dup = false;
    for (int j = 0; j < np; ++j) {
      const float dx = p.x - pts[j].x, dy = p.y - pts[j].y;
      const float qx = dx * dx, qy = dy * dy;
      if (qx + qy < 1e-10f) {
        dup = true;
        break;
      }
    }
    if (!dup) pts[np++] = p;
  }
  return np;
}

// the rounded ends of a segment; false if either lies outside the full image
RX_MS_HD bool rx_ms_segment(const RxMsPoint* a, const RxMsPoint* b, int w, int h, int* x0, int* y0, int* x1, int* y1) {
  *x0 = rx_ms_rint(a->x), *y0 = rx_ms_rint(a->y), *x1 = rx_ms_rint(b->x), *y1 = rx_ms_rint(b->y);
  return *x0 >= 0 && *x0 < w && *y0 >= 0 && *y0 < h && *x1 >= 0 && *x1 < w && *y1 >= 0 && *y1 < h;
}

// max(int(2 * sqrt(dx^2 + dy^2)), |dx|, |dy|) + 1, the root and the product in double (ends inside an image of < 2^30 pixels a side)
RX_MS_HD int rx_ms_steps(int x0, int y0, int x1, int y1) {
  const long dx = (long)x1 - x0, dy = (long)y1 - y0;
  const double dist = sqrt((double)(dx * dx + dy * dy));
  const double twice = dist * 2.0;
  const long a = (long)twice, adx = dx < 0 ? -dx : dx, ady = dy < 0 ? -dy : dy;
  const long m = adx > ady ? adx : ady;
  return (int)((a > m ? a : m) + 1);
}

// the float64 position and the float32 unit normal at `step` of `steps`
RX_MS_HD void rx_ms_step_state(int x0, int y0, int x1, int y1, const float* na, const float* nb, int steps, int step, double* x, double* y,
                               float n[3]) {
  const double t = steps > 1 ? (double)step / (double)(steps - 1) : 0.0;
  const double tx = t * (double)(x1 - x0), ty = t * (double)(y1 - y0);
  *x = (double)x0 + tx;
  *y = (double)y0 + ty;
  const double one_t = 1.0 - t;
  const float a = (float)one_t, b = (float)t;
  for (int k = 0; k < 3; ++k) {
    const float pa = a * na[k], pb = b * nb[k];
    n[k] = pa + pb;
  }
  rx_ms_normalise(n);
}

// float32(((e / (E - 1)) * 2 - 1) * eff), the product in double
RX_MS_HD float rx_ms_exp_offset(int e, int n_exp, double eff) {
  const double q = (double)e / (double)(n_exp - 1);
  const double q2 = q * 2.0;
  const double u = q2 - 1.0;
  const double ue = u * eff;
  return (float)ue;
}

// the pixel of one expansion sample along one axis: round(float32(c) + off * n_axis)
RX_MS_HD int rx_ms_exp_pixel(double c, float off, float n_axis) {
  const float cf = (float)c;
  const float d = off * n_axis;
  return rx_ms_rint(cf + d);
}

// uint16((n + 1) * 32767.5), truncated
RX_MS_HD uint16_t rx_ms_code(float n) {
  const float a = n + 1.0f;
  const float b = a * 32767.5f;
  const int i = b > 0.0f ? (b < 65535.0f ? (int)b : 65535) : 0;
  return (uint16_t)i;
}

// (code * 255) // 65535 in uint16: the product wraps
RX_MS_HD uint8_t rx_ms_viz(uint16_t code) { return (uint8_t)((uint16_t)(code * 255u) / 65535u); }

// ---- labels --------------------------------------------------------------------------------------------------------------------
RX_MS_HD bool rx_ms_edge_labels(const float* s, const float* e, int z, float* px, float* py) {
  const double zp = (double)z;
  if (fabs((double)s[2] - zp) < 1e-8) {
    *px = s[0], *py = s[1];
    return true;
  }
  if (fabs((double)e[2] - zp) < 1e-8) {
    *px = e[0], *py = e[1];
    return true;
  }
  const float dz = e[2] - s[2];
  if (fabsf(dz) < 1e-15f) return false;
  const double t = (zp - (double)s[2]) / (double)dz;
  if (!(0.0 - 1e-3 <= t && t <= 1.0 + 1e-3)) return false;
  const float ex = e[0] - s[0], ey = e[1] - s[1];
  const double tx = t * (double)ex, ty = t * (double)ey;
  const double x = (double)s[0] + tx, y = (double)s[1] + ty;
  *px = (float)x, *py = (float)y;
  return true;
}

RX_MS_HD int rx_ms_tri_points_labels(const float v[3][3], int z, RxMsPoint pts[3]) {
  const float lo = fminf(fminf(v[0][2], v[1][2]), v[2][2]), hi = fmaxf(fmaxf(v[0][2], v[1][2]), v[2][2]);
  const double zp = (double)z;
  if (!((double)lo <= zp && zp <= (double)hi)) return 0;
  int np = 0;
  for (int a = 0; a < 3; ++a) {
    const int b = a == 2 ? 0 : a + 1;
    float x, y;
    if (!rx_ms_edge_labels(v[a], v[b], z, &x, &y)) continue;
    bool dup = false;
    for (int j = 0; j < np; ++j) {
      const float dx = x - pts[j].x, dy = y - pts[j].y;
      const float qx = dx * dx, qy = dy * dy;
      if (qx + qy < 1e-12f) {
        dup = true;
        break;
      }
    }
    if (!dup) pts[np].x = x, pts[np].y = y, ++np;
  }
  return np;
}

// the float32 DDA of one label segment: steps = int(max(|dx|, |dy|)); steps + 1 points, (x, y) += (dx, dy) / steps after each
struct RxMsDda {
  float x, y, xi, yi;
  int steps;
};
RX_MS_HD RxMsDda rx_ms_dda(float x0, float y0, float x1, float y1) {
  RxMsDda d;
  const float dx = x1 - x0, dy = y1 - y0;
  float m = fmaxf(fabsf(dx), fabsf(dy));
  m = m < RX_MS_INT_GUARD ? m : RX_MS_INT_GUARD;      // (also a NaN)
  d.steps = (int)m;
  d.x = x0, d.y = y0;
  d.xi = d.steps ? dx / (float)d.steps : 0.0f;
  d.yi = d.steps ? dy / (float)d.steps : 0.0f;
  return d;
}
RX_MS_HD void rx_ms_dda_next(RxMsDda* d) {
  d->x = d->x + d->xi;
  d->y = d->y + d->yi;
}
