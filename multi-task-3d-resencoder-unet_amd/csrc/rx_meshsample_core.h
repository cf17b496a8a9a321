// rx_meshsample_core.h -- the per-vertex and per-triangle work of the mesh orientation passes (rx_meshsample.hip), written so that
// it compiles for the host as well: csrc/tools/meshsample_host_check.cpp runs exactly these functions serially against a direct
// restatement, under the address and undefined-behaviour sanitizers.  postprocess/orient.py (sample_points_numpy, unit_numpy,
// face_cos_numpy, side_numpy) is the statement; every float32 operation here is one rounding (contraction is off, denormals are
// kept, / and sqrtf are correctly rounded: IEEE on the host, hipcc's default on the device).
//
// A volume is (C, Zs, Y, X) contiguous and holds planes [z_base, z_base + Zs) of a volume of z_total planes.  Every index a load
// goes through is clamped into the slab first, whatever the coordinates hold, so no load leaves it.
#ifndef RX_MESHSAMPLE_CORE_H
#define RX_MESHSAMPLE_CORE_H
#include <math.h>
#include <stdint.h>

#include "rx_meshrefine_core.h"      // mr_face_vector, mr_triangle_ok

#pragma clang fp contract(off)

#define RX_MSP_COPY 0
#define RX_MSP_U8 1
#define RX_MSP_U16 2
#define RX_MSP_NORMAL_U16 3
#define RX_MSP_MAX_CHANNELS 8
#define RX_MSP_MAX_EXTENT 16777214      // 2^24 - 2: an index must be an exact float32 (include/rxunet.h says the same)

// float32(v), then the rule: copy keeps the bits; u8 v / 255; u16 v / 65535; normal_u16 (v / 65535) * 2 - 1
template <int RULE, typename T>
RX_MR_HD float msp_decode(T v) {
  const float f = (float)v;
  if (RULE == RX_MSP_COPY) return f;
  if (RULE == RX_MSP_U8) return f / 255.0f;
  const float q = f / 65535.0f;
  if (RULE == RX_MSP_U16) return q;
  const float d = q * 2.0f;
  return d - 1.0f;
}

// one axis of one point: i = floor(p) squashed into [-2, n] as a float (a NaN becomes n: the conversion cannot overflow), the
// corners i and i + 1 clamped to [0, n - 1], f = p - floor(p)
struct MsAxis {
  int i0, i1;
  float f;
};

RX_MR_HD int msp_clampi(int i, int n) { return i < 0 ? 0 : (i > n - 1 ? n - 1 : i); }

RX_MR_HD MsAxis msp_axis(float p, int n) {
  MsAxis r;
  const float fl = floorf(p);
  r.f = p - fl;
  const int i = (int)fmaxf(fminf(fl, (float)n), -2.0f);
  r.i0 = msp_clampi(i, n);
  r.i1 = msp_clampi(i + 1, n);
  return r;
}

// lerp(u, w, f) = u + f * (w - u)
RX_MR_HD float msp_lerp(float u, float w, float f) {
  const float d = w - u;
  const float fd = f * d;
  return u + fd;
}

// the slab owns a point when both of its clamped global z indices lie in [z_base, z_base + z_depth)
RX_MR_HD bool msp_owned(const MsAxis& az, int z_base, int z_depth) { return az.i0 >= z_base && az.i1 < z_base + z_depth; }

// one channel volume `src` (z_depth planes of Y rows of X values) at the eight corners: the x-pair of each row is loaded together,
// every corner decoded, then the lerps along x, y and z.  lz0 / lz1: the z indices inside the slab.
template <int RULE, typename T>
RX_MR_HD float msp_sample_channel(const T* src, int64_t YX, int X, int lz0, int lz1, const MsAxis& ay, const MsAxis& ax, float fz) {
  const T* r00 = src + (int64_t)lz0 * YX + (int64_t)ay.i0 * X;
  const T* r01 = src + (int64_t)lz0 * YX + (int64_t)ay.i1 * X;
  const T* r10 = src + (int64_t)lz1 * YX + (int64_t)ay.i0 * X;
  const T* r11 = src + (int64_t)lz1 * YX + (int64_t)ay.i1 * X;
  const T a000 = r00[ax.i0], a001 = r00[ax.i1];
  const T a010 = r01[ax.i0], a011 = r01[ax.i1];
  const T a100 = r10[ax.i0], a101 = r10[ax.i1];
  const T a110 = r11[ax.i0], a111 = r11[ax.i1];
  const float x00 = msp_lerp(msp_decode<RULE, T>(a000), msp_decode<RULE, T>(a001), ax.f);
  const float x01 = msp_lerp(msp_decode<RULE, T>(a010), msp_decode<RULE, T>(a011), ax.f);
  const float x10 = msp_lerp(msp_decode<RULE, T>(a100), msp_decode<RULE, T>(a101), ax.f);
  const float x11 = msp_lerp(msp_decode<RULE, T>(a110), msp_decode<RULE, T>(a111), ax.f);
  return msp_lerp(msp_lerp(x00, x01, ay.f), msp_lerp(x10, x11, ay.f), fz);
}

// v / l, l = sqrt(x*x + y*y + z*z) summed left to right, where l > 0; else exactly (0, 0, 0)
RX_MR_HD void msp_unit(float v[3]) {
  const float len = sqrtf(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
  if (len > 0.0f) v[0] = v[0] / len, v[1] = v[1] / len, v[2] = v[2] / len;
  else v[0] = 0.0f, v[1] = 0.0f, v[2] = 0.0f;
}

// The point p = (x, y, z) of a (C, z_depth, Y, X) slab: indices once, then every channel.  Returns false, and leaves `out` alone,
// where the slab does not own the point.  out: C values, `stride` apart.  unit: C == 3, and the three values are made unit.
template <int RULE, typename T>
RX_MR_HD bool msp_sample_point(const T* vol, int C, int z_base, int z_depth, int z_total, int Y, int X, const float p[3], bool unit, float* out) {
  const MsAxis az = msp_axis(p[2], z_total);
  if (!msp_owned(az, z_base, z_depth)) return false;
  const MsAxis ay = msp_axis(p[1], Y), ax = msp_axis(p[0], X);
  const int lz0 = msp_clampi(az.i0 - z_base, z_depth), lz1 = msp_clampi(az.i1 - z_base, z_depth);      // inside already: the clamp is a guard
  const int64_t YX = (int64_t)Y * X, ZYX = YX * z_depth;
  if (unit) {
    float v[3];
    for (int c = 0; c < 3; ++c) v[c] = msp_sample_channel<RULE, T>(vol + c * ZYX, YX, X, lz0, lz1, ay, ax, az.f);
    msp_unit(v);
    out[0] = v[0], out[1] = v[1], out[2] = v[2];
  } else {
    for (int c = 0; c < C; ++c) out[c] = msp_sample_channel<RULE, T>(vol + c * ZYX, YX, X, lz0, lz1, ay, ax, az.f);
  }
  return true;
}

// a . b: three products summed left to right
RX_MR_HD float msp_dot(const float a[3], const float b[3]) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }

// cos between the face vector g = cross(pb - pa, pc - pa) and m = (na + nb) + nc: (g . m) / sqrt((g . g) * (m . m)); 0 / 0 = NaN
// where a factor is zero
RX_MR_HD float msp_face_cos(const float* pa, const float* pb, const float* pc, const float* na, const float* nb, const float* nc) {
  float g[3], m[3];
  mr_face_vector(pa, pb, pc, g);
  for (int k = 0; k < 3; ++k) {
    const float ab = na[k] + nb[k];
    m[k] = ab + nc[k];
  }
  const float d = msp_dot(g, m), gg = msp_dot(g, g), mm = msp_dot(m, m);
  const float q = gg * mm;
  return d / sqrtf(q);
}

// +1 (front) where cos > min_cos, -1 (back) where cos < -min_cos, else 0 (rim), a NaN included
RX_MR_HD int msp_side(float cos, float min_cos) { return (cos > min_cos ? 1 : 0) - (cos < -min_cos ? 1 : 0); }
#endif
