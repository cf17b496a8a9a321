// rx_affine_core.h -- the per-voxel arithmetic of rx_affine_apply (rx_affine.hip), host- and device-callable: the kernel calls
// these functions, and a plain C++ program can run the same ones on the CPU (tools/affine_host_check.cpp does, under
// AddressSanitizer, against a dump of dataloading/spatial_device.py: affine_numpy).  The statement is affine_numpy's docstring;
// every line below is one float32 operation of it, in its order.  NOTHING here may be contracted into an fma.
#pragma once
#include <math.h>
#include <stdint.h>

#pragma clang fp contract(off)

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RX_AFF_HD __host__ __device__ inline
#else
#define RX_AFF_HD inline
#endif

#define RX_AFF_LINEAR 0
#define RX_AFF_NEAREST 1
#define RX_AFF_CONSTANT 0
#define RX_AFF_CLAMP 1

// one axis of one voxel: clamped indices (ALWAYS inside [0, n - 1], whatever the coordinate: a load through them cannot leave
// the sample), whether the unclamped ones were inside, and the weight of the upper one
struct RxAffAxis {
  int i0, i1;
  bool in0, in1;
  float f;
};

// c_d = float32(n_d - 1) * 0.5
RX_AFF_HD float rx_aff_centre(int n) { return (float)(n - 1) * 0.5f; }

// p_d = ((m0 * t_z + m1 * t_y) + m2 * t_x) + c_d
RX_AFF_HD float rx_aff_coord(float m0, float m1, float m2, float tz, float ty, float tx, float c) {
  const float a = m0 * tz;
  const float b = m1 * ty;
  const float d = m2 * tx;
  const float ab = a + b;
  const float abd = ab + d;
  return abd + c;
}

// a whole-number float -> int, squashed into [lo, n] first (a NaN becomes n): the conversion cannot overflow, and everything
// outside [0, n - 1] stays outside
RX_AFF_HD int rx_aff_index(float v, int n, float lo) { return (int)fmaxf(fminf(v, (float)n), lo); }

RX_AFF_HD int rx_aff_clampi(int i, int n) { return i < 0 ? 0 : (i > n - 1 ? n - 1 : i); }

// linear: i = floor(p), f = p - i, corners i and i + 1.  The float is squashed into [-2, n], so i + 1 is outside whenever the
// true i + 1 is.
RX_AFF_HD RxAffAxis rx_aff_linear_axis(float p, int n) {
  RxAffAxis r;
  const float fl = floorf(p);
  r.f = p - fl;
  const int i = rx_aff_index(fl, n, -2.0f), j = i + 1;
  r.in0 = i >= 0 && i < n;
  r.in1 = j >= 0 && j < n;
  r.i0 = rx_aff_clampi(i, n);
  r.i1 = rx_aff_clampi(j, n);
  return r;
}

// nearest: floor(p + 0.5)
RX_AFF_HD RxAffAxis rx_aff_nearest_axis(float p, int n) {
  RxAffAxis r;
  const float h = p + 0.5f;
  const int i = rx_aff_index(floorf(h), n, -1.0f);
  r.in0 = r.in1 = i >= 0 && i < n;
  r.i0 = r.i1 = rx_aff_clampi(i, n);
  r.f = 0.0f;
  return r;
}

// lerp(a, b, f) = a + f * (b - a)
RX_AFF_HD float rx_aff_lerp(float a, float b, float f) {
  const float d = b - a;
  const float fd = f * d;
  return a + fd;
}

// one channel volume `src` (z, y, x contiguous, strides YX and X) at the taps of one voxel.  Every load goes through a clamped
// index; under RX_AFF_CONSTANT a tap whose true index was outside takes `fill` instead of what was loaded.
template <int INTERP, int BORDER>
RX_AFF_HD float rx_aff_sample(const float* src, long YX, int X, const RxAffAxis& az, const RxAffAxis& ay, const RxAffAxis& ax, float fill) {
  const long z0 = (long)az.i0 * YX, y0 = (long)ay.i0 * X;
  if (INTERP == RX_AFF_NEAREST) {
    const float v = src[z0 + y0 + ax.i0];
    return (BORDER == RX_AFF_CONSTANT && !(az.in0 && ay.in0 && ax.in0)) ? fill : v;
  }
  const long z1 = (long)az.i1 * YX, y1 = (long)ay.i1 * X;
  float v000 = src[z0 + y0 + ax.i0], v001 = src[z0 + y0 + ax.i1];
  float v010 = src[z0 + y1 + ax.i0], v011 = src[z0 + y1 + ax.i1];
  float v100 = src[z1 + y0 + ax.i0], v101 = src[z1 + y0 + ax.i1];
  float v110 = src[z1 + y1 + ax.i0], v111 = src[z1 + y1 + ax.i1];
  if (BORDER == RX_AFF_CONSTANT) {
    const bool zy00 = az.in0 && ay.in0, zy01 = az.in0 && ay.in1, zy10 = az.in1 && ay.in0, zy11 = az.in1 && ay.in1;
    v000 = (zy00 && ax.in0) ? v000 : fill, v001 = (zy00 && ax.in1) ? v001 : fill;
    v010 = (zy01 && ax.in0) ? v010 : fill, v011 = (zy01 && ax.in1) ? v011 : fill;
    v100 = (zy10 && ax.in0) ? v100 : fill, v101 = (zy10 && ax.in1) ? v101 : fill;
    v110 = (zy11 && ax.in0) ? v110 : fill, v111 = (zy11 && ax.in1) ? v111 : fill;
  }
  const float x00 = rx_aff_lerp(v000, v001, ax.f), x01 = rx_aff_lerp(v010, v011, ax.f);
  const float x10 = rx_aff_lerp(v100, v101, ax.f), x11 = rx_aff_lerp(v110, v111, ax.f);
  const float y0v = rx_aff_lerp(x00, x01, ay.f), y1v = rx_aff_lerp(x10, x11, ay.f);
  return rx_aff_lerp(y0v, y1v, az.f);
}

// out_c = (v0 * s_0 + v1 * s_1) + v2 * s_2
RX_AFF_HD float rx_aff_vector(float v0, float v1, float v2, float s0, float s1, float s2) {
  const float a = v0 * s0;
  const float b = v1 * s1;
  const float d = v2 * s2;
  const float ab = a + b;
  return ab + d;
}
