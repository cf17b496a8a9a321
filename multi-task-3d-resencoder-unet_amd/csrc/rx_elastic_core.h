// rx_elastic_core.h -- the arithmetic of rx_elastic_apply (rx_elastic.hip) that is new over rx_affine_core.h, host- and
// device-callable: the kernel calls these functions, and a plain C++ program runs the same ones on the CPU
// (tools/elastic_host_check.cpp does, under AddressSanitizer, against a dump of dataloading/elastic_device.py: elastic_numpy).
// The statement is elastic_numpy's docstring; every line below is one float32 operation of it, in its order.  NOTHING here may
// be contracted into an fma.  From the coordinate on, sampling is rx_affine_core.h's (rx_aff_linear_axis, rx_aff_nearest_axis,
// rx_aff_sample): every load goes through an index clamped into the sample, whatever the nodes hold.
#pragma once
#include "rx_affine_core.h"

#pragma clang fp contract(off)

#define RX_ELA_HD RX_AFF_HD

// sum_a w[a] * v_a: the first product, then + the others left to right
RX_ELA_HD float rx_ela_sum4(const float* w, float v0, float v1, float v2, float v3) {
  const float p0 = w[0] * v0;
  const float p1 = w[1] * v1;
  const float p2 = w[2] * v2;
  const float p3 = w[3] * v3;
  const float a = p0 + p1;
  const float b = a + p2;
  return b + p3;
}

// an index from a device table, forced into [0, hi]: a table of anything cannot steer a load out of its array
RX_ELA_HD int rx_ela_clampi(int i, int hi) { return i < 0 ? 0 : (i > hi ? hi : i); }

// p_d = float32(o_d) + D_d
RX_ELA_HD float rx_ela_coord(int o, float d) { return (float)o + d; }

// the vector rule.  s: the sampled components (Nx, Ny, Nz); E[d][e] = dD_d / do_e in (z, y, x) order:
//   (n_z, n_y, n_x) = (s2, s1, s0)      t_e = n_e + ((E[z][e] * n_z + E[y][e] * n_y) + E[x][e] * n_x)
//   q = (s0*s0 + s1*s1) + s2*s2         r = (t_x*t_x + t_y*t_y) + t_z*t_z         k = sqrt(q / r) if r > 0 else 0
//   out = (t_x, t_y, t_z) * k           (sqrt and / correctly rounded: IEEE on the host, hipcc's default on the device)
RX_ELA_HD void rx_ela_vector(const float E[3][3], float s0, float s1, float s2, float* o0, float* o1, float* o2) {
  const float n[3] = {s2, s1, s0};
  float t[3];
  for (int e = 0; e < 3; ++e) {
    const float a = E[0][e] * n[0];
    const float b = E[1][e] * n[1];
    const float d = E[2][e] * n[2];
    const float ab = a + b;
    const float abd = ab + d;
    t[e] = n[e] + abd;
  }
  const float q0 = s0 * s0, q1 = s1 * s1, q2 = s2 * s2;
  const float q01 = q0 + q1;
  const float q = q01 + q2;
  const float r0 = t[2] * t[2], r1 = t[1] * t[1], r2 = t[0] * t[0];
  const float r01 = r0 + r1;
  const float r = r01 + r2;
  float k = 0.0f;
  if (r > 0.0f) {
    const float qr = q / r;
    k = sqrtf(qr);
  }
  *o0 = t[2] * k;
  *o1 = t[1] * k;
  *o2 = t[0] * k;
}
