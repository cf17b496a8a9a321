// elastic_host_check.cpp -- runs the arithmetic of rx_elastic_apply (../rx_elastic_core.h and ../rx_affine_core.h, the functions
// the kernel calls) on the CPU over the cases of a dump written by tests/test_elastic_cpu.py and compares every output voxel with
// elastic_device.elastic_numpy, bit for bit.  Built by that test with -fsanitize=address,undefined: nodes, tables and samples
// sit in heap buffers of exactly their size, so an index that left one would be reported.  The sums are taken per voxel here
// (the kernel shares L1 and L2 across a brick: the same products in the same order).
//
//   dump := int32 n_cases, then per case: int32 C, Z, Y, X, interp, border, vector, sz, sy, sx; float fill;
//           float nodes[3*Gz*Gy*Gx] (G_d = (n_d - 1) / s_d + 4); per axis z, y, x: int32 idx[n], float w[4n], float dw[4n];
//           float in[C*Z*Y*X]; float want[C*Z*Y*X]
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../rx_elastic_core.h"

struct Axis {
  std::vector<int> idx;
  std::vector<float> w, dw;
};

// one of D_c (which = -1) or E[c][which]: dw on axis `which`, w on the others
static float field_sum(const float* nodes, int Gz, int Gy, int Gx, const Axis& tz, const Axis& ty, const Axis& tx, int c, int oz, int oy, int ox,
                       int which) {
  const float* wz = (which == 0 ? tz.dw : tz.w).data() + 4 * oz;
  const float* wy = (which == 1 ? ty.dw : ty.w).data() + 4 * oy;
  const float* wx = (which == 2 ? tx.dw : tx.w).data() + 4 * ox;
  const int iz = rx_ela_clampi(tz.idx[oz], Gz - 4), iy = rx_ela_clampi(ty.idx[oy], Gy - 4), ix = rx_ela_clampi(tx.idx[ox], Gx - 4);
  const long GYX = (long)Gy * Gx;
  float l2[4];
  for (int k = 0; k < 4; ++k) {
    float l1[4];
    for (int b = 0; b < 4; ++b) {
      const float* p = nodes + ((long)c * Gz + iz) * GYX + (long)(iy + b) * Gx + (ix + k);
      l1[b] = rx_ela_sum4(wz, p[0], p[GYX], p[2 * GYX], p[3 * GYX]);
    }
    l2[k] = rx_ela_sum4(wy, l1[0], l1[1], l1[2], l1[3]);
  }
  return rx_ela_sum4(wx, l2[0], l2[1], l2[2], l2[3]);
}

template <int INTERP, int BORDER>
static void run_case(const float* in, float* out, int C, int Z, int Y, int X, const float* nodes, const int* G, const Axis* t, float fill,
                     bool vector) {
  const long YX = (long)Y * X, vol = YX * Z;
  for (int oz = 0; oz < Z; ++oz)
    for (int oy = 0; oy < Y; ++oy)
      for (int ox = 0; ox < X; ++ox) {
        float D[3];
        for (int c = 0; c < 3; ++c) D[c] = field_sum(nodes, G[0], G[1], G[2], t[0], t[1], t[2], c, oz, oy, ox, -1);
        const float pz = rx_ela_coord(oz, D[0]), py = rx_ela_coord(oy, D[1]), px = rx_ela_coord(ox, D[2]);
        const RxAffAxis az = INTERP == RX_AFF_LINEAR ? rx_aff_linear_axis(pz, Z) : rx_aff_nearest_axis(pz, Z);
        const RxAffAxis ay = INTERP == RX_AFF_LINEAR ? rx_aff_linear_axis(py, Y) : rx_aff_nearest_axis(py, Y);
        const RxAffAxis ax = INTERP == RX_AFF_LINEAR ? rx_aff_linear_axis(px, X) : rx_aff_nearest_axis(px, X);
        float* o = out + (long)oz * YX + (long)oy * X + ox;
        if (vector) {
          float E[3][3];
          for (int d = 0; d < 3; ++d)
            for (int e = 0; e < 3; ++e) E[d][e] = field_sum(nodes, G[0], G[1], G[2], t[0], t[1], t[2], d, oz, oy, ox, e);
          const float s0 = rx_aff_sample<INTERP, BORDER>(in, YX, X, az, ay, ax, fill);
          const float s1 = rx_aff_sample<INTERP, BORDER>(in + vol, YX, X, az, ay, ax, fill);
          const float s2 = rx_aff_sample<INTERP, BORDER>(in + 2 * vol, YX, X, az, ay, ax, fill);
          rx_ela_vector(E, s0, s1, s2, o, o + vol, o + 2 * vol);
        } else {
          for (int c = 0; c < C; ++c) o[c * vol] = rx_aff_sample<INTERP, BORDER>(in + c * vol, YX, X, az, ay, ax, fill);
        }
      }
}

int main(int argc, char** argv) {
  if (argc != 2) return fprintf(stderr, "usage: %s dump\n", argv[0]), 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return perror(argv[1]), 2;
  int n_cases = 0;
  if (fread(&n_cases, 4, 1, f) != 1) return fprintf(stderr, "empty dump\n"), 2;
  long bad_total = 0;
  for (int i = 0; i < n_cases; ++i) {
    int h[10];
    float fill;
    if (fread(h, 4, 10, f) != 10 || fread(&fill, 4, 1, f) != 1) return fprintf(stderr, "case %d: short header\n", i), 2;
    const int C = h[0], ext[3] = {h[1], h[2], h[3]}, interp = h[4], border = h[5], vector = h[6];
    int G[3];
    for (int d = 0; d < 3; ++d) {
      if (ext[d] < 1 || h[7 + d] < 1) return fprintf(stderr, "case %d: bad extent or spacing\n", i), 2;
      G[d] = (ext[d] - 1) / h[7 + d] + 4;
    }
    const size_t ng = (size_t)3 * G[0] * G[1] * G[2], n = (size_t)C * ext[0] * ext[1] * ext[2];
    std::vector<float> nodes(ng), in(n), want(n), got(n);
    if (fread(nodes.data(), 4, ng, f) != ng) return fprintf(stderr, "case %d: short nodes\n", i), 2;
    Axis t[3];
    for (int d = 0; d < 3; ++d) {
      const size_t e = (size_t)ext[d];
      t[d].idx.resize(e), t[d].w.resize(4 * e), t[d].dw.resize(4 * e);
      if (fread(t[d].idx.data(), 4, e, f) != e || fread(t[d].w.data(), 4, 4 * e, f) != 4 * e || fread(t[d].dw.data(), 4, 4 * e, f) != 4 * e)
        return fprintf(stderr, "case %d: short tables\n", i), 2;
    }
    if (fread(in.data(), 4, n, f) != n || fread(want.data(), 4, n, f) != n) return fprintf(stderr, "case %d: short data\n", i), 2;
    const int Z = ext[0], Y = ext[1], X = ext[2];
    if (interp == RX_AFF_LINEAR && border == RX_AFF_CONSTANT) run_case<RX_AFF_LINEAR, RX_AFF_CONSTANT>(in.data(), got.data(), C, Z, Y, X, nodes.data(), G, t, fill, vector);
    else if (interp == RX_AFF_LINEAR) run_case<RX_AFF_LINEAR, RX_AFF_CLAMP>(in.data(), got.data(), C, Z, Y, X, nodes.data(), G, t, fill, vector);
    else if (border == RX_AFF_CONSTANT) run_case<RX_AFF_NEAREST, RX_AFF_CONSTANT>(in.data(), got.data(), C, Z, Y, X, nodes.data(), G, t, fill, vector);
    else run_case<RX_AFF_NEAREST, RX_AFF_CLAMP>(in.data(), got.data(), C, Z, Y, X, nodes.data(), G, t, fill, vector);
    long bad = 0;
    for (size_t k = 0; k < n; ++k) bad += memcmp(&got[k], &want[k], 4) != 0;
    if (bad) printf("case %d (%d x %d x %d x %d, interp %d, border %d, vector %d): %ld of %zu voxels differ\n", i, C, Z, Y, X, interp, border, vector, bad, n);
    bad_total += bad;
  }
  fclose(f);
  printf("%d cases, %ld voxels differ\n", n_cases, bad_total);
  return bad_total ? 1 : 0;
}
