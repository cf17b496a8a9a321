// affine_host_check.cpp -- runs the per-voxel arithmetic of rx_affine_apply (../rx_affine_core.h, the functions the kernel calls)
// on the CPU over the cases of a dump written by tests/test_spatial_cpu.py and compares every output voxel with
// spatial_device.affine_numpy, bit for bit.  Built by that test with -fsanitize=address,undefined: every load goes through heap
// buffers of exactly the sample's size, so an index that left the sample would be reported.
//
//   dump := int32 n_cases, then per case: int32 C, Z, Y, X, interp, border, vector; float fill, point[9], vector[9];
//           float in[C*Z*Y*X]; float want[C*Z*Y*X]
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../rx_affine_core.h"

template <int INTERP, int BORDER>
static void run_case(const float* in, float* out, int C, int Z, int Y, int X, const float* m, const float* v, float fill, bool vector) {
  const long YX = (long)Y * X, vol = YX * Z;
  const float cz = rx_aff_centre(Z), cy = rx_aff_centre(Y), cx = rx_aff_centre(X);
  for (int oz = 0; oz < Z; ++oz)
    for (int oy = 0; oy < Y; ++oy)
      for (int ox = 0; ox < X; ++ox) {
        const float tz = (float)oz - cz, ty = (float)oy - cy, tx = (float)ox - cx;
        const float pz = rx_aff_coord(m[0], m[1], m[2], tz, ty, tx, cz);
        const float py = rx_aff_coord(m[3], m[4], m[5], tz, ty, tx, cy);
        const float px = rx_aff_coord(m[6], m[7], m[8], tz, ty, tx, cx);
        const RxAffAxis az = INTERP == RX_AFF_LINEAR ? rx_aff_linear_axis(pz, Z) : rx_aff_nearest_axis(pz, Z);
        const RxAffAxis ay = INTERP == RX_AFF_LINEAR ? rx_aff_linear_axis(py, Y) : rx_aff_nearest_axis(py, Y);
        const RxAffAxis ax = INTERP == RX_AFF_LINEAR ? rx_aff_linear_axis(px, X) : rx_aff_nearest_axis(px, X);
        float* o = out + (long)oz * YX + (long)oy * X + ox;
        if (vector) {
          const float s0 = rx_aff_sample<INTERP, BORDER>(in, YX, X, az, ay, ax, fill);
          const float s1 = rx_aff_sample<INTERP, BORDER>(in + vol, YX, X, az, ay, ax, fill);
          const float s2 = rx_aff_sample<INTERP, BORDER>(in + 2 * vol, YX, X, az, ay, ax, fill);
          for (int k = 0; k < 3; ++k) o[k * vol] = rx_aff_vector(v[3 * k], v[3 * k + 1], v[3 * k + 2], s0, s1, s2);
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
    int h[7];
    float fill, m[9], v[9];
    if (fread(h, 4, 7, f) != 7 || fread(&fill, 4, 1, f) != 1 || fread(m, 4, 9, f) != 9 || fread(v, 4, 9, f) != 9)
      return fprintf(stderr, "case %d: short header\n", i), 2;
    const int C = h[0], Z = h[1], Y = h[2], X = h[3], interp = h[4], border = h[5], vector = h[6];
    const size_t n = (size_t)C * Z * Y * X;
    std::vector<float> in(n), want(n), got(n);
    if (fread(in.data(), 4, n, f) != n || fread(want.data(), 4, n, f) != n) return fprintf(stderr, "case %d: short data\n", i), 2;
    if (interp == RX_AFF_LINEAR && border == RX_AFF_CONSTANT) run_case<RX_AFF_LINEAR, RX_AFF_CONSTANT>(in.data(), got.data(), C, Z, Y, X, m, v, fill, vector);
    else if (interp == RX_AFF_LINEAR) run_case<RX_AFF_LINEAR, RX_AFF_CLAMP>(in.data(), got.data(), C, Z, Y, X, m, v, fill, vector);
    else if (border == RX_AFF_CONSTANT) run_case<RX_AFF_NEAREST, RX_AFF_CONSTANT>(in.data(), got.data(), C, Z, Y, X, m, v, fill, vector);
    else run_case<RX_AFF_NEAREST, RX_AFF_CLAMP>(in.data(), got.data(), C, Z, Y, X, m, v, fill, vector);
    long bad = 0;
    for (size_t k = 0; k < n; ++k) bad += memcmp(&got[k], &want[k], 4) != 0;
    if (bad) printf("case %d (%d x %d x %d x %d, interp %d, border %d, vector %d): %ld of %zu voxels differ\n", i, C, Z, Y, X, interp, border, vector, bad, n);
    bad_total += bad;
  }
  fclose(f);
  printf("%d cases, %ld voxels differ\n", n_cases, bad_total);
  return bad_total ? 1 : 0;
}
