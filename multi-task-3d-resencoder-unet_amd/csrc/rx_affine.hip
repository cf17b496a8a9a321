// rx_affine.hip -- rotation and isotropic scaling about the patch centre of a contiguous fp32 (B, C, Z, Y, X) batch, with the
// vector rule of a 3-component field: one resampling pass per tensor,
//   out[b][c][o] = sum_k vector_b[c][k] * sample(in[b][k], point_b (o - centre) + centre)        (vector tensors)
//   out[b][c][o] =                        sample(in[b][c], point_b (o - centre) + centre)        (every other tensor)
// `sample` trilinear or nearest, out-of-volume taps a constant or clamped.  The ops are drawn and composed on the host
// (dataloading/spatial_device.py) and arrive as one `rx_affine_sample` per sample; the records ride in the KERNEL ARGUMENTS
// (RX_AFF_CHUNK samples per launch): no device table, no copy, no allocation.  The arithmetic is spatial_device.affine_numpy's,
// one float32 operation at a time (rx_affine_core.h; fp contraction is off for this file and denormals are kept), so the result
// has its bits.
//
// A workgroup owns a brick of RX_AFF_BX x RX_AFF_BY x RX_AFF_BZ output voxels of one sample: lanes run along x (a wave stores whole
// contiguous runs of RX_AFF_BX floats), the workgroup's waves stack along y, and every thread walks the brick's z planes.  The
// coordinates, indices, border flags and weights of a voxel are computed once and reused for every channel.  The source
// footprint of a brick is a slanted box of about its own volume: it is NOT staged in LDS -- neighbouring lanes share taps through
// the vector L1, and the z walk re-touches the lines of the previous plane; DESIGN §19 has the measurement behind that choice.
// Every load goes through an index clamped into the sample (rx_aff_*_axis), whatever the matrix holds.
#include "rx_common.h"
#include "rx_affine_core.h"

#pragma clang fp contract(off)

#define RX_AFF_CHUNK 16      // samples per launch: 16 x 72 bytes of kernel arguments
#ifndef RX_AFF_BX
#define RX_AFF_BX 32
#endif
#ifndef RX_AFF_BY
#define RX_AFF_BY 8
#endif
#ifndef RX_AFF_BZ
#define RX_AFF_BZ 4
#endif
#define RX_AFF_BLOCK (RX_AFF_BX * RX_AFF_BY)
static_assert(RX_AFF_BLOCK == 256 && RX_AFF_BX % 16 == 0, "a brick layer is one 256-thread workgroup, runs of at least 64 bytes");

struct AffArgs {
  rx_affine_sample s[RX_AFF_CHUNK];
  int C, Z, Y, X;
  int nbx, nby;      // bricks along x and y (z: the rest of grid.x)
  float fill;
};

template <int INTERP, int BORDER, bool VECTOR>
__global__ __launch_bounds__(RX_AFF_BLOCK) void affine_kernel(const float* __restrict__ in, float* __restrict__ out, const AffArgs a) {
  const int b = blockIdx.y;
  const rx_affine_sample& s = a.s[b];
  int brick = blockIdx.x;
  const int bx = brick % a.nbx;
  brick /= a.nbx;
  const int by = brick % a.nby, bz = brick / a.nby;
  const int ox = bx * RX_AFF_BX + (int)(threadIdx.x % RX_AFF_BX), oy = by * RX_AFF_BY + (int)(threadIdx.x / RX_AFF_BX);
  if (ox >= a.X || oy >= a.Y) return;      // (no barrier in this kernel)
  const float cz = rx_aff_centre(a.Z), cy = rx_aff_centre(a.Y), cx = rx_aff_centre(a.X);
  const float ty = (float)oy - cy, tx = (float)ox - cx;
  const long YX = (long)a.Y * a.X, vol = YX * a.Z;
  const float* __restrict__ src = in + (long)b * a.C * vol;
  float* __restrict__ dst = out + (long)b * a.C * vol + ((long)oy * a.X + ox);
  const int z0 = bz * RX_AFF_BZ, z1 = z0 + RX_AFF_BZ < a.Z ? z0 + RX_AFF_BZ : a.Z;
  for (int oz = z0; oz < z1; ++oz) {
    const float tz = (float)oz - cz;
    const float pz = rx_aff_coord(s.point[0], s.point[1], s.point[2], tz, ty, tx, cz);
    const float py = rx_aff_coord(s.point[3], s.point[4], s.point[5], tz, ty, tx, cy);
    const float px = rx_aff_coord(s.point[6], s.point[7], s.point[8], tz, ty, tx, cx);
    const RxAffAxis az = INTERP == RX_AFF_LINEAR ? rx_aff_linear_axis(pz, a.Z) : rx_aff_nearest_axis(pz, a.Z);
    const RxAffAxis ay = INTERP == RX_AFF_LINEAR ? rx_aff_linear_axis(py, a.Y) : rx_aff_nearest_axis(py, a.Y);
    const RxAffAxis ax = INTERP == RX_AFF_LINEAR ? rx_aff_linear_axis(px, a.X) : rx_aff_nearest_axis(px, a.X);
    float* __restrict__ o = dst + (long)oz * YX;
    if (VECTOR) {      // C == 3 (checked on the host)
      const float s0 = rx_aff_sample<INTERP, BORDER>(src, YX, a.X, az, ay, ax, a.fill);
      const float s1 = rx_aff_sample<INTERP, BORDER>(src + vol, YX, a.X, az, ay, ax, a.fill);
      const float s2 = rx_aff_sample<INTERP, BORDER>(src + 2 * vol, YX, a.X, az, ay, ax, a.fill);
      o[0] = rx_aff_vector(s.vector[0], s.vector[1], s.vector[2], s0, s1, s2);
      o[vol] = rx_aff_vector(s.vector[3], s.vector[4], s.vector[5], s0, s1, s2);
      o[2 * vol] = rx_aff_vector(s.vector[6], s.vector[7], s.vector[8], s0, s1, s2);
    } else {
      for (int c = 0; c < a.C; ++c) o[(long)c * vol] = rx_aff_sample<INTERP, BORDER>(src + (long)c * vol, YX, a.X, az, ay, ax, a.fill);
    }
  }
}

// ---- host side -----------------------------------------------------------------------------------------------------------------
template <int INTERP, int BORDER>
static void affine_launch(bool vector, dim3 grid, hipStream_t st, const float* in, float* out, const AffArgs& a) {
  if (vector)
    hipLaunchKernelGGL((affine_kernel<INTERP, BORDER, true>), grid, dim3(RX_AFF_BLOCK), 0, st, in, out, a);
  else
    hipLaunchKernelGGL((affine_kernel<INTERP, BORDER, false>), grid, dim3(RX_AFF_BLOCK), 0, st, in, out, a);
}

extern "C" int rx_affine_apply(const float* in, float* out, int batch, int c, int z, int y, int x, const rx_affine_sample* host_table,
                               int interp, int border, float fill, int vector, void* stream) {
  if (!in || !out) RX_FAIL(RX_EINVAL, "rx_affine_apply: null tensor pointer");
  if (in == out) RX_FAIL(RX_EINVAL, "rx_affine_apply: in place is not supported");
  if (!host_table) RX_FAIL(RX_EINVAL, "rx_affine_apply: null sample table");
  if (batch < 1 || c < 1 || z < 1 || y < 1 || x < 1)
    RX_FAIL(RX_EINVAL, "rx_affine_apply: batch and sizes must be positive (got %d x %d x %d x %d x %d)", batch, c, z, y, x);
  if (interp != RX_AFFINE_LINEAR && interp != RX_AFFINE_NEAREST) RX_FAIL(RX_EINVAL, "rx_affine_apply: unknown interp %d", interp);
  if (border != RX_AFFINE_CONSTANT && border != RX_AFFINE_CLAMP) RX_FAIL(RX_EINVAL, "rx_affine_apply: unknown border %d", border);
  if (vector && c != 3) RX_FAIL(RX_EINVAL, "rx_affine_apply: a vector tensor has 3 channels, not %d", c);
  // 32-bit indices inside one channel volume, float32 coordinates that hold every index exactly; rx_geom_apply's extent and
  // channel limits
  if ((long)z * y * x > 0x7fffffffL || z > 65535 || y > 65535 || x > (1 << 24) || c > 65535 / RX_AFF_CHUNK)
    RX_FAIL(RX_EINVAL, "rx_affine_apply: %d x %d x %d x %d per sample is beyond the index arithmetic (z * y * x < 2^31, z, y <= 65535, x <= 2^24, c <= %d)",
            c, z, y, x, 65535 / RX_AFF_CHUNK);
  for (int i = 0; i < batch; ++i)
    for (int k = 0; k < 9; ++k)
      if (!isfinite(host_table[i].point[k]) || !isfinite(host_table[i].vector[k]))
        RX_FAIL(RX_EINVAL, "rx_affine_apply: sample %d: matrix entry %d is not finite", i, k);
  const long vol = (long)z * y * x;
  const int nbx = (x + RX_AFF_BX - 1) / RX_AFF_BX, nby = (y + RX_AFF_BY - 1) / RX_AFF_BY, nbz = (z + RX_AFF_BZ - 1) / RX_AFF_BZ;
  const long bricks = (long)nbx * nby * nbz;
  if (bricks > 0x7fffffffL) RX_FAIL(RX_EINVAL, "rx_affine_apply: %ld bricks are beyond a grid dimension", bricks);
  hipStream_t st = (hipStream_t)stream;
  for (int b0 = 0; b0 < batch; b0 += RX_AFF_CHUNK) {
    const int nb = batch - b0 < RX_AFF_CHUNK ? batch - b0 : RX_AFF_CHUNK;
    AffArgs a;
    memset(&a, 0, sizeof(a));
    memcpy(a.s, host_table + b0, (size_t)nb * sizeof(rx_affine_sample));
    a.C = c, a.Z = z, a.Y = y, a.X = x, a.nbx = nbx, a.nby = nby, a.fill = fill;
    const float* in_b = in + (long)b0 * c * vol;      // 64-bit sample base
    float* out_b = out + (long)b0 * c * vol;
    const dim3 grid((unsigned)bricks, (unsigned)nb);
    if (interp == RX_AFFINE_LINEAR) {
      if (border == RX_AFFINE_CONSTANT) affine_launch<RX_AFF_LINEAR, RX_AFF_CONSTANT>(vector != 0, grid, st, in_b, out_b, a);
      else affine_launch<RX_AFF_LINEAR, RX_AFF_CLAMP>(vector != 0, grid, st, in_b, out_b, a);
    } else {
      if (border == RX_AFFINE_CONSTANT) affine_launch<RX_AFF_NEAREST, RX_AFF_CONSTANT>(vector != 0, grid, st, in_b, out_b, a);
      else affine_launch<RX_AFF_NEAREST, RX_AFF_CLAMP>(vector != 0, grid, st, in_b, out_b, a);
    }
    RX_CHECK_LAUNCH("rx_affine_apply");
  }
  return RX_OK;
}
