// rx_elastic.hip -- smooth non-rigid deformation of a contiguous fp32 (B, C, Z, Y, X) batch, with the vector rule of a
// 3-component normal field: one resampling pass per tensor,
//   out[b][c][o] = sample(in[b][c], o + D_b(o))                                      (every tensor)
//   out[b][.][o] = (I + E_b(o))^T sample(in[b][.], o + D_b(o)), at the sampled length   (vector tensors)
// D_b is a cubic B-spline displacement field over a coarse node lattice (device, (B, 3, Gz, Gy, Gx)), E_b its Jacobian.  The
// output grid is regular, so the splines arrive as per-axis tables (first node, four weights, four weight derivatives per
// voxel index): the kernel never evaluates a polynomial.  The arithmetic is elastic_device.elastic_numpy's, one float32
// operation at a time (rx_elastic_core.h, rx_affine_core.h; fp contraction is off for this file and denormals are kept), so the
// result has its bits.
//
// A workgroup owns a brick of RX_ELA_BX x RX_ELA_BY x RX_ELA_BZ output voxels of one sample: the 64 lanes of a wave run along x
// (a wave stores whole contiguous runs of 64 floats; lanes past X are masked: the tail), the four waves stack along y, and every
// thread walks the brick's z planes.  The sums are separable in the order z, y, x, and the workgroup shares the first two:
//   per plane   L1[kind][c][r][col] = sum_a (w_z | dw_z)[oz][a] * nodes[c][iz + a][gy0 + r][gx0 + col]      built cooperatively
//   per row     L2[row][line][col]  = sum_b (w_y | dw_y)[oy][b] * L1[..][c][iy - gy0 + b][col]              built cooperatively
//   per voxel   D_c = sum_k w_x[ox][k] * L2[row][c][ix - gx0 + k]                      4 products per voxel and component
// With a spacing >= 8 the 64 voxels of a row touch at most 12 node columns and the 4 rows of a brick at most 5 node rows, so the
// LDS lines have a FIXED size (3.2 KB with the six derivative lines of a vector tensor), whatever the lattice is.  Nodes and
// tables are a few KB per sample and stay in L1 / L2.  The coordinates, indices, border flags and weights of a voxel are
// computed once and reused for every channel; source voxels are read through L1 / L2 as rx_affine_apply reads them (DESIGN
// section 21).  Every load goes through a clamped index -- node indices into the lattice, line offsets into the LDS lines,
// source indices into the sample (rx_aff_*_axis) -- whatever the nodes and the tables hold.
#include "rx_common.h"
#include "rx_elastic_core.h"

#pragma clang fp contract(off)

#define RX_ELA_BX 64
#define RX_ELA_BY 4
#ifndef RX_ELA_BZ
#define RX_ELA_BZ 8
#endif
#define RX_ELA_BLOCK (RX_ELA_BX * RX_ELA_BY)
#define RX_ELA_MIN_SPACING 8
#define RX_ELA_NC 12      // node columns under 64 voxels: ceil(63 / 8) + 1 + 3
#define RX_ELA_NR 5       // node rows under 4 voxels:     ceil(3 / 8) + 1 + 3
static_assert(RX_ELA_BLOCK == 256 && RX_ELA_BX == 64, "a brick layer is one 256-thread workgroup, one wave per x row");
static_assert(RX_ELA_NC == (RX_ELA_BX - 1 + RX_ELA_MIN_SPACING - 1) / RX_ELA_MIN_SPACING + 4, "node columns of a row");
static_assert(RX_ELA_NR == (RX_ELA_BY - 1 + RX_ELA_MIN_SPACING - 1) / RX_ELA_MIN_SPACING + 4, "node rows of a brick");

struct ElaArgs {
  rx_elastic_tables t;
  int C, Z, Y, X;
  int Gz, Gy, Gx;
  int nbx, nby;      // bricks along x and y (z: the rest of grid.x)
  float fill;
};

template <int INTERP, int BORDER, bool VECTOR>
__global__ __launch_bounds__(RX_ELA_BLOCK) void elastic_kernel(const float* __restrict__ in, float* __restrict__ out,
                                                               const float* __restrict__ nodes, const ElaArgs a) {
  constexpr int K1 = VECTOR ? 2 : 1;      // L1 kinds: w_z, dw_z
  constexpr int NL = VECTOR ? 9 : 3;      // L2 lines per row: (w_z, w_y) x 3, then (dw_z, w_y) x 3, (w_z, dw_y) x 3
  __shared__ float L1[K1][3][RX_ELA_NR][RX_ELA_NC];
  __shared__ float L2[RX_ELA_BY][NL][RX_ELA_NC];
  const int tid = (int)threadIdx.x, lane = tid % RX_ELA_BX, row = tid / RX_ELA_BX;
  const int b = blockIdx.y;
  int brick = blockIdx.x;
  const int bx = brick % a.nbx;
  brick /= a.nbx;
  const int by = brick % a.nby, bz = brick / a.nby;
  const int ox0 = bx * RX_ELA_BX, oy0 = by * RX_ELA_BY;      // both inside the sample: the brick exists
  const int ox = ox0 + lane, oy = oy0 + row;
  const bool valid = ox < a.X && oy < a.Y;                   // (no early return: the barriers below are for everybody)
  const int oxc = ox < a.X ? ox : a.X - 1, oyc = oy < a.Y ? oy : a.Y - 1;
  const int gx0 = rx_ela_clampi(a.t.x.idx[ox0], a.Gx - 4), gy0 = rx_ela_clampi(a.t.y.idx[oy0], a.Gy - 4);
  // this thread's voxel column and row: constant over the z walk
  const int cx = rx_ela_clampi(a.t.x.idx[oxc] - gx0, RX_ELA_NC - 4);
  float wx[4], dwx[4];
  for (int k = 0; k < 4; ++k) wx[k] = a.t.x.w[4 * oxc + k], dwx[k] = a.t.x.dw[4 * oxc + k];
  const long YX = (long)a.Y * a.X, vol = YX * a.Z;
  const float* __restrict__ src = in + (long)b * a.C * vol;
  float* __restrict__ dst = out + (long)b * a.C * vol + ((long)oyc * a.X + oxc);
  const long GYX = (long)a.Gy * a.Gx;
  const float* __restrict__ nb = nodes + (long)b * 3 * a.Gz * GYX;
  const int z0 = bz * RX_ELA_BZ, z1 = z0 + RX_ELA_BZ < a.Z ? z0 + RX_ELA_BZ : a.Z;
  for (int oz = z0; oz < z1; ++oz) {
    const int iz = rx_ela_clampi(a.t.z.idx[oz], a.Gz - 4);
    for (int t = tid; t < K1 * 3 * RX_ELA_NR * RX_ELA_NC; t += RX_ELA_BLOCK) {
      const int col = t % RX_ELA_NC, r = (t / RX_ELA_NC) % RX_ELA_NR, c = (t / (RX_ELA_NC * RX_ELA_NR)) % 3;
      const int kind = t / (RX_ELA_NC * RX_ELA_NR * 3);
      const int gy = rx_ela_clampi(gy0 + r, a.Gy - 1), gx = rx_ela_clampi(gx0 + col, a.Gx - 1);
      const float* __restrict__ p = nb + ((long)c * a.Gz + iz) * GYX + (long)gy * a.Gx + gx;
      const float* __restrict__ w = (kind ? a.t.z.dw : a.t.z.w) + 4 * oz;
      L1[kind][c][r][col] = rx_ela_sum4(w, p[0], p[GYX], p[2 * GYX], p[3 * GYX]);
    }
    __syncthreads();
    for (int t = tid; t < RX_ELA_BY * NL * RX_ELA_NC; t += RX_ELA_BLOCK) {
      const int col = t % RX_ELA_NC, line = (t / RX_ELA_NC) % NL, rw = t / (RX_ELA_NC * NL);
      const int c = line % 3, kind = line / 3;
      const int oyr = oy0 + rw < a.Y ? oy0 + rw : a.Y - 1;
      const int ry = rx_ela_clampi(a.t.y.idx[oyr] - gy0, RX_ELA_NR - 4);
      const float* __restrict__ w = (kind == 2 ? a.t.y.dw : a.t.y.w) + 4 * oyr;
      const int k1 = (VECTOR && kind == 1) ? 1 : 0;
      L2[rw][line][col] = rx_ela_sum4(w, L1[k1][c][ry][col], L1[k1][c][ry + 1][col], L1[k1][c][ry + 2][col], L1[k1][c][ry + 3][col]);
    }
    __syncthreads();      // (the next plane's L1 is written after every read of this one's: the barrier above; its L2 after the
                          //  barrier that follows, which no thread reaches before it has left the voxel below)
    if (!valid) continue;
    const float* l2 = &L2[row][0][cx];
    const float dz = rx_ela_sum4(wx, l2[0], l2[1], l2[2], l2[3]);
    const float dy = rx_ela_sum4(wx, l2[RX_ELA_NC], l2[RX_ELA_NC + 1], l2[RX_ELA_NC + 2], l2[RX_ELA_NC + 3]);
    const float dx = rx_ela_sum4(wx, l2[2 * RX_ELA_NC], l2[2 * RX_ELA_NC + 1], l2[2 * RX_ELA_NC + 2], l2[2 * RX_ELA_NC + 3]);
    const float pz = rx_ela_coord(oz, dz), py = rx_ela_coord(oy, dy), px = rx_ela_coord(ox, dx);
    const RxAffAxis az = INTERP == RX_AFF_LINEAR ? rx_aff_linear_axis(pz, a.Z) : rx_aff_nearest_axis(pz, a.Z);
    const RxAffAxis ay = INTERP == RX_AFF_LINEAR ? rx_aff_linear_axis(py, a.Y) : rx_aff_nearest_axis(py, a.Y);
    const RxAffAxis ax = INTERP == RX_AFF_LINEAR ? rx_aff_linear_axis(px, a.X) : rx_aff_nearest_axis(px, a.X);
    float* __restrict__ o = dst + (long)oz * YX;
    if (VECTOR) {      // C == 3 (checked on the host)
      float E[3][3];
      for (int d = 0; d < 3; ++d) {
        const float* lz = l2 + (3 + d) * RX_ELA_NC;
        const float* ly = l2 + (6 + d) * RX_ELA_NC;
        const float* lx = l2 + d * RX_ELA_NC;
        E[d][0] = rx_ela_sum4(wx, lz[0], lz[1], lz[2], lz[3]);
        E[d][1] = rx_ela_sum4(wx, ly[0], ly[1], ly[2], ly[3]);
        E[d][2] = rx_ela_sum4(dwx, lx[0], lx[1], lx[2], lx[3]);
      }
      const float s0 = rx_aff_sample<INTERP, BORDER>(src, YX, a.X, az, ay, ax, a.fill);
      const float s1 = rx_aff_sample<INTERP, BORDER>(src + vol, YX, a.X, az, ay, ax, a.fill);
      const float s2 = rx_aff_sample<INTERP, BORDER>(src + 2 * vol, YX, a.X, az, ay, ax, a.fill);
      float r0, r1, r2;
      rx_ela_vector(E, s0, s1, s2, &r0, &r1, &r2);
      o[0] = r0;
      o[vol] = r1;
      o[2 * vol] = r2;
    } else {
      for (int c = 0; c < a.C; ++c) o[(long)c * vol] = rx_aff_sample<INTERP, BORDER>(src + (long)c * vol, YX, a.X, az, ay, ax, a.fill);
    }
  }
}

// ---- host side -----------------------------------------------------------------------------------------------------------------
template <int INTERP, int BORDER>
static void elastic_launch(bool vector, dim3 grid, hipStream_t st, const float* in, float* out, const float* nodes, const ElaArgs& a) {
  if (vector)
    hipLaunchKernelGGL((elastic_kernel<INTERP, BORDER, true>), grid, dim3(RX_ELA_BLOCK), 0, st, in, out, nodes, a);
  else
    hipLaunchKernelGGL((elastic_kernel<INTERP, BORDER, false>), grid, dim3(RX_ELA_BLOCK), 0, st, in, out, nodes, a);
}

extern "C" int rx_elastic_apply(const float* in, float* out, int batch, int c, int z, int y, int x, const float* nodes,
                                const int32_t spacing[3], const rx_elastic_tables* tables, int interp, int border, float fill,
                                int vector, void* stream) {
  if (!in || !out) RX_FAIL(RX_EINVAL, "rx_elastic_apply: null tensor pointer");
  if (in == out) RX_FAIL(RX_EINVAL, "rx_elastic_apply: in place is not supported");
  if (!nodes || !spacing || !tables) RX_FAIL(RX_EINVAL, "rx_elastic_apply: null nodes, spacing or tables");
  const rx_elastic_axis* ax[3] = {&tables->z, &tables->y, &tables->x};
  for (int d = 0; d < 3; ++d)
    if (!ax[d]->idx || !ax[d]->w || !ax[d]->dw) RX_FAIL(RX_EINVAL, "rx_elastic_apply: null table pointer (axis %d)", d);
  if (batch < 1 || c < 1 || z < 1 || y < 1 || x < 1)
    RX_FAIL(RX_EINVAL, "rx_elastic_apply: batch and sizes must be positive (got %d x %d x %d x %d x %d)", batch, c, z, y, x);
  if (interp != RX_AFFINE_LINEAR && interp != RX_AFFINE_NEAREST) RX_FAIL(RX_EINVAL, "rx_elastic_apply: unknown interp %d", interp);
  if (border != RX_AFFINE_CONSTANT && border != RX_AFFINE_CLAMP) RX_FAIL(RX_EINVAL, "rx_elastic_apply: unknown border %d", border);
  if (vector && c != 3) RX_FAIL(RX_EINVAL, "rx_elastic_apply: a vector tensor has 3 channels, not %d", c);
  for (int d = 0; d < 3; ++d)
    if (spacing[d] < RX_ELA_MIN_SPACING)
      RX_FAIL(RX_EINVAL, "rx_elastic_apply: spacing %d x %d x %d: every axis needs at least %d voxels between nodes (the LDS lines are sized for it)",
              spacing[0], spacing[1], spacing[2], RX_ELA_MIN_SPACING);
  // rx_affine_apply's limits: 32-bit indices inside one channel volume, float32 coordinates that hold every index exactly; the
  // batch rides in grid.y
  if ((long)z * y * x > 0x7fffffffL || z > 65535 || y > 65535 || x > (1 << 24) || c > 4095 || batch > 65535)
    RX_FAIL(RX_EINVAL, "rx_elastic_apply: %d x %d x %d x %d x %d is beyond the index arithmetic (z * y * x < 2^31, z, y <= 65535, x <= 2^24, c <= 4095, batch <= 65535)",
            batch, c, z, y, x);
  const int nbx = (x + RX_ELA_BX - 1) / RX_ELA_BX, nby = (y + RX_ELA_BY - 1) / RX_ELA_BY, nbz = (z + RX_ELA_BZ - 1) / RX_ELA_BZ;
  const long bricks = (long)nbx * nby * nbz;
  if (bricks > 0x7fffffffL) RX_FAIL(RX_EINVAL, "rx_elastic_apply: %ld bricks are beyond a grid dimension", bricks);
  ElaArgs a;
  memset(&a, 0, sizeof(a));
  a.t = *tables;
  a.C = c, a.Z = z, a.Y = y, a.X = x, a.nbx = nbx, a.nby = nby, a.fill = fill;
  a.Gz = (z - 1) / spacing[0] + 4, a.Gy = (y - 1) / spacing[1] + 4, a.Gx = (x - 1) / spacing[2] + 4;
  const dim3 grid((unsigned)bricks, (unsigned)batch);
  hipStream_t st = (hipStream_t)stream;
  if (interp == RX_AFFINE_LINEAR) {
    if (border == RX_AFFINE_CONSTANT) elastic_launch<RX_AFF_LINEAR, RX_AFF_CONSTANT>(vector != 0, grid, st, in, out, nodes, a);
    else elastic_launch<RX_AFF_LINEAR, RX_AFF_CLAMP>(vector != 0, grid, st, in, out, nodes, a);
  } else {
    if (border == RX_AFFINE_CONSTANT) elastic_launch<RX_AFF_NEAREST, RX_AFF_CONSTANT>(vector != 0, grid, st, in, out, nodes, a);
    else elastic_launch<RX_AFF_NEAREST, RX_AFF_CLAMP>(vector != 0, grid, st, in, out, nodes, a);
  }
  RX_CHECK_LAUNCH("rx_elastic_apply");
  return RX_OK;
}
