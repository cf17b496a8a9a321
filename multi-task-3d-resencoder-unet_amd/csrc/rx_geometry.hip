// rx_geometry.hip -- axis flips and 90-degree rotations (and every composition of them) of a contiguous fp32 (B, C, Z, Y, X)
// batch, with the component rule of a 3-vector field: one gather pass per tensor,
//   out[b][c][o] = (+/-) in[b][ch(c)][src(o)],
// `src` a signed permutation of the (z, y, x) axes, `ch` a signed permutation of the three components (identity for tensors that
// are not vector fields).  The behaviour is the reference's training/transforms/geometric/geometry.py (RandomFlipWithNormals,
// RandomRotate90WithNormals); the ops are drawn and composed on the host (dataloading/geometry_device.py) and arrive as one
// `rx_geom_sample` per sample.  The host checks each and turns it into a base offset and three signed element strides
// (rx_geom_core.h, shared with the test-time-augmentation entry points of rx_infer.hip), so the device computes
//   src(o) = base + oz * sz + oy * sy + ox * sx
// and the records ride in the KERNEL ARGUMENTS (RX_GEOM_CHUNK samples per launch): no device table, no copy, no allocation.
// Two access patterns, picked per sample; a workgroup belongs to one sample, so the choice is a scalar branch:
//   geom_rows_kernel   x stays innermost (src_axis[2] == 2): whole rows move.  16 bytes per lane when x % 4 == 0 and the buffers are
//                      16-byte aligned (an x flip reads the mirrored quad and reverses it in registers), 4 bytes otherwise.
//   geom_tile_kernel   x moves (odd rotations about z or y and what they compose to): a 64 x 64 tile of the (input-x, output-x)
//                      plane goes through LDS -- loads run along input x, stores along output x, 256 contiguous bytes per wave
//                      either way.  Tile rows are padded to 65 words: ds_write_b32 / ds_read_b32 bank = word % 32 within a
//                      32-lane half, the row-wise write meets banks (65 r + l) % 32 and the transposed read (65 l + r) % 32 =
//                      (l + r) % 32 -- 32 different banks per half both ways.
// Negation flips the sign bit (an XOR on the bits: 0.0 becomes -0.0, as numpy's unary minus and `*= -1` give); there is no
// floating-point arithmetic in this file.  Every output voxel is written once by one thread.
#include "rx_common.h"
#include "rx_geom_core.h"

#define RX_GEOM_BLOCK 256
#define RX_GEOM_CHUNK 16      // samples per launch: 16 x 36 bytes of kernel arguments
#define RX_GEOM_TILE 64
#define RX_GEOM_LDS_ROW 65

struct GeomArgs {
  RxGeomView s[RX_GEOM_CHUNK];   // feeds == 2: the row kernel's sample; 0 or 1: the tile kernel's
  int C, Z, Y, X, XQ;       // XQ: quads of 4 voxels per row
  int vol;                  // Z * Y * X (checked < 2^31 on the host)
  int vector;
};

__device__ inline void geom_channel(const RxGeomView& s, int vector, int c, int& cin, uint32_t& sign) {
  cin = c, sign = 0u;
  if (vector) {
    cin = c == 0 ? s.ch[0] : c == 1 ? s.ch[1] : s.ch[2];
    sign = ((s.neg >> c) & 1u) << 31;
  }
}

// ---- x stays innermost ---------------------------------------------------------------------------------------------------------
template <bool VEC>
__global__ __launch_bounds__(RX_GEOM_BLOCK) void geom_rows_kernel(const uint32_t* __restrict__ in, uint32_t* __restrict__ out,
                                                                  const GeomArgs a) {
  const int bc = blockIdx.y, b = bc / a.C, c = bc - b * a.C;
  const RxGeomView& s = a.s[b];
  if (s.feeds != 2) return;      // the tile kernel's sample
  int cin;
  uint32_t sign;
  geom_channel(s, a.vector, c, cin, sign);
  const uint32_t* __restrict__ src = in + ((long)b * a.C + cin) * a.vol;
  uint32_t* __restrict__ dst = out + (long)bc * a.vol;
  const long ql = (long)blockIdx.x * RX_GEOM_BLOCK + threadIdx.x;      // the last block may reach past 2^31
  if (ql >= (VEC ? (long)a.Z * a.Y * a.XQ : (long)a.vol)) return;
  const int q = (int)ql;
  if (VEC) {
    const int xq = q % a.XQ, r = q / a.XQ;
    const int y = r % a.Y, z = r / a.Y;
    const int x0 = 4 * xq;
    const int row = s.base + z * s.sz + y * s.sy;      // source of output x = 0
    u32x4 v;
    if (s.sx == 1) {
      v = *reinterpret_cast<const u32x4*>(src + row + x0);
    } else {      // outputs x0 .. x0+3 read row - x0 .. row - x0 - 3: one aligned quad (x % 4 == 0), reversed
      const u32x4 t = *reinterpret_cast<const u32x4*>(src + row - x0 - 3);
      v = u32x4{t[3], t[2], t[1], t[0]};
    }
    v ^= u32x4{sign, sign, sign, sign};
    *reinterpret_cast<u32x4*>(dst + (z * a.Y + y) * a.X + x0) = v;
  } else {
    const int x = q % a.X, r = q / a.X;
    const int y = r % a.Y, z = r / a.Y;
    dst[q] = src[s.base + z * s.sz + y * s.sy + x * s.sx] ^ sign;
  }
}

// ---- x moves: output x walks input axis z or y, and input x feeds output axis z or y ----------------------------------------------
// grid.x: tiles of (output x = j, the output axis fed by input x = k); grid.y: the third output axis; grid.z: (sample, channel)
__global__ __launch_bounds__(RX_GEOM_BLOCK) void geom_tile_kernel(const uint32_t* __restrict__ in, uint32_t* __restrict__ out,
                                                                  const GeomArgs a) {
  __shared__ uint32_t tile[RX_GEOM_TILE * RX_GEOM_LDS_ROW];
  const int bc = blockIdx.z, b = bc / a.C, c = bc - b * a.C;
  const RxGeomView& s = a.s[b];
  if (s.feeds == 2) return;      // the row kernel's sample
  // input x feeds output axis k (z or y, source stride +/-1); the other one of the two is the third axis (e)
  const bool k_is_z = s.feeds == 0;
  const int nk = k_is_z ? a.Z : a.Y, ne = k_is_z ? a.Y : a.Z;
  const int sk = k_is_z ? s.sz : s.sy, se = k_is_z ? s.sy : s.sz;
  const int ok = k_is_z ? a.Y * a.X : a.X, oe = k_is_z ? a.X : a.Y * a.X;      // output strides of k and e
  const int e = blockIdx.y;
  if (e >= ne) return;      // grid.y is max(Z, Y): the samples of a launch may differ in which axis is the third
  const int tiles_j = (a.X + RX_GEOM_TILE - 1) / RX_GEOM_TILE, tiles_k = (nk + RX_GEOM_TILE - 1) / RX_GEOM_TILE;
  const int tj = blockIdx.x % tiles_j, tk = blockIdx.x / tiles_j;
  if (tk >= tiles_k) return;
  const int j0 = tj * RX_GEOM_TILE, k0 = tk * RX_GEOM_TILE;
  int cin;
  uint32_t sign;
  geom_channel(s, a.vector, c, cin, sign);
  const uint32_t* __restrict__ src = in + ((long)b * a.C + cin) * a.vol + (s.base + e * se);
  uint32_t* __restrict__ dst = out + (long)bc * a.vol + e * oe;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  constexpr int ROWS = RX_GEOM_TILE / (RX_GEOM_BLOCK / 64);      // 16 tile rows per wave
  // load: tile row = j (a step of sx in the input), lanes along k (input x, ascending or descending): contiguous per wave
  uint32_t v[ROWS];
  const int k = k0 + lane;
#pragma unroll
  for (int i = 0; i < ROWS; ++i) {
    const int j = j0 + wave * ROWS + i;
    v[i] = (j < a.X && k < nk) ? src[j * s.sx + k * sk] : 0u;
  }
#pragma unroll
  for (int i = 0; i < ROWS; ++i) tile[(wave * ROWS + i) * RX_GEOM_LDS_ROW + lane] = v[i];
  __syncthreads();
  // store: row = k, lanes along j (output x)
  const int j = j0 + lane;
#pragma unroll
  for (int i = 0; i < ROWS; ++i) {
    const int kr = wave * ROWS + i;
    const uint32_t t = tile[lane * RX_GEOM_LDS_ROW + kr] ^ sign;
    if (j < a.X && k0 + kr < nk) dst[(k0 + kr) * ok + j] = t;
  }
}

// ---- host side -----------------------------------------------------------------------------------------------------------------
extern "C" int rx_geom_apply(const float* in, float* out, int batch, int c, int z, int y, int x, const rx_geom_sample* host_table,
                             int vector, void* stream) {
  if (!in || !out) RX_FAIL(RX_EINVAL, "rx_geom_apply: null tensor pointer");
  if (in == out) RX_FAIL(RX_EINVAL, "rx_geom_apply: in place is not supported");
  if (!host_table) RX_FAIL(RX_EINVAL, "rx_geom_apply: null sample table");
  if (batch < 1 || c < 1 || z < 1 || y < 1 || x < 1)
    RX_FAIL(RX_EINVAL, "rx_geom_apply: batch and sizes must be positive (got %d x %d x %d x %d x %d)", batch, c, z, y, x);
  if (vector && c != 3) RX_FAIL(RX_EINVAL, "rx_geom_apply: a vector tensor has 3 channels, not %d", c);
  // 32-bit element offsets inside one channel volume; grid.y carries an extent or 16 * c, grid.z 16 * c
  if ((long)z * y * x > 0x7fffffffL || z > 65535 || y > 65535 || c > 65535 / RX_GEOM_CHUNK)
    RX_FAIL(RX_EINVAL, "rx_geom_apply: %d x %d x %d x %d per sample is beyond the 32-bit index arithmetic (z * y * x < 2^31, z, y <= 65535, c <= %d)",
            c, z, y, x, 65535 / RX_GEOM_CHUNK);
  for (int i = 0; i < batch; ++i)
    if (const int verdict = rx_geom_check(host_table, z, y, x, i)) {
      char text[160];
      rx_geom_refusal(text, sizeof(text), verdict, host_table, z, y, x, i, "sample", "shape");
      RX_FAIL(RX_EINVAL, "rx_geom_apply: %s", text);
    }
  const bool vec = (x & 3) == 0 && (((uintptr_t)in | (uintptr_t)out) & 15) == 0;
  const long vol = (long)z * y * x;
  hipStream_t st = (hipStream_t)stream;
  for (int b0 = 0; b0 < batch; b0 += RX_GEOM_CHUNK) {
    const int nb = batch - b0 < RX_GEOM_CHUNK ? batch - b0 : RX_GEOM_CHUNK;
    GeomArgs a;
    memset(&a, 0, sizeof(a));
    a.C = c, a.Z = z, a.Y = y, a.X = x, a.XQ = (x + 3) / 4, a.vol = (int)vol, a.vector = vector ? 1 : 0;
    bool rows = false, tiles = false;
    for (int i = 0; i < nb; ++i) {
      a.s[i] = rx_geom_lower(host_table[b0 + i], z, y, x);
      if (a.s[i].feeds == 2) rows = true;
      else tiles = true;
    }
    const float* in_b = in + (long)b0 * c * vol;
    float* out_b = out + (long)b0 * c * vol;
    if (rows) {
      const long n = vec ? (long)z * y * a.XQ : vol;
      const dim3 grid((unsigned)((n + RX_GEOM_BLOCK - 1) / RX_GEOM_BLOCK), (unsigned)(nb * c));
      if (vec)
        hipLaunchKernelGGL(geom_rows_kernel<true>, grid, dim3(RX_GEOM_BLOCK), 0, st, (const uint32_t*)in_b, (uint32_t*)out_b, a);
      else
        hipLaunchKernelGGL(geom_rows_kernel<false>, grid, dim3(RX_GEOM_BLOCK), 0, st, (const uint32_t*)in_b, (uint32_t*)out_b, a);
    }
    if (tiles) {
      const int tj = (x + RX_GEOM_TILE - 1) / RX_GEOM_TILE;
      const int tk = ((z > y ? z : y) + RX_GEOM_TILE - 1) / RX_GEOM_TILE;
      const dim3 grid((unsigned)(tj * tk), (unsigned)(z > y ? z : y), (unsigned)(nb * c));
      hipLaunchKernelGGL(geom_tile_kernel, grid, dim3(RX_GEOM_BLOCK), 0, st, (const uint32_t*)in_b, (uint32_t*)out_b, a);
    }
    RX_CHECK_LAUNCH("rx_geom_apply");
  }
  return RX_OK;
}
