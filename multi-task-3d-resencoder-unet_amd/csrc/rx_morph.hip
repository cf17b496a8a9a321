// rx_morph.hip -- binary dilation of label targets with the digital ball of radius r (skimage.morphology.ball(r): the voxels with
// dz^2 + dy^2 + dx^2 <= r^2), on a contiguous fp32 (B, C, Z, Y, X) batch, every (sample, channel) volume on its own:
//   out[v] = 1.0f if some voxel u with in[u] > 0.0f lies within |u - v|^2 <= r^2, else +0.0f;   nothing outside the volume is on.
// The behaviour is the reference's `dilate_label` (dataloading/dataset.py: dilation(t > 0, ball(5))); the host statement is
// dataloading/dilate_device.py: dilate_numpy.  0/1 data in and out: there is no floating-point arithmetic in this file.
//
// The ball is a union of x-runs: for every (dz, dy) with dz^2 + dy^2 <= r^2 it holds |dx| <= h(dz, dy) = isqrt(r^2 - dz^2 - dy^2).
// Two launches:
//   dilate_pack_kernel     the fp32 input -> one bit per voxel, 64 voxels of a row to a word (bit i of word w is x = 64 w + i; the
//                          bits of a row's last word beyond x are 0).  A wave reads 256 contiguous bytes per word, __ballot is the
//                          word.  This is the only read of the input, so out == in is allowed.
//   dilate_unpack_kernel   a lane owns one output word; the lanes of a wave own consecutive words, so every load below is one
//                          contiguous piece of a bit row.  Dilating by an x-run commutes with OR, so the rows of all runs of ONE
//                          half-width h are ORed first (the word and its two x-neighbours: three ORs per run) and shifted once per
//                          distinct h (h < 64: one neighbour word on each side is enough) -- r = 5: 81 runs, 5 half-widths.  The
//                          eight waves of a workgroup share the same 64 words and split the runs; their partial words meet in LDS
//                          (4 KiB), then each wave writes 8 of the words as 8 x 64 floats, 256 contiguous bytes per store.
// The bit volume is 1/32 of the input (256 KiB for 2 x 128^3) and is served from L2; HBM sees one fp32 read and one fp32 write
// per voxel.  The run table rides in the kernel arguments (< 512 bytes), grouped by half-width on the host.
#include "rx_common.h"

#define RX_DIL_BLOCK 512            // the unpack kernel: 8 waves share 64 words (short load chains, 8 waves per SIMD resident)
#define RX_DIL_WAVES (RX_DIL_BLOCK / 64)
#define RX_DIL_PACK_BLOCK 256
#define RX_DIL_PACK_WAVES (RX_DIL_PACK_BLOCK / 64)
#define RX_DIL_MAX_RADIUS 8
#define RX_DIL_MAX_RUNS 200         // (dz, dy) with dz^2 + dy^2 <= 64: 197
#define RX_DIL_PACK_WORDS 4         // words per wave of the pack kernel: four independent 256-byte loads in flight

struct DilRuns {
  int8_t dz[RX_DIL_MAX_RUNS], dy[RX_DIL_MAX_RUNS];
  int16_t start[RX_DIL_MAX_RADIUS + 2];      // the runs of half-width h are entries start[h] .. start[h + 1] - 1
};

// ---- fp32 -> bits ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(RX_DIL_PACK_BLOCK) void dilate_pack_kernel(const float* __restrict__ in, unsigned long long* __restrict__ bits,
                                                                   int X, int W, int nwords) {
  const int lane = threadIdx.x & 63;      // word indices fit 32 bits (checked on the host): 64-bit division is emulated and costly
  const int w0 = (blockIdx.x * RX_DIL_PACK_WAVES + (threadIdx.x >> 6)) * RX_DIL_PACK_WORDS;
  float v[RX_DIL_PACK_WORDS];
#pragma unroll
  for (int k = 0; k < RX_DIL_PACK_WORDS; ++k) {
    const int g = w0 + k;
    v[k] = 0.0f;
    if (g < nwords) {
      const int row = g / W;
      const int x = (g - row * W) * 64 + lane;
      if (x < X) v[k] = in[(long)row * X + x];
    }
  }
#pragma unroll
  for (int k = 0; k < RX_DIL_PACK_WORDS; ++k) {
    const unsigned long long word = __ballot(v[k] > 0.0f);      // NaN, -0.0 and negatives compare false
    if (lane == 0 && w0 + k < nwords) bits[w0 + k] = word;
  }
}

// ---- bits -> dilated fp32 ----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(RX_DIL_BLOCK) void dilate_unpack_kernel(const unsigned long long* __restrict__ bits, float* __restrict__ out,
                                                                     const DilRuns t, int radius, int Z, int Y, int X, int W,
                                                                     int nwords) {
  __shared__ unsigned long long part[RX_DIL_WAVES][64];
  __shared__ long obase[64];      // element offset of each word's first voxel in `out` ...
  __shared__ int ox[64];          // ... and its x
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);      // uniform: the run loop and its table reads stay scalar
  // workgroups that share bit rows (neighbours in y and z) run on one XCD and meet in its L2 (a speed choice only)
  const int first = rx_xcd_remap((int)blockIdx.x, (int)gridDim.x) * 64;      // word indices fit 32 bits (checked on the host)
  const int g = first + lane < nwords ? first + lane : nwords - 1;      // lanes past the end redo the last word and store nothing
  const int row = g / W;                                                   // ((v * Z + z) * Y + y)
  const int w = g - row * W;
  const int zrow = row / Y;
  const int y = row - zrow * Y, z = zrow % Z;
  const unsigned long long* __restrict__ p0 = bits + (long)row * W;
  const int wl = w > 0 ? w - 1 : w, wr = w + 1 < W ? w + 1 : w;
  const unsigned long long ml = w > 0 ? ~0ull : 0ull, mr = w + 1 < W ? ~0ull : 0ull;
  unsigned long long acc = 0;
  for (int h = 0; h <= radius; ++h) {
    unsigned long long c = 0, l = 0, r = 0;
    const int end = t.start[h + 1];
#pragma unroll 4
    for (int i = t.start[h] + wave; i < end; i += RX_DIL_WAVES) {
      const int dz = t.dz[i], dy = t.dy[i];
      const bool ok = (unsigned)(z + dz) < (unsigned)Z && (unsigned)(y + dy) < (unsigned)Y;      // rows out of range count as zero:
      const unsigned long long* __restrict__ q = p0 + (ok ? ((long)dz * Y + dy) * W : 0l);       // load the lane's own row, mask it
      const unsigned long long m = ok ? ~0ull : 0ull;
      c |= q[w] & m;
      l |= q[wl] & (m & ml);
      r |= q[wr] & (m & mr);
    }
    acc |= c;
    for (int d = 1; d <= h; ++d) acc |= (c << d) | (l >> (64 - d)) | (c >> d) | (r << (64 - d));
  }
  part[wave][lane] = acc;
  if (wave == 0) obase[lane] = (long)row * X + w * 64, ox[lane] = w * 64;
  __syncthreads();
  constexpr int PER = 64 / RX_DIL_WAVES;
#pragma unroll 4
  for (int j = 0; j < PER; ++j) {
    const int k = wave * PER + j;
    if (first + k >= nwords) break;
    unsigned long long word = part[0][k];
#pragma unroll
    for (int u = 1; u < RX_DIL_WAVES; ++u) word |= part[u][k];
    if (ox[k] + lane < X) out[obase[k] + lane] = (word >> lane) & 1ull ? 1.0f : 0.0f;
  }
}

// ---- host side -----------------------------------------------------------------------------------------------------------------
static bool dilate_sizes_ok(int batch, int c, int z, int y, int x) { return batch > 0 && c > 0 && z > 0 && y > 0 && x > 0; }

static long dilate_words(int batch, int c, int z, int y, int x) { return (long)batch * c * z * y * ((x + 63) / 64); }
#define RX_DIL_MAX_WORDS 0x7fffff00L      // 32-bit word indices in the kernels (2^37 voxels: more than a device holds)

extern "C" size_t rx_dilate_workspace(int batch, int c, int z, int y, int x) {
  if (!dilate_sizes_ok(batch, c, z, y, x)) return 0;
  return (size_t)dilate_words(batch, c, z, y, x) * sizeof(unsigned long long);
}

extern "C" int rx_label_dilate(const float* in, float* out, void* scratch, size_t scratch_bytes, int batch, int c, int z, int y,
                               int x, int radius, void* stream) {
  if (!in || !out) RX_FAIL(RX_EINVAL, "rx_label_dilate: null tensor pointer");
  if (!scratch) RX_FAIL(RX_EINVAL, "rx_label_dilate: null scratch pointer");
  if (!dilate_sizes_ok(batch, c, z, y, x))
    RX_FAIL(RX_EINVAL, "rx_label_dilate: batch and sizes must be positive (got %d x %d x %d x %d x %d)", batch, c, z, y, x);
  if (radius < 1 || radius > RX_DIL_MAX_RADIUS)
    RX_FAIL(RX_EINVAL, "rx_label_dilate: radius %d is outside 1..%d", radius, RX_DIL_MAX_RADIUS);
  const long nwords = dilate_words(batch, c, z, y, x);
  if ((long)z * y * x > 0x7fffffffL || nwords > RX_DIL_MAX_WORDS)
    RX_FAIL(RX_EINVAL, "rx_label_dilate: %d x %d x %d x %d x %d is beyond the index arithmetic (z * y * x < 2^31 per sample, "
            "fewer than 2^31 words of 64 voxels in all)", batch, c, z, y, x);
  if (((uintptr_t)scratch & 7) != 0) RX_FAIL(RX_EINVAL, "rx_label_dilate: scratch must be 8-byte aligned");
  if (scratch_bytes < rx_dilate_workspace(batch, c, z, y, x))
    RX_FAIL(RX_EWORKSPACE, "rx_label_dilate: scratch of %zu bytes, rx_dilate_workspace says %zu", scratch_bytes,
            rx_dilate_workspace(batch, c, z, y, x));
  // the runs (dz, dy, h) in (dz, dy) order, bucketed by h
  DilRuns t;
  memset(&t, 0, sizeof(t));
  int n = 0;
  for (int h = 0; h <= radius; ++h) {
    t.start[h] = (int16_t)n;
    for (int dz = -radius; dz <= radius; ++dz)
      for (int dy = -radius; dy <= radius; ++dy) {
        const int rest = radius * radius - dz * dz - dy * dy;
        if (rest < 0) continue;
        int hh = 0;
        while ((hh + 1) * (hh + 1) <= rest) ++hh;
        if (hh == h) t.dz[n] = (int8_t)dz, t.dy[n] = (int8_t)dy, ++n;
      }
  }
  t.start[radius + 1] = (int16_t)n;
  const int W = (x + 63) / 64;
  hipStream_t st = (hipStream_t)stream;
  unsigned long long* bits = (unsigned long long*)scratch;
  const long per_block = (long)RX_DIL_PACK_WAVES * RX_DIL_PACK_WORDS;
  hipLaunchKernelGGL(dilate_pack_kernel, dim3((unsigned)((nwords + per_block - 1) / per_block)), dim3(RX_DIL_PACK_BLOCK), 0, st, in, bits,
                     x, W, (int)nwords);
  RX_CHECK_LAUNCH("rx_label_dilate");
  hipLaunchKernelGGL(dilate_unpack_kernel, dim3((unsigned)((nwords + 63) / 64)), dim3(RX_DIL_BLOCK), 0, st,
                     (const unsigned long long*)bits, out, t, radius, z, y, x, W, (int)nwords);
  RX_CHECK_LAUNCH("rx_label_dilate");
  return RX_OK;
}
