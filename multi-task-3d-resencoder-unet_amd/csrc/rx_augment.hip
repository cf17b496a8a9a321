// rx_augment.hip -- the per-item training augmentation stack (reference dataloading/dataset.py:171-205, restated on the host in
// dataloading/augment.py) on the contiguous fp32 (B, C, Z, Y, X) image batch as it sits in HBM.  Parameters are DRAWN ON THE HOST
// (dataloading/augment_device.py: draw_params) and arrive as one table per batch: B `rx_aug_sample` records followed by a pool of
// 4-byte words (the (Z, Y) factor planes, the k x k filter weights, the index tables of downscale).  Two passes:
//   rx_aug_pointwise   groups 1 and 2 (clip(v * F + b), F a scalar or a (Z, Y) plane; or clip(v + sigma * n(key, voxel))) and, for
//                      a sample WITHOUT a group-3 member, the dropout boxes: in -> out.  A sample with a group-3 member goes to
//                      the scratch batch instead and gets its boxes at the end of the next pass (dropout comes last on the host).
//   rx_aug_filter_zy   group 3, scratch -> out: a k x k correlation in the (Z, Y) plane (the same kernel for every x, border
//                      reflect-101) or the nearest-neighbour gather of downscale; then clip, then the boxes.
// Every output voxel is written by one thread from a fixed-order sum: no atomics, no float reductions, bit-reproducible.
// Floating-point contraction is off in this file: every product and sum rounds like the numpy statement it restates
// (augment_device.apply_params_numpy).
#include "rx_common.h"

#pragma clang fp contract(off)

#define RX_AUG_BLOCK 256
// filter tile: 16 x 16 x 16 outputs per workgroup; a thread owns 4 consecutive x (one 16-byte LDS read) of 4 consecutive y
#define RX_AUG_T 16
#define RX_AUG_RY 4
// LDS row of 16 floats padded to 20 and the plane stride rounded up to 64 words: the four 16-lane groups of ds_read_b128 then
// meet four different 16-bank quarters of the 64-bank row (y-group stride 4 * 20 = 80 words = 16 mod 64, z stride = 0 mod 64)
#define RX_AUG_ROW 20

struct AugGeom {
  int B, C, Z, Y, X, XQ;   // XQ: quads of 4 voxels per row
  long vol;                // Z * Y * X
};

__device__ inline float aug_clip(float v) { return fminf(fmaxf(v, 0.f), 1.f); }

// ---- noise generator: Philox4x32-10 (Salmon et al., SC'11), key = the patch's 64-bit key, counter = (voxel / 4, 0, 0, 0) ---------
__device__ inline void aug_philox(uint32_t ctr_lo, uint32_t ctr_hi, uint32_t k0, uint32_t k1, uint32_t (&r)[4]) {
  uint32_t c0 = ctr_lo, c1 = ctr_hi, c2 = 0u, c3 = 0u;
#pragma unroll
  for (int i = 0; i < 10; ++i) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    const uint32_t n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
    c0 = n0, c1 = lo1, c2 = n2, c3 = lo0;
    k0 += 0x9E3779B9u, k1 += 0xBB67AE85u;
  }
  r[0] = c0, r[1] = c1, r[2] = c2, r[3] = c3;
}

// the top 24 bits -> a uniform in (0, 1], exact in fp32; two Box-Muller pairs with the accurate logf / sincosf
__device__ inline float aug_uniform(uint32_t r) { return (float)((r >> 8) + 1u) * 5.9604644775390625e-8f; }

__device__ inline void aug_normals(long quad, uint32_t k0, uint32_t k1, float (&n)[4]) {
  uint32_t r[4];
  aug_philox((uint32_t)quad, (uint32_t)((unsigned long)quad >> 32), k0, k1, r);
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    const float rad = sqrtf(-2.0f * logf(aug_uniform(r[2 * p])));
    float s, c;
    sincosf(6.28318530717958647692f * aug_uniform(r[2 * p + 1]), &s, &c);
    n[2 * p] = rad * c, n[2 * p + 1] = rad * s;
  }
}

__device__ inline float aug_boxes(const rx_aug_sample& s, int z, int y, int x, float v) {
  for (int i = 0; i < s.nbox; ++i) {
    const int32_t* bx = s.box[i];
    if (z >= bx[0] && z < bx[0] + bx[3] && y >= bx[1] && y < bx[1] + bx[4] && x >= bx[2] && x < bx[2] + bx[5]) v = s.fill;
  }
  return v;
}

template <bool VEC>
__device__ inline void aug_load4(const float* __restrict__ row, int x0, int X, float (&v)[4]) {
  if (VEC) {      // X % 4 == 0 and a 16-byte aligned batch: a quad is inside the row or outside it as a whole
    const f32x4 t = *reinterpret_cast<const f32x4*>(row + x0);
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = t[i];
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = x0 + i < X ? row[x0 + i] : 0.f;
  }
}

template <bool VEC>
__device__ inline void aug_store4(float* __restrict__ row, int x0, int X, const float (&v)[4]) {
  if (VEC) {
    *reinterpret_cast<f32x4*>(row + x0) = f32x4{v[0], v[1], v[2], v[3]};
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (x0 + i < X) row[x0 + i] = v[i];
  }
}

// ---- pass 1: pointwise stages (+ boxes when no group-3 member follows) -----------------------------------------------------
template <bool VEC>
__global__ __launch_bounds__(RX_AUG_BLOCK) void aug_pointwise_kernel(const float* __restrict__ in, float* __restrict__ out,
                                                                     float* __restrict__ scratch,
                                                                     const rx_aug_sample* __restrict__ S,
                                                                     const float* __restrict__ pool, AugGeom g) {
  const long q = (long)blockIdx.x * RX_AUG_BLOCK + threadIdx.x;
  if (q >= (long)g.Z * g.Y * g.XQ) return;
  const int bc = blockIdx.y, b = bc / g.C;
  const rx_aug_sample& s = S[b];      // wave-uniform: scalar loads
  const int xq = (int)(q % g.XQ);
  const int y = (int)((q / g.XQ) % g.Y), z = (int)(q / ((long)g.XQ * g.Y));
  const int x0 = 4 * xq;
  const long rowoff = (long)bc * g.vol + ((long)z * g.Y + y) * g.X;
  float v[4];
  aug_load4<VEC>(in + rowoff, x0, g.X, v);
#pragma unroll
  for (int st = 0; st < 2; ++st) {
    const int mode = s.pw_mode[st];
    if (mode == RX_AUG_PW_AFFINE || mode == RX_AUG_PW_PLANE) {
      const float f = mode == RX_AUG_PW_PLANE ? pool[s.pw_off[st] + z * g.Y + y] : s.pw_a[st];
      const float off = s.pw_b[st];
#pragma unroll
      for (int i = 0; i < 4; ++i) v[i] = aug_clip(v[i] * f + off);
    } else if (mode == RX_AUG_PW_NOISE) {
      const float sigma = s.pw_a[st];
      const long lin = ((long)z * g.Y + y) * g.X + x0;      // channel excluded: every channel of a patch gets the same noise
      if (VEC) {
        float n[4];
        aug_normals(lin >> 2, s.key_lo, s.key_hi, n);
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = aug_clip(v[i] + sigma * n[i]);
      } else {      // a quad of the row straddles two counters
        float n[4];
        long have = -1;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const long l = lin + i;
          if ((l >> 2) != have) aug_normals(l >> 2, s.key_lo, s.key_hi, n), have = l >> 2;
          const int lane = (int)(l & 3);
          const float ni = lane == 0 ? n[0] : lane == 1 ? n[1] : lane == 2 ? n[2] : n[3];
          v[i] = aug_clip(v[i] + sigma * ni);
        }
      }
    }
  }
  if (s.g3_mode == RX_AUG_G3_NONE) {
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = aug_boxes(s, z, y, x0 + i, v[i]);
    aug_store4<VEC>(out + rowoff, x0, g.X, v);
  } else {
    aug_store4<VEC>(scratch + rowoff, x0, g.X, v);
  }
}

// ---- pass 2a: k x k correlation in the (Z, Y) plane ----------------------------------------------------------------------------
// scipy's "mirror" (cv2 reflect-101): period 2 (n - 1), any distance outside the array
__device__ inline int aug_mirror(int i, int n) {
  if (n == 1) return 0;
  const int m = 2 * (n - 1);
  i %= m;
  if (i < 0) i += m;
  return i < n ? i : m - i;
}

template <int K, bool VEC>
__global__ __launch_bounds__(RX_AUG_BLOCK) void aug_filter_kernel(const float* __restrict__ src, float* __restrict__ out,
                                                                  const rx_aug_sample* __restrict__ S,
                                                                  const float* __restrict__ pool, AugGeom g, int tiles_x,
                                                                  int tiles_y) {
  constexpr int H = RX_AUG_T + K - 1, R = K / 2;
  constexpr int PLANE = ((RX_AUG_T + K - 1) * RX_AUG_ROW + 63) / 64 * 64;
  __shared__ __attribute__((aligned(16))) float tile[H * PLANE];
  const int bc = blockIdx.z, b = bc / g.C;
  const rx_aug_sample& s = S[b];
  if (s.g3_mode != RX_AUG_G3_FILTER || s.k != K) return;      // block-uniform: this instantiation serves the samples with its k
  int t = blockIdx.x;
  const int x0 = (t % tiles_x) * RX_AUG_T;
  t /= tiles_x;
  const int y0 = (t % tiles_y) * RX_AUG_T, z0 = (t / tiles_y) * RX_AUG_T;
  const float* vol = src + (long)bc * g.vol;
  // stage the (16 + K - 1)^2 x 16 halo once; columns beyond X are zero-filled and never stored
  for (int i = threadIdx.x; i < H * H * 4; i += RX_AUG_BLOCK) {
    const int xq = i & 3, hy = (i >> 2) % H, hz = (i >> 2) / H;
    const int gz = aug_mirror(z0 - R + hz, g.Z), gy = aug_mirror(y0 - R + hy, g.Y), gx = x0 + 4 * xq;
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    if (gx < g.X) aug_load4<VEC>(vol + ((long)gz * g.Y + gy) * g.X, gx, g.X, v);
    *reinterpret_cast<f32x4*>(&tile[hz * PLANE + hy * RX_AUG_ROW + 4 * xq]) = f32x4{v[0], v[1], v[2], v[3]};
  }
  __syncthreads();
  const int xq = threadIdx.x & 3, yq = (threadIdx.x >> 2) & 3, tz = threadIdx.x >> 4;
  const float* __restrict__ w = pool + s.g3_off;      // uniform address: the k weights of a tap row are scalar loads
  f32x4 acc[RX_AUG_RY];
#pragma unroll
  for (int r = 0; r < RX_AUG_RY; ++r) acc[r] = f32x4{0.f, 0.f, 0.f, 0.f};
  // taps in row-major order for every output; one 16-byte LDS read feeds up to RY x 4 multiply-adds
#pragma unroll 1
  for (int dz = 0; dz < K; ++dz) {
    const float* rowp = &tile[(tz + dz) * PLANE + (yq * RX_AUG_RY) * RX_AUG_ROW + 4 * xq];
    float wr[K];
#pragma unroll
    for (int dy = 0; dy < K; ++dy) wr[dy] = w[dz * K + dy];
#pragma unroll
    for (int j = 0; j < K + RX_AUG_RY - 1; ++j) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(rowp + j * RX_AUG_ROW);
#pragma unroll
      for (int r = 0; r < RX_AUG_RY; ++r) {
        const int dy = j - r;
        if (dy >= 0 && dy < K) acc[r] = acc[r] + wr[dy] * v;
      }
    }
  }
  const int z = z0 + tz, gx = x0 + 4 * xq;
  if (z >= g.Z || gx >= g.X) return;
#pragma unroll
  for (int r = 0; r < RX_AUG_RY; ++r) {
    const int y = y0 + yq * RX_AUG_RY + r;
    if (y >= g.Y) break;
    float o[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) o[i] = aug_boxes(s, z, y, gx + i, aug_clip(acc[r][i]));
    aug_store4<VEC>(out + (long)bc * g.vol + ((long)z * g.Y + y) * g.X, gx, g.X, o);
  }
}

// ---- pass 2b: downscale = nearest-neighbour gather through the composed (down, up) index tables ---------------------------------
template <bool VEC>
__global__ __launch_bounds__(RX_AUG_BLOCK) void aug_downscale_kernel(const float* __restrict__ src, float* __restrict__ out,
                                                                     const rx_aug_sample* __restrict__ S,
                                                                     const float* __restrict__ pool, AugGeom g) {
  const long q = (long)blockIdx.x * RX_AUG_BLOCK + threadIdx.x;
  if (q >= (long)g.Z * g.Y * g.XQ) return;
  const int bc = blockIdx.y, b = bc / g.C;
  const rx_aug_sample& s = S[b];
  if (s.g3_mode != RX_AUG_G3_DOWNSCALE) return;
  const int xq = (int)(q % g.XQ);
  const int y = (int)((q / g.XQ) % g.Y), z = (int)(q / ((long)g.XQ * g.Y));
  const int32_t* idx = reinterpret_cast<const int32_t*>(pool) + s.g3_off;      // Z source rows, then Y source columns
  const int sz = idx[z], sy = idx[g.Z + y];
  float v[4];
  aug_load4<VEC>(src + (long)bc * g.vol + ((long)sz * g.Y + sy) * g.X, 4 * xq, g.X, v);
#pragma unroll
  for (int i = 0; i < 4; ++i) v[i] = aug_boxes(s, z, y, 4 * xq + i, v[i]);
  aug_store4<VEC>(out + (long)bc * g.vol + ((long)z * g.Y + y) * g.X, 4 * xq, g.X, v);
}

// test-only: the raw 32-bit Philox outputs of the first n voxels of a patch (out[i] = philox(key, i / 4)[i % 4])
__global__ __launch_bounds__(RX_AUG_BLOCK) void aug_philox_kernel(uint32_t k0, uint32_t k1, long n, uint32_t* __restrict__ out) {
  const long q = (long)blockIdx.x * RX_AUG_BLOCK + threadIdx.x;
  if (4 * q >= n) return;
  uint32_t r[4];
  aug_philox((uint32_t)q, (uint32_t)((unsigned long)q >> 32), k0, k1, r);
  for (int i = 0; i < 4 && 4 * q + i < n; ++i) out[4 * q + i] = r[i];
}

// ---- host side -----------------------------------------------------------------------------------------------------------------
// everything a kernel will index with is checked here, on the host copy of the records, before anything is launched
static int aug_check(const char* who, const void* a, const void* b, int batch, int c, int z, int y, int x,
                     const rx_aug_sample* samples, const void* table, long pool_words, AugGeom& g, bool& any_g3) {
  if (!a || !b) RX_FAIL(RX_EINVAL, "%s: null batch pointer", who);
  if (batch < 1 || c < 1 || z < 1 || y < 1 || x < 1) RX_FAIL(RX_EINVAL, "%s: batch and sizes must be positive (got %d x %d x %d x %d x %d)", who, batch, c, z, y, x);
  if ((long)batch * c > 65535) RX_FAIL(RX_EUNSUPPORTED, "%s: batch * channels > 65535", who);
  if (!samples || !table) RX_FAIL(RX_EINVAL, "%s: null parameter table", who);
  if (((uintptr_t)table & 15) || pool_words < 0) RX_FAIL(RX_EINVAL, "%s: the device table must be 16-byte aligned", who);
  any_g3 = false;
  for (int i = 0; i < batch; ++i) {
    const rx_aug_sample& s = samples[i];
    for (int st = 0; st < 2; ++st) {
      const int m = s.pw_mode[st];
      if (m < RX_AUG_PW_NONE || m > RX_AUG_PW_NOISE) RX_FAIL(RX_EINVAL, "%s: sample %d: unknown pointwise mode %d", who, i, m);
      if (m == RX_AUG_PW_PLANE && (s.pw_off[st] < 0 || (long)s.pw_off[st] + (long)z * y > pool_words))
        RX_FAIL(RX_EINVAL, "%s: sample %d: factor plane outside the table", who, i);
    }
    if (s.g3_mode < RX_AUG_G3_NONE || s.g3_mode > RX_AUG_G3_DOWNSCALE) RX_FAIL(RX_EINVAL, "%s: sample %d: unknown group-3 mode %d", who, i, s.g3_mode);
    if (s.g3_mode == RX_AUG_G3_FILTER) {
      if (s.k < 3 || s.k > RX_AUG_MAX_K || !(s.k & 1)) RX_FAIL(RX_EINVAL, "%s: sample %d: filter size %d (odd, 3..%d)", who, i, s.k, RX_AUG_MAX_K);
      if (s.g3_off < 0 || (long)s.g3_off + s.k * s.k > pool_words) RX_FAIL(RX_EINVAL, "%s: sample %d: filter weights outside the table", who, i);
    } else if (s.g3_mode == RX_AUG_G3_DOWNSCALE) {
      if (s.g3_off < 0 || (long)s.g3_off + z + y > pool_words) RX_FAIL(RX_EINVAL, "%s: sample %d: index tables outside the table", who, i);
      const int32_t* idx = reinterpret_cast<const int32_t*>(samples + batch) + s.g3_off;      // the host image has the same layout
      for (int j = 0; j < z + y; ++j)
        if (idx[j] < 0 || idx[j] >= (j < z ? z : y)) RX_FAIL(RX_EINVAL, "%s: sample %d: downscale index %d out of range", who, i, idx[j]);
    }
    any_g3 = any_g3 || s.g3_mode != RX_AUG_G3_NONE;
    if (s.nbox < 0 || s.nbox > RX_AUG_MAX_BOXES) RX_FAIL(RX_EINVAL, "%s: sample %d: %d dropout boxes (0..%d)", who, i, s.nbox, RX_AUG_MAX_BOXES);
    for (int j = 0; j < s.nbox; ++j) {
      const int32_t* bx = s.box[j];
      if (bx[0] < 0 || bx[1] < 0 || bx[2] < 0 || bx[3] < 1 || bx[4] < 1 || bx[5] < 1 || bx[0] + bx[3] > z || bx[1] + bx[4] > y || bx[2] + bx[5] > x)
        RX_FAIL(RX_EINVAL, "%s: sample %d: dropout box %d leaves the patch", who, i, j);
    }
  }
  g.B = batch, g.C = c, g.Z = z, g.Y = y, g.X = x, g.XQ = (x + 3) / 4;
  g.vol = (long)z * y * x;
  return RX_OK;
}

extern "C" size_t rx_aug_workspace(int batch, int c, int z, int y, int x) {
  if (batch < 1 || c < 1 || z < 1 || y < 1 || x < 1) return 0;
  return (size_t)batch * c * z * y * x * sizeof(float);
}

extern "C" int rx_aug_pointwise(const float* in, float* out, float* scratch, size_t scratch_bytes, int batch, int c, int z, int y,
                                int x, const rx_aug_sample* samples, const void* table, long pool_words, void* stream) {
  AugGeom g;
  bool any_g3;
  if (int rc = aug_check("rx_aug_pointwise", in, out, batch, c, z, y, x, samples, table, pool_words, g, any_g3)) return rc;
  if (in == out) RX_FAIL(RX_EINVAL, "rx_aug_pointwise: in place is not supported");
  if (any_g3 && (!scratch || scratch_bytes < rx_aug_workspace(batch, c, z, y, x)))
    RX_FAIL(RX_EWORKSPACE, "rx_aug_pointwise: a group-3 sample needs rx_aug_workspace() bytes of scratch");
  const rx_aug_sample* S = (const rx_aug_sample*)table;
  const float* pool = (const float*)(S + batch);
  const bool vec = (x & 3) == 0 && (((uintptr_t)in | (uintptr_t)out | (uintptr_t)scratch) & 15) == 0;
  const long nq = (long)z * y * g.XQ;
  const dim3 grid((unsigned)((nq + RX_AUG_BLOCK - 1) / RX_AUG_BLOCK), (unsigned)(batch * c));
  hipStream_t st = (hipStream_t)stream;
  if (vec)
    hipLaunchKernelGGL(aug_pointwise_kernel<true>, grid, dim3(RX_AUG_BLOCK), 0, st, in, out, scratch, S, pool, g);
  else
    hipLaunchKernelGGL(aug_pointwise_kernel<false>, grid, dim3(RX_AUG_BLOCK), 0, st, in, out, scratch, S, pool, g);
  RX_CHECK_LAUNCH("rx_aug_pointwise");
  return RX_OK;
}

template <int K>
static void aug_launch_filter(bool vec, dim3 grid, hipStream_t st, const float* src, float* out, const rx_aug_sample* S,
                              const float* pool, const AugGeom& g, int tx, int ty) {
  if (vec)
    hipLaunchKernelGGL((aug_filter_kernel<K, true>), grid, dim3(RX_AUG_BLOCK), 0, st, src, out, S, pool, g, tx, ty);
  else
    hipLaunchKernelGGL((aug_filter_kernel<K, false>), grid, dim3(RX_AUG_BLOCK), 0, st, src, out, S, pool, g, tx, ty);
}

extern "C" int rx_aug_filter_zy(const float* scratch, float* out, int batch, int c, int z, int y, int x,
                                const rx_aug_sample* samples, const void* table, long pool_words, void* stream) {
  AugGeom g;
  bool any_g3;
  if (int rc = aug_check("rx_aug_filter_zy", scratch, out, batch, c, z, y, x, samples, table, pool_words, g, any_g3)) return rc;
  if (scratch == out) RX_FAIL(RX_EINVAL, "rx_aug_filter_zy: in place is not supported");
  if (!any_g3) return RX_OK;
  const rx_aug_sample* S = (const rx_aug_sample*)table;
  const float* pool = (const float*)(S + batch);
  const bool vec = (x & 3) == 0 && (((uintptr_t)scratch | (uintptr_t)out) & 15) == 0;
  hipStream_t st = (hipStream_t)stream;
  unsigned ks = 0;      // bit (k - 3) / 2: a sample of the batch filters with that k
  bool down = false;
  for (int i = 0; i < batch; ++i) {
    if (samples[i].g3_mode == RX_AUG_G3_FILTER) ks |= 1u << ((samples[i].k - 3) / 2);
    down = down || samples[i].g3_mode == RX_AUG_G3_DOWNSCALE;
  }
  const int tx = (x + RX_AUG_T - 1) / RX_AUG_T, ty = (y + RX_AUG_T - 1) / RX_AUG_T, tz = (z + RX_AUG_T - 1) / RX_AUG_T;
  const dim3 grid((unsigned)(tx * ty * tz), 1, (unsigned)(batch * c));
#define RX_AUG_K(K) \
  if (ks & (1u << ((K - 3) / 2))) aug_launch_filter<K>(vec, grid, st, scratch, out, S, pool, g, tx, ty);
  RX_AUG_K(3) RX_AUG_K(5) RX_AUG_K(7) RX_AUG_K(9) RX_AUG_K(11) RX_AUG_K(13) RX_AUG_K(15) RX_AUG_K(17) RX_AUG_K(19) RX_AUG_K(21)
#undef RX_AUG_K
  if (down) {
    const long nq = (long)z * y * g.XQ;
    const dim3 dgrid((unsigned)((nq + RX_AUG_BLOCK - 1) / RX_AUG_BLOCK), (unsigned)(batch * c));
    if (vec)
      hipLaunchKernelGGL(aug_downscale_kernel<true>, dgrid, dim3(RX_AUG_BLOCK), 0, st, scratch, out, S, pool, g);
    else
      hipLaunchKernelGGL(aug_downscale_kernel<false>, dgrid, dim3(RX_AUG_BLOCK), 0, st, scratch, out, S, pool, g);
  }
  RX_CHECK_LAUNCH("rx_aug_filter_zy");
  return RX_OK;
}

extern "C" int rx_aug_philox_u32(uint64_t key, long n, uint32_t* out, void* stream) {
  if (!out || n < 1) RX_FAIL(RX_EINVAL, "rx_aug_philox_u32: bad arguments");
  const long nq = (n + 3) / 4;
  hipLaunchKernelGGL(aug_philox_kernel, dim3((unsigned)((nq + RX_AUG_BLOCK - 1) / RX_AUG_BLOCK)), dim3(RX_AUG_BLOCK), 0,
                     (hipStream_t)stream, (uint32_t)key, (uint32_t)(key >> 32), n, out);
  RX_CHECK_LAUNCH("rx_aug_philox_u32");
  return RX_OK;
}
