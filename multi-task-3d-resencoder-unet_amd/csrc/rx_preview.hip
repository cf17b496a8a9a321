// rx_preview.hip -- the validation preview on the device: one panel of the debug GIF per launch (host side
// training/visualization/preview.py, whose panel_numpy is the statement).  The source is one sample's contiguous (c, z, h, w)
// block, fp32, bf16 or fp16; the panel of kept slice j (source slice j * z_step) is h x w x 3 bytes inside a larger frame buffer.
//
//   preview_panel_kernel<T, CD>   one workgroup = one kept slice with its CD = 1 (grey) or 3 (one byte each) drawn channels.
//     pass 1  lo = min, hi = max and a "not finite" flag per channel: per lane, per wave (xor shuffles), per workgroup (LDS).  min,
//             max and `or` do not depend on the order, and no atomic is involved.
//     pass 2  after the barrier the slice (a few hundred KB at most, now in L2) is read again a tile of RX_PV_BLOCK 16-byte units
//             at a time; a lane turns its unit into 3 * P bytes (P = 4 or 8 pixels) and puts them, as whole dwords, into LDS in
//             pixel order.  The tile is then a byte stream that maps onto the destination row by row (dest = row bias + stream
//             index), and the workgroup stores it dword by dword: a destination dword that lies wholly inside a panel row takes
//             its four bytes from two LDS words, the few dwords that straddle a row end are byte stores.  Neither row_stride nor
//             3 * x0 needs to be a multiple of 4, and no byte outside the panel is touched (no read-modify-write).
//
// Reading a slice: a scalar head up to the first 16-byte boundary of the slice of channel 0, `nvec` units of 16 bytes, a scalar
// tail.  The slices of channels 1 and 2 start z * h * w elements further on; when that is no multiple of P they are loaded through
// a struct that promises only the element's alignment (PvRun: still one multi-dword load for fp32, narrower loads for 16-bit
// types), behind a launch-uniform branch.  Nothing outside the slice is read; every offset is 64-bit.
// Contraction is off: the subtraction, the IEEE division and the product round once each, as in the numpy statement.
#include "rx_common.h"

#include <float.h>

#pragma clang fp contract(off)

#define RX_PV_BLOCK 256
#define RX_PV_WAVES (RX_PV_BLOCK / 64)
#define RX_PV_TILE_BYTES (RX_PV_BLOCK * 8 * 3)      // the widest tile: 256 units of 8 pixels, 3 bytes each

template <typename E, int P>
struct PvRun {
  E v[P];
};

template <typename T>
__device__ inline void pv_load(const T* __restrict__ p, bool al16, float (&o)[Elem<T>::PER16]) {
  constexpr int P = Elem<T>::PER16;
  if (al16) {
    const Vec16<T> r = ld16(p);
#pragma unroll
    for (int j = 0; j < P; ++j) o[j] = Elem<T>::to_f(r.v[j]);
  } else {
    const PvRun<T, P> r = *reinterpret_cast<const PvRun<T, P>*>(p);
#pragma unroll
    for (int j = 0; j < P; ++j) o[j] = Elem<T>::to_f(r.v[j]);
  }
}

__device__ inline float pv_act(float v, bool sigmoid) { return sigmoid ? 1.0f / (1.0f + expf(-v)) : v; }

struct PvRange {
  float lo, hi;
  int bad;
  __device__ inline void take(float v) {
    bad |= !(fabsf(v) <= FLT_MAX);      // a NaN or an infinity
    lo = v < lo ? v : lo;
    hi = v > hi ? v : hi;
  }
};

struct PvScale {
  float lo, r;
  bool ok;
  __device__ inline unsigned byte(float v) const { return ok ? (unsigned)(int)(((v - lo) / r) * 255.0f) : 127u; }
};

template <typename T, int CD>
__global__ __launch_bounds__(RX_PV_BLOCK) void preview_panel_kernel(const T* __restrict__ src, int z, int h, int w, int z_step, int zk,
                                                                    int sigmoid, uint8_t* __restrict__ frames, long frame_stride,
                                                                    long row_stride, int y0, int x0, float* __restrict__ minmax) {
  constexpr int P = Elem<T>::PER16;
  constexpr int WPU = 3 * P / 4;      // dwords of bytes a unit makes: 3 or 6
  __shared__ float s_lo[CD][RX_PV_WAVES], s_hi[CD][RX_PV_WAVES];
  __shared__ int s_bad[CD][RX_PV_WAVES];
  __shared__ __attribute__((aligned(16))) unsigned s_w[RX_PV_TILE_BYTES / 4 + 1];      // (+1: the funnel below reads one word on)
  const int j = blockIdx.x, tid = threadIdx.x;
  const long V = (long)h * w;
  const bool sg = sigmoid != 0;
  const T* __restrict__ ch[CD];
#pragma unroll
  for (int k = 0; k < CD; ++k) ch[k] = src + ((long)k * z + (long)j * z_step) * V;
  long hd = (long)(((16u - (unsigned)((uintptr_t)ch[0] & 15u)) & 15u) / (unsigned)sizeof(T));
  hd = hd < V ? hd : V;
  const long nvec = (V - hd) / P, tail = hd + nvec * P;
  const bool al16 = CD == 1 || ((long)z * V) % P == 0;      // channels 1 and 2 share the alignment of channel 0

  // ---- pass 1: the range of every drawn channel -----------------------------------------------------------------------------------
  PvRange rg[CD];
#pragma unroll
  for (int k = 0; k < CD; ++k) rg[k] = PvRange{INFINITY, -INFINITY, 0};
#pragma unroll 2
  for (long u = tid; u < nvec; u += RX_PV_BLOCK) {
    const long off = hd + u * P;
#pragma unroll
    for (int k = 0; k < CD; ++k) {
      float x[P];
      pv_load<T>(ch[k] + off, k == 0 || al16, x);
#pragma unroll
      for (int i = 0; i < P; ++i) rg[k].take(pv_act(x[i], sg));
    }
  }
  {      // head and tail: fewer than P pixels each, one lane per pixel
    long i = -1;
    if ((long)tid < hd) i = tid;
    else if (tid >= 64 && tail + (tid - 64) < V) i = tail + (tid - 64);
    if (i >= 0)
#pragma unroll
      for (int k = 0; k < CD; ++k) rg[k].take(pv_act(Elem<T>::to_f(ch[k][i]), sg));
  }
#pragma unroll
  for (int k = 0; k < CD; ++k) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float a = __shfl_xor(rg[k].lo, o, 64), b = __shfl_xor(rg[k].hi, o, 64);
      rg[k].lo = a < rg[k].lo ? a : rg[k].lo;
      rg[k].hi = b > rg[k].hi ? b : rg[k].hi;
      rg[k].bad |= __shfl_xor(rg[k].bad, o, 64);
    }
    if ((tid & 63) == 0) s_lo[k][tid >> 6] = rg[k].lo, s_hi[k][tid >> 6] = rg[k].hi, s_bad[k][tid >> 6] = rg[k].bad;
  }
  __syncthreads();
  PvScale sc[CD];
#pragma unroll
  for (int k = 0; k < CD; ++k) {
    float lo = s_lo[k][0], hi = s_hi[k][0];
    int bad = s_bad[k][0];
#pragma unroll
    for (int q = 1; q < RX_PV_WAVES; ++q) {
      lo = s_lo[k][q] < lo ? s_lo[k][q] : lo;
      hi = s_hi[k][q] > hi ? s_hi[k][q] : hi;
      bad |= s_bad[k][q];
    }
    const float r = hi - lo;
    sc[k] = PvScale{lo, r, !bad && r > 1e-6f && r <= FLT_MAX};
    if (minmax && tid == 0) {
      float* m = minmax + ((long)k * zk + j) * 2;
      m[0] = bad ? __builtin_nanf("") : lo;
      m[1] = bad ? __builtin_nanf("") : hi;
    }
  }

  // ---- pass 2: the bytes ----------------------------------------------------------------------------------------------------------
  uint8_t* __restrict__ panel = frames + (long)j * frame_stride + (long)y0 * row_stride + 3 * (long)x0;      // pixel (0, 0)
  const long row_bias = row_stride - 3 * (long)w;      // dest of stream byte s of row r: panel + r * row_bias + s
  {      // head and tail pixels: three byte stores each
    long i = -1;
    if ((long)tid < hd) i = tid;
    else if (tid >= 64 && tail + (tid - 64) < V) i = tail + (tid - 64);
    if (i >= 0) {
      uint8_t* d = panel + (i / w) * row_bias + 3 * i;
      if (CD == 1) {
        const uint8_t g = (uint8_t)sc[0].byte(pv_act(Elem<T>::to_f(ch[0][i]), sg));
        d[0] = g, d[1] = g, d[2] = g;
      } else {
#pragma unroll
        for (int k = 0; k < CD; ++k) d[k] = (uint8_t)sc[k].byte(pv_act(Elem<T>::to_f(ch[k][i]), sg));
      }
    }
  }
  const uint8_t* s_b = reinterpret_cast<const uint8_t*>(s_w);
  const int wcap = w < RX_PV_BLOCK * P ? w : RX_PV_BLOCK * P;
  const int spr = (3 * wcap + 3) / 4 + 1;      // dword slots per row segment: no fewer than a segment of a tile can touch
  for (long u0 = 0; u0 < nvec; u0 += RX_PV_BLOCK) {
    if (u0 + tid < nvec) {
      const long off = hd + (u0 + tid) * P;
      unsigned b[P][3];
      if (CD == 1) {
        float x[P];
        pv_load<T>(ch[0] + off, true, x);
#pragma unroll
        for (int i = 0; i < P; ++i) b[i][0] = b[i][1] = b[i][2] = sc[0].byte(pv_act(x[i], sg));
      } else {
#pragma unroll
        for (int k = 0; k < CD; ++k) {
          float x[P];
          pv_load<T>(ch[k] + off, k == 0 || al16, x);
#pragma unroll
          for (int i = 0; i < P; ++i) b[i][k] = sc[k].byte(pv_act(x[i], sg));
        }
      }
#pragma unroll
      for (int q = 0; q < WPU; ++q) {      // stream bytes 4q .. 4q+3 of this unit: byte s is pixel s / 3, channel s % 3
        unsigned word = 0u;
#pragma unroll
        for (int e = 0; e < 4; ++e) word |= b[(4 * q + e) / 3][(4 * q + e) % 3] << (8 * e);
        s_w[tid * WPU + q] = word;
      }
    }
    __syncthreads();
    // the tile holds pixels [tp0, tp1); LDS byte 3 * (p - tp0) + k is pixel p, channel k
    const long left = nvec - u0;
    const long tp0 = hd + u0 * P, tp1 = tp0 + (left < RX_PV_BLOCK ? left : RX_PV_BLOCK) * P;
    const long r0 = tp0 / w, r1 = (tp1 - 1) / w;
    const int total = (int)(r1 - r0 + 1) * spr;
    for (int q = tid; q < total; q += RX_PV_BLOCK) {
      const long row = r0 + q / spr;
      const int slot = q % spr;
      const long pa = row * w > tp0 ? row * w : tp0, pb = (row + 1) * w < tp1 ? (row + 1) * w : tp1;      // the row's pixels in the tile
      uint8_t* const rowp = panel + row * row_bias;
      const uintptr_t da = (uintptr_t)(rowp + 3 * pa), db = (uintptr_t)(rowp + 3 * pb);                   // their bytes: [da, db)
      const uintptr_t wd = (da & ~(uintptr_t)3) + 4 * (uintptr_t)slot;
      if (wd >= db) continue;
      const long lds0 = 3 * (pa - tp0) - (long)da;      // LDS byte of address a: lds0 + a
      if (wd >= da && wd + 4 <= db) {
        const unsigned o = (unsigned)(lds0 + (long)wd), sh = (o & 3u) * 8u;
        const unsigned lo = s_w[o >> 2], hi = s_w[(o >> 2) + 1];
        *reinterpret_cast<unsigned*>(wd) = sh ? (lo >> sh) | (hi << (32u - sh)) : lo;
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (wd + e >= da && wd + e < db) *reinterpret_cast<uint8_t*>(wd + e) = s_b[lds0 + (long)(wd + e)];
      }
    }
    __syncthreads();      // the next tile overwrites the stage
  }
}

// ---- host side -------------------------------------------------------------------------------------------------------------------
extern "C" int rx_preview_panel(const void* src, int dtype, int c, int z, int h, int w, int z_step, int sigmoid, uint8_t* frames,
                                long frame_stride, long row_stride, int y0, int x0, float* minmax, void* stream) {
  if (!src) RX_FAIL(RX_EINVAL, "rx_preview_panel: null src");
  if (!frames) RX_FAIL(RX_EINVAL, "rx_preview_panel: null frames");
  if (c <= 0 || z <= 0 || h <= 0 || w <= 0) RX_FAIL(RX_EINVAL, "rx_preview_panel: sizes must be positive (got c=%d z=%d h=%d w=%d)", c, z, h, w);
  if (z_step <= 0) RX_FAIL(RX_EINVAL, "rx_preview_panel: z_step must be positive (got %d)", z_step);
  if (dtype != RX_F32 && dtype != RX_BF16 && dtype != RX_F16) RX_FAIL(RX_EINVAL, "rx_preview_panel: unknown dtype %d (RX_F32, RX_BF16 or RX_F16)", dtype);
  if (((uintptr_t)src & (uintptr_t)(rx_dtype_size(dtype) - 1)) != 0)
    RX_FAIL(RX_EINVAL, "rx_preview_panel: src must be aligned to its %zu-byte element", rx_dtype_size(dtype));
  if (((uintptr_t)minmax & 3) != 0) RX_FAIL(RX_EINVAL, "rx_preview_panel: minmax must be 4-byte aligned");
  if (y0 < 0 || x0 < 0) RX_FAIL(RX_EINVAL, "rx_preview_panel: y0 and x0 must not be negative (got y0=%d x0=%d)", y0, x0);
  if (row_stride < 3 * ((long)x0 + w))
    RX_FAIL(RX_EINVAL, "rx_preview_panel: row_stride %ld is below 3 * (x0 + w) = %ld", row_stride, 3 * ((long)x0 + w));
  long need = 0;
  if (__builtin_mul_overflow((long)y0 + h, row_stride, &need) || frame_stride < need)
    RX_FAIL(RX_EINVAL, "rx_preview_panel: frame_stride %ld is below (y0 + h) * row_stride", frame_stride);
  const int zk = (int)(((long)z + z_step - 1) / z_step);
  const int cd = c == 3 ? 3 : 1;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)zk), block(RX_PV_BLOCK);
#define RX_PV_LAUNCH(T, CD)                                                                                                         \
  hipLaunchKernelGGL((preview_panel_kernel<T, CD>), grid, block, 0, st, (const T*)src, z, h, w, z_step, zk, sigmoid, frames, frame_stride, \
                     row_stride, y0, x0, minmax)
  RX_DISPATCH_DTYPE(dtype, T, if (cd == 3) RX_PV_LAUNCH(T, 3); else RX_PV_LAUNCH(T, 1));
#undef RX_PV_LAUNCH
  RX_CHECK_LAUNCH("rx_preview_panel");
  return RX_OK;
}
