// rx_ingest.hip -- raw training patches as the store holds them -> the float32, channel-first batch every later stage expects
// (reference dataloading/dataset.py: `astype(np.float32)`, the /255, /65535, /32767.5 - 1 or *2 - 1 scaling, and for a
// channels-last normals store `transpose(3, 0, 1, 2)`).  In: `batch` samples of uint8, uint16 or float32, each (Z, Y, X) or
// channels-last (Z, Y, X, C), contiguous; out: contiguous fp32 (batch, C, Z, Y, X).  One rule per call (rx_ingest_rule), the
// float32 arithmetic of the numpy statement dataloading/ingest_device.py: ingest_numpy -- true IEEE division, no reciprocal:
//   COPY v   DIV255 v / 255   DIV65535 v / 65535   NORMAL_U16 v / 32767.5 - 1   NORMAL_MUL2 v * 2 - 1  (v * 2 is exact: an FMA
//   gives the same bits).  COPY of float32 moves the 32 bits through integer registers: -0.0, NaN payloads, denormals as they are.
//
// Two kernels, both pure streams (1, 2 or 4 bytes read, 4 written per element):
//   ingest_flat_kernel   C == 1.  A sample is a scalar head up to the first 16-byte boundary of ITS input, 16-byte loads (each
//                        feeding 16-byte stores), a scalar tail: a uint8 sample of 5*7*13 voxels puts the next one at an odd
//                        address, so the head is per sample.  Input and output advance together, so the stores are aligned
//                        where the loads are iff (in % 16) / esize == (out % 16) / 4 (mod 4) -- true for every allocator's
//                        pointers; otherwise (`wide` = 0, decided once on the host) the whole call takes the scalar path.
//   ingest_cl_kernel     C > 1.  A workgroup takes 1024 voxels: their n * C contiguous elements go to LDS raw (scalar head,
//                        16-byte loads, scalar tail; a tile is a multiple of 16 bytes, so every tile of a sample has the
//                        sample's head), then each plane c is written as one run of n floats, element (i, c) read from LDS at
//                        i * C + c: per plane a scalar head up to the first 16-byte boundary of the OUTPUT, 16-byte stores,
//                        a scalar tail.  No thread reads global memory at stride C or writes a plane uncoalesced.
// Element offsets inside a sample are 32-bit (z * y * x * c < 2^31, checked on the host), sample bases 64-bit.
#include "rx_common.h"

#define RX_ING_BLOCK 256
#define RX_ING_VPT 4                                // flat kernel: 16-byte loads in flight per thread
#define RX_ING_CHUNK (RX_ING_BLOCK * RX_ING_VPT)    // ... and vectors per workgroup
#define RX_ING_SCALARS 16                           // flat kernel, scalar path: elements per thread and workgroup
#define RX_ING_TILE 1024                            // channels-last kernel: voxels per workgroup (a multiple of 16)
#define RX_ING_MAX_C 8

template <typename T>
__device__ inline float ing_value(T v) { return (float)v; }
template <>
__device__ inline float ing_value<uint32_t>(uint32_t v) { return __builtin_bit_cast(float, v); }      // float32 by its bits

// one element -> the bits of its float32
template <typename T, int RULE>
__device__ inline uint32_t ing_cvt(T v) {
  if constexpr (RULE == RX_INGEST_COPY && sizeof(T) == 4) return (uint32_t)v;
  const float f = ing_value<T>(v);
  float r;
  if constexpr (RULE == RX_INGEST_COPY) r = f;
  else if constexpr (RULE == RX_INGEST_DIV255) r = f / 255.0f;
  else if constexpr (RULE == RX_INGEST_DIV65535) r = f / 65535.0f;
  else if constexpr (RULE == RX_INGEST_NORMAL_U16) r = f / 32767.5f - 1.0f;
  else r = f * 2.0f - 1.0f;
  return __builtin_bit_cast(uint32_t, r);
}

// element j of a 16-byte vector
template <typename T>
__device__ inline T ing_lane(const u32x4& v, int j) {
  if constexpr (sizeof(T) == 1) return (T)((v[j >> 2] >> ((j & 3) * 8)) & 0xffu);
  else if constexpr (sizeof(T) == 2) return (T)((v[j >> 1] >> ((j & 1) * 16)) & 0xffffu);
  else return (T)v[j];
}

// elements of `p` before its first 16-byte boundary
template <typename T>
__device__ inline int ing_head(const T* p) {
  return (int)(((16u - (unsigned)((uintptr_t)p & 15u)) & 15u) / (unsigned)sizeof(T));
}

// ---- C == 1 --------------------------------------------------------------------------------------------------------------------
template <typename T, int RULE>
__global__ __launch_bounds__(RX_ING_BLOCK) void ingest_flat_kernel(const T* __restrict__ in, uint32_t* __restrict__ out, int N, int chunks,
                                                                   int wide) {
  constexpr int P = 16 / (int)sizeof(T);      // elements per 16-byte load
  const int b = (int)(blockIdx.x / (unsigned)chunks), k = (int)(blockIdx.x - (unsigned)b * (unsigned)chunks);
  const T* __restrict__ src = in + (long)b * N;
  uint32_t* __restrict__ dst = out + (long)b * N;
  int h = N;
  if (wide) {
    h = ing_head(src);
    h = h < N ? h : N;
  }
  const int nvec = (N - h) / P, tail0 = h + nvec * P;
  u32x4 v[RX_ING_VPT];
#pragma unroll
  for (int j = 0; j < RX_ING_VPT; ++j) {
    const int m = k * RX_ING_CHUNK + j * RX_ING_BLOCK + (int)threadIdx.x;
    if (m < nvec) v[j] = *reinterpret_cast<const u32x4*>(src + h + m * P);
  }
#pragma unroll
  for (int j = 0; j < RX_ING_VPT; ++j) {
    const int m = k * RX_ING_CHUNK + j * RX_ING_BLOCK + (int)threadIdx.x;
    if (m < nvec) {
      uint32_t* __restrict__ o = dst + h + m * P;
#pragma unroll
      for (int q = 0; q < P / 4; ++q) {
        u32x4 r;
#pragma unroll
        for (int e = 0; e < 4; ++e) r[e] = ing_cvt<T, RULE>(ing_lane<T>(v[j], q * 4 + e));
        *reinterpret_cast<u32x4*>(o + q * 4) = r;
      }
    }
  }
  // the head and the tail (the whole sample when the call is not `wide`), dealt over the sample's workgroups
  const int nsc = h + (N - tail0);
  for (long i = (long)k * RX_ING_BLOCK + threadIdx.x; i < nsc; i += (long)chunks * RX_ING_BLOCK) {
    const int e = i < h ? (int)i : tail0 + ((int)i - h);
    dst[e] = ing_cvt<T, RULE>(src[e]);
  }
}

// ---- C > 1: channels-last in, planes out -------------------------------------------------------------------------------------
template <typename T, int RULE>
__global__ __launch_bounds__(RX_ING_BLOCK) void ingest_cl_kernel(const T* __restrict__ in, uint32_t* __restrict__ out, int S, int C, int tiles) {
  extern __shared__ __attribute__((aligned(16))) unsigned char ing_lds[];      // (RX_ING_TILE * C + P) elements of T
  T* __restrict__ s = reinterpret_cast<T*>(ing_lds);
  constexpr int P = 16 / (int)sizeof(T);
  const int b = (int)(blockIdx.x / (unsigned)tiles), t = (int)(blockIdx.x - (unsigned)b * (unsigned)tiles);
  const int v0 = t * RX_ING_TILE;
  const int n = S - v0 < RX_ING_TILE ? S - v0 : RX_ING_TILE, nel = n * C;
  const T* __restrict__ src = in + ((long)b * S + v0) * C;
  int h = ing_head(src);
  h = h < nel ? h : nel;
  const int sh = (P - h) & (P - 1);      // element j sits at s[sh + j]: the first vector lands on a 16-byte boundary of the LDS
  const int nvec = (nel - h) / P, tail0 = h + nvec * P;
  for (int m = threadIdx.x; m < nvec; m += RX_ING_BLOCK)
    *reinterpret_cast<u32x4*>(s + sh + h + m * P) = *reinterpret_cast<const u32x4*>(src + h + m * P);
  if ((int)threadIdx.x < h + (nel - tail0)) {      // fewer than 2 P <= 32 elements
    const int e = (int)threadIdx.x < h ? (int)threadIdx.x : tail0 + ((int)threadIdx.x - h);
    s[sh + e] = src[e];
  }
  __syncthreads();
  for (int c = 0; c < C; ++c) {
    uint32_t* __restrict__ dst = out + ((long)b * C + c) * S + v0;
    int ho = ing_head(dst);
    ho = ho < n ? ho : n;
    const int nv = (n - ho) / 4, t0 = ho + nv * 4;
    const T* __restrict__ sc = s + sh + c;
    for (int m = threadIdx.x; m < nv; m += RX_ING_BLOCK) {
      const int i = ho + m * 4;
      u32x4 r;
#pragma unroll
      for (int e = 0; e < 4; ++e) r[e] = ing_cvt<T, RULE>(sc[(i + e) * C]);
      *reinterpret_cast<u32x4*>(dst + i) = r;
    }
    const int j = (int)threadIdx.x - (RX_ING_BLOCK - 8);      // the last lanes: fewer than 8 elements of head and tail
    if (j >= 0 && j < ho + (n - t0)) {
      const int i = j < ho ? j : t0 + (j - ho);
      dst[i] = ing_cvt<T, RULE>(sc[i * C]);
    }
  }
}

// ---- host side -----------------------------------------------------------------------------------------------------------------
template <typename T, int RULE>
static void ingest_launch(const void* in, float* out, int batch, int S, int C, int wide, hipStream_t st) {
  constexpr int P = 16 / (int)sizeof(T);
  if (C == 1) {
    const long work = wide ? ((long)S / P + 1 + RX_ING_CHUNK - 1) / RX_ING_CHUNK
                           : ((long)S + RX_ING_BLOCK * RX_ING_SCALARS - 1) / (RX_ING_BLOCK * RX_ING_SCALARS);
    const int chunks = (int)(work > 0 ? work : 1);
    hipLaunchKernelGGL((ingest_flat_kernel<T, RULE>), dim3((unsigned)((long)batch * chunks)), dim3(RX_ING_BLOCK), 0, st, (const T*)in,
                       (uint32_t*)out, S, chunks, wide);
  } else {
    const int tiles = (S + RX_ING_TILE - 1) / RX_ING_TILE;
    const size_t lds = ((size_t)RX_ING_TILE * C + P) * sizeof(T);
    hipLaunchKernelGGL((ingest_cl_kernel<T, RULE>), dim3((unsigned)((long)batch * tiles)), dim3(RX_ING_BLOCK), lds, st, (const T*)in,
                       (uint32_t*)out, S, C, tiles);
  }
}

template <typename T>
static void ingest_rule_dispatch(int rule, const void* in, float* out, int batch, int S, int C, int wide, hipStream_t st) {
  switch (rule) {
    case RX_INGEST_COPY: ingest_launch<T, RX_INGEST_COPY>(in, out, batch, S, C, wide, st); break;
    case RX_INGEST_DIV255: ingest_launch<T, RX_INGEST_DIV255>(in, out, batch, S, C, wide, st); break;
    case RX_INGEST_DIV65535: ingest_launch<T, RX_INGEST_DIV65535>(in, out, batch, S, C, wide, st); break;
    case RX_INGEST_NORMAL_U16: ingest_launch<T, RX_INGEST_NORMAL_U16>(in, out, batch, S, C, wide, st); break;
    default: ingest_launch<T, RX_INGEST_NORMAL_MUL2>(in, out, batch, S, C, wide, st); break;
  }
}

extern "C" int rx_ingest(const void* in, int dtype, float* out, int batch, int z, int y, int x, int c, int rule, void* stream) {
  if (!in || !out) RX_FAIL(RX_EINVAL, "rx_ingest: null tensor pointer");
  if ((const void*)in == (const void*)out) RX_FAIL(RX_EINVAL, "rx_ingest: in and out must be distinct buffers");
  if (dtype != RX_SW_U8 && dtype != RX_SW_U16 && dtype != RX_SW_F32)
    RX_FAIL(RX_EINVAL, "rx_ingest: unknown dtype %d (RX_SW_U8, RX_SW_U16 or RX_SW_F32)", dtype);
  if (rule < RX_INGEST_COPY || rule > RX_INGEST_NORMAL_MUL2)
    RX_FAIL(RX_EINVAL, "rx_ingest: unknown rule %d (RX_INGEST_COPY .. RX_INGEST_NORMAL_MUL2)", rule);
  if (batch <= 0 || z <= 0 || y <= 0 || x <= 0 || c <= 0)
    RX_FAIL(RX_EINVAL, "rx_ingest: batch and sizes must be positive (got %d x %d x %d x %d x %d)", batch, z, y, x, c);
  if (c > RX_ING_MAX_C) RX_FAIL(RX_EINVAL, "rx_ingest: %d channels (at most %d)", c, RX_ING_MAX_C);
  long voxels = (long)z * y;      // each factor is below 2^31: no step overflows 64 bits before it is checked
  if (voxels <= 0x7fffffffL) voxels *= x;
  if (voxels > 0x7fffffffL || voxels * c > 0x7fffffffL)
    RX_FAIL(RX_EINVAL, "rx_ingest: a sample of %d x %d x %d x %d is beyond the index arithmetic (z * y * x * c < 2^31)", z, y, x, c);
  const int esize = dtype == RX_SW_U8 ? 1 : dtype == RX_SW_U16 ? 2 : 4;
  if (((uintptr_t)in & (uintptr_t)(esize - 1)) != 0) RX_FAIL(RX_EINVAL, "rx_ingest: in must be aligned to its %d-byte element", esize);
  if (((uintptr_t)out & 3) != 0) RX_FAIL(RX_EINVAL, "rx_ingest: out must be 4-byte aligned");
  const int S = (int)voxels;
  const long per_sample = c == 1 ? ((long)S + RX_ING_CHUNK - 1) / RX_ING_CHUNK + 1 : ((long)S + RX_ING_TILE - 1) / RX_ING_TILE;
  if (per_sample * batch > 0x7fffffffL)
    RX_FAIL(RX_EINVAL, "rx_ingest: %d samples of %d x %d x %d x %d are more workgroups than a launch holds", batch, z, y, x, c);
  // 16-byte loads and 16-byte stores line up (C == 1) iff input and output reach a boundary at the same element
  const int wide = ((((uintptr_t)in & 15) / (uintptr_t)esize) & 3) == ((((uintptr_t)out & 15) / 4) & 3) ? 1 : 0;
  hipStream_t st = (hipStream_t)stream;
  if (dtype == RX_SW_U8) ingest_rule_dispatch<uint8_t>(rule, in, out, batch, S, c, wide, st);
  else if (dtype == RX_SW_U16) ingest_rule_dispatch<uint16_t>(rule, in, out, batch, S, c, wide, st);
  else ingest_rule_dispatch<uint32_t>(rule, in, out, batch, S, c, wide, st);
  RX_CHECK_LAUNCH("rx_ingest");
  return RX_OK;
}
