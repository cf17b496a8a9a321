// rx_stem.hip -- the stem convolution on the NCDHW fp32 image and its weight gradient: the VALU kernels and the entry points,
// which try the MFMA variants of rx_stem_wgrad.hip first.
#include "rx_common.h"
#include "rx_internal.h"
#include "rx_reduce.h"

// ---- stem convolution on the NCDHW fp32 image (Cin <= 16; the MFMA variants of rx_stem_wgrad.hip take Cin <= 4) ----------
// thread -> (voxel, vector of P output channels); weights in LDS as [tap*Cin][Cout]
template <typename T>
__global__ __launch_bounds__(256) void stem_fwd_kernel(const float* __restrict__ x, int Cin, int Z, int Y, int X, const float* __restrict__ w,
                                                       const float* __restrict__ bias, T* __restrict__ out, int ldo, long so, int Co, int kz,
                                                       int ky, int kx) {
  constexpr int P = Elem<T>::PER16;
  extern __shared__ __attribute__((aligned(16))) float sw[];  // [Cin*T][Co]
  const int TT = kz * ky * kx;
  for (int i = threadIdx.x; i < Co * Cin * TT; i += 256) {
    int co = i / (Cin * TT), r = i - co * (Cin * TT);  // r = ci*TT + t  (torch layout (Co,Ci,T))
    sw[r * Co + co] = w[i];
  }
  __syncthreads();
  const int n = blockIdx.y;
  const int CV = Co / P;
  const long V = (long)Z * Y * X;
  const long total = V * CV;
  const int pz = (kz - 1) / 2, py = (ky - 1) / 2, px = (kx - 1) / 2;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    int cv = (int)(i % CV);
    long v = i / CV;
    int xx = (int)(v % X), yy = (int)((v / X) % Y), zz = (int)(v / ((long)X * Y));
    float acc[P];
#pragma unroll
    for (int j = 0; j < P; ++j) acc[j] = bias ? bias[cv * P + j] : 0.f;
    for (int ci = 0; ci < Cin; ++ci) {
      const float* xc = x + ((size_t)n * Cin + ci) * V;
      for (int a = 0; a < kz; ++a) {
        int z2 = zz + a - pz;
        if ((unsigned)z2 >= (unsigned)Z) continue;
        for (int b = 0; b < ky; ++b) {
          int y2 = yy + b - py;
          if ((unsigned)y2 >= (unsigned)Y) continue;
          for (int c = 0; c < kx; ++c) {
            int x2 = xx + c - px;
            if ((unsigned)x2 >= (unsigned)X) continue;
            float xv = xc[((long)z2 * Y + y2) * X + x2];
            const float* wr = sw + ((ci * TT) + (a * ky + b) * kx + c) * Co + cv * P;
#pragma unroll
            for (int j = 0; j < P; ++j) acc[j] += xv * wr[j];
          }
        }
      }
    }
    Vec16<T> o;
#pragma unroll
    for (int j = 0; j < P; ++j) o.v[j] = Elem<T>::from_f(acc[j]);
    st16(out + n * so + v * ldo + cv * P, o);
  }
}

// One thread per voxel, 32 output channels at a time (16-bit output types): the taps of the voxel are loaded ONCE into
// registers and every weight comes from LDS as a wave-uniform (broadcast) 16-byte read.  The first version above gave a
// voxel to 4 threads of 8 channels each: 4x the image loads and bounds checks (428 us for the cfg2 stem; this one is
// bound by its 864 FMAs per voxel).
template <typename T>
__global__ __launch_bounds__(256) void stem_fwd32_kernel(const float* __restrict__ x, int Cin, int Z, int Y, int X, const float* __restrict__ w,
                                                         const float* __restrict__ bias, T* __restrict__ out, int ldo, long so, int Co,
                                                         int kz, int ky, int kx) {
  extern __shared__ __attribute__((aligned(16))) float sw[];  // [Cin*TT][Co]
  const int TT = kz * ky * kx;
  for (int i = threadIdx.x; i < Co * Cin * TT; i += 256) {
    int co = i / (Cin * TT), r = i - co * (Cin * TT);
    sw[r * Co + co] = w[i];
  }
  __syncthreads();
  const int n = blockIdx.y;
  const long V = (long)Z * Y * X;
  const int pz = (kz - 1) / 2, py = (ky - 1) / 2, px = (kx - 1) / 2;
  for (long v = (long)blockIdx.x * 256 + threadIdx.x; v < V; v += (long)gridDim.x * 256) {
    const int xx = (int)(v % X), yy = (int)((v / X) % Y), zz = (int)(v / ((long)X * Y));
    for (int c0 = 0; c0 < Co; c0 += 32) {
      float acc[32];
#pragma unroll
      for (int j = 0; j < 32; ++j) acc[j] = bias ? bias[c0 + j] : 0.f;
      for (int ci = 0; ci < Cin; ++ci) {
        const float* xc = x + ((size_t)n * Cin + ci) * V;
        for (int a = 0; a < kz; ++a) {
          const int z2 = zz + a - pz;
          for (int b = 0; b < ky; ++b) {
            const int y2 = yy + b - py;
            for (int c = 0; c < kx; ++c) {
              const int x2 = xx + c - px;
              const bool ok = (unsigned)z2 < (unsigned)Z && (unsigned)y2 < (unsigned)Y && (unsigned)x2 < (unsigned)X;
              const float xv = ok ? xc[((long)z2 * Y + y2) * X + x2] : 0.f;
              const f32x4* wr = reinterpret_cast<const f32x4*>(sw + ((ci * TT) + (a * ky + b) * kx + c) * Co + c0);
#pragma unroll
              for (int q = 0; q < 8; ++q) {
                const f32x4 wv = wr[q];           // wave-uniform address: LDS broadcast
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[4 * q + j] += xv * wv[j];
              }
            }
          }
        }
      }
      T* op = out + n * so + v * ldo + c0;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        T vals[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) vals[j] = Elem<T>::from_f(acc[8 * q + j]);
        *reinterpret_cast<u32x4*>(op + 8 * q) = *reinterpret_cast<u32x4*>(vals);
      }
    }
  }
}

static int check_kernel13(const int32_t k[3], const char* who) {
  for (int i = 0; i < 3; ++i)
    if (k[i] != 1 && k[i] != 3) RX_FAIL(RX_EUNSUPPORTED, "%s: kernel sizes must be 1 or 3", who);
  return RX_OK;
}

// the stem conv and the InstanceNorm statistics of its output (encoder.py:84 + simple_conv_blocks.py:58-72): one pass on the
// MFMA kernel (the separate statistics pass read the 268 MB output of the cfg2 stem again: 109 us of a 17 ms step), the two
// calls otherwise.  Same statistics either way (sums of the values as stored).
extern "C" int rx_stem_conv_fwd_stats(rx_dtype dt, const float* x_ncdhw, int n, int cin, int z, int y, int x, const float* w,
                                      const float* bias, const rx_act* out, const int32_t kernel[3], float eps, float* stats, void* ws,
                                      size_t ws_bytes, void* stream) {
  RX_RECORD(stream, [=, out_ = RxActV(out), kernel_ = RxI3V(kernel)](void* s) { return rx_stem_conv_fwd_stats(dt, x_ncdhw, n, cin, z, y, x, w, bias, out_.p(), kernel_.v, eps, stats, ws, ws_bytes, s); });
  int rc;
  if ((rc = check_vec_channels(out, dt, "rx_stem_conv_fwd_stats(out)"))) return rc;
  if ((rc = check_kernel13(kernel, "rx_stem_conv_fwd_stats"))) return rc;
  if (!x_ncdhw || !w || !stats || !ws || cin < 1 || cin > 16) RX_FAIL(RX_EINVAL, "rx_stem_conv_fwd_stats: bad arguments");
  if (out->n != n || out->z != z || out->y != y || out->x != x) RX_FAIL(RX_EINVAL, "rx_stem_conv_fwd_stats: geometry mismatch");
  int chunks = 0;
  if (rx_stem_fwd_mfma_try(dt, x_ncdhw, n, cin, z, y, x, w, bias, out, kernel, (hipStream_t)stream, (float*)ws, ws_bytes, &chunks) == 1) {
    if (chunks > 0) {
      rx_stats_finalize_launch((const float*)ws, n, chunks, out->c, (double)rx_act_voxels(out), eps, stats, (hipStream_t)stream);
      RX_CHECK_LAUNCH("rx_stem_conv_fwd_stats");
      return RX_OK;
    }
    RX_CHECK_LAUNCH("rx_stem_conv_fwd_stats(mfma)");
    return rx_instnorm_stats(dt, out, eps, stats, ws, ws_bytes, stream);
  }
  if ((rc = rx_stem_conv_fwd(dt, x_ncdhw, n, cin, z, y, x, w, bias, out, kernel, stream))) return rc;
  return rx_instnorm_stats(dt, out, eps, stats, ws, ws_bytes, stream);
}

extern "C" int rx_stem_conv_fwd(rx_dtype dt, const float* x_ncdhw, int n, int cin, int z, int y, int x, const float* w,
                                const float* bias, const rx_act* out, const int32_t kernel[3], void* stream) {
  RX_RECORD(stream, [=, out_ = RxActV(out), kernel_ = RxI3V(kernel)](void* s) { return rx_stem_conv_fwd(dt, x_ncdhw, n, cin, z, y, x, w, bias, out_.p(), kernel_.v, s); });
  int rc;
  if ((rc = check_vec_channels(out, dt, "rx_stem_conv_fwd(out)"))) return rc;
  if ((rc = check_kernel13(kernel, "rx_stem_conv_fwd"))) return rc;
  if (!x_ncdhw || !w || cin < 1 || cin > 16) RX_FAIL(RX_EUNSUPPORTED, "rx_stem_conv_fwd: 1 <= Cin <= 16");
  {      // the VALU kernels keep all weights in LDS: [Cin * taps][Cout] floats
    const size_t wl = (size_t)out->c * cin * kernel[0] * kernel[1] * kernel[2] * sizeof(float);
    if (wl > 160 * 1024) RX_FAIL(RX_EUNSUPPORTED, "rx_stem_conv_fwd: %d x %d channels x %d taps do not fit the LDS", cin, out->c, kernel[0] * kernel[1] * kernel[2]);
    if (wl > 48 * 1024) {
      (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&stem_fwd32_kernel<bf16_t>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
      (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&stem_fwd32_kernel<f16_t>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
      (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&stem_fwd_kernel<float>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
      (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&stem_fwd_kernel<bf16_t>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
      (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&stem_fwd_kernel<f16_t>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    }
  }
  if (out->n != n || out->z != z || out->y != y || out->x != x) RX_FAIL(RX_EINVAL, "rx_stem_conv_fwd: geometry mismatch");
  hipStream_t st = (hipStream_t)stream;
  const int TT = kernel[0] * kernel[1] * kernel[2];
  if (rx_stem_fwd_mfma_try(dt, x_ncdhw, n, cin, z, y, x, w, bias, out, kernel, st, nullptr, 0, nullptr) == 1) {
    RX_CHECK_LAUNCH("rx_stem_conv_fwd(mfma)");
    return RX_OK;
  }
  if (dt != RX_F32 && out->c % 32 == 0 && (out->c * 4) % 16 == 0) {   // one thread per voxel x 32 channels
    const long V = rx_act_voxels(out);
    const int G = (int)((V + 255) / 256 > 16384 ? 16384 : (V + 255) / 256);
    const size_t lds = (size_t)out->c * cin * TT * sizeof(float);
    if (dt == RX_BF16)
      hipLaunchKernelGGL((stem_fwd32_kernel<bf16_t>), dim3(G, n), dim3(256), lds, st, x_ncdhw, cin, z, y, x, w, bias, (bf16_t*)out->ptr, out->ld,
                         V * out->ld, out->c, kernel[0], kernel[1], kernel[2]);
    else
      hipLaunchKernelGGL((stem_fwd32_kernel<f16_t>), dim3(G, n), dim3(256), lds, st, x_ncdhw, cin, z, y, x, w, bias, (f16_t*)out->ptr, out->ld,
                         V * out->ld, out->c, kernel[0], kernel[1], kernel[2]);
    RX_CHECK_LAUNCH("rx_stem_conv_fwd(32)");
    return RX_OK;
  }
  RX_DISPATCH_DTYPE(dt, T, {
    constexpr int P = Elem<T>::PER16;
    long total = rx_act_voxels(out) * (out->c / P);
    int G = (int)((total + 255) / 256 > 8192 ? 8192 : (total + 255) / 256);
    hipLaunchKernelGGL((stem_fwd_kernel<T>), dim3(G, n), dim3(256), (size_t)out->c * cin * TT * sizeof(float), st, x_ncdhw, cin, z, y, x, w,
                       bias, (T*)out->ptr, out->ld, rx_act_voxels(out) * out->ld, out->c, kernel[0], kernel[1], kernel[2]);
  });
  RX_CHECK_LAUNCH("rx_stem_conv_fwd");
  return RX_OK;
}

// stem weight gradient: dw[co][ci][t] = sum_{n,v} dy[n][v][co] * x[n][ci][v + t - pad]
// thread -> (voxel lane, vector of 4 output channels); 27 accumulators x 4 channels per input
// channel (grid.z = ci); lanes of equal channel-vector are combined with xor-shuffles, waves
// through LDS, blocks through the partial buffer.
template <typename T>
__global__ __launch_bounds__(256) void stem_wgrad_kernel(const float* __restrict__ x, int Cin, int Z, int Y, int X, const T* __restrict__ dy,
                                                         int ldy, long sy, int Co, int kz, int ky, int kx, int N, int chunk_vox,
                                                         float* __restrict__ partial /*[nch][Cin][27][Co]*/) {
  const int ci = blockIdx.z;
  const int CQ = Co / 4;  // channel quads; requires CQ | 64
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int cq = lane % CQ, vl = (threadIdx.x) / CQ;  // vl in [0, 256/CQ)
  const int VPB = 256 / CQ;
  const long V = (long)Z * Y * X;
  const long NV = (long)N * V;
  const int TT = kz * ky * kx;
  const int pz = (kz - 1) / 2, py = (ky - 1) / 2, px = (kx - 1) / 2;
  float acc[27][4];
#pragma unroll
  for (int t = 0; t < 27; ++t)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[t][j] = 0.f;
  const long q_begin = (long)blockIdx.x * chunk_vox;
  const long q_end = q_begin + chunk_vox < NV ? q_begin + chunk_vox : NV;
  for (long q = q_begin + vl; q < q_end; q += VPB) {
    int n = (int)(q / V);
    long v = q - (long)n * V;
    int xx = (int)(v % X), yy = (int)((v / X) % Y), zz = (int)(v / ((long)X * Y));
    const T* dp = dy + n * sy + v * ldy + cq * 4;
    float d[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) d[j] = Elem<T>::to_f(dp[j]);
    const float* xc = x + ((size_t)n * Cin + ci) * V;
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int b = 0; b < 3; ++b)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          if (a < kz && b < ky && c < kx) {
            int z2 = zz + a - pz, y2 = yy + b - py, x2 = xx + c - px;
            float xv = 0.f;
            if ((unsigned)z2 < (unsigned)Z && (unsigned)y2 < (unsigned)Y && (unsigned)x2 < (unsigned)X)
              xv = xc[((long)z2 * Y + y2) * X + x2];
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[a * 9 + b * 3 + c][j] += xv * d[j];  // static index: stays in VGPRs
          }
        }
  }
  // combine lanes with equal cq inside the wave (lane = k*CQ + cq)
  for (int o = CQ; o < 64; o <<= 1) {
#pragma unroll
    for (int t = 0; t < 27; ++t)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[t][j] += __shfl_xor(acc[t][j], o, 64);
  }
  __shared__ float red[4][27][64];  // [wave][t][co]  (Co <= 64)
  if (lane < CQ) {
#pragma unroll
    for (int t = 0; t < 27; ++t)
#pragma unroll
      for (int j = 0; j < 4; ++j) red[wave][t][cq * 4 + j] = acc[t][j];
  }
  __syncthreads();
  (void)TT;
  for (int i = threadIdx.x; i < 27 * Co; i += 256) {
    int t = i / Co, co = i - t * Co;  // t = a*9 + b*3 + c slot
    float s = red[0][t][co] + red[1][t][co] + red[2][t][co] + red[3][t][co];
    partial[(((size_t)blockIdx.x * Cin + ci) * 27 + t) * Co + co] = s;
  }
}

__global__ __launch_bounds__(256) void stem_wgrad_finalize(const float* __restrict__ partial, int nch, int Cin, int ky, int kx, int TT, int Co,
                                                           float* __restrict__ dw) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);  // one wave per (co, ci, t) of the torch layout
  if (i >= Co * Cin * TT) return;
  int co = i / (Cin * TT), r = i - co * (Cin * TT), ci = r / TT, t = r - ci * TT;
  int a = t / (ky * kx), b = (t / kx) % ky, c = t % kx;
  int slot = a * 9 + b * 3 + c;
  double s = 0.0;
  for (int k = lane; k < nch; k += 64) s += (double)partial[(((size_t)k * Cin + ci) * 27 + slot) * Co + co];
  s = wave_sum_d(s);
  if (lane == 0) dw[i] = (float)s;
}

#define RX_STEM_CHUNKS 1024
extern "C" size_t rx_stem_conv_bwd_weight_workspace(int cin, int cout, int taps) {
  (void)taps;
  return (size_t)RX_STEM_CHUNKS * cin * 27 * cout * sizeof(float) + 256;
}

extern "C" int rx_stem_conv_bwd_weight(rx_dtype dt, const float* x_ncdhw, int n, int cin, int z, int y, int x, const rx_act* dy, float* dw,
                                       const int32_t kernel[3], void* ws, size_t ws_bytes, void* stream) {
  RX_RECORD(stream, [=, dy_ = RxActV(dy), kernel_ = RxI3V(kernel)](void* s) { return rx_stem_conv_bwd_weight(dt, x_ncdhw, n, cin, z, y, x, dy_.p(), dw, kernel_.v, ws, ws_bytes, s); });
  int rc;
  if ((rc = check_vec_channels(dy, dt, "rx_stem_conv_bwd_weight(dy)"))) return rc;
  if ((rc = check_kernel13(kernel, "rx_stem_conv_bwd_weight"))) return rc;
  if (!x_ncdhw || !dw || !ws || cin < 1 || cin > 16) RX_FAIL(RX_EUNSUPPORTED, "rx_stem_conv_bwd_weight: 1 <= Cin <= 16");
  const int Co = dy->c;
  if (Co > 64 || Co % 4 || 64 % (Co / 4)) RX_FAIL(RX_EUNSUPPORTED, "rx_stem_conv_bwd_weight: Cout must be 4,8,16,32 or 64 (got %d)", Co);
  if (dy->n != n || dy->z != z || dy->y != y || dy->x != x) RX_FAIL(RX_EINVAL, "rx_stem_conv_bwd_weight: geometry mismatch");
  if (ws_bytes < rx_stem_conv_bwd_weight_workspace(cin, Co, 27)) RX_FAIL(RX_EWORKSPACE, "rx_stem_conv_bwd_weight: workspace too small");
  hipStream_t st0 = (hipStream_t)stream;
  {
    int nb = 0;
    if (rx_stem_wgrad_mfma_try(dt, x_ncdhw, n, cin, z, y, x, dy, kernel, (float*)ws, RX_STEM_CHUNKS, &nb, st0) == 1) {
      const int TT0 = kernel[0] * kernel[1] * kernel[2];
      int tot0 = Co * cin * TT0;
      hipLaunchKernelGGL(stem_wgrad_finalize, dim3((tot0 + 3) / 4), dim3(256), 0, st0, (const float*)ws, nb, cin, kernel[1], kernel[2],
                         TT0, Co, dw);
      RX_CHECK_LAUNCH("rx_stem_conv_bwd_weight(mfma)");
      return RX_OK;
    }
  }
  const long NV = (long)n * z * y * x;
  const int VPB = 256 / (Co / 4);
  long chunk = (NV + RX_STEM_CHUNKS - 1) / RX_STEM_CHUNKS;
  chunk = (chunk + VPB - 1) / VPB * VPB;
  int nch = (int)((NV + chunk - 1) / chunk);
  const int TT = kernel[0] * kernel[1] * kernel[2];
  hipStream_t st = (hipStream_t)stream;
  RX_DISPATCH_DTYPE(dt, T, {
    hipLaunchKernelGGL((stem_wgrad_kernel<T>), dim3(nch, 1, cin), dim3(256), 0, st, x_ncdhw, cin, z, y, x, (const T*)dy->ptr, dy->ld,
                       rx_act_voxels(dy) * dy->ld, Co, kernel[0], kernel[1], kernel[2], n, (int)chunk, (float*)ws);
    int tot = Co * cin * TT;
    hipLaunchKernelGGL(stem_wgrad_finalize, dim3((tot + 3) / 4), dim3(256), 0, st, (const float*)ws, nch, cin, kernel[1], kernel[2], TT, Co,
                       dw);
  });
  RX_CHECK_LAUNCH("rx_stem_conv_bwd_weight");
  return RX_OK;
}
