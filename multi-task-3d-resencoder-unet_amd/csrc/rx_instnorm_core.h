// rx_instnorm_core.h -- the arithmetic of the InstanceNorm + LeakyReLU family (rx_instnorm.hip, rx_head.hip, rx_se.hip), once:
//   xhat = (y - mean) * rstd;   g' = g * lrelu'(.);   dy = rstd * (g' - m1 - xhat * m2)
// A kernel that fuses one of these passes into something else calls the helpers below and inherits the rounding points: every
// helper works in fp32 on values already read back from the storage type; what a kernel rounds, and when, stays in the kernel.
#pragma once
#include "rx_common.h"

// where the LeakyReLU mask of a backward pass comes from
enum InMask {
  IN_MASK_NONE = 0,  // slope 1: no mask
  IN_MASK_OUT = 1,   // sign of the saved output (residual blocks)
  IN_MASK_XHAT = 2   // no residual: out > 0 <=> xhat > 0, the output tensor is not read at all (`out` may be NULL)
};
static inline InMask in_mask_of(float slope, const rx_act* out) { return slope == 1.0f ? IN_MASK_NONE : (out ? IN_MASK_OUT : IN_MASK_XHAT); }

// the interleaved (mean, rstd) / (m1, m2) tables: tab[2 * (n*C + c)], tab[2 * (n*C + c) + 1] for the P channels from c0
template <int P>
__device__ inline void load_pair(const float* tab, int n, int C, int c0, float (&a)[P], float (&b)[P]) {
#pragma unroll
  for (int j = 0; j < P; ++j) {
    a[j] = tab[2 * ((size_t)n * C + c0 + j)];
    b[j] = tab[2 * ((size_t)n * C + c0 + j) + 1];
  }
}

// Sweep of grid = (G, N) over the `voxels` * CV 16-byte vectors of sample n = blockIdx.y.  sweep_grid (rx_reduce.h) gives
// (G * 256) % CV == 0, so a thread keeps the channel vector `cv` it starts with and its per-channel values stay in registers:
//   for (Sweep<P> s(V, C); s.more(); s.next()) { ... s.v() ... s.cv * P ... }
template <int P>
struct Sweep {
  int CV, n, cv;
  long total, step, i;
  __device__ inline Sweep(long voxels, int C)
      : CV(C / P), n(blockIdx.y), total(voxels * CV), step((long)gridDim.x * 256), i((long)blockIdx.x * 256 + threadIdx.x) {
    cv = (int)(i % CV);
  }
  __device__ inline bool more() const { return i < total; }
  __device__ inline void next() { i += step; }
  __device__ inline long v() const { return i / CV; }
};

template <typename T>
__device__ inline float in_xhat(T y, float mean, float rstd) {
  return (Elem<T>::to_f(y) - mean) * rstd;
}

// forward element: lrelu(xhat [* mult] [+ res]) rounded to T; `res` is read only with HAS_RES, `mult` only with GATED
template <typename T, bool HAS_RES, bool GATED = false>
__device__ inline T in_fwd_elem(T y, float mean, float rstd, const T& res, float slope, float mult = 1.f) {
  float f = in_xhat(y, mean, rstd);
  if (GATED) f *= mult;
  if (HAS_RES) f += Elem<T>::to_f(res);
  f = f > 0.f ? f : f * slope;
  return Elem<T>::from_f(f);
}

// backward element pair.  in_bwd_gprime turns g into g' in place (by value, the compiler contracts a different multiply-add
// in in_small_bwd_kernel<float, 32>); `out` is read only under IN_MASK_OUT, the first form is for layers that never have one.
__device__ inline void in_bwd_gprime(float& g, float xh, InMask mask, float slope) {
  if (mask == IN_MASK_XHAT && !(xh > 0.f)) g *= slope;
}
template <typename T>
__device__ inline void in_bwd_gprime(float& g, float xh, InMask mask, const T& out, float slope) {
  if (mask == IN_MASK_OUT && !(Elem<T>::to_f(out) > 0.f)) g *= slope;
  in_bwd_gprime(g, xh, mask, slope);
}
__device__ inline float in_bwd_dy(float gp, float xh, float rstd, float m1, float m2) { return rstd * (gp - m1 - xh * m2); }

// rank-K gradient under a task head: gk[k] = dout[n][k][v], d[j] = sum_k gk[k] * w[k][j] (k ascending), K <= MAXK
template <int MAXK, int P>
__device__ inline void head_grad_vec(const float* dout, int n, int K, int V, long v, const float (&w)[MAXK][P], float (&d)[P],
                                     float (&gk)[MAXK]) {
#pragma unroll
  for (int j = 0; j < P; ++j) d[j] = 0.f;
#pragma unroll
  for (int k = 0; k < MAXK; ++k) {
    gk[k] = 0.f;
    if (k < K) {
      gk[k] = dout[((size_t)n * K + k) * V + v];
#pragma unroll
      for (int j = 0; j < P; ++j) d[j] += gk[k] * w[k][j];
    }
  }
}

// Block reduction of the single-launch kernels (256 threads; thread = (voxel lane, 16-byte chunk ck = tid % (G / P)) of a G-channel
// group): xor-shuffle across the voxel lanes of a wave, one fp64 row per wave in LDS.  in_small_total adds the four waves in order.
template <int G, int P>
__device__ inline void in_small_reduce(float (&s)[P], float (&q)[P], double (&red)[4][2][G]) {
  constexpr int CPG = G / P;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int o = CPG; o < 64; o <<= 1) {
#pragma unroll
    for (int j = 0; j < P; ++j) {
      s[j] += __shfl_xor(s[j], o, 64);
      q[j] += __shfl_xor(q[j], o, 64);
    }
  }
  if (lane < CPG) {
#pragma unroll
    for (int j = 0; j < P; ++j) {
      red[wave][0][lane * P + j] = (double)s[j];
      red[wave][1][lane * P + j] = (double)q[j];
    }
  }
  __syncthreads();
}
template <int G>
__device__ inline double in_small_total(const double (&red)[4][2][G], int a, int c) {
  return red[0][a][c] + red[1][a][c] + red[2][a][c] + red[3][a][c];
}
