// rx_instnorm.hip -- HBM-bound kernels of the hot path: InstanceNorm statistics, the fused
// InstanceNorm-apply + LeakyReLU + residual-add forward / backward, per-channel sums and AvgPool.
//
// All activations are channels-last; every thread moves 16-byte channel vectors (8 bf16 / 4 f32),
// adjacent lanes touch adjacent addresses, per-(n,c) reductions are deterministic two-stage
// reductions (per-block partials in a workspace, finalised in fp64) -- no float atomics.
#include <math.h>

#include "rx_common.h"
#include "rx_internal.h"
#include "rx_reduce.h"
#include "rx_instnorm_core.h"

__global__ __launch_bounds__(256) void colreduce_finalize(const float* __restrict__ partial, int N, int nchunks, int nacc, int C, double V,
                                                          float eps, int mode, float* __restrict__ out) {
  const int i = blockIdx.x;  // element index
  double s0 = 0.0, s1 = 0.0;
  if (mode == FIN_SUM_OVER_N) {
    const int a = i / C, c = i - a * C;
    fin_gather(partial + (size_t)a * C + c, (size_t)nacc * C, N * nchunks, 0, s0, s1);
    if (threadIdx.x == 0) out[i] = (float)s0;
    return;
  }
  const int n = i / C, c = i - n * C;
  fin_gather(partial + ((size_t)n * nchunks * 2) * C + c, (size_t)2 * C, nchunks, C, s0, s1);
  if (threadIdx.x != 0) return;
  if (mode == FIN_STATS) {
    double mean = s0 / V;
    double var = s1 / V - mean * mean;
    if (var < 0.0) var = 0.0;
    out[2 * i] = (float)mean;
    out[2 * i + 1] = (float)(1.0 / sqrt(var + (double)eps));
  } else {
    out[2 * i] = (float)(s0 / V);
    out[2 * i + 1] = (float)(s1 / V);
  }
}

void rx_colreduce_finalize_launch(hipStream_t st, const float* partial, int N, int nchunks, int nacc, int C, double V, float eps, int mode,
                                  float* out) {
  const int elems = mode == FIN_SUM_OVER_N ? nacc * C : N * C;
  hipLaunchKernelGGL(colreduce_finalize, dim3(elems), dim3(256), 0, st, partial, N, nchunks, nacc, C, V, eps, mode, out);
}

// ---- InstanceNorm statistics ----------------------------------------------------------------
template <typename T>
struct StatsOp {
  ActView<T> y;
  __device__ inline void prepare(int, int) {}
  __device__ inline void accumulate(int n, int v, int c0, float (&acc)[2][Elem<T>::PER16]) const {
    Vec16<T> x = ld16(y.at(n, v, c0));
#pragma unroll
    for (int j = 0; j < Elem<T>::PER16; ++j) {
      float f = Elem<T>::to_f(x.v[j]);
      acc[0][j] += f;
      acc[1][j] += f * f;
    }
  }
};

extern "C" size_t rx_instnorm_stats_workspace(const rx_act* y) {
  if (!rx_act_ok(y)) return 0;
  return rx_reduce_ws_bytes(y->n, rx_act_voxels(y), y->c, 2);
}

extern "C" int rx_instnorm_stats(rx_dtype dt, const rx_act* y, float eps, float* stats, void* ws, size_t ws_bytes,
                                 void* stream) {
  RX_RECORD(stream, [=, y_ = RxActV(y)](void* s) { return rx_instnorm_stats(dt, y_.p(), eps, stats, ws, ws_bytes, s); });
  int rc = check_vec_channels(y, dt, "rx_instnorm_stats");
  if (rc) return rc;
  if (!stats || !ws) RX_FAIL(RX_EINVAL, "rx_instnorm_stats: null stats/workspace");
  if (ws_bytes < rx_instnorm_stats_workspace(y)) RX_FAIL(RX_EWORKSPACE, "rx_instnorm_stats: workspace too small");
  const long V = rx_act_voxels(y);
  hipStream_t st = (hipStream_t)stream;
  RX_DISPATCH_DTYPE(dt, T, {
    ReducePlan p = launch_colreduce<T, 2>(StatsOp<T>{make_view<T>(y)}, y->n, V, y->c, (float*)ws, st);
    rx_colreduce_finalize_launch(st, (const float*)ws, y->n, p.nchunks, 2, y->c, (double)V, eps, (int)FIN_STATS, stats);
  });
  RX_CHECK_LAUNCH("rx_instnorm_stats");
  return RX_OK;
}

// ---- nn.Dropout3d / nn.Dropout2d in front of an InstanceNorm (simple_conv_blocks.py:57-66: conv -> dropout -> norm) --------
// Channel dropout multiplies a whole (n, c) plane by 0 or by s = 1/(1-p).  InstanceNorm(affine=False) of s*y is
// (y - mean) / sqrt(var + eps/s^2): the kept planes need no pass over y at all, only the smaller eps (the caller passes
// eps*(1-p)^2 to the statistics); a dropped plane normalises to exactly 0, which is rstd = 0 in the (mean, rstd) pair every
// forward AND backward InstanceNorm kernel of this library works from (xhat = 0, dy = rstd * (...) = 0).  This entry point
// applies the second half: stats[i].rstd *= keep[i], keep[n*C + c] in {0, 1}.
__global__ __launch_bounds__(256) void stats_mask_kernel(float* __restrict__ stats, const float* __restrict__ keep, int count) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < count) stats[2 * i + 1] *= keep[i];
}

extern "C" int rx_instnorm_stats_mask(float* stats, const float* keep, int count, void* stream) {
  RX_RECORD(stream, [=](void* s) { return rx_instnorm_stats_mask(stats, keep, count, s); });
  if (!stats || !keep || count < 0) RX_FAIL(RX_EINVAL, "rx_instnorm_stats_mask: bad arguments");
  if (count == 0) return RX_OK;
  hipLaunchKernelGGL(stats_mask_kernel, dim3((count + 255) / 256), dim3(256), 0, (hipStream_t)stream, stats, keep, count);
  RX_CHECK_LAUNCH("rx_instnorm_stats_mask");
  return RX_OK;
}

// (mean, rstd) from per-chunk partial sums laid out like colreduce_kernel's (rx_conv_halo.hip leaves such partials behind
// when a persistent conv kernel accumulates the statistics of its own output)
void rx_stats_finalize_launch(const float* partial, int N, int nchunks, int C, double V, float eps, float* stats, hipStream_t st) {
  rx_colreduce_finalize_launch(st, partial, N, nchunks, 2, C, V, eps, (int)FIN_STATS, stats);
}

// ---- per-channel sum over (n, voxels) -------------------------------------------------------
template <typename T>
struct SumOp {
  ActView<T> x;
  __device__ inline void prepare(int, int) {}
  __device__ inline void accumulate(int n, int v, int c0, float (&acc)[1][Elem<T>::PER16]) const {
    Vec16<T> a = ld16(x.at(n, v, c0));
#pragma unroll
    for (int j = 0; j < Elem<T>::PER16; ++j) acc[0][j] += Elem<T>::to_f(a.v[j]);
  }
};
extern "C" size_t rx_channel_sum_workspace(const rx_act* x) {
  if (!rx_act_ok(x)) return 0;
  return rx_reduce_ws_bytes(x->n, rx_act_voxels(x), x->c, 1);
}
extern "C" int rx_channel_sum(rx_dtype dt, const rx_act* x, float* out, void* ws, size_t ws_bytes, void* stream) {
  RX_RECORD(stream, [=, x_ = RxActV(x)](void* s) { return rx_channel_sum(dt, x_.p(), out, ws, ws_bytes, s); });
  int rc = check_vec_channels(x, dt, "rx_channel_sum");
  if (rc) return rc;
  if (!out || !ws) RX_FAIL(RX_EINVAL, "rx_channel_sum: null out/workspace");
  if (ws_bytes < rx_channel_sum_workspace(x)) RX_FAIL(RX_EWORKSPACE, "rx_channel_sum: workspace too small");
  const long V = rx_act_voxels(x);
  hipStream_t st = (hipStream_t)stream;
  RX_DISPATCH_DTYPE(dt, T, {
    ReducePlan p = launch_colreduce<T, 1>(SumOp<T>{make_view<T>(x)}, x->n, V, x->c, (float*)ws, st);
    rx_colreduce_finalize_launch(st, (const float*)ws, x->n, p.nchunks, 1, x->c, (double)V, 0.f, (int)FIN_SUM_OVER_N, out);
  });
  RX_CHECK_LAUNCH("rx_channel_sum");
  return RX_OK;
}

// ---- fused InstanceNorm-apply + residual + LeakyReLU forward -------------------------------
// grid = (G, N); a thread keeps its channel vector fixed (G*256 % CV == 0) so mean/rstd live in
// registers for the whole sweep.
template <typename T, bool HAS_RES>
__global__ __launch_bounds__(256) void in_act_fwd_kernel(const T* __restrict__ y, int ldy, long sy, const float* __restrict__ stats,
                                                         const T* __restrict__ res, int ldr, long sr, T* __restrict__ out, int ldo,
                                                         long so, int V, int C, float slope) {
  constexpr int P = Elem<T>::PER16;
  Sweep<P> s(V, C);
  const int n = s.n, c0 = s.cv * P;
  float mean[P], rstd[P];
  load_pair(stats, n, C, c0, mean, rstd);
  const T* yn = y + n * sy;
  const T* rn = HAS_RES ? res + n * sr : nullptr;
  T* on = out + n * so;
  for (; s.more(); s.next()) {
    const long v = s.v();
    Vec16<T> a = ld16(yn + v * ldy + c0);
    Vec16<T> r;
    if (HAS_RES) r = ld16(rn + v * ldr + c0);
    Vec16<T> o;
#pragma unroll
    for (int j = 0; j < P; ++j) o.v[j] = in_fwd_elem<T, HAS_RES>(a.v[j], mean[j], rstd[j], r.v[j], slope);
    st16(on + v * ldo + c0, o);
  }
}

extern "C" int rx_instnorm_act_fwd(rx_dtype dt, const rx_act* y, const float* stats, const rx_act* residual,
                                   const rx_act* out, float slope, void* stream) {
  RX_RECORD(stream, [=, y_ = RxActV(y), residual_ = RxActV(residual), out_ = RxActV(out)](void* s) { return rx_instnorm_act_fwd(dt, y_.p(), stats, residual_.p(), out_.p(), slope, s); });
  int rc = check_acts(dt, "rx_instnorm_act_fwd", y, {{"y", y, true}, {"out", out, true}, {"residual", residual, false}});
  if (rc) return rc;
  if (!stats) RX_FAIL(RX_EINVAL, "rx_instnorm_act_fwd: null stats");
  const long V = rx_act_voxels(y);
  hipStream_t st = (hipStream_t)stream;
  RX_DISPATCH_DTYPE(dt, T, {
    const int CV = y->c / Elem<T>::PER16, G = sweep_grid(V * CV, CV);
    const ActView<T> r = make_view<T>(residual);
    hipLaunchKernelGGL((residual ? in_act_fwd_kernel<T, true> : in_act_fwd_kernel<T, false>), dim3(G, y->n), dim3(256), 0, st, (const T*)y->ptr,
                       y->ld, V * y->ld, stats, r.ptr, r.ld, r.sample_stride, (T*)out->ptr, out->ld, V * out->ld, (int)V, y->c, slope);
  });
  RX_CHECK_LAUNCH("rx_instnorm_act_fwd");
  return RX_OK;
}

// ---- fused backward --------------------------------------------------------------------------
// g' = g * (out > 0 ? 1 : slope);  xhat = (y-mean)*rstd
// pass 1: m1 = mean(g'), m2 = mean(g'*xhat) per (n,c);  pass 2: dy = rstd*(g' - m1 - xhat*m2)
template <typename T>
struct InBwdOp {
  ActView<T> g, y, out;
  const float* stats;
  int C;
  float slope;
  InMask mask;
  float mean[Elem<T>::PER16], rstd[Elem<T>::PER16];
  __device__ inline void prepare(int n, int c0) { load_pair(stats, n, C, c0, mean, rstd); }
  __device__ inline void accumulate(int n, int v, int c0, float (&acc)[2][Elem<T>::PER16]) const {
    constexpr int P = Elem<T>::PER16;
    Vec16<T> gv = ld16(g.at(n, v, c0));
    Vec16<T> yv = ld16(y.at(n, v, c0));
    Vec16<T> ov;
    if (mask == IN_MASK_OUT) ov = ld16(out.at(n, v, c0));
#pragma unroll
    for (int j = 0; j < P; ++j) {
      const float xh = in_xhat(yv.v[j], mean[j], rstd[j]);
      float gg = Elem<T>::to_f(gv.v[j]);
      in_bwd_gprime(gg, xh, mask, ov.v[j], slope);
      acc[0][j] += gg;
      acc[1][j] += gg * xh;
    }
  }
};

template <typename T, bool HAS_DRES, bool ACC_DRES>
__global__ __launch_bounds__(256) void in_act_bwd_apply_kernel(const T* __restrict__ g, int ldg, long sg, const T* __restrict__ y, int ldy,
                                                               long sy, const T* __restrict__ out, int ldo, long so,
                                                               const float* __restrict__ stats, const float* __restrict__ m12,
                                                               T* __restrict__ dy, int lddy, long sdy, T* __restrict__ dres, int lddr,
                                                               long sdr, int V, int C, float slope, InMask mask) {
  constexpr int P = Elem<T>::PER16;
  Sweep<P> s(V, C);
  const int n = s.n, c0 = s.cv * P;
  float mean[P], rstd[P], m1[P], m2[P];
  load_pair(stats, n, C, c0, mean, rstd);
  load_pair(m12, n, C, c0, m1, m2);
  for (; s.more(); s.next()) {
    const long v = s.v();
    Vec16<T> gv = ld16(g + n * sg + v * ldg + c0);
    Vec16<T> yv = ld16(y + n * sy + v * ldy + c0);
    Vec16<T> ov;
    if (mask == IN_MASK_OUT) ov = ld16(out + n * so + v * ldo + c0);
    Vec16<T> dv, rv;
    if (HAS_DRES && ACC_DRES) rv = ld16(dres + n * sdr + v * lddr + c0);
#pragma unroll
    for (int j = 0; j < P; ++j) {
      const float xh = in_xhat(yv.v[j], mean[j], rstd[j]);
      float gg = Elem<T>::to_f(gv.v[j]);
      in_bwd_gprime(gg, xh, mask, ov.v[j], slope);
      dv.v[j] = Elem<T>::from_f(in_bwd_dy(gg, xh, rstd[j], m1[j], m2[j]));
      if (HAS_DRES) {
        float r = gg;
        if (ACC_DRES) r += Elem<T>::to_f(rv.v[j]);
        rv.v[j] = Elem<T>::from_f(r);
      }
    }
    st16(dy + n * sdy + v * lddy + c0, dv);
    if (HAS_DRES) st16(dres + n * sdr + v * lddr + c0, rv);
  }
}

// apply pass on (g, y[, out]) -> dy[, d_residual]; `out` is passed on only under IN_MASK_OUT
template <typename T>
static void launch_bwd_apply(const rx_act* g, const rx_act* y, const float* stats, const rx_act* out, float slope, InMask mask, const float* m12,
                             const rx_act* dy, const rx_act* d_residual, int accumulate_residual, hipStream_t st) {
  const long V = rx_act_voxels(y);
  const int CV = y->c / Elem<T>::PER16, G = sweep_grid(V * CV, CV);
  const ActView<T> o = make_view<T>(mask == IN_MASK_OUT ? out : nullptr), dr = make_view<T>(d_residual);
  auto kern = !d_residual ? in_act_bwd_apply_kernel<T, false, false>
                          : (accumulate_residual ? in_act_bwd_apply_kernel<T, true, true> : in_act_bwd_apply_kernel<T, true, false>);
  hipLaunchKernelGGL(kern, dim3(G, y->n), dim3(256), 0, st, (const T*)g->ptr, g->ld, V * g->ld, (const T*)y->ptr, y->ld, V * y->ld, o.ptr, o.ld,
                     o.sample_stride, stats, m12, (T*)dy->ptr, dy->ld, V * dy->ld, (T*)dr.ptr, dr.ld, dr.sample_stride, (int)V, y->c, slope, mask);
}

// ---- single-launch InstanceNorm forward / backward for SMALL tensors (low-resolution stages) ---------------------
// At 8^3 and below (measured: 16^3 is already better off with the chip-filling three-launch path; narrower 8-channel
// groups did not change that) a layer's tensor is a few hundred KB and the three launches (partials, finalize, apply) are pure
// launch latency on the critical chain.  One workgroup owns (sample n, 32 consecutive channels): pass 1 reduces over all
// voxels (thread = (voxel lane, 16-byte channel chunk); xor-shuffle across the 16 voxel lanes of a wave, LDS across the
// 4 waves, fp64 for the final combination), pass 2 re-reads the (L2-resident) data and applies.
template <typename T, int G, bool HAS_RES>
__global__ __launch_bounds__(256) void in_small_fwd_kernel(const T* __restrict__ y, int ldy, long sy, const T* __restrict__ res, int ldr,
                                                           long sr, T* __restrict__ out, int ldo, long so, float* __restrict__ stats, int V,
                                                           int C, float eps, float slope) {
  constexpr int P = Elem<T>::PER16;
  constexpr int CPG = G / P;  // 16-byte chunks per G-channel group
  __shared__ double red[4][2][G];
  __shared__ float mr[2][G];
  const int tid = threadIdx.x;
  const int n = blockIdx.y, c0 = blockIdx.x * G;
  const int ck = tid % CPG, vl = tid / CPG;
  const int VL = 256 / CPG;
  const T* yn = y + n * sy + c0 + ck * P;
  float s[P], q[P];
#pragma unroll
  for (int j = 0; j < P; ++j) s[j] = q[j] = 0.f;
  for (int v = vl; v < V; v += VL) {
    Vec16<T> a = ld16(yn + (long)v * ldy);
#pragma unroll
    for (int j = 0; j < P; ++j) {
      float f = Elem<T>::to_f(a.v[j]);
      s[j] += f;
      q[j] += f * f;
    }
  }
  in_small_reduce<G>(s, q, red);
  if (tid < G) {
    double s0 = in_small_total(red, 0, tid), s1 = in_small_total(red, 1, tid);
    double mean = s0 / V, var = s1 / V - mean * mean;
    if (var < 0.0) var = 0.0;
    float m = (float)mean, r = (float)(1.0 / sqrt(var + (double)eps));
    mr[0][tid] = m;
    mr[1][tid] = r;
    stats[2 * ((size_t)n * C + c0 + tid)] = m;
    stats[2 * ((size_t)n * C + c0 + tid) + 1] = r;
  }
  __syncthreads();
  float mean[P], rstd[P];
#pragma unroll
  for (int j = 0; j < P; ++j) {
    mean[j] = mr[0][ck * P + j];
    rstd[j] = mr[1][ck * P + j];
  }
  const T* rn = HAS_RES ? res + n * sr + c0 + ck * P : nullptr;
  T* on = out + n * so + c0 + ck * P;
  for (int v = vl; v < V; v += VL) {
    Vec16<T> a = ld16(yn + (long)v * ldy);
    Vec16<T> r;
    if (HAS_RES) r = ld16(rn + (long)v * ldr);
    Vec16<T> o;
#pragma unroll
    for (int j = 0; j < P; ++j) o.v[j] = in_fwd_elem<T, HAS_RES>(a.v[j], mean[j], rstd[j], r.v[j], slope);
    st16(on + (long)v * ldo, o);
  }
}

template <typename T, int G>
__global__ __launch_bounds__(256) void in_small_bwd_kernel(const T* __restrict__ g, int ldg, long sg, const T* __restrict__ y, int ldy, long sy,
                                                           const T* __restrict__ out, int ldo, long so, const float* __restrict__ stats,
                                                           T* __restrict__ dy, int lddy, long sdy, T* __restrict__ dres, int lddr, long sdr,
                                                           int acc_res, int V, int C, float slope, InMask mask) {
  constexpr int P = Elem<T>::PER16;
  constexpr int CPG = G / P;
  __shared__ double red[4][2][G];
  __shared__ float mm[2][G];
  const int tid = threadIdx.x;
  const int n = blockIdx.y, c0 = blockIdx.x * G;
  const int ck = tid % CPG, vl = tid / CPG;
  const int VL = 256 / CPG;
  const long co = c0 + ck * P;
  float mean[P], rstd[P];
  load_pair(stats, n, C, c0 + ck * P, mean, rstd);
  auto gprime = [&](int v, float (&gg)[P], float (&xh)[P]) {
    Vec16<T> gv = ld16(g + n * sg + (long)v * ldg + co);
    Vec16<T> yv = ld16(y + n * sy + (long)v * ldy + co);
    Vec16<T> ov;
    if (mask == IN_MASK_OUT) ov = ld16(out + n * so + (long)v * ldo + co);
#pragma unroll
    for (int j = 0; j < P; ++j) {
      xh[j] = in_xhat(yv.v[j], mean[j], rstd[j]);
      gg[j] = Elem<T>::to_f(gv.v[j]);
      in_bwd_gprime(gg[j], xh[j], mask, ov.v[j], slope);
    }
  };
  float s[P], q[P];
#pragma unroll
  for (int j = 0; j < P; ++j) s[j] = q[j] = 0.f;
  for (int v = vl; v < V; v += VL) {
    float gg[P], xh[P];
    gprime(v, gg, xh);
#pragma unroll
    for (int j = 0; j < P; ++j) {
      s[j] += gg[j];
      q[j] += gg[j] * xh[j];
    }
  }
  in_small_reduce<G>(s, q, red);
  if (tid < G) {
    mm[0][tid] = (float)(in_small_total(red, 0, tid) / V);
    mm[1][tid] = (float)(in_small_total(red, 1, tid) / V);
  }
  __syncthreads();
  float m1[P], m2[P];
#pragma unroll
  for (int j = 0; j < P; ++j) {
    m1[j] = mm[0][ck * P + j];
    m2[j] = mm[1][ck * P + j];
  }
  for (int v = vl; v < V; v += VL) {
    float gg[P], xh[P];
    gprime(v, gg, xh);
    Vec16<T> dv, rv;
    if (dres && acc_res) rv = ld16(dres + n * sdr + (long)v * lddr + co);
#pragma unroll
    for (int j = 0; j < P; ++j) {
      dv.v[j] = Elem<T>::from_f(in_bwd_dy(gg[j], xh[j], rstd[j], m1[j], m2[j]));
      if (dres) {
        float r = gg[j];
        if (acc_res) r += Elem<T>::to_f(rv.v[j]);
        rv.v[j] = Elem<T>::from_f(r);
      }
    }
    st16(dy + n * sdy + (long)v * lddy + co, dv);
    if (dres) st16(dres + n * sdr + (long)v * lddr + co, rv);
  }
}

// largest per-sample voxel count that takes the single-launch path
constexpr long RX_IN_SMALL_MAX_VOXELS = 512;
// channels per workgroup of the single-launch kernels: 32, or 8 from this many voxels per sample upwards (the 8^3 stage; 80
// workgroups instead of 20 for 320 channels x 2 samples, one 16-byte vector per voxel and thread.  Alone 12.4 -> 7.6 us for
// the backward of a 320-channel 8^3 layer, 17.42 / 17.37 -> 17.32 / 17.30 ms per cfg2 step on one box)
constexpr long RX_IN_SMALL_NARROW_VOXELS = 256;

extern "C" int rx_instnorm_act_bwd(rx_dtype dt, const rx_act* g, const rx_act* y, const float* stats, const rx_act* out,
                                   float slope, const rx_act* dy, const rx_act* d_residual, int accumulate_residual, void* ws,
                                   size_t ws_bytes, void* stream) {
  RX_RECORD(stream, [=, g_ = RxActV(g), y_ = RxActV(y), out_ = RxActV(out), dy_ = RxActV(dy), d_residual_ = RxActV(d_residual)](void* s) { return rx_instnorm_act_bwd(dt, g_.p(), y_.p(), stats, out_.p(), slope, dy_.p(), d_residual_.p(), accumulate_residual, ws, ws_bytes, s); });
  // `out` may be NULL (no residual) and is read only where its sign is the mask
  const InMask mask = in_mask_of(slope, out);
  int rc = check_acts(dt, "rx_instnorm_act_bwd", y, {{"y", y, true}, {"g", g, true}, {"dy", dy, true},
                      {"out", mask == IN_MASK_OUT ? out : nullptr, false}, {"d_residual", d_residual, false}});
  if (rc) return rc;
  if (!stats || !ws) RX_FAIL(RX_EINVAL, "rx_instnorm_act_bwd: bad arguments");
  const long V = rx_act_voxels(y);
  const int N = y->n, C = y->c;
  hipStream_t st = (hipStream_t)stream;
  if (V <= RX_IN_SMALL_MAX_VOXELS && C % 32 == 0) {   // low-resolution stages: one launch instead of three
    const bool narrow = dt != RX_F32 && V >= RX_IN_SMALL_NARROW_VOXELS;   // (fp32 = parity mode: the summation order the goldens' seeds were screened with)
    RX_DISPATCH_DTYPE(dt, T, {
      const ActView<T> o = make_view<T>(mask == IN_MASK_OUT ? out : nullptr), dr = make_view<T>(d_residual);
      hipLaunchKernelGGL((narrow ? in_small_bwd_kernel<T, 8> : in_small_bwd_kernel<T, 32>), dim3(narrow ? C / 8 : C / 32, N), dim3(256), 0, st,
                         (const T*)g->ptr, g->ld, V * g->ld, (const T*)y->ptr, y->ld, V * y->ld, o.ptr, o.ld, o.sample_stride, stats, (T*)dy->ptr,
                         dy->ld, V * dy->ld, (T*)dr.ptr, dr.ld, dr.sample_stride, accumulate_residual, (int)V, C, slope, mask);
    });
    RX_CHECK_LAUNCH("rx_instnorm_act_bwd(small)");
    return RX_OK;
  }
  const ReduceWs w = reduce_ws(ws, N, V, C, 2);
  if (ws_bytes < w.need) RX_FAIL(RX_EWORKSPACE, "rx_instnorm_act_bwd: workspace too small (%zu < %zu)", ws_bytes, w.need);
  RX_DISPATCH_DTYPE(dt, T, {
    InBwdOp<T> op{make_view<T>(g), make_view<T>(y), make_view<T>(mask == IN_MASK_OUT ? out : y), stats, C, slope, mask, {}, {}};
    ReducePlan p = launch_colreduce<T, 2>(op, N, V, C, w.partial, st);
    rx_colreduce_finalize_launch(st, w.partial, N, p.nchunks, 2, C, (double)V, 0.f, (int)FIN_MEAN2, w.m12);
    launch_bwd_apply<T>(g, y, stats, out, slope, mask, w.m12, dy, d_residual, accumulate_residual, st);
  });
  RX_CHECK_LAUNCH("rx_instnorm_act_bwd");
  return RX_OK;
}


// ---- residual-block epilogue backward with the MASKED gradient materialised once --------------------------------------
// out = lrelu(IN(y) + res) (resblocks.py:113-114).  The masked gradient g' = g * lrelu'(out) is BOTH the input of the
// InstanceNorm backward and the gradient of the residual.  rx_instnorm_act_bwd read (g, y, out) twice and wrote dy and
// d_residual in its second pass: 3R + 3R 2W = 8 tensor passes.  Here the reduce pass writes g' into the residual-gradient
// buffer while it accumulates sum g' / sum g'*xhat (3R 1W) and the apply pass reads only (g', y) and writes dy (2R 1W): 7
// passes, and the apply kernel is the mask-free, residual-free instantiation.  pool_dy (optional): the gradient of the
// AvgPool that opens the NEXT stage's skip path (resblocks.py:95) -- g is then old_g + pool_dy[v / f] / |f| formed on the fly
// (the separate avgpool_bwd pass over the full-resolution gradient, 1R 1W, disappears as well).
// Sums are taken of g' AS STORED (rounded to the compute type): the apply pass sees exactly the values that were summed.
template <typename T, bool POOL>
struct InBwdResOp {
  ActView<T> g, y, out, pool;
  T* gp;            // masked gradient out (= d_residual), same geometry as y
  long gp_ss;
  int gp_ld;
  const float* stats;
  int C;
  float slope;
  int Yi, Xi, Yo, Xo, fz, fy, fx;
  float inv;
  float mean[Elem<T>::PER16], rstd[Elem<T>::PER16];
  __device__ inline void prepare(int n, int c0) { load_pair(stats, n, C, c0, mean, rstd); }
  __device__ inline void accumulate(int n, int v, int c0, float (&acc)[2][Elem<T>::PER16]) const {
    constexpr int P = Elem<T>::PER16;
    Vec16<T> gv = ld16(g.at(n, v, c0));
    Vec16<T> yv = ld16(y.at(n, v, c0));
    Vec16<T> ov = ld16(out.at(n, v, c0));
    Vec16<T> pv;
    if (POOL) {
      const int xi = v % Xi, t = v / Xi;
      const int yi = t % Yi, zi = t / Yi;
      const int vo = ((zi / fz) * Yo + (yi / fy)) * Xo + (xi / fx);
      pv = ld16(pool.at(n, vo, c0));
    }
    Vec16<T> w;
#pragma unroll
    for (int j = 0; j < P; ++j) {
      float gg = Elem<T>::to_f(gv.v[j]);
      if (POOL) gg += Elem<T>::to_f(pv.v[j]) * inv;
      const float xh = in_xhat(yv.v[j], mean[j], rstd[j]);
      in_bwd_gprime(gg, xh, IN_MASK_OUT, ov.v[j], slope);
      w.v[j] = Elem<T>::from_f(gg);
      gg = Elem<T>::to_f(w.v[j]);      // summed AS STORED
      acc[0][j] += gg;
      acc[1][j] += gg * xh;
    }
    st16(gp + n * gp_ss + (long)v * gp_ld + c0, w);
  }
};

extern "C" int rx_instnorm_act_bwd_res(rx_dtype dt, const rx_act* g, const rx_act* y, const float* stats, const rx_act* out, float slope,
                                       const rx_act* pool_dy, const int32_t pool_stride[3], const rx_act* d_residual, const rx_act* dy,
                                       void* ws, size_t ws_bytes, void* stream) {
  static const int32_t one3[3] = {1, 1, 1};
  if (!pool_stride) pool_stride = one3;
  RX_RECORD(stream, [=, g_ = RxActV(g), y_ = RxActV(y), out_ = RxActV(out), pool_dy_ = RxActV(pool_dy), pool_stride_ = RxI3V(pool_stride), d_residual_ = RxActV(d_residual), dy_ = RxActV(dy)](void* s) { return rx_instnorm_act_bwd_res(dt, g_.p(), y_.p(), stats, out_.p(), slope, pool_dy_.p(), pool_stride_.v, d_residual_.p(), dy_.p(), ws, ws_bytes, s); });
  int rc = check_acts(dt, "rx_instnorm_act_bwd_res", y, {{"y", y, true}, {"g", g, true}, {"out", out, true}, {"dy", dy, true},
                      {"d_residual", d_residual, true}});
  if (rc) return rc;
  if (!stats || !ws) RX_FAIL(RX_EINVAL, "rx_instnorm_act_bwd_res: bad arguments");
  if (d_residual->ptr == dy->ptr) RX_FAIL(RX_EINVAL, "rx_instnorm_act_bwd_res: d_residual and dy must be different buffers");
  if (pool_dy) {
    if ((rc = check_vec_channels(pool_dy, dt, "rx_instnorm_act_bwd_res(pool_dy)"))) return rc;
    if ((rc = check_pool(y, pool_dy, pool_stride, "rx_instnorm_act_bwd_res"))) return rc;
  }
  const long V = rx_act_voxels(y);
  const int N = y->n, C = y->c;
  const ReduceWs w = reduce_ws(ws, N, V, C, 2);
  if (ws_bytes < w.need) RX_FAIL(RX_EWORKSPACE, "rx_instnorm_act_bwd_res: workspace too small (%zu < %zu)", ws_bytes, w.need);
  hipStream_t st = (hipStream_t)stream;
  RX_DISPATCH_DTYPE(dt, T, {
    ReducePlan p;
    if (pool_dy) {
      InBwdResOp<T, true> op{make_view<T>(g), make_view<T>(y), make_view<T>(out), make_view<T>(pool_dy), (T*)d_residual->ptr,
                             V * (long)d_residual->ld, d_residual->ld, stats, C, slope, y->y, y->x, pool_dy->y, pool_dy->x,
                             pool_stride[0], pool_stride[1], pool_stride[2], 1.f / (float)(pool_stride[0] * pool_stride[1] * pool_stride[2]), {}, {}};
      p = launch_colreduce<T, 2>(op, N, V, C, w.partial, st);
    } else {
      InBwdResOp<T, false> op{make_view<T>(g), make_view<T>(y), make_view<T>(out), make_view<T>(y), (T*)d_residual->ptr,
                              V * (long)d_residual->ld, d_residual->ld, stats, C, slope, y->y, y->x, 1, 1, 1, 1, 1, 1.f, {}, {}};
      p = launch_colreduce<T, 2>(op, N, V, C, w.partial, st);
    }
    rx_colreduce_finalize_launch(st, w.partial, N, p.nchunks, 2, C, (double)V, 0.f, (int)FIN_MEAN2, w.m12);
    // apply: dy = rstd * (g' - m1 - xhat * m2) from (g', y) alone -- no mask, no residual output
    launch_bwd_apply<T>(d_residual, y, stats, nullptr, slope, IN_MASK_NONE, w.m12, dy, nullptr, 0, st);
  });
  RX_CHECK_LAUNCH("rx_instnorm_act_bwd_res");
  return RX_OK;
}

// ---- InstanceNorm backward with the two means supplied by the caller ------------------------------------------------
// (rx_conv3d_bwd_data_instats: the persistent backward-data kernel accumulates sum g' and sum g'*(y - mean) in its epilogue)
__global__ __launch_bounds__(256) void inbwd_fused_finalize(const float* __restrict__ partial, int N, int nchunks, int C, double V,
                                                            const float* __restrict__ stats, float* __restrict__ m12) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= N * C) return;
  const int n = i / C, c = i - n * C;
  double s0 = 0.0, s1 = 0.0;
  for (int k = lane; k < nchunks; k += 64) {
    const float* p = partial + ((size_t)(n * nchunks + k) * 2) * C + c;
    s0 += (double)p[0];
    s1 += (double)p[C];
  }
  s0 = wave_sum_d(s0);
  s1 = wave_sum_d(s1);
  if (lane != 0) return;
  m12[2 * i] = (float)(s0 / V);
  m12[2 * i + 1] = (float)((double)stats[2 * i + 1] * s1 / V);     // sum g'*xhat = rstd * sum g'*(y - mean)
}
void rx_inbwd_fused_finalize_launch(const float* partial, int N, int nchunks, int C, double V, const float* stats, float* m12, hipStream_t st) {
  hipLaunchKernelGGL(inbwd_fused_finalize, dim3((N * C + 3) / 4), dim3(256), 0, st, partial, N, nchunks, C, V, stats, m12);
}

extern "C" int rx_instnorm_act_bwd_apply(rx_dtype dt, const rx_act* g, const rx_act* y, const float* stats, const rx_act* out, float slope,
                                         const float* m12, const rx_act* dy, const rx_act* d_residual, int accumulate_residual,
                                         void* stream) {
  RX_RECORD(stream, [=, g_ = RxActV(g), y_ = RxActV(y), out_ = RxActV(out), dy_ = RxActV(dy), d_residual_ = RxActV(d_residual)](void* s) { return rx_instnorm_act_bwd_apply(dt, g_.p(), y_.p(), stats, out_.p(), slope, m12, dy_.p(), d_residual_.p(), accumulate_residual, s); });
  const InMask mask = in_mask_of(slope, out);
  int rc = check_acts(dt, "rx_instnorm_act_bwd_apply", y, {{"y", y, true}, {"g", g, true}, {"dy", dy, true},
                      {"out", mask == IN_MASK_OUT ? out : nullptr, false}, {"d_residual", d_residual, false}});
  if (rc) return rc;
  if (!stats || !m12) RX_FAIL(RX_EINVAL, "rx_instnorm_act_bwd_apply: bad arguments");
  RX_DISPATCH_DTYPE(dt, T, { launch_bwd_apply<T>(g, y, stats, out, slope, mask, m12, dy, d_residual, accumulate_residual, (hipStream_t)stream); });
  RX_CHECK_LAUNCH("rx_instnorm_act_bwd_apply");
  return RX_OK;
}

extern "C" int rx_instnorm_fwd(rx_dtype dt, const rx_act* y, float eps, float* stats, const rx_act* residual, const rx_act* out,
                               float slope, void* ws, size_t ws_bytes, void* stream) {
  RX_RECORD(stream, [=, y_ = RxActV(y), residual_ = RxActV(residual), out_ = RxActV(out)](void* s) { return rx_instnorm_fwd(dt, y_.p(), eps, stats, residual_.p(), out_.p(), slope, ws, ws_bytes, s); });
  int rc;
  if ((rc = check_vec_channels(y, dt, "rx_instnorm_fwd(y)"))) return rc;
  const long V = rx_act_voxels(y);
  if (V > RX_IN_SMALL_MAX_VOXELS || y->c % 32) {   // large tensors: bandwidth-bound three-launch path
    if ((rc = rx_instnorm_stats(dt, y, eps, stats, ws, ws_bytes, stream))) return rc;
    return rx_instnorm_act_fwd(dt, y, stats, residual, out, slope, stream);
  }
  if ((rc = check_acts(dt, "rx_instnorm_fwd", y, {{"out", out, true}, {"residual", residual, false}}))) return rc;
  if (!stats) RX_FAIL(RX_EINVAL, "rx_instnorm_fwd: null stats");
  hipStream_t st = (hipStream_t)stream;
  const bool narrow = dt != RX_F32 && V >= RX_IN_SMALL_NARROW_VOXELS;   // (fp32 = parity mode: the summation order the goldens' seeds were screened with)
  RX_DISPATCH_DTYPE(dt, T, {
    auto kern = residual ? (narrow ? in_small_fwd_kernel<T, 8, true> : in_small_fwd_kernel<T, 32, true>)
                         : (narrow ? in_small_fwd_kernel<T, 8, false> : in_small_fwd_kernel<T, 32, false>);
    const ActView<T> r = make_view<T>(residual);
    hipLaunchKernelGGL(kern, dim3(narrow ? y->c / 8 : y->c / 32, y->n), dim3(256), 0, st, (const T*)y->ptr, y->ld, V * y->ld, r.ptr, r.ld,
                       r.sample_stride, (T*)out->ptr, out->ld, V * out->ld, stats, (int)V, y->c, eps, slope);
  });
  RX_CHECK_LAUNCH("rx_instnorm_fwd");
  return RX_OK;
}

// ---- AvgPool (kernel = stride, per axis 1 or 2) ---------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void avgpool_fwd_kernel(const T* __restrict__ x, int ldx, long sx, T* __restrict__ y, int ldy, long sy,
                                                          int Zo, int Yo, int Xo, int Yi, int Xi, int C, int fz, int fy, int fx) {
  constexpr int P = Elem<T>::PER16;
  const int CV = C / P;
  const int n = blockIdx.y;
  const long total = (long)Zo * Yo * Xo * CV;
  const float inv = 1.f / (float)(fz * fy * fx);
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    int cv = (int)(i % CV);
    long vo = i / CV;
    int xo = (int)(vo % Xo);
    int yo = (int)((vo / Xo) % Yo);
    int zo = (int)(vo / ((long)Xo * Yo));
    float acc[P];
#pragma unroll
    for (int j = 0; j < P; ++j) acc[j] = 0.f;
    for (int a = 0; a < fz; ++a)
      for (int b = 0; b < fy; ++b)
        for (int c = 0; c < fx; ++c) {
          long vi = ((long)(zo * fz + a) * Yi + (yo * fy + b)) * Xi + (xo * fx + c);
          Vec16<T> t = ld16(x + n * sx + vi * ldx + cv * P);
#pragma unroll
          for (int j = 0; j < P; ++j) acc[j] += Elem<T>::to_f(t.v[j]);
        }
    Vec16<T> o;
#pragma unroll
    for (int j = 0; j < P; ++j) o.v[j] = Elem<T>::from_f(acc[j] * inv);
    st16(y + n * sy + vo * ldy + cv * P, o);
  }
}

template <typename T, bool ACC>
__global__ __launch_bounds__(256) void avgpool_bwd_kernel(const T* __restrict__ dy, int ldy, long sy, T* __restrict__ dx, int ldx, long sx,
                                                          int Zi, int Yi, int Xi, int Yo, int Xo, int C, int fz, int fy, int fx) {
  constexpr int P = Elem<T>::PER16;
  const int CV = C / P;
  const int n = blockIdx.y;
  const long total = (long)Zi * Yi * Xi * CV;
  const float inv = 1.f / (float)(fz * fy * fx);
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    int cv = (int)(i % CV);
    long vi = i / CV;
    int xi = (int)(vi % Xi);
    int yi = (int)((vi / Xi) % Yi);
    int zi = (int)(vi / ((long)Xi * Yi));
    long vo = ((long)(zi / fz) * Yo + (yi / fy)) * Xo + (xi / fx);
    Vec16<T> t = ld16(dy + n * sy + vo * ldy + cv * P);
    Vec16<T> o;
    if (ACC) o = ld16(dx + n * sx + vi * ldx + cv * P);
#pragma unroll
    for (int j = 0; j < P; ++j) {
      float f = Elem<T>::to_f(t.v[j]) * inv;
      if (ACC) f += Elem<T>::to_f(o.v[j]);
      o.v[j] = Elem<T>::from_f(f);
    }
    st16(dx + n * sx + vi * ldx + cv * P, o);
  }
}

extern "C" int rx_avgpool_fwd(rx_dtype dt, const rx_act* x, const rx_act* y, const int32_t stride[3], void* stream) {
  RX_RECORD(stream, [=, x_ = RxActV(x), y_ = RxActV(y), stride_ = RxI3V(stride)](void* s) { return rx_avgpool_fwd(dt, x_.p(), y_.p(), stride_.v, s); });
  int rc;
  if ((rc = check_vec_channels(x, dt, "rx_avgpool_fwd(x)"))) return rc;
  if ((rc = check_vec_channels(y, dt, "rx_avgpool_fwd(y)"))) return rc;
  if ((rc = check_pool(x, y, stride, "rx_avgpool_fwd"))) return rc;
  hipStream_t st = (hipStream_t)stream;
  RX_DISPATCH_DTYPE(dt, T, {
    constexpr int P = Elem<T>::PER16;
    long total = rx_act_voxels(y) * (y->c / P);
    int G = (int)((total + 255) / 256 > 4096 ? 4096 : (total + 255) / 256);
    hipLaunchKernelGGL((avgpool_fwd_kernel<T>), dim3(G, x->n), dim3(256), 0, st, (const T*)x->ptr, x->ld, rx_act_voxels(x) * x->ld,
                       (T*)y->ptr, y->ld, rx_act_voxels(y) * y->ld, y->z, y->y, y->x, x->y, x->x, x->c, stride[0], stride[1], stride[2]);
  });
  RX_CHECK_LAUNCH("rx_avgpool_fwd");
  return RX_OK;
}

// ---- block epilogue + the AvgPool of the next block's skip path in ONE pass -----------------------------------------------
// out = lrelu((y-mean)*rstd + res) and pooled = avgpool(out): a thread owns one POOLED voxel's channel vector, produces the
// fz*fy*fx outputs under it and averages them as stored (same values, same summation order as avgpool_fwd_kernel reading
// `out` back -- which moves the whole tensor through HBM a second time).
template <typename T, bool HAS_RES>
__global__ __launch_bounds__(256) void in_act_pool_fwd_kernel(const T* __restrict__ y, int ldy, long sy, const float* __restrict__ stats,
                                                              const T* __restrict__ res, int ldr, long sr, T* __restrict__ out, int ldo, long so,
                                                              T* __restrict__ pooled, int ldp, long sp, int Zo, int Yo, int Xo, int Yi, int Xi,
                                                              int C, int fz, int fy, int fx, float slope) {
  constexpr int P = Elem<T>::PER16;
  Sweep<P> s((long)Zo * Yo * Xo, C);
  const int n = s.n, c0 = s.cv * P;
  float mean[P], rstd[P];
  load_pair(stats, n, C, c0, mean, rstd);
  const float inv = 1.f / (float)(fz * fy * fx);
  for (; s.more(); s.next()) {
    const long vo = s.v();
    const int xo = (int)(vo % Xo), yo = (int)((vo / Xo) % Yo), zo = (int)(vo / ((long)Xo * Yo));
    float acc[P];
#pragma unroll
    for (int j = 0; j < P; ++j) acc[j] = 0.f;
    for (int a = 0; a < fz; ++a)
      for (int b = 0; b < fy; ++b)
        for (int c = 0; c < fx; ++c) {
          const long vi = ((long)(zo * fz + a) * Yi + (yo * fy + b)) * Xi + (xo * fx + c);
          Vec16<T> t = ld16(y + n * sy + vi * ldy + c0), r, o;
          if (HAS_RES) r = ld16(res + n * sr + vi * ldr + c0);
#pragma unroll
          for (int j = 0; j < P; ++j) {
            o.v[j] = in_fwd_elem<T, HAS_RES>(t.v[j], mean[j], rstd[j], r.v[j], slope);
            acc[j] += Elem<T>::to_f(o.v[j]);      // averaged AS STORED
          }
          st16(out + n * so + vi * ldo + c0, o);
        }
    Vec16<T> p;
#pragma unroll
    for (int j = 0; j < P; ++j) p.v[j] = Elem<T>::from_f(acc[j] * inv);
    st16(pooled + n * sp + vo * ldp + c0, p);
  }
}

extern "C" int rx_instnorm_act_pool_fwd(rx_dtype dt, const rx_act* y, const float* stats, const rx_act* residual, const rx_act* out,
                                        const rx_act* pooled, const int32_t stride[3], float slope, void* stream) {
  RX_RECORD(stream, [=, y_ = RxActV(y), residual_ = RxActV(residual), out_ = RxActV(out), pooled_ = RxActV(pooled), stride_ = RxI3V(stride)](void* s) { return rx_instnorm_act_pool_fwd(dt, y_.p(), stats, residual_.p(), out_.p(), pooled_.p(), stride_.v, slope, s); });
  int rc = check_acts(dt, "rx_instnorm_act_pool_fwd", y, {{"y", y, true}, {"out", out, true}, {"residual", residual, false}});
  if (rc) return rc;
  if ((rc = check_vec_channels(pooled, dt, "rx_instnorm_act_pool_fwd(pooled)"))) return rc;
  if (!stats) RX_FAIL(RX_EINVAL, "rx_instnorm_act_pool_fwd: null stats");
  if ((rc = check_pool(out, pooled, stride, "rx_instnorm_act_pool_fwd"))) return rc;
  const long V = rx_act_voxels(y), Vp = rx_act_voxels(pooled);
  hipStream_t st = (hipStream_t)stream;
  RX_DISPATCH_DTYPE(dt, T, {
    const int CV = y->c / Elem<T>::PER16;
    const int G = sweep_grid(Vp * CV * 4, CV);      // a thread produces up to 8 outputs: 4x the blocks of a plain sweep of Vp
    const ActView<T> r = make_view<T>(residual);
    hipLaunchKernelGGL((residual ? in_act_pool_fwd_kernel<T, true> : in_act_pool_fwd_kernel<T, false>), dim3(G, y->n), dim3(256), 0, st,
                       (const T*)y->ptr, y->ld, V * y->ld, stats, r.ptr, r.ld, r.sample_stride, (T*)out->ptr, out->ld, V * out->ld,
                       (T*)pooled->ptr, pooled->ld, Vp * pooled->ld, pooled->z, pooled->y, pooled->x, y->y, y->x, y->c, stride[0], stride[1],
                       stride[2], slope);
  });
  RX_CHECK_LAUNCH("rx_instnorm_act_pool_fwd");
  return RX_OK;
}

extern "C" int rx_avgpool_bwd(rx_dtype dt, const rx_act* dy, const rx_act* dx, const int32_t stride[3], int accumulate,
                              void* stream) {
  RX_RECORD(stream, [=, dy_ = RxActV(dy), dx_ = RxActV(dx), stride_ = RxI3V(stride)](void* s) { return rx_avgpool_bwd(dt, dy_.p(), dx_.p(), stride_.v, accumulate, s); });
  int rc;
  if ((rc = check_vec_channels(dx, dt, "rx_avgpool_bwd(dx)"))) return rc;
  if ((rc = check_vec_channels(dy, dt, "rx_avgpool_bwd(dy)"))) return rc;
  if ((rc = check_pool(dx, dy, stride, "rx_avgpool_bwd"))) return rc;
  hipStream_t st = (hipStream_t)stream;
  RX_DISPATCH_DTYPE(dt, T, {
    constexpr int P = Elem<T>::PER16;
    long total = rx_act_voxels(dx) * (dx->c / P);
    int G = (int)((total + 255) / 256 > 4096 ? 4096 : (total + 255) / 256);
    if (accumulate)
      hipLaunchKernelGGL((avgpool_bwd_kernel<T, true>), dim3(G, dx->n), dim3(256), 0, st, (const T*)dy->ptr, dy->ld,
                         rx_act_voxels(dy) * dy->ld, (T*)dx->ptr, dx->ld, rx_act_voxels(dx) * dx->ld, dx->z, dx->y, dx->x, dy->y,
                         dy->x, dx->c, stride[0], stride[1], stride[2]);
    else
      hipLaunchKernelGGL((avgpool_bwd_kernel<T, false>), dim3(G, dx->n), dim3(256), 0, st, (const T*)dy->ptr, dy->ld,
                         rx_act_voxels(dy) * dy->ld, (T*)dx->ptr, dx->ld, rx_act_voxels(dx) * dx->ld, dx->z, dx->y, dx->x, dy->y,
                         dy->x, dx->c, stride[0], stride[1], stride[2]);
  });
  RX_CHECK_LAUNCH("rx_avgpool_bwd");
  return RX_OK;
}
