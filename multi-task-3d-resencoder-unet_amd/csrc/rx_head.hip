// rx_head.hip -- the 1x1x1 task head (forward with the eval-mode activations, backward) and the two InstanceNorm kernels of
// the layer under a head that carry the head's work along: rx_instnorm_act_head_fwd and rx_instnorm_act_bwd_head.
#include <math.h>

#include "rx_common.h"
#include "rx_internal.h"
#include "rx_reduce.h"
#include "rx_instnorm_core.h"

// ---- task head: 1x1x1 conv with bias (forward: accumulator arrays sized 8 / 16 / 32 / 64, K <= 8 keeps the lean kernel, more
// than 64 classes run in chunks of 64 with the eval-mode softmax as a separate pass over the logits; backward: weight / bias
// gradients in chunks of <= 16 output channels, the data gradient over all K in chunk 0).  decoder.py:131 puts no bound on
// num_classes (whole-body label sets have 100+); RX_HEAD_MAXK only bounds the LDS-resident weight table of the backward. ---
#define RX_HEAD_MAXK 1024
template <typename T, int MAXK>
__global__ __launch_bounds__(256) void head_fwd_kernel(const T* __restrict__ x, int ldx, long sx, const float* __restrict__ w,
                                                       const float* __restrict__ b, int K, int k0, int Kt, float* __restrict__ out, int V,
                                                       int C, int act) {
  constexpr int P = Elem<T>::PER16;
  extern __shared__ __attribute__((aligned(16))) float sw[];  // [K][C]: output channels [k0, k0 + K) of a head with Kt of them
  w += (size_t)k0 * C;
  b += k0;
  for (int i = threadIdx.x; i < K * C; i += 256) sw[i] = w[i];
  __syncthreads();
  const int n = blockIdx.y;
  const int CV = C / P;
  for (long v = (long)blockIdx.x * 256 + threadIdx.x; v < V; v += (long)gridDim.x * 256) {
    float acc[MAXK];
#pragma unroll
    for (int k = 0; k < MAXK; ++k) acc[k] = k < K ? b[k] : 0.f;
    const T* xp = x + n * sx + v * ldx;
    for (int cv = 0; cv < CV; ++cv) {
      Vec16<T> t = ld16(xp + cv * P);
#pragma unroll
      for (int k = 0; k < MAXK; ++k)
        if (k < K) {
#pragma unroll
          for (int j = 0; j < P; ++j) acc[k] += Elem<T>::to_f(t.v[j]) * sw[k * C + cv * P + j];
        }
    }
    if (act == RX_ACT_SIGMOID) {
#pragma unroll
      for (int k = 0; k < MAXK; ++k) acc[k] = 1.f / (1.f + expf(-acc[k]));
    } else if (act == RX_ACT_SOFTMAX) {
      float m = -INFINITY, s = 0.f;
#pragma unroll
      for (int k = 0; k < MAXK; ++k)
        if (k < K) m = fmaxf(m, acc[k]);
#pragma unroll
      for (int k = 0; k < MAXK; ++k)
        if (k < K) {
          acc[k] = expf(acc[k] - m);
          s += acc[k];
        }
#pragma unroll
      for (int k = 0; k < MAXK; ++k) acc[k] = acc[k] / s;
    }
#pragma unroll
    for (int k = 0; k < MAXK; ++k)
      if (k < K) out[((size_t)n * Kt + k0 + k) * V + v] = acc[k];
  }
}

// softmax over the channel axis of (N, K, V) fp32 logits, in place (heads with more than 64 classes in eval mode)
__global__ __launch_bounds__(256) void softmax_ncdhw_kernel(float* __restrict__ out, int K, long V) {
  const int n = blockIdx.y;
  float* o = out + (size_t)n * K * V;
  for (long v = (long)blockIdx.x * 256 + threadIdx.x; v < V; v += (long)gridDim.x * 256) {
    float m = -INFINITY, s = 0.f;
    for (int k = 0; k < K; ++k) m = fmaxf(m, o[(size_t)k * V + v]);
    for (int k = 0; k < K; ++k) s += expf(o[(size_t)k * V + v] - m);
    const float inv = 1.f / s;
    for (int k = 0; k < K; ++k) o[(size_t)k * V + v] = expf(o[(size_t)k * V + v] - m) * inv;
  }
}

extern "C" int rx_head_fwd(rx_dtype dt, const rx_act* x, const float* w, const float* b, int k, float* out_ncdhw, int act,
                           void* stream) {
  RX_RECORD(stream, [=, x_ = RxActV(x)](void* s) { return rx_head_fwd(dt, x_.p(), w, b, k, out_ncdhw, act, s); });
  int rc;
  if ((rc = check_vec_channels(x, dt, "rx_head_fwd"))) return rc;
  if (!w || !b || !out_ncdhw) RX_FAIL(RX_EINVAL, "rx_head_fwd: null pointer");
  if (k < 1 || k > RX_HEAD_MAXK) RX_FAIL(RX_EUNSUPPORTED, "rx_head_fwd: 1 <= K <= %d (got %d)", RX_HEAD_MAXK, k);
  const long V = rx_act_voxels(x);
  hipStream_t st = (hipStream_t)stream;
  RX_DISPATCH_DTYPE(dt, T, {
    int G = (int)((V + 255) / 256 > 4096 ? 4096 : (V + 255) / 256);
    const int act_here = (k > 64 && act == RX_ACT_SOFTMAX) ? (int)RX_ACT_NONE : act;      // softmax needs every class: second pass
    for (int k0 = 0; k0 < k; k0 += 64) {
      const int kc = k - k0 < 64 ? k - k0 : 64;
      auto kern = kc <= 8 ? head_fwd_kernel<T, 8> : kc <= 16 ? head_fwd_kernel<T, 16> : kc <= 32 ? head_fwd_kernel<T, 32> : head_fwd_kernel<T, 64>;
      hipLaunchKernelGGL(kern, dim3(G, x->n), dim3(256), (size_t)kc * x->c * sizeof(float), st, (const T*)x->ptr, x->ld, V * x->ld, w, b, kc, k0, k,
                         out_ncdhw, (int)V, x->c, act_here);
    }
    if (k > 64 && act == RX_ACT_SOFTMAX) hipLaunchKernelGGL(softmax_ncdhw_kernel, dim3(G, x->n), dim3(256), 0, st, out_ncdhw, k, V);
  });
  RX_CHECK_LAUNCH("rx_head_fwd");
  return RX_OK;
}

// backward: dx[v][c] = sum_k dout[k][v] w[k][c]; dw[k][c] = sum_v dout[k][v] x[v][c]; db[k] = sum_v dout[k][v]
// One launch handles the output channels [k0, k0 + K) of a head with Kt of them: dw / db of that range; dx (over ALL Kt channels,
// a run-time loop: it needs no per-channel registers) when dx != nullptr -- the caller passes it with the first chunk only.
template <typename T, int MAXK>
__global__ __launch_bounds__(256) void head_bwd_kernel(const float* __restrict__ dout, const T* __restrict__ x, int ldx, long sx,
                                                       const float* __restrict__ w, int K, int k0, int Kt, T* __restrict__ dx, int lddx,
                                                       long sdx, int V, int C, int chunk_vox,
                                                       float* __restrict__ partial /*[N][nch][K+1][C]*/) {
  constexpr int P = Elem<T>::PER16;
  extern __shared__ __attribute__((aligned(16))) float sm[];  // sw[Kt][C] then red[(K+1)][VP][C]
  float* sw = sm;
  const int CV = C / P;
  const int VP = 256 / CV > 0 ? 256 / CV : 1;
  float* red = sm + Kt * C;
  for (int i = threadIdx.x; i < Kt * C; i += 256) sw[i] = w[i];
  __syncthreads();
  const int tid = threadIdx.x, n = blockIdx.y, chunk = blockIdx.x;
  const int vl = tid / CV, cv = tid - vl * CV;
  float aw[MAXK][P];
  float ab[MAXK];
#pragma unroll
  for (int k = 0; k < MAXK; ++k) {
    ab[k] = 0.f;
#pragma unroll
    for (int j = 0; j < P; ++j) aw[k][j] = 0.f;
  }
  const int v_begin = chunk * chunk_vox, v_end = min(V, v_begin + chunk_vox);
  if (vl < VP) {
    for (int v = v_begin + vl; v < v_end; v += VP) {
      Vec16<T> xv = ld16(x + n * sx + (long)v * ldx + cv * P);
      float d[P];
#pragma unroll
      for (int j = 0; j < P; ++j) d[j] = 0.f;
#pragma unroll
      for (int k = 0; k < MAXK; ++k)
        if (k < K) {
          float gk = dout[((size_t)n * Kt + k0 + k) * V + v];
          ab[k] += gk;
#pragma unroll
          for (int j = 0; j < P; ++j) {
            aw[k][j] += gk * Elem<T>::to_f(xv.v[j]);
            if (Kt == K) d[j] += gk * sw[k * C + cv * P + j];
          }
        }
      if (dx && Kt != K) {      // more channels than this launch's chunk: the data gradient sums over all of them (k ascending)
        for (int k = 0; k < Kt; ++k) {
          const float gk = dout[((size_t)n * Kt + k) * V + v];
#pragma unroll
          for (int j = 0; j < P; ++j) d[j] += gk * sw[k * C + cv * P + j];
        }
      }
      if (dx) {
        Vec16<T> o;
#pragma unroll
        for (int j = 0; j < P; ++j) o.v[j] = Elem<T>::from_f(d[j]);
        st16(dx + n * sdx + (long)v * lddx + cv * P, o);
      }
    }
    for (int k = 0; k < K; ++k)
#pragma unroll
      for (int j = 0; j < P; ++j) red[(k * VP + vl) * C + cv * P + j] = aw[k][j];
    // bias plane: only column cv==0 carries the sum, stored at channel 0 of plane K
    if (cv == 0)
      for (int k = 0; k < K; ++k) red[(K * VP + vl) * C + k] = ab[k];
  }
  __syncthreads();
  float* pout = partial + (size_t)(n * gridDim.x + chunk) * (K + 1) * C;
  for (int i = tid; i < (K + 1) * C; i += 256) {
    int a = i / C, c = i - a * C;
    if (a == K && c >= K) {
      pout[i] = 0.f;
      continue;
    }
    float s = 0.f;
    for (int r = 0; r < VP; ++r) s += red[(a * VP + r) * C + c];
    pout[i] = s;
  }
}

extern "C" size_t rx_head_bwd_workspace(const rx_act* x, int k) {
  if (!rx_act_ok(x)) return 0;
  return rx_reduce_ws_bytes(x->n, rx_act_voxels(x), x->c, k + 1) + (size_t)(k + 1) * x->c * sizeof(float) + 256;
}

extern "C" int rx_head_bwd(rx_dtype dt, const float* dout_ncdhw, const rx_act* x, const float* w, int k, const rx_act* dx, float* dw,
                           float* db, void* ws, size_t ws_bytes, void* stream) {
  RX_RECORD(stream, [=, x_ = RxActV(x), dx_ = RxActV(dx)](void* s) { return rx_head_bwd(dt, dout_ncdhw, x_.p(), w, k, dx_.p(), dw, db, ws, ws_bytes, s); });
  int rc;
  if ((rc = check_vec_channels(x, dt, "rx_head_bwd(x)"))) return rc;
  if (dx) {
    if ((rc = check_vec_channels(dx, dt, "rx_head_bwd(dx)"))) return rc;
    if (!same_geom(x, dx)) RX_FAIL(RX_EINVAL, "rx_head_bwd: dx geometry mismatch");
  }
  if (!dout_ncdhw || !w || !dw || !db || !ws) RX_FAIL(RX_EINVAL, "rx_head_bwd: null pointer");
  if (k < 1 || k > RX_HEAD_MAXK || (k <= 16 && k > x->c) || x->c < 16) RX_FAIL(RX_EUNSUPPORTED, "rx_head_bwd: 1 <= K <= %d", RX_HEAD_MAXK);
  const long V = rx_act_voxels(x);
  const int N = x->n, C = x->c;
  hipStream_t st = (hipStream_t)stream;
  RX_DISPATCH_DTYPE(dt, T, {
    constexpr int P = Elem<T>::PER16;
    ReducePlan p = rx_reduce_plan(V, C, P);
    int kc_max = k <= 16 ? k : 16;                 // output channels per launch
    {   // many classes: the LDS-resident weight table grows with K -- halve the chunk until table + reduction planes fit
      const int VP0 = 256 / (C / P);
      while (kc_max > 4 && ((size_t)k * C + (size_t)(kc_max + 1) * VP0 * C) * sizeof(float) > 150 * 1024) kc_max /= 2;
    }
    size_t need = (size_t)N * p.nchunks * (kc_max + 1) * C * sizeof(float) + (size_t)(kc_max + 1) * C * sizeof(float) + 256;
    if (ws_bytes < need) RX_FAIL(RX_EWORKSPACE, "rx_head_bwd: workspace too small (%zu < %zu)", ws_bytes, need);
    int CV = C / P, VP = 256 / CV;
    float* partial = (float*)ws;
    float* fin = partial + (size_t)N * p.nchunks * (kc_max + 1) * C;
    size_t lds = ((size_t)k * C + (size_t)(kc_max + 1) * VP * C) * sizeof(float);
    if (lds > 160 * 1024) RX_FAIL(RX_EUNSUPPORTED, "rx_head_bwd: K = %d needs %zu bytes of LDS", k, lds);
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&head_bwd_kernel<T, 8>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&head_bwd_kernel<T, 16>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    for (int k0 = 0; k0 < k; k0 += kc_max) {
      const int kc = k - k0 < kc_max ? k - k0 : kc_max;
      T* dxp = (dx && k0 == 0) ? (T*)dx->ptr : (T*)nullptr;
      if (kc <= 8) {
        hipLaunchKernelGGL((head_bwd_kernel<T, 8>), dim3(p.nchunks, N), dim3(256), lds, st, dout_ncdhw, (const T*)x->ptr, x->ld, V * x->ld, w, kc,
                           k0, k, dxp, dx ? dx->ld : 0, dx ? V * dx->ld : 0L, (int)V, C, p.chunk_vox, partial);
      } else {
        hipLaunchKernelGGL((head_bwd_kernel<T, 16>), dim3(p.nchunks, N), dim3(256), lds, st, dout_ncdhw, (const T*)x->ptr, x->ld, V * x->ld, w, kc,
                           k0, k, dxp, dx ? dx->ld : 0, dx ? V * dx->ld : 0L, (int)V, C, p.chunk_vox, partial);
      }
      rx_colreduce_finalize_launch(st, (const float*)partial, N, p.nchunks, kc + 1,
                         C, (double)V, 0.f, (int)FIN_SUM_OVER_N, fin);
      (void)hipMemcpyAsync(dw + (size_t)k0 * C, fin, (size_t)kc * C * sizeof(float), hipMemcpyDeviceToDevice, st);
      (void)hipMemcpyAsync(db + k0, fin + (size_t)kc * C, (size_t)kc * sizeof(float), hipMemcpyDeviceToDevice, st);
    }
  });
  RX_CHECK_LAUNCH("rx_head_bwd");
  return RX_OK;
}

#define RX_HEADG_MAXK 4
// the head's weights for a thread's channel vector: w[k][j] = hw[k][c0 + j], 0 past K
template <int P>
__device__ inline void load_head_w(const float* hw, int K, int C, int c0, float (&w)[RX_HEADG_MAXK][P]) {
#pragma unroll
  for (int j = 0; j < P; ++j)
#pragma unroll
    for (int k = 0; k < RX_HEADG_MAXK; ++k) w[k][j] = k < K ? hw[k * C + c0 + j] : 0.f;
}
// ---- InstanceNorm + LeakyReLU of the layer under a task head, with the head's 1x1x1 conv in the same pass -----------
// rx_head_fwd re-read the activated output (268 MB at cfg2) to form K logits per voxel.  Here the CV lanes that hold one voxel's
// channel vectors pass the running sums along (lane cv adds the partial dot product of its 8 channels to what lane cv-1 holds, from
// the rounded output values; logits agree with head_fwd_kernel's sequential sum to fp32 round-off); the last lane
// applies the eval-mode activation and writes the NCDHW fp32 logits.  K <= 4, no residual (decoder.py:115-131).
template <typename T>
__global__ __launch_bounds__(256) void in_act_head_fwd_kernel(const T* __restrict__ y, int ldy, long sy, const float* __restrict__ stats,
                                                              T* __restrict__ out, int ldo, long so, int V, int C, float slope,
                                                              const float* __restrict__ hw, const float* __restrict__ hb, int K,
                                                              float* __restrict__ logits, int act) {
  constexpr int P = Elem<T>::PER16;
  Sweep<P> sw(V, C);
  const int CV = sw.CV, n = sw.n, cv = sw.cv;
  float mean[P], rstd[P], w[RX_HEADG_MAXK][P], b[RX_HEADG_MAXK];
  load_pair(stats, n, C, cv * P, mean, rstd);
  load_head_w(hw, K, C, cv * P, w);
#pragma unroll
  for (int k = 0; k < RX_HEADG_MAXK; ++k) b[k] = k < K ? hb[k] : 0.f;
  const T* yn = y + n * sy;
  T* on = out ? out + n * so : nullptr;
  for (; sw.more(); sw.next()) {
    const long v = sw.v();
    Vec16<T> a = ld16(yn + v * ldy + cv * P);
    Vec16<T> o;
    float of[P];
#pragma unroll
    for (int j = 0; j < P; ++j) {
      o.v[j] = in_fwd_elem<T, false>(a.v[j], mean[j], rstd[j], a.v[j], slope);
      of[j] = Elem<T>::to_f(o.v[j]);      // logits from the output AS STORED
    }
    if (on) st16(on + v * ldo + cv * P, o);      // (out == NULL: nobody reads the activated output -- see rx_instnorm_act_bwd_head's dw / db)
    // The CV lanes of a voxel each form the partial dot products of THEIR 8 channels, then hand a running sum along in channel
    // order (lane cv adds its partial to what lane cv-1 holds).  No divergent region between the cross-lane moves: every lane
    // computes, a select keeps the owner's value.  (The first version did the adds inside `if (cv == s)`; with a SECOND process
    // time-slicing the GPU -- two DDP ranks rehearsed on one device -- a few logits per pass then came out different while every
    // other tensor of the pass stayed bit-identical, with ds_bpermute and with DPP moves alike; 0 of 120 passes with this form,
    // scripts/fwd_layer_diag.py.  Never observed with one process per GPU.)
    float part[RX_HEADG_MAXK], acc[RX_HEADG_MAXK];
#pragma unroll
    for (int k = 0; k < RX_HEADG_MAXK; ++k) {
      part[k] = 0.f, acc[k] = b[k];
      if (k < K) {
#pragma unroll
        for (int j = 0; j < P; ++j) part[k] += of[j] * w[k][j];
      }
    }
    for (int s = 0; s < CV; ++s) {
#pragma unroll
      for (int k = 0; k < RX_HEADG_MAXK; ++k)
        if (k < K) {                     // K is uniform: a scalar branch
          const float prev = __shfl_up(acc[k], 1, 64);
          const float t = (s == 0 ? b[k] : prev) + part[k];
          acc[k] = cv == s ? t : acc[k];
        }
    }
    if (cv == CV - 1) {
      if (act == RX_ACT_SIGMOID) {
#pragma unroll
        for (int k = 0; k < RX_HEADG_MAXK; ++k) acc[k] = 1.f / (1.f + expf(-acc[k]));
      } else if (act == RX_ACT_SOFTMAX) {
        float m = -INFINITY, sum = 0.f;
#pragma unroll
        for (int k = 0; k < RX_HEADG_MAXK; ++k)
          if (k < K) m = fmaxf(m, acc[k]);
#pragma unroll
        for (int k = 0; k < RX_HEADG_MAXK; ++k)
          if (k < K) {
            acc[k] = expf(acc[k] - m);
            sum += acc[k];
          }
#pragma unroll
        for (int k = 0; k < RX_HEADG_MAXK; ++k) acc[k] = acc[k] / sum;
      }
#pragma unroll
      for (int k = 0; k < RX_HEADG_MAXK; ++k)
        if (k < K) logits[((size_t)n * K + k) * V + v] = acc[k];
    }
  }
}

// out = lrelu((y - mean) * rstd) AND out_ncdhw = head(out) (+ eval-mode activation) in one pass; `stats` = (mean, rstd) of y.
// Same `out` bit for bit and the same logits to fp32 round-off as rx_instnorm_act_fwd followed by rx_head_fwd.  K <= 4, 64 % (C / 8) == 0.
extern "C" int rx_instnorm_act_head_fwd(rx_dtype dt, const rx_act* y, const float* stats, const rx_act* out, float slope,
                                        const float* head_w, const float* head_b, int k, float* out_ncdhw, int act, void* stream) {
  RX_RECORD(stream, [=, y_ = RxActV(y), out_ = RxActV(out)](void* s) { return rx_instnorm_act_head_fwd(dt, y_.p(), stats, out_.p(), slope, head_w, head_b, k, out_ncdhw, act, s); });
  int rc = check_vec_channels(y, dt, "rx_instnorm_act_head_fwd(y)");
  if (rc) return rc;
  if (out && (rc = check_vec_channels(out, dt, "rx_instnorm_act_head_fwd(out)"))) return rc;
  if (!stats || !head_w || !head_b || !out_ncdhw || (out && !same_geom(y, out))) RX_FAIL(RX_EINVAL, "rx_instnorm_act_head_fwd: bad arguments");
  if (dt == RX_F32 || k < 1 || k > RX_HEADG_MAXK || 64 % (y->c / 8) != 0)
    RX_FAIL(RX_EUNSUPPORTED, "rx_instnorm_act_head_fwd: 16-bit types, K <= %d, C / 8 dividing 64", RX_HEADG_MAXK);
  const long V = rx_act_voxels(y);
  hipStream_t st = (hipStream_t)stream;
  RX_DISPATCH_DTYPE(dt, T, {
    const int CV = y->c / Elem<T>::PER16, G = sweep_grid(V * CV, CV);
    const ActView<T> o = make_view<T>(out);
    hipLaunchKernelGGL((in_act_head_fwd_kernel<T>), dim3(G, y->n), dim3(256), 0, st, (const T*)y->ptr, y->ld, V * y->ld, stats, (T*)o.ptr, o.ld,
                       o.sample_stride, (int)V, y->c, slope, head_w, head_b, k, out_ncdhw, act);
  });
  RX_CHECK_LAUNCH("rx_instnorm_act_head_fwd");
  return RX_OK;
}

// ---- InstanceNorm backward of the layer that feeds a task head, with the head's data gradient formed on the fly ------
// The gradient that reaches the last decoder conv block is rank K: g[v][c] = sum_k dlogit[k][v] * w_head[k][c] (K = 1 for a
// segmentation head, 3 for normals).  rx_head_bwd used to write it as a full (N, V, C) tensor (268 MB at cfg2) that the two
// passes of the InstanceNorm backward then read back twice.  Here both passes rebuild g from the fp32 logit gradient (4*K bytes
// per voxel instead of 2*C) and the head's weights; rx_head_bwd is called with dx = NULL and only reduces dw / db.  g is
// rounded to the storage type exactly where rx_head_bwd rounded it, so dy is bit-identical to the three-tensor path.
// KW > 0 (round 3): the same pass also reduces the HEAD's parameter gradients, dw[k][c] = sum_v dout[k][v] * a[v][c] and db[k] =
// sum_v dout[k][v], with a = lrelu(xhat) recomputed from y and rounded to the storage type as the forward stored it -- the
// activated output of the layer under a head (268 MB at cfg2) is then neither written by the forward nor read by rx_head_bwd
// (a 131 us launch at cfg2), which is not called at all.  Accumulators 2 .. 2+K-1 hold dw, accumulator 2+K holds db[k] in lane k
// (only the threads of channel vector 0 add to it: every channel vector of a voxel sees the same dout).
template <typename T, int KW = 0>
struct InBwdHeadOp {
  ActView<T> y;
  const float* stats;
  const float* dout;  // (N, K, V) fp32
  const float* hw;    // (K, C)
  int C, K, V;
  float slope;
  InMask mask;   // IN_MASK_XHAT or IN_MASK_NONE: the layer under a head has no residual
  float mean[Elem<T>::PER16], rstd[Elem<T>::PER16], w[RX_HEADG_MAXK][Elem<T>::PER16];
  __device__ inline void prepare(int n, int c0) {
    load_pair(stats, n, C, c0, mean, rstd);
    load_head_w(hw, K, C, c0, w);
  }
  __device__ inline void accumulate(int n, int v, int c0, float (&acc)[KW ? KW + 3 : 2][Elem<T>::PER16]) const {
    constexpr int P = Elem<T>::PER16;
    Vec16<T> yv = ld16(y.at(n, v, c0));
    float d[P], gk[RX_HEADG_MAXK];
    head_grad_vec(dout, n, K, V, v, w, d, gk);
#pragma unroll
    for (int j = 0; j < P; ++j) {
      const float xh = in_xhat(yv.v[j], mean[j], rstd[j]);
      float gg = Elem<T>::to_f(Elem<T>::from_f(d[j]));      // g rounded to T BEFORE the mask
      in_bwd_gprime(gg, xh, mask, slope);
      acc[0][j] += gg;
      acc[1][j] += gg * xh;
      if (KW) {
        const float a = Elem<T>::to_f(Elem<T>::from_f(xh > 0.f ? xh : xh * slope));      // what rx_instnorm_act_head_fwd stored
#pragma unroll
        for (int k = 0; k < KW; ++k) acc[2 + k][j] += gk[k] * a;
      }
    }
    if (KW && c0 == 0) {
#pragma unroll
      for (int k = 0; k < KW; ++k) acc[2 + KW][k] += gk[k];
    }
  }
};

// finalize of the pass above: m12[n][c] (both means), dw[k][c] and db[k] (sums over n and chunks), one workgroup per output
__global__ __launch_bounds__(256) void inbwd_head_finalize(const float* __restrict__ partial, int N, int nchunks, int nacc, int C, int K, double V,
                                                           float* __restrict__ m12, float* __restrict__ dw, float* __restrict__ db) {
  const int i = blockIdx.x;
  double s0 = 0.0, s1 = 0.0;
  if (i < N * C) {
    const int n = i / C, c = i - n * C;
    fin_gather(partial + ((size_t)n * nchunks * nacc) * C + c, (size_t)nacc * C, nchunks, C, s0, s1);
    if (threadIdx.x == 0) m12[2 * i] = (float)(s0 / V), m12[2 * i + 1] = (float)(s1 / V);
    return;
  }
  const int j = i - N * C;
  if (j < K * C) {
    const int k = j / C, c = j - k * C;
    fin_gather(partial + (size_t)(2 + k) * C + c, (size_t)nacc * C, N * nchunks, 0, s0, s1);
    if (threadIdx.x == 0) dw[j] = (float)s0;
    return;
  }
  const int k = j - K * C;
  fin_gather(partial + (size_t)(2 + K) * C + k, (size_t)nacc * C, N * nchunks, 0, s0, s1);
  if (threadIdx.x == 0) db[k] = (float)s0;
}

template <typename T>
__global__ __launch_bounds__(256) void in_act_bwd_apply_head_kernel(const float* __restrict__ dout, int K, const float* __restrict__ hw,
                                                                    const T* __restrict__ y, int ldy, long sy,
                                                                    const float* __restrict__ stats, const float* __restrict__ m12,
                                                                    T* __restrict__ dy, int lddy, long sdy, int V, int C, float slope,
                                                                    InMask mask) {
  constexpr int P = Elem<T>::PER16;
  Sweep<P> s(V, C);
  const int n = s.n, c0 = s.cv * P;
  float mean[P], rstd[P], m1[P], m2[P], w[RX_HEADG_MAXK][P];
  load_pair(stats, n, C, c0, mean, rstd);
  load_pair(m12, n, C, c0, m1, m2);
  load_head_w(hw, K, C, c0, w);
  for (; s.more(); s.next()) {
    const long v = s.v();
    Vec16<T> yv = ld16(y + n * sy + v * ldy + c0);
    float d[P], gk[RX_HEADG_MAXK];
    head_grad_vec(dout, n, K, V, v, w, d, gk);
    Vec16<T> dv;
#pragma unroll
    for (int j = 0; j < P; ++j) {
      const float xh = in_xhat(yv.v[j], mean[j], rstd[j]);
      float gg = Elem<T>::to_f(Elem<T>::from_f(d[j]));
      in_bwd_gprime(gg, xh, mask, slope);
      dv.v[j] = Elem<T>::from_f(in_bwd_dy(gg, xh, rstd[j], m1[j], m2[j]));
    }
    st16(dy + n * sdy + v * lddy + c0, dv);
  }
}

// dy = InstanceNorm+LeakyReLU backward of a layer WITHOUT residual whose output gradient is the data gradient of a 1x1x1 head:
// g = dout (N,K,Z,Y,X fp32) x head_w (K,C), never materialised.  Same result as rx_head_bwd(dx = g) + rx_instnorm_act_bwd(g, ...,
// out = NULL).  K <= 4.
template <typename T, int KW>
static ReducePlan launch_head_reduce(const rx_act* y, const float* stats, const float* dout, const float* hw, int k, float slope, InMask mask,
                                     float* partial, hipStream_t st) {
  const long V = rx_act_voxels(y);
  InBwdHeadOp<T, KW> op{make_view<T>(y), stats, dout, hw, y->c, k, (int)V, slope, mask, {}, {}, {}};
  return launch_colreduce<T, (KW ? KW + 3 : 2)>(op, y->n, V, y->c, partial, st);
}
extern "C" int rx_instnorm_act_bwd_head(rx_dtype dt, const float* dout_ncdhw, int k, const float* head_w, const rx_act* y,
                                        const float* stats, float slope, const rx_act* dy, float* head_dw, float* head_db, void* ws,
                                        size_t ws_bytes, void* stream) {
  RX_RECORD(stream, [=, y_ = RxActV(y), dy_ = RxActV(dy)](void* s) { return rx_instnorm_act_bwd_head(dt, dout_ncdhw, k, head_w, y_.p(), stats, slope, dy_.p(), head_dw, head_db, ws, ws_bytes, s); });
  int rc = check_acts(dt, "rx_instnorm_act_bwd_head", y, {{"y", y, true}, {"dy", dy, true}});
  if (rc) return rc;
  if (!dout_ncdhw || !head_w || !stats || !ws || k < 1 || k > RX_HEADG_MAXK)
    RX_FAIL(RX_EINVAL, "rx_instnorm_act_bwd_head: bad arguments (K must be 1..%d)", RX_HEADG_MAXK);
  const long V = rx_act_voxels(y);
  const int N = y->n, C = y->c;
  if (V > 0x7fffffffL) RX_FAIL(RX_EUNSUPPORTED, "rx_instnorm_act_bwd_head: volume too large");
  if ((head_dw == nullptr) != (head_db == nullptr)) RX_FAIL(RX_EINVAL, "rx_instnorm_act_bwd_head: head_dw and head_db come together");
  const int nacc = head_dw ? k + 3 : 2;
  const ReduceWs w = reduce_ws(ws, N, V, C, nacc);
  if (ws_bytes < w.need) RX_FAIL(RX_EWORKSPACE, "rx_instnorm_act_bwd_head: workspace too small (%zu < %zu)", ws_bytes, w.need);
  hipStream_t st = (hipStream_t)stream;
  const InMask mask = in_mask_of(slope, nullptr);
  RX_DISPATCH_DTYPE(dt, T, {
    auto reduce = !head_dw ? launch_head_reduce<T, 0>
                  : k == 1 ? launch_head_reduce<T, 1>
                  : k == 2 ? launch_head_reduce<T, 2>
                  : k == 3 ? launch_head_reduce<T, 3>
                           : launch_head_reduce<T, 4>;
    const ReducePlan p = reduce(y, stats, dout_ncdhw, head_w, k, slope, mask, w.partial, st);
    if (!head_dw)
      rx_colreduce_finalize_launch(st, w.partial, N, p.nchunks, 2, C, (double)V, 0.f, (int)FIN_MEAN2, w.m12);
    else
      hipLaunchKernelGGL(inbwd_head_finalize, dim3(N * C + k * C + k), dim3(256), 0, st, (const float*)w.partial, N, p.nchunks, nacc, C, k,
                         (double)V, w.m12, head_dw, head_db);
    const int CV = C / Elem<T>::PER16, G = sweep_grid(V * CV, CV);
    hipLaunchKernelGGL((in_act_bwd_apply_head_kernel<T>), dim3(G, N), dim3(256), 0, st, dout_ncdhw, k, head_w, (const T*)y->ptr, y->ld,
                       V * y->ld, stats, (const float*)w.m12, (T*)dy->ptr, dy->ld, V * dy->ld, (int)V, C, slope, mask);
  });
  RX_CHECK_LAUNCH("rx_instnorm_act_bwd_head");
  return RX_OK;
}
#undef RX_HEAD_REDUCE
