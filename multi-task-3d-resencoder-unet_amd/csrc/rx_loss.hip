// rx_loss.hip -- the two task losses of the train step as single-pass HBM-bound kernels.
//
// The torch formulation (reference training/losses/losses.py) makes 5-8 full passes over the (N,C,Z,Y,X) fp32 logits
// per task and direction; here forward = ONE read of logits + target (per-block partial sums -> a one-block fp64
// finalize that also leaves the per-channel coefficients the backward needs on the device), backward = one read of
// both + one write of d(logits).  No host synchronisation: the loss value and the upstream gradient stay device scalars.
//
//   BCEDiceLoss(alpha, beta)   losses.py:307-318
//     bce  = mean over all elements of BCE-with-logits(x, t*(1-2s)+s)             (:217-238, s = 0.1)
//     dice = 1 - mean_c 2*sum(p t) / max(sum(p^2) + sum(t^2), 1e-6),  p = sigmoid(x), sums over (N, spatial)  (:17-43,128-138)
//   MaskedCosineLoss           losses.py:187-215
//     1 - sum(cos(pred/|pred|, t) * m) / (sum(m) + 1e-8),  m = |t| > 1e-6
//
// The other six names of the reference's loss map (train.py:43-66) follow further down, on the same reduction pattern
// (per-block fp32 partials -> a one-block fp64 finalize -> device-scalar loss):
//   element-wise family (rx_elem_loss_*): BCEWithLogitsLoss, BCEWithLogitsLossLabelSmoothing (losses.py:217-238),
//     BCEWithLogitsLossZSmooth (:240-304), nn.BCELoss, nn.MSELoss -- mean or sum of a per-element term
//   cross entropy over the channel axis (rx_cross_entropy_loss_*): nn.CrossEntropyLoss with probability or class-index targets
#include "rx_common.h"

#define RX_LOSS_BLOCK 256
#define RX_LOSS_ELEMS_PER_BLOCK (RX_LOSS_BLOCK * 4 * 8)   // 8 float4 per thread

template <int NACC>
__device__ inline void block_reduce_store(float (&acc)[NACC], float* out) {
  __shared__ float red[NACC][RX_LOSS_BLOCK / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int a = 0; a < NACC; ++a) {
    float v = acc[a];
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if (lane == 0) red[a][wave] = v;
  }
  __syncthreads();
  if (threadIdx.x < NACC) {
    float s = 0.f;
#pragma unroll
    for (int w = 0; w < RX_LOSS_BLOCK / 64; ++w) s += red[threadIdx.x][w];
    out[threadIdx.x] = s;
  }
}

__device__ inline float sigmoidf_(float x) { return 1.f / (1.f + __expf(-x)); }

// grid (chunks, N*C): plane nc = one (sample, channel) of V contiguous floats
__global__ __launch_bounds__(RX_LOSS_BLOCK) void bce_dice_partial_kernel(const float* __restrict__ x, const float* __restrict__ t, long V,
                                                                          float smoothing, int aligned, float* __restrict__ partial) {
  const long plane = (long)blockIdx.y * V;
  const long begin = (long)blockIdx.x * RX_LOSS_ELEMS_PER_BLOCK;
  const long end = begin + RX_LOSS_ELEMS_PER_BLOCK < V ? begin + RX_LOSS_ELEMS_PER_BLOCK : V;
  float acc[4] = {0.f, 0.f, 0.f, 0.f};  // bce, p*t, p*p, t*t
  auto one = [&](float xv, float tv) {
    const float ts = tv * (1.f - 2.f * smoothing) + smoothing;
    const float ax = fabsf(xv);
    acc[0] += fmaxf(xv, 0.f) - xv * ts + log1pf(__expf(-ax));
    const float p = sigmoidf_(xv);
    acc[1] += p * tv;
    acc[2] += p * p;
    acc[3] += tv * tv;
  };
  const bool vec = aligned && ((plane & 3) == 0) && ((V & 3) == 0);   // aligned: the base pointers, from the host
  if (vec) {
    for (long i = begin + 4 * threadIdx.x; i < end; i += 4 * RX_LOSS_BLOCK) {
      const f32x4 xv = *reinterpret_cast<const f32x4*>(x + plane + i);
      const f32x4 tv = *reinterpret_cast<const f32x4*>(t + plane + i);
#pragma unroll
      for (int j = 0; j < 4; ++j) one(xv[j], tv[j]);
    }
  } else {
    for (long i = begin + threadIdx.x; i < end; i += RX_LOSS_BLOCK) one(x[plane + i], t[plane + i]);
  }
  block_reduce_store<4>(acc, partial + ((long)blockIdx.y * gridDim.x + blockIdx.x) * 4);
}

// one block: fp64 combination, loss value, per-channel backward coefficients
//   coef[2c]   = a_c = 2 / max(D_c, eps)                 d dice_c / d p = a_c t - b_c p
//   coef[2c+1] = b_c = 4 I_c / D_c^2  (0 where the clamp is active)
__global__ __launch_bounds__(256) void bce_dice_finalize_kernel(const float* __restrict__ partial, int N, int C, int chunks, double count,
                                                                float alpha, float beta, float eps, float* __restrict__ loss,
                                                                float* __restrict__ coef) {
  // one block; per channel the N*chunks partial quadruples are summed by all 256 threads (fp64), then thread 0 combines
  __shared__ double red[4][256];
  double bce = 0.0, dice = 0.0;   // meaningful in thread 0 only
  for (int c = 0; c < C; ++c) {
    double s[4] = {0, 0, 0, 0};
    for (int i = threadIdx.x; i < N * chunks; i += 256) {
      const int n = i / chunks, k = i - n * chunks;
      const float* p = partial + (((long)n * C + c) * chunks + k) * 4;
      s[0] += p[0], s[1] += p[1], s[2] += p[2], s[3] += p[3];
    }
#pragma unroll
    for (int a = 0; a < 4; ++a) red[a][threadIdx.x] = s[a];
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
      if (threadIdx.x < o)
#pragma unroll
        for (int a = 0; a < 4; ++a) red[a][threadIdx.x] += red[a][threadIdx.x + o];
      __syncthreads();
    }
    if (threadIdx.x == 0) {
      const double den = red[2][0] + red[3][0];
      const double D = den > (double)eps ? den : (double)eps;
      bce += red[0][0];
      dice += 2.0 * red[1][0] / D;
      coef[2 * c] = (float)(2.0 / D);
      coef[2 * c + 1] = den > (double)eps ? (float)(4.0 * red[1][0] / (D * D)) : 0.f;
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) *loss = (float)((double)alpha * (bce / count) + (double)beta * (1.0 - dice / C));
}

__global__ __launch_bounds__(RX_LOSS_BLOCK) void bce_dice_bwd_kernel(const float* __restrict__ x, const float* __restrict__ t, long V, int C,
                                                                      float smoothing, float k_bce, float k_dice,
                                                                      const float* __restrict__ coef, const float* __restrict__ gloss,
                                                                      int aligned, float* __restrict__ dx) {
  const int c = blockIdx.y % C;
  const long plane = (long)blockIdx.y * V;
  const long begin = (long)blockIdx.x * RX_LOSS_ELEMS_PER_BLOCK;
  const long end = begin + RX_LOSS_ELEMS_PER_BLOCK < V ? begin + RX_LOSS_ELEMS_PER_BLOCK : V;
  const float g = gloss ? *gloss : 1.f;
  const float a = coef[2 * c], b = coef[2 * c + 1];
  // no contraction: the 16-byte and the scalar path must round alike, so that a misaligned call gives the aligned call's bits
  auto one = [&](float xv, float tv) {
#pragma clang fp contract(off)
    const float ts = tv * (1.f - 2.f * smoothing) + smoothing;
    const float p = sigmoidf_(xv);
    return g * (k_bce * (p - ts) - k_dice * (a * tv - b * p) * p * (1.f - p));
  };
  const bool vec = aligned && ((plane & 3) == 0) && ((V & 3) == 0);   // aligned: the base pointers, from the host
  if (vec) {
    for (long i = begin + 4 * threadIdx.x; i < end; i += 4 * RX_LOSS_BLOCK) {
      const f32x4 xv = *reinterpret_cast<const f32x4*>(x + plane + i);
      const f32x4 tv = *reinterpret_cast<const f32x4*>(t + plane + i);
      f32x4 o;
#pragma unroll
      for (int j = 0; j < 4; ++j) o[j] = one(xv[j], tv[j]);
      *reinterpret_cast<f32x4*>(dx + plane + i) = o;
    }
  } else {
    for (long i = begin + threadIdx.x; i < end; i += RX_LOSS_BLOCK) dx[plane + i] = one(x[plane + i], t[plane + i]);
  }
}

// ---- masked cosine: grid (chunks, N); a thread walks voxels, its C channel values sit V apart ---------------------------
#define RX_COS_MAXC 8
__global__ __launch_bounds__(RX_LOSS_BLOCK) void masked_cosine_partial_kernel(const float* __restrict__ pr, const float* __restrict__ tg, long V,
                                                                               int C, float* __restrict__ partial) {
  const long base = (long)blockIdx.y * C * V;
  const long begin = (long)blockIdx.x * RX_LOSS_ELEMS_PER_BLOCK;
  const long end = begin + RX_LOSS_ELEMS_PER_BLOCK < V ? begin + RX_LOSS_ELEMS_PER_BLOCK : V;
  float acc[2] = {0.f, 0.f};  // sum cos*mask, sum mask
  for (long i = begin + threadIdx.x; i < end; i += RX_LOSS_BLOCK) {
    float pp = 0.f, tt = 0.f, pt = 0.f;
    for (int c = 0; c < C; ++c) {
      const float p = pr[base + c * V + i], t = tg[base + c * V + i];
      pp += p * p, tt += t * t, pt += p * t;
    }
    const float pn = sqrtf(pp), tn = sqrtf(tt);
    if (tn > 1e-6f) {
      // u = pred / max(|pred|, 1e-8); cos = (u . t) / (max(|u|, 1e-8) * max(|t|, 1e-8))
      const float pc = fmaxf(pn, 1e-8f);
      const float un = pn / pc;
      acc[0] += (pt / pc) / (fmaxf(un, 1e-8f) * fmaxf(tn, 1e-8f));
      acc[1] += 1.f;
    }
  }
  block_reduce_store<2>(acc, partial + ((long)blockIdx.y * gridDim.x + blockIdx.x) * 2);
}

__global__ __launch_bounds__(256) void masked_cosine_finalize_kernel(const float* __restrict__ partial, int nblocks, float* __restrict__ loss,
                                                                     float* __restrict__ coef) {
  __shared__ double s0[256], s1[256];
  double a = 0.0, m = 0.0;
  for (int i = threadIdx.x; i < nblocks; i += 256) a += partial[2 * i], m += partial[2 * i + 1];
  s0[threadIdx.x] = a, s1[threadIdx.x] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    a = m = 0.0;
    for (int i = 0; i < 256; ++i) a += s0[i], m += s1[i];
    *loss = (float)(1.0 - a / (m + 1e-8));
    coef[0] = (float)(1.0 / (m + 1e-8));
  }
}

__global__ __launch_bounds__(RX_LOSS_BLOCK) void masked_cosine_bwd_kernel(const float* __restrict__ pr, const float* __restrict__ tg, long V, int C,
                                                                           const float* __restrict__ coef, const float* __restrict__ gloss,
                                                                           float* __restrict__ dp) {
  const long base = (long)blockIdx.y * C * V;
  const long begin = (long)blockIdx.x * RX_LOSS_ELEMS_PER_BLOCK;
  const long end = begin + RX_LOSS_ELEMS_PER_BLOCK < V ? begin + RX_LOSS_ELEMS_PER_BLOCK : V;
  const float k = -(gloss ? *gloss : 1.f) * coef[0];
  for (long i = begin + threadIdx.x; i < end; i += RX_LOSS_BLOCK) {
    float p[RX_COS_MAXC], t[RX_COS_MAXC];
    float pp = 0.f, tt = 0.f, pt = 0.f;
#pragma unroll
    for (int c = 0; c < RX_COS_MAXC; ++c)
      if (c < C) {
        p[c] = pr[base + c * V + i], t[c] = tg[base + c * V + i];
        pp += p[c] * p[c], tt += t[c] * t[c], pt += p[c] * t[c];
      }
    const float pn = sqrtf(pp), tn = sqrtf(tt);
    // The graph of the host formulation, u = pred / pc with pc = max(|pred|, 1e-8), cos = (u . t) / (uc * |t|) with uc = max(|u|, 1e-8):
    //   d cos / d pred = (t/|t| - cos * pred/|pred|) / (uc * pc)
    // Where |pred| >= 1e-8 both clamps are inactive and uc * pc = |pred|.  Below that u = pred / 1e-8 is still linear in pred and the
    // cosine is scale-invariant, so down to |pred| = 1e-16 (|u| = 1e-8) the product is |pred| again: the same expression.  Below
    // 1e-16 the second clamp holds uc at 1e-8 and cos shrinks with |u|; at pred == 0 what is left is t/|t| * 1e16.
    const bool on = tn > 1e-6f;
    const float pc = fmaxf(pn, 1e-8f);
    const float scale = pn >= 1e-8f ? 1.f / pn : 1.f / (fmaxf(pn / pc, 1e-8f) * pc);
    const float inv_p = pn > 0.f ? 1.f / pn : 0.f, inv_t = on ? 1.f / tn : 0.f;
    const float cs = pt * scale * inv_t;
#pragma unroll
    for (int c = 0; c < RX_COS_MAXC; ++c)
      if (c < C) dp[base + c * V + i] = on ? k * (t[c] * inv_t - cs * p[c] * inv_p) * scale : 0.f;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
static inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
static inline int loss_chunks(long V) { return (int)((V + RX_LOSS_ELEMS_PER_BLOCK - 1) / RX_LOSS_ELEMS_PER_BLOCK); }

extern "C" size_t rx_loss_workspace(int n, int c, long v) {
  if (n < 1 || c < 1 || v < 1) return 0;
  return (size_t)n * c * loss_chunks(v) * 4 * sizeof(float) + 256;
}

static int loss_args_ok(const void* a, const void* b, int n, int c, long v) { return a && b && n >= 1 && c >= 1 && v >= 1 && (long)n * c < 65536; }

extern "C" int rx_bce_dice_loss_fwd(const float* logits, const float* target, int n, int c, long v, float alpha, float beta, float smoothing,
                                    float eps, float* loss, float* coef, void* ws, size_t ws_bytes, void* stream) {
  if (!loss_args_ok(logits, target, n, c, v) || !loss || !coef || !ws) RX_FAIL(RX_EINVAL, "rx_bce_dice_loss_fwd: bad arguments");
  if (ws_bytes < rx_loss_workspace(n, c, v)) RX_FAIL(RX_EWORKSPACE, "rx_bce_dice_loss_fwd: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  const int chunks = loss_chunks(v), aligned = aligned16(logits) && aligned16(target);
  hipLaunchKernelGGL(bce_dice_partial_kernel, dim3(chunks, n * c), dim3(RX_LOSS_BLOCK), 0, st, logits, target, v, smoothing, aligned,
                     (float*)ws);
  hipLaunchKernelGGL(bce_dice_finalize_kernel, dim3(1), dim3(256), 0, st, (const float*)ws, n, c, chunks, (double)n * c * (double)v, alpha,
                     beta, eps, loss, coef);
  RX_CHECK_LAUNCH("rx_bce_dice_loss_fwd");
  return RX_OK;
}

extern "C" int rx_bce_dice_loss_bwd(const float* logits, const float* target, int n, int c, long v, float alpha, float beta, float smoothing,
                                    const float* coef, const float* grad_loss, float* dlogits, void* stream) {
  if (!loss_args_ok(logits, target, n, c, v) || !coef || !dlogits) RX_FAIL(RX_EINVAL, "rx_bce_dice_loss_bwd: bad arguments");
  hipStream_t st = (hipStream_t)stream;
  const float k_bce = (float)((double)alpha / ((double)n * c * (double)v)), k_dice = beta / c;
  const int aligned = aligned16(logits) && aligned16(target) && aligned16(dlogits);
  hipLaunchKernelGGL(bce_dice_bwd_kernel, dim3(loss_chunks(v), n * c), dim3(RX_LOSS_BLOCK), 0, st, logits, target, v, c, smoothing, k_bce,
                     k_dice, coef, grad_loss, aligned, dlogits);
  RX_CHECK_LAUNCH("rx_bce_dice_loss_bwd");
  return RX_OK;
}

extern "C" int rx_masked_cosine_loss_fwd(const float* pred, const float* target, int n, int c, long v, float* loss, float* coef, void* ws,
                                         size_t ws_bytes, void* stream) {
  if (!loss_args_ok(pred, target, n, c, v) || !loss || !coef || !ws) RX_FAIL(RX_EINVAL, "rx_masked_cosine_loss_fwd: bad arguments");
  if (c > RX_COS_MAXC) RX_FAIL(RX_EUNSUPPORTED, "rx_masked_cosine_loss: at most %d channels (got %d)", RX_COS_MAXC, c);
  if (ws_bytes < rx_loss_workspace(n, c, v)) RX_FAIL(RX_EWORKSPACE, "rx_masked_cosine_loss_fwd: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  const int chunks = loss_chunks(v);
  hipLaunchKernelGGL(masked_cosine_partial_kernel, dim3(chunks, n), dim3(RX_LOSS_BLOCK), 0, st, pred, target, v, c, (float*)ws);
  hipLaunchKernelGGL(masked_cosine_finalize_kernel, dim3(1), dim3(256), 0, st, (const float*)ws, chunks * n, loss, coef);
  RX_CHECK_LAUNCH("rx_masked_cosine_loss_fwd");
  return RX_OK;
}

extern "C" int rx_masked_cosine_loss_bwd(const float* pred, const float* target, int n, int c, long v, const float* coef,
                                         const float* grad_loss, float* dpred, void* stream) {
  if (!loss_args_ok(pred, target, n, c, v) || !coef || !dpred) RX_FAIL(RX_EINVAL, "rx_masked_cosine_loss_bwd: bad arguments");
  if (c > RX_COS_MAXC) RX_FAIL(RX_EUNSUPPORTED, "rx_masked_cosine_loss: at most %d channels (got %d)", RX_COS_MAXC, c);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(masked_cosine_bwd_kernel, dim3(loss_chunks(v), n), dim3(RX_LOSS_BLOCK), 0, st, pred, target, v, c, coef, grad_loss,
                     dpred);
  RX_CHECK_LAUNCH("rx_masked_cosine_loss_bwd");
  return RX_OK;
}

// =====================================================================================================================
// Element-wise family: loss = sum (or mean) over all elements of l(x, t).  grid (chunks, N*C) as bce_dice_partial_kernel.
//   kind RX_LOSS_BCE_LOGITS  l = max(x,0) - x*ts + log1p(exp(-|x|)),  ts = t*(1-2a) + a          dl/dx = sigmoid(x) - ts
//        RX_LOSS_BCE_PROB    l = -(t*max(log x, -100) + (1-t)*max(log(1-x), -100))  (nn.BCELoss)  dl/dx = (x-t) / max(x*(1-x), 1e-12)
//        RX_LOSS_MSE         l = (x-t)^2                                                          dl/dx = 2(x-t)
//   a: one constant (`smoothing`), or -- TABLE -- alpha_z[z] with z = (index inside the plane) / yx, the slice-dependent
//   smoothing of BCEWithLogitsLossZSmooth (the table is built by the caller with the reference's own fp32 expression).
// Bytes moved, E = N*C*V elements:  forward  reads 8E (x, t), writes 4 per block;  backward reads 8E, writes 4E (dx).
// Nothing is saved between the two.
template <int KIND>
__device__ inline float elem_term(float xv, float tv, float a) {
  if (KIND == RX_LOSS_BCE_LOGITS) {
    const float ts = tv * (1.f - 2.f * a) + a;
    return fmaxf(xv, 0.f) - xv * ts + log1pf(__expf(-fabsf(xv)));
  } else if (KIND == RX_LOSS_BCE_PROB) {
    return -(tv * fmaxf(logf(xv), -100.f) + (1.f - tv) * fmaxf(log1pf(-xv), -100.f));
  } else {
    const float d = xv - tv;
    return d * d;
  }
}
template <int KIND>
__device__ inline float elem_grad(float xv, float tv, float a) {
  if (KIND == RX_LOSS_BCE_LOGITS) {
    return sigmoidf_(xv) - (tv * (1.f - 2.f * a) + a);
  } else if (KIND == RX_LOSS_BCE_PROB) {
    return (xv - tv) / fmaxf(xv * (1.f - xv), 1e-12f);
  } else {
    return 2.f * (xv - tv);
  }
}

// the smoothing of the 4 consecutive elements starting at plane index i (TABLE: at most one slice boundary per step since yx >= 1)
template <bool TABLE>
struct ElemAlpha {
  float a;
  const float* tab;
  unsigned yx;
  __device__ inline float at(long i) const { return TABLE ? tab[(unsigned)i / yx] : a; }
  __device__ inline void at4(long i, float (&o)[4]) const {
    if (TABLE) {
      unsigned z = (unsigned)i / yx, lim = (z + 1) * yx;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if ((unsigned)i + j >= lim) ++z, lim += yx;
        o[j] = tab[z];
      }
    } else {
      o[0] = o[1] = o[2] = o[3] = a;
    }
  }
};

template <int KIND, bool TABLE>
__global__ __launch_bounds__(RX_LOSS_BLOCK) void elem_loss_partial_kernel(const float* __restrict__ x, const float* __restrict__ t, long V,
                                                                           ElemAlpha<TABLE> al, int aligned, float* __restrict__ partial) {
  const long plane = (long)blockIdx.y * V;
  const long begin = (long)blockIdx.x * RX_LOSS_ELEMS_PER_BLOCK;
  const long end = begin + RX_LOSS_ELEMS_PER_BLOCK < V ? begin + RX_LOSS_ELEMS_PER_BLOCK : V;
  float acc[1] = {0.f};
  const bool vec = aligned && ((plane & 3) == 0) && ((V & 3) == 0);
  if (vec) {
    for (long i = begin + 4 * threadIdx.x; i < end; i += 4 * RX_LOSS_BLOCK) {
      const f32x4 xv = *reinterpret_cast<const f32x4*>(x + plane + i);
      const f32x4 tv = *reinterpret_cast<const f32x4*>(t + plane + i);
      float a[4];
      al.at4(i, a);
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[0] += elem_term<KIND>(xv[j], tv[j], a[j]);
    }
  } else {
    for (long i = begin + threadIdx.x; i < end; i += RX_LOSS_BLOCK) acc[0] += elem_term<KIND>(x[plane + i], t[plane + i], al.at(i));
  }
  block_reduce_store<1>(acc, partial + ((long)blockIdx.y * gridDim.x + blockIdx.x));
}

template <int KIND, bool TABLE>
__global__ __launch_bounds__(RX_LOSS_BLOCK) void elem_loss_bwd_kernel(const float* __restrict__ x, const float* __restrict__ t, long V,
                                                                       ElemAlpha<TABLE> al, int aligned, float k,
                                                                       const float* __restrict__ gloss, float* __restrict__ dx) {
  const long plane = (long)blockIdx.y * V;
  const long begin = (long)blockIdx.x * RX_LOSS_ELEMS_PER_BLOCK;
  const long end = begin + RX_LOSS_ELEMS_PER_BLOCK < V ? begin + RX_LOSS_ELEMS_PER_BLOCK : V;
  const float gk = (gloss ? *gloss : 1.f) * k;
  const bool vec = aligned && ((plane & 3) == 0) && ((V & 3) == 0);
  if (vec) {
    for (long i = begin + 4 * threadIdx.x; i < end; i += 4 * RX_LOSS_BLOCK) {
      const f32x4 xv = *reinterpret_cast<const f32x4*>(x + plane + i);
      const f32x4 tv = *reinterpret_cast<const f32x4*>(t + plane + i);
      float a[4];
      al.at4(i, a);
      f32x4 o;
#pragma unroll
      for (int j = 0; j < 4; ++j) o[j] = gk * elem_grad<KIND>(xv[j], tv[j], a[j]);
      *reinterpret_cast<f32x4*>(dx + plane + i) = o;
    }
  } else {
    for (long i = begin + threadIdx.x; i < end; i += RX_LOSS_BLOCK) dx[plane + i] = gk * elem_grad<KIND>(x[plane + i], t[plane + i], al.at(i));
  }
}

// one block: fp64 sum of the per-block partials (NACC floats per block; accumulator 1, where present, counts the contributing
// voxels).  denom > 0: loss = sum / denom;  denom == 0: loss = sum / (summed count) -- NaN when nothing contributed, as torch's
// 0/0, with the backward factor 0 so that the gradient is the zero torch returns;  denom < 0: loss = sum.
// coef (optional) receives the factor the backward multiplies by (1/denominator, or 1).
template <int NACC>
__global__ __launch_bounds__(256) void loss_sum_finalize_kernel(const float* __restrict__ partial, int nblocks, double denom,
                                                                float* __restrict__ loss, float* __restrict__ coef) {
  __shared__ double s0[256], s1[256];
  double a = 0.0, m = 0.0;
  for (int i = threadIdx.x; i < nblocks; i += 256) {
    a += partial[NACC * i];
    if (NACC > 1) m += partial[NACC * i + 1];
  }
  s0[threadIdx.x] = a, s1[threadIdx.x] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    a = m = 0.0;
    for (int i = 0; i < 256; ++i) a += s0[i], m += s1[i];
    const double den = denom > 0.0 ? denom : denom == 0.0 ? m : 1.0;
    *loss = (float)(a / den);
    if (coef) coef[0] = den > 0.0 ? (float)(1.0 / den) : 0.f;
  }
}

// =====================================================================================================================
// Cross entropy over the channel axis.  logits (N, C, V) fp32; grid (chunks, N): a thread owns W voxels (W = 4 consecutive
// ones as 16-byte accesses when V % 4 == 0 and the operands are 16-byte aligned, else 1); its C values sit V apart, so every
// load is coalesced across the wave.  Targets: probabilities (N, C, V) fp32, or -- INDEX -- class indices (N, V) int64 with
// ignore_index (an index outside [0, C) contributes nothing, like an ignored one: nothing is read out of bounds).
//   forward : one pass over C with an online max / sum of exponentials (one exp per value);
//             loss_v = lse * s - sum_c t_c x_c,  s = sum_c t_c   (INDEX: lse - x[target], s = 1, or 0 where ignored)
//             saves lse per voxel, and s in probability mode
//   backward: dx_c = g * k * (exp(x_c - lse) * s - t_c),  k from the forward's finalize (coef[0])
// Bytes moved, E = N*C*V, P = N*V:
//   probability targets  forward reads 8E (x, t), writes 8P (lse, s);      backward reads 8E + 8P, writes 4E
//   index targets        forward reads 4E + 8P (x, target), writes 4P;    backward reads 4E + 12P, writes 4E
#define RX_CE_VOX_PER_BLOCK (RX_LOSS_BLOCK * 4 * 2)
#define RX_CE_MAXC 1024

template <int W>
__device__ inline void ce_load(const float* p, float (&o)[W]) {
  if (W == 4) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(p);
#pragma unroll
    for (int j = 0; j < W; ++j) o[j] = v[j];
  } else {
    o[0] = *p;
  }
}
template <int W>
__device__ inline void ce_store(float* p, const float (&o)[W]) {
  if (W == 4) {
    *reinterpret_cast<f32x4*>(p) = f32x4{o[0], o[1 % W], o[2 % W], o[3 % W]};
  } else {
    *p = o[0];
  }
}

template <int W, bool INDEX>
__global__ __launch_bounds__(RX_LOSS_BLOCK) void ce_partial_kernel(const float* __restrict__ x, const float* __restrict__ tp,
                                                                    const long long* __restrict__ ti, long long ignore, long V, int C,
                                                                    float* __restrict__ saved, long P, float* __restrict__ partial) {
  const long base = (long)blockIdx.y * C * V, vox0 = (long)blockIdx.y * V;
  const long begin = (long)blockIdx.x * RX_CE_VOX_PER_BLOCK;
  const long end = begin + RX_CE_VOX_PER_BLOCK < V ? begin + RX_CE_VOX_PER_BLOCK : V;
  float acc[2] = {0.f, 0.f};  // sum of voxel losses, number of contributing voxels
  for (long i = begin + W * threadIdx.x; i < end; i += W * RX_LOSS_BLOCK) {
    float m[W], s[W], st[W], stx[W], xv[W], tv[W];
    int tg[W];
    if (INDEX) {
#pragma unroll
      for (int j = 0; j < W; ++j) {
        const long long g = ti[vox0 + i + j];
        tg[j] = (g != ignore && g >= 0 && g < C) ? (int)g : -1;
      }
    }
#pragma unroll
    for (int j = 0; j < W; ++j) s[j] = 0.f, st[j] = 0.f, stx[j] = 0.f, m[j] = 0.f;
    for (int c = 0; c < C; ++c) {
      ce_load<W>(x + base + (long)c * V + i, xv);
      if (!INDEX) ce_load<W>(tp + base + (long)c * V + i, tv);
#pragma unroll
      for (int j = 0; j < W; ++j) {
        if (c == 0) {
          m[j] = xv[j], s[j] = 1.f;
        } else {
          const float d = xv[j] - m[j];
          const float e = __expf(-fabsf(d));
          s[j] = d > 0.f ? s[j] * e + 1.f : s[j] + e;
          m[j] = fmaxf(m[j], xv[j]);
        }
        if (INDEX) {
          if (c == tg[j]) stx[j] = xv[j];
        } else {
          st[j] += tv[j];
          stx[j] += tv[j] * xv[j];
        }
      }
    }
    float lse[W];
#pragma unroll
    for (int j = 0; j < W; ++j) {
      lse[j] = m[j] + logf(s[j]);
      if (INDEX) {
        if (tg[j] >= 0) acc[0] += lse[j] - stx[j], acc[1] += 1.f;
      } else {
        acc[0] += lse[j] * st[j] - stx[j];
      }
    }
    ce_store<W>(saved + vox0 + i, lse);
    if (!INDEX) ce_store<W>(saved + P + vox0 + i, st);
  }
  block_reduce_store<2>(acc, partial + ((long)blockIdx.y * gridDim.x + blockIdx.x) * 2);
}

template <int W, bool INDEX>
__global__ __launch_bounds__(RX_LOSS_BLOCK) void ce_bwd_kernel(const float* __restrict__ x, const float* __restrict__ tp,
                                                                const long long* __restrict__ ti, long long ignore, long V, int C,
                                                                const float* __restrict__ saved, long P, const float* __restrict__ coef,
                                                                const float* __restrict__ gloss, float* __restrict__ dx) {
  const long base = (long)blockIdx.y * C * V, vox0 = (long)blockIdx.y * V;
  const long begin = (long)blockIdx.x * RX_CE_VOX_PER_BLOCK;
  const long end = begin + RX_CE_VOX_PER_BLOCK < V ? begin + RX_CE_VOX_PER_BLOCK : V;
  const float gk = (gloss ? *gloss : 1.f) * coef[0];
  for (long i = begin + W * threadIdx.x; i < end; i += W * RX_LOSS_BLOCK) {
    float lse[W], s[W], xv[W], tv[W], o[W];
    int tg[W];
    ce_load<W>(saved + vox0 + i, lse);
    if (INDEX) {
#pragma unroll
      for (int j = 0; j < W; ++j) {
        const long long g = ti[vox0 + i + j];
        tg[j] = (g != ignore && g >= 0 && g < C) ? (int)g : -1;
        s[j] = tg[j] >= 0 ? 1.f : 0.f;
      }
    } else {
      ce_load<W>(saved + P + vox0 + i, s);
    }
    for (int c = 0; c < C; ++c) {
      ce_load<W>(x + base + (long)c * V + i, xv);
      if (!INDEX) ce_load<W>(tp + base + (long)c * V + i, tv);
#pragma unroll
      for (int j = 0; j < W; ++j) {
        const float t = INDEX ? (c == tg[j] ? 1.f : 0.f) : tv[j];
        o[j] = gk * (__expf(xv[j] - lse[j]) * s[j] - t);
      }
      ce_store<W>(dx + base + (long)c * V + i, o);
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
static int elem_args_ok(int kind, const float* alpha_z, int z, int n, int c, long v, int reduction) {
  if (kind < RX_LOSS_BCE_LOGITS || kind > RX_LOSS_MSE) return 0;
  if (reduction != RX_REDUCE_MEAN && reduction != RX_REDUCE_SUM) return 0;
  if (alpha_z && (kind != RX_LOSS_BCE_LOGITS || z < 1 || v % z != 0 || v > 0x7fffffffL)) return 0;
  return 1;
}

#define RX_ELEM_DISPATCH(kind, table, ...)                                   \
  do {                                                                       \
    if (table) {                                                             \
      constexpr int KIND = RX_LOSS_BCE_LOGITS;                               \
      constexpr bool TABLE = true;                                           \
      __VA_ARGS__;                                                           \
    } else if ((kind) == RX_LOSS_BCE_LOGITS) {                               \
      constexpr int KIND = RX_LOSS_BCE_LOGITS;                               \
      constexpr bool TABLE = false;                                          \
      __VA_ARGS__;                                                           \
    } else if ((kind) == RX_LOSS_BCE_PROB) {                                 \
      constexpr int KIND = RX_LOSS_BCE_PROB;                                 \
      constexpr bool TABLE = false;                                          \
      __VA_ARGS__;                                                           \
    } else {                                                                 \
      constexpr int KIND = RX_LOSS_MSE;                                      \
      constexpr bool TABLE = false;                                          \
      __VA_ARGS__;                                                           \
    }                                                                        \
  } while (0)

extern "C" int rx_elem_loss_fwd(int kind, const float* x, const float* target, int n, int c, long v, float smoothing, const float* alpha_z,
                                int z, int reduction, float* loss, void* ws, size_t ws_bytes, void* stream) {
  if (!loss_args_ok(x, target, n, c, v) || !loss || !ws || !elem_args_ok(kind, alpha_z, z, n, c, v, reduction))
    RX_FAIL(RX_EINVAL, "rx_elem_loss_fwd: bad arguments");
  if (ws_bytes < rx_loss_workspace(n, c, v)) RX_FAIL(RX_EWORKSPACE, "rx_elem_loss_fwd: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  const int chunks = loss_chunks(v), aligned = aligned16(x) && aligned16(target);
  RX_ELEM_DISPATCH(kind, alpha_z != nullptr, {
    const ElemAlpha<TABLE> al{smoothing, alpha_z, alpha_z ? (unsigned)(v / z) : 1u};
    hipLaunchKernelGGL((elem_loss_partial_kernel<KIND, TABLE>), dim3(chunks, n * c), dim3(RX_LOSS_BLOCK), 0, st, x, target, v, al, aligned,
                       (float*)ws);
  });
  hipLaunchKernelGGL(loss_sum_finalize_kernel<1>, dim3(1), dim3(256), 0, st, (const float*)ws, chunks * n * c,
                     reduction == RX_REDUCE_MEAN ? (double)n * c * (double)v : -1.0, loss, (float*)nullptr);
  RX_CHECK_LAUNCH("rx_elem_loss_fwd");
  return RX_OK;
}

extern "C" int rx_elem_loss_bwd(int kind, const float* x, const float* target, int n, int c, long v, float smoothing, const float* alpha_z,
                                int z, int reduction, const float* grad_loss, float* dx, void* stream) {
  if (!loss_args_ok(x, target, n, c, v) || !dx || !elem_args_ok(kind, alpha_z, z, n, c, v, reduction))
    RX_FAIL(RX_EINVAL, "rx_elem_loss_bwd: bad arguments");
  hipStream_t st = (hipStream_t)stream;
  const int aligned = aligned16(x) && aligned16(target) && aligned16(dx);
  const float k = reduction == RX_REDUCE_MEAN ? (float)(1.0 / ((double)n * c * (double)v)) : 1.f;
  RX_ELEM_DISPATCH(kind, alpha_z != nullptr, {
    const ElemAlpha<TABLE> al{smoothing, alpha_z, alpha_z ? (unsigned)(v / z) : 1u};
    hipLaunchKernelGGL((elem_loss_bwd_kernel<KIND, TABLE>), dim3(loss_chunks(v), n * c), dim3(RX_LOSS_BLOCK), 0, st, x, target, v, al,
                       aligned, k, grad_loss, dx);
  });
  RX_CHECK_LAUNCH("rx_elem_loss_bwd");
  return RX_OK;
}

static inline int ce_chunks(long v) { return (int)((v + RX_CE_VOX_PER_BLOCK - 1) / RX_CE_VOX_PER_BLOCK); }

extern "C" size_t rx_cross_entropy_loss_workspace(int n, int c, long v) {
  if (n < 1 || c < 1 || v < 1) return 0;
  return (size_t)n * ce_chunks(v) * 2 * sizeof(float) + 256;
}

// grid y is N here (not N*C): N < 65536, 1 <= C <= RX_CE_MAXC; exactly one target kind
static int ce_args_ok(const float* x, const float* tp, const int64_t* ti, int n, int c, long v) {
  return x && ((tp != nullptr) != (ti != nullptr)) && n >= 1 && n < 65536 && c >= 1 && v >= 1;
}

#define RX_CE_DISPATCH(vec, index, ...)        \
  do {                                         \
    if ((vec) && (index)) {                    \
      constexpr int W = 4;                     \
      constexpr bool INDEX = true;             \
      __VA_ARGS__;                             \
    } else if (vec) {                          \
      constexpr int W = 4;                     \
      constexpr bool INDEX = false;            \
      __VA_ARGS__;                             \
    } else if (index) {                        \
      constexpr int W = 1;                     \
      constexpr bool INDEX = true;             \
      __VA_ARGS__;                             \
    } else {                                   \
      constexpr int W = 1;                     \
      constexpr bool INDEX = false;            \
      __VA_ARGS__;                             \
    }                                          \
  } while (0)

extern "C" int rx_cross_entropy_loss_fwd(const float* logits, const float* target_prob, const int64_t* target_index, int64_t ignore_index,
                                         int n, int c, long v, int reduction, float* loss, float* coef, float* saved, void* ws,
                                         size_t ws_bytes, void* stream) {
  if (!ce_args_ok(logits, target_prob, target_index, n, c, v) || !loss || !coef || !saved || !ws ||
      (reduction != RX_REDUCE_MEAN && reduction != RX_REDUCE_SUM))
    RX_FAIL(RX_EINVAL, "rx_cross_entropy_loss_fwd: bad arguments");
  if (c > RX_CE_MAXC) RX_FAIL(RX_EUNSUPPORTED, "rx_cross_entropy_loss_fwd: at most %d classes (got %d)", RX_CE_MAXC, c);
  if (ws_bytes < rx_cross_entropy_loss_workspace(n, c, v)) RX_FAIL(RX_EWORKSPACE, "rx_cross_entropy_loss_fwd: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  const int chunks = ce_chunks(v);
  const bool index = target_index != nullptr;
  const bool vec = (v & 3) == 0 && aligned16(logits) && aligned16(saved) && (index || aligned16(target_prob));
  const long P = (long)n * v;
  RX_CE_DISPATCH(vec, index, {
    hipLaunchKernelGGL((ce_partial_kernel<W, INDEX>), dim3(chunks, n), dim3(RX_LOSS_BLOCK), 0, st, logits, target_prob,
                       (const long long*)target_index, (long long)ignore_index, v, c, saved, P, (float*)ws);
  });
  const double denom = reduction == RX_REDUCE_SUM ? -1.0 : index ? 0.0 : (double)n * (double)v;
  hipLaunchKernelGGL(loss_sum_finalize_kernel<2>, dim3(1), dim3(256), 0, st, (const float*)ws, chunks * n, denom, loss, coef);
  RX_CHECK_LAUNCH("rx_cross_entropy_loss_fwd");
  return RX_OK;
}

extern "C" int rx_cross_entropy_loss_bwd(const float* logits, const float* target_prob, const int64_t* target_index, int64_t ignore_index,
                                         int n, int c, long v, const float* coef, const float* saved, const float* grad_loss,
                                         float* dlogits, void* stream) {
  if (!ce_args_ok(logits, target_prob, target_index, n, c, v) || !coef || !saved || !dlogits)
    RX_FAIL(RX_EINVAL, "rx_cross_entropy_loss_bwd: bad arguments");
  if (c > RX_CE_MAXC) RX_FAIL(RX_EUNSUPPORTED, "rx_cross_entropy_loss_bwd: at most %d classes (got %d)", RX_CE_MAXC, c);
  hipStream_t st = (hipStream_t)stream;
  const bool index = target_index != nullptr;
  const bool vec = (v & 3) == 0 && aligned16(logits) && aligned16(saved) && aligned16(dlogits) && (index || aligned16(target_prob));
  const long P = (long)n * v;
  RX_CE_DISPATCH(vec, index, {
    hipLaunchKernelGGL((ce_bwd_kernel<W, INDEX>), dim3(ce_chunks(v), n), dim3(RX_LOSS_BLOCK), 0, st, logits, target_prob,
                       (const long long*)target_index, (long long)ignore_index, v, c, saved, P, coef, grad_loss, dlogits);
  });
  RX_CHECK_LAUNCH("rx_cross_entropy_loss_bwd");
  return RX_OK;
}
