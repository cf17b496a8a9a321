// rx_pack_optim.hip -- per-step work on the parameters: the weight packers of the conv kernels, AdamW (fused with the re-pack,
// flat, and table-driven over many tensors), SGD with momentum / Nesterov in the same two shapes, and the global gradient norm with
// its clip coefficient.
#include <math.h>

#include "rx_common.h"

// ---- weight packing --------------------------------------------------------------------------
// in: w[A][B][T] fp32.  same[t'][A][B], swap[t''][B][A] where t' / t'' optionally reversed.
// One block handles a 32(A) x 32(B) tile for all T taps through LDS.
// Weight packing runs on EVERY training step (all 68 conv / convT weights of cfg2, 1.7 GB of traffic) on the side stream.
// A block owns a 32(A) x 32(B) tile for all TT taps.  The tile is transposed into LDS as [t][a][b] in the compute dtype
// (80-byte b-rows: 16-byte aligned, 16 consecutive rows hit 16 distinct bank slots) while it is loaded with 16-byte
// global reads; `same[t][a][b..b+7]` then leaves as one 16-byte LDS read + one 16-byte store, `swap[t][b][a..a+7]` as
// eight 2-byte LDS reads + one 16-byte store.  (The first version stored every bf16 element with its own 2-byte global
// store and two runtime integer divisions: 97 us per launch, 6.4 ms of kernel time per step.)
#define RX_PACK_PB 40   // LDS pitch of a b-row in elements (80 bytes)
// 1024 threads per tile: the load loop is one 16-byte load + four 2-byte LDS writes per iteration, so the loads in flight per
// CU scale with the thread count (one workgroup per CU for the 512-channel weights: 256 tiles).  256 threads: 34 us per 7 M-parameter
// weight; see DESIGN.md row ai
#ifndef RX_PACK_THREADS
#define RX_PACK_THREADS 1024
#endif

template <typename T>
__device__ __forceinline__ void pack_tile(const float* __restrict__ w, int A, int B, int TT, unsigned inv_tt, T* __restrict__ same,
                                          int flip_same, T* __restrict__ swp, int flip_swap, const int a0, const int b0) {
  extern __shared__ __attribute__((aligned(16))) unsigned char pack_smem[];
  T* L = reinterpret_cast<T*>(pack_smem);               // [TT][32 a][RX_PACK_PB]
  const int rowlen = 32 * TT;
  const bool full = a0 + 32 <= A && b0 + 32 <= B && sizeof(T) == 2 && (B & 7) == 0 && (A & 7) == 0;
  // ---- load + convert + transpose into LDS
  if (full && TT > 1 && (rowlen & 3) == 0 && ((size_t)B * TT & 3) == 0) {
    const int q4 = rowlen >> 2;                           // float4 pieces per a-row
    for (int q = threadIdx.x; q < 32 * q4; q += RX_PACK_THREADS) {
      const int a = q / q4, c = q - a * q4;
      const f32x4 v = *reinterpret_cast<const f32x4*>(w + ((size_t)(a0 + a) * B + b0) * TT + 4 * c);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const unsigned r = 4 * c + j;                     // r = b*TT + t
        const unsigned b = __umulhi(r, inv_tt), t = r - b * TT;
        L[((int)t * 32 + a) * RX_PACK_PB + (int)b] = Elem<T>::from_f(v[j]);
      }
    }
  } else {
    for (int i = threadIdx.x; i < 32 * rowlen; i += RX_PACK_THREADS) {
      const int a = i / rowlen, r = i - a * rowlen;
      const int b = r / TT, t = r - b * TT;
      float v = 0.f;
      if (a0 + a < A && b0 + b < B) v = w[((size_t)(a0 + a) * B + b0) * TT + r];
      L[(t * 32 + a) * RX_PACK_PB + b] = Elem<T>::from_f(v);
    }
  }
  __syncthreads();
  if (full) {
    // ---- 16-byte stores: 4 vectors of 8 per (t, row)
    for (int v = threadIdx.x; v < TT * 128; v += RX_PACK_THREADS) {
      const int t = v >> 7, rem = v & 127, row = rem >> 2, c8 = (rem & 3) * 8;
      if (same) {   // row = a, 8 consecutive b
        const int to = flip_same ? TT - 1 - t : t;
        const u32x4 x = *reinterpret_cast<const u32x4*>(L + (t * 32 + row) * RX_PACK_PB + c8);
        *reinterpret_cast<u32x4*>(same + ((size_t)to * A + a0 + row) * B + b0 + c8) = x;
      }
      if (swp) {    // row = b, 8 consecutive a
        const int to = flip_swap ? TT - 1 - t : t;
        T vals[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) vals[j] = L[(t * 32 + c8 + j) * RX_PACK_PB + row];
        *reinterpret_cast<u32x4*>(swp + ((size_t)to * B + b0 + row) * A + a0 + c8) = *reinterpret_cast<u32x4*>(vals);
      }
    }
    return;
  }
  for (int i = threadIdx.x; i < TT * 32 * 32; i += RX_PACK_THREADS) {
    const int t = i / 1024, r = i - t * 1024;
    {
      const int a = r >> 5, b = r & 31;
      if (same && a0 + a < A && b0 + b < B) {
        const int to = flip_same ? TT - 1 - t : t;
        same[((size_t)to * A + a0 + a) * B + b0 + b] = L[(t * 32 + a) * RX_PACK_PB + b];
      }
    }
    {
      const int b = r >> 5, a = r & 31;
      if (swp && a0 + a < A && b0 + b < B) {
        const int to = flip_swap ? TT - 1 - t : t;
        swp[((size_t)to * B + b0 + b) * A + a0 + a] = L[(t * 32 + a) * RX_PACK_PB + b];
      }
    }
  }
}

// more than 27 taps (5- / 7-wide kernels, stride-3 / -4 transposed convs): the [TT][32][40] LDS tile of pack_tile does not fit;
// these layers are rare and small -- one thread per weight, coalesced reads, scattered 2-byte writes
template <typename T>
__global__ __launch_bounds__(256) void pack_naive_kernel(const float* __restrict__ w, int A, int B, int TT, T* __restrict__ same, T* __restrict__ swp) {
  const long total = (long)A * B * TT;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int t = (int)(i % TT);
    const long ab = i / TT;
    const int b = (int)(ab % B), a = (int)(ab / B);
    const T v = Elem<T>::from_f(w[i]);
    if (same) same[((long)t * A + a) * B + b] = v;
    if (swp) swp[((long)t * B + b) * A + a] = v;
  }
}
template <typename T>
static void pack_naive_launch(hipStream_t st, const float* w, int A, int B, int TT, void* same, void* swp) {
  long blocks = ((long)A * B * TT + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL((pack_naive_kernel<T>), dim3((unsigned)blocks), dim3(256), 0, st, w, A, B, TT, (T*)same, (T*)swp);
}

template <typename T>
__global__ __launch_bounds__(RX_PACK_THREADS) void pack_kernel(const float* __restrict__ w, int A, int B, int TT, unsigned inv_tt, T* __restrict__ same,
                                                   int flip_same, T* __restrict__ swp, int flip_swap) {
  pack_tile<T>(w, A, B, TT, inv_tt, same, flip_same, swp, flip_swap, blockIdx.y * 32, blockIdx.x * 32);
}

// Table-driven pack: up to RX_PM_MAX weight tensors per launch (pointer / shape table in the kernel arguments, workgroup ->
// tensor by binary search over the first-tile index, as adamw_multi_kernel does).  A cfg2 step re-packs 66 tensors; one
// launch each averaged 17 us (1.13 ms per step on the side stream, 1.5 TB/s: the small tensors are launch-bound).
#define RX_PM_MAX 40
struct PackMulti {
  const float* w[RX_PM_MAX];
  void* same[RX_PM_MAX];
  void* swp[RX_PM_MAX];
  int A[RX_PM_MAX], B[RX_PM_MAX], TT[RX_PM_MAX];
  unsigned inv_tt[RX_PM_MAX];
  int start[RX_PM_MAX + 1];       // first workgroup of tensor i; start[count] = grid size
  int count;
};

template <typename T>
__global__ __launch_bounds__(RX_PACK_THREADS) void pack_multi_kernel(const PackMulti tab) {
  int lo = 0, hi = tab.count - 1;
  const int blk = blockIdx.x;
  while (lo < hi) {               // last i with start[i] <= blk
    const int mid = (lo + hi + 1) >> 1;
    if (tab.start[mid] <= blk) lo = mid; else hi = mid - 1;
  }
  const int i = lo, local = blk - tab.start[i];
  const int nb = (tab.B[i] + 31) >> 5;
  const int ta = local / nb, tb = local - ta * nb;
  pack_tile<T>(tab.w[i], tab.A[i], tab.B[i], tab.TT[i], tab.inv_tt[i], (T*)tab.same[i], 0, (T*)tab.swp[i], 0, ta * 32, tb * 32);
}

static int pack_generic(rx_dtype dt, const float* w, int A, int B, int TT, void* same, int flip_same, void* swp, int flip_swap,
                        void* stream) {
  if (!w || A < 1 || B < 1 || TT < 1 || TT > RX_MAX_TAPS - 1) RX_FAIL(RX_EINVAL, "rx_pack: bad arguments");
  hipStream_t st = (hipStream_t)stream;
  if (TT > 27) {
    if (flip_same || flip_swap) RX_FAIL(RX_EUNSUPPORTED, "rx_pack: flipped packs exist for <= 27 taps only");
    RX_DISPATCH_DTYPE(dt, T, pack_naive_launch<T>(st, w, A, B, TT, same, swp));
    RX_CHECK_LAUNCH("rx_pack(naive)");
    return RX_OK;
  }
  RX_DISPATCH_DTYPE(dt, T, {
    size_t lds = (size_t)TT * 32 * RX_PACK_PB * sizeof(T);
    const unsigned inv_tt = (unsigned)(((1ull << 32) + TT - 1) / TT);   // r / TT == umulhi(r, inv_tt) for r < 2^16
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&pack_kernel<T>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL((pack_kernel<T>), dim3((B + 31) / 32, (A + 31) / 32), dim3(RX_PACK_THREADS), lds, st, w, A, B, TT, inv_tt, (T*)same, flip_same, (T*)swp,
                       flip_swap);
  });
  RX_CHECK_LAUNCH("rx_pack");
  return RX_OK;
}

extern "C" int rx_pack_conv_weight(rx_dtype dt, const float* w, int co, int ci, int taps, void* w_fwd, void* w_bwd, void* stream) {
  RX_RECORD(stream, [=](void* s) { return rx_pack_conv_weight(dt, w, co, ci, taps, w_fwd, w_bwd, s); });
  // w (Co,Ci,T): w_fwd[t][co][ci] = same; w_bwd[t][ci][co] = swap
  return pack_generic(dt, w, co, ci, taps, w_fwd, 0, w_bwd, 0, stream);
}
extern "C" int rx_pack_convT_weight(rx_dtype dt, const float* w, int ci, int co, int taps, void* w_fwd, void* w_bwd, void* stream) {
  RX_RECORD(stream, [=](void* s) { return rx_pack_convT_weight(dt, w, ci, co, taps, w_fwd, w_bwd, s); });
  // w (Ci,Co,T): w_fwd[t][co][ci] = swap; w_bwd[t][ci][co] = same
  return pack_generic(dt, w, ci, co, taps, w_bwd, 0, w_fwd, 0, stream);
}

// `count` weights in ceil(count / RX_PM_MAX) launches.  kind[i] 0: Conv3d weight (A = Co, B = Ci), 1: ConvTranspose3d weight
// (A = Ci, B = Co); w_fwd[i] / w_bwd[i] as in rx_pack_conv_weight / rx_pack_convT_weight (either may be NULL).  HOST arrays.
extern "C" int rx_pack_multi(rx_dtype dt, int count, const float* const* w, const int* kind, const int* A, const int* B, const int* taps,
                             void* const* w_fwd, void* const* w_bwd, void* stream) {
  if (count < 1 || !w || !kind || !A || !B || !taps || !w_fwd || !w_bwd) RX_FAIL(RX_EINVAL, "rx_pack_multi: bad arguments");
  RxRecScope rx_scope__;
  if (rx_scope__.rec) {       // host arrays: the program keeps its own copies
    std::vector<const float*> w_(w, w + count);
    std::vector<int> kind_(kind, kind + count), A_(A, A + count), B_(B, B + count), taps_(taps, taps + count);
    std::vector<void*> f_(w_fwd, w_fwd + count), b_(w_bwd, w_bwd + count);
    rx_rec_push(RxCmdFn([=](void* s) { return rx_pack_multi(dt, count, w_.data(), kind_.data(), A_.data(), B_.data(), taps_.data(), f_.data(), b_.data(), s); }),
                stream, __func__);
  }
  for (int i = 0; i < count; ++i)
    if (!w[i] || A[i] < 1 || B[i] < 1 || taps[i] < 1 || taps[i] > RX_MAX_TAPS - 1 || (kind[i] != 0 && kind[i] != 1))
      RX_FAIL(RX_EINVAL, "rx_pack_multi: bad entry %d", i);
  hipStream_t st = (hipStream_t)stream;
  {   // entries with more than 27 taps: one naive launch each, the rest goes through the table kernel
    std::vector<const float*> w2;
    std::vector<int> kind2, A2, B2, taps2;
    std::vector<void*> f2, b2;
    bool any_big = false;
    for (int i = 0; i < count; ++i) {
      if (taps[i] > 27) {
        any_big = true;
        void* same = kind[i] == 0 ? w_fwd[i] : w_bwd[i];
        void* swp = kind[i] == 0 ? w_bwd[i] : w_fwd[i];
        RX_DISPATCH_DTYPE(dt, T, pack_naive_launch<T>(st, w[i], A[i], B[i], taps[i], same, swp));
      } else {
        w2.push_back(w[i]), kind2.push_back(kind[i]), A2.push_back(A[i]), B2.push_back(B[i]), taps2.push_back(taps[i]);
        f2.push_back(w_fwd[i]), b2.push_back(w_bwd[i]);
      }
    }
    if (any_big) {
      RX_CHECK_LAUNCH("rx_pack_multi(naive)");
      if (w2.empty()) return RX_OK;
      // (the nested call must not record itself again: rx_scope__ above already pushed this whole call)
      return rx_pack_multi(dt, (int)w2.size(), w2.data(), kind2.data(), A2.data(), B2.data(), taps2.data(), f2.data(), b2.data(), stream);
    }
  }
  for (int i0 = 0; i0 < count; i0 += RX_PM_MAX) {
    PackMulti t;
    memset(&t, 0, sizeof(t));
    const int k = count - i0 < RX_PM_MAX ? count - i0 : RX_PM_MAX;
    long blocks = 0;
    int max_tt = 1;
    for (int j = 0; j < k; ++j) {
      const int i = i0 + j;
      t.w[j] = w[i], t.A[j] = A[i], t.B[j] = B[i], t.TT[j] = taps[i];
      t.inv_tt[j] = (unsigned)(((1ull << 32) + taps[i] - 1) / taps[i]);
      t.same[j] = kind[i] == 0 ? w_fwd[i] : w_bwd[i];
      t.swp[j] = kind[i] == 0 ? w_bwd[i] : w_fwd[i];
      t.start[j] = (int)blocks;
      blocks += (long)((A[i] + 31) / 32) * ((B[i] + 31) / 32);
      if (taps[i] > max_tt) max_tt = taps[i];
    }
    for (int q = k; q <= RX_PM_MAX; ++q) t.start[q] = (int)blocks;
    t.count = k;
    RX_DISPATCH_DTYPE(dt, T, {
      const size_t lds = (size_t)max_tt * 32 * RX_PACK_PB * sizeof(T);
      (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&pack_multi_kernel<T>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
      hipLaunchKernelGGL((pack_multi_kernel<T>), dim3((unsigned)blocks), dim3(RX_PACK_THREADS), lds, st, t);
    });
  }
  RX_CHECK_LAUNCH("rx_pack_multi");
  return RX_OK;
}

// ---- AdamW fused with the weight re-pack (and with gradient clipping) ------------------------------------------------
// The train step ends with clip_grad_norm_ (norm pass + a scale pass over all gradients), the optimizer update (7 fp32
// accesses per parameter) and -- at the start of the next forward -- the re-pack of every conv weight (another read of the
// parameter, two compute-dtype writes): 3.7 ms of kernel time per cfg2 step in 150 launches.  This kernel does the
// last three in ONE pass over a conv / convT weight: the pack kernel's 32 x 32 x T tile walk reads p, g, m, v, applies
// g *= clip (device scalar), the decoupled-weight-decay Adam update (torch.optim.AdamW arithmetic), writes p, m, v back and
// hands the updated tile to the transposed LDS stage of the pack.  `adamw_flat_kernel` is the same update for the
// parameters that are not packed (stem, biases, heads).  Measured: 1 ms less kernel time per step, same wall time (the
// update moves from a side-stream pack that overlapped the forward to the serial end of the step) -> opt-in.
struct AdamArgs {
  float lr, beta1, beta2, eps, weight_decay, bc1, bc2_sqrt;   // bc1 = 1 - beta1^t, bc2_sqrt = sqrt(1 - beta2^t)
  float omb1, omb2;                                            // 1 - beta, rounded from double like torch does
};

__device__ inline float adamw_update(float p, float g, float& m, float& v, const AdamArgs a) {
  p -= a.lr * a.weight_decay * p;
  m += a.omb1 * (g - m);                               // lerp(m, g, 1 - beta1)
  v = a.beta2 * v + a.omb2 * g * g;
  const float denom = sqrtf(v) / a.bc2_sqrt + a.eps;
  return p - (a.lr / a.bc1) * (m / denom);
}

// The packed copies must be the cast of the STORED fp32 weight -- what a later re-pack of that weight writes.  Left alone, the f16
// kernel evaluates the last FMA of the update a second time as v_fma_mixlo_f16, which rounds the unrounded result to f16 once:
// one f16 ulp away from the cast of the fp32 value wherever that value is a rounding tie (3 of 25920 elements of a 40 x 24 x 27
// weight).  The empty statement makes the rounded fp32 value the only thing the conversion can see.
__device__ __forceinline__ float stored_f32(float x) {
  asm("" : "+v"(x));
  return x;
}

template <typename T>
__global__ __launch_bounds__(256) void adamw_pack_kernel(float* __restrict__ w, const float* __restrict__ grad, float* __restrict__ m,
                                                         float* __restrict__ v, const float* __restrict__ clip, const AdamArgs aa, int A,
                                                         int B, int TT, unsigned inv_tt, T* __restrict__ same, T* __restrict__ swp) {
  extern __shared__ __attribute__((aligned(16))) unsigned char pack_smem[];
  T* L = reinterpret_cast<T*>(pack_smem);               // [TT][32 a][RX_PACK_PB]
  const int a0 = blockIdx.y * 32, b0 = blockIdx.x * 32;
  const int rowlen = 32 * TT;
  const float cs = clip ? *clip : 1.f;
  const bool full = a0 + 32 <= A && b0 + 32 <= B && sizeof(T) == 2 && (B & 7) == 0 && (A & 7) == 0;
  if (full && TT > 1 && (rowlen & 3) == 0 && ((size_t)B * TT & 3) == 0) {
    const int q4 = rowlen >> 2;
    for (int q = threadIdx.x; q < 32 * q4; q += 256) {
      const int a = q / q4, c = q - a * q4;
      const size_t off = ((size_t)(a0 + a) * B + b0) * TT + 4 * c;
      f32x4 pw = *reinterpret_cast<const f32x4*>(w + off);
      const f32x4 pg = *reinterpret_cast<const f32x4*>(grad + off);
      f32x4 pm = *reinterpret_cast<const f32x4*>(m + off), pv = *reinterpret_cast<const f32x4*>(v + off);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float mj = pm[j], vj = pv[j];
        pw[j] = stored_f32(adamw_update(pw[j], pg[j] * cs, mj, vj, aa));
        pm[j] = mj, pv[j] = vj;
      }
      *reinterpret_cast<f32x4*>(w + off) = pw;
      *reinterpret_cast<f32x4*>(m + off) = pm;
      *reinterpret_cast<f32x4*>(v + off) = pv;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const unsigned r = 4 * c + j;
        const unsigned b = __umulhi(r, inv_tt), t = r - b * TT;
        L[((int)t * 32 + a) * RX_PACK_PB + (int)b] = Elem<T>::from_f(pw[j]);
      }
    }
  } else {
    for (int i = threadIdx.x; i < 32 * rowlen; i += 256) {
      const int a = i / rowlen, r = i - a * rowlen;
      const int b = r / TT, t = r - b * TT;
      float nw = 0.f;
      if (a0 + a < A && b0 + b < B) {
        const size_t off = ((size_t)(a0 + a) * B + b0) * TT + r;
        float mj = m[off], vj = v[off];
        nw = stored_f32(adamw_update(w[off], grad[off] * cs, mj, vj, aa));
        w[off] = nw, m[off] = mj, v[off] = vj;
      }
      L[(t * 32 + a) * RX_PACK_PB + b] = Elem<T>::from_f(nw);
    }
  }
  __syncthreads();
  if (full) {
    for (int vv = threadIdx.x; vv < TT * 128; vv += 256) {
      const int t = vv >> 7, rem = vv & 127, row = rem >> 2, c8 = (rem & 3) * 8;
      if (same) {
        const u32x4 x = *reinterpret_cast<const u32x4*>(L + (t * 32 + row) * RX_PACK_PB + c8);
        *reinterpret_cast<u32x4*>(same + ((size_t)t * A + a0 + row) * B + b0 + c8) = x;
      }
      if (swp) {
        T vals[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) vals[j] = L[(t * 32 + c8 + j) * RX_PACK_PB + row];
        *reinterpret_cast<u32x4*>(swp + ((size_t)t * B + b0 + row) * A + a0 + c8) = *reinterpret_cast<u32x4*>(vals);
      }
    }
    return;
  }
  for (int i = threadIdx.x; i < TT * 32 * 32; i += 256) {
    const int t = i / 1024, r = i - t * 1024;
    {
      const int a = r >> 5, b = r & 31;
      if (same && a0 + a < A && b0 + b < B) same[((size_t)t * A + a0 + a) * B + b0 + b] = L[(t * 32 + a) * RX_PACK_PB + b];
    }
    {
      const int b = r >> 5, a = r & 31;
      if (swp && a0 + a < A && b0 + b < B) swp[((size_t)t * B + b0 + b) * A + a0 + a] = L[(t * 32 + a) * RX_PACK_PB + b];
    }
  }
}

__global__ __launch_bounds__(256) void adamw_flat_kernel(float* __restrict__ w, const float* __restrict__ grad, float* __restrict__ m,
                                                         float* __restrict__ v, const float* __restrict__ clip, const AdamArgs aa, long n) {
  const float cs = clip ? *clip : 1.f;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    float mj = m[i], vj = v[i];
    w[i] = adamw_update(w[i], grad[i] * cs, mj, vj, aa);
    m[i] = mj, v[i] = vj;
  }
}

static AdamArgs adam_args(double lr, double beta1, double beta2, double eps, double wd, int step) {
  AdamArgs a;
  a.lr = (float)lr, a.beta1 = (float)beta1, a.beta2 = (float)beta2, a.eps = (float)eps, a.weight_decay = (float)wd;
  a.omb1 = (float)(1.0 - beta1), a.omb2 = (float)(1.0 - beta2);
  a.bc1 = (float)(1.0 - pow(beta1, (double)step));
  a.bc2_sqrt = (float)sqrt(1.0 - pow(beta2, (double)step));
  return a;
}

// p (A,B,T) fp32 conv weight (kind 0: A = Co, B = Ci -> w_fwd = [t][A][B], w_bwd = [t][B][A]; kind 1: transposed conv,
// A = Ci, B = Co -> w_bwd = [t][A][B], w_fwd = [t][B][A]).  `clip` = optional device scalar multiplied into the gradient.
extern "C" int rx_adamw_pack(rx_dtype dt, float* p, const float* grad, float* exp_avg, float* exp_avg_sq, const float* clip, double lr,
                             double beta1, double beta2, double eps, double weight_decay, int step, int kind, int A, int B, int taps,
                             void* w_fwd, void* w_bwd, void* stream) {
  if (!p || !grad || !exp_avg || !exp_avg_sq || A < 1 || B < 1 || taps < 1 || taps > 27 || step < 1)
    RX_FAIL(RX_EINVAL, "rx_adamw_pack: bad arguments");
  hipStream_t st = (hipStream_t)stream;
  const AdamArgs aa = adam_args(lr, beta1, beta2, eps, weight_decay, step);
  void* same = kind == 0 ? w_fwd : w_bwd;
  void* swp = kind == 0 ? w_bwd : w_fwd;
  RX_DISPATCH_DTYPE(dt, T, {
    size_t lds = (size_t)taps * 32 * RX_PACK_PB * sizeof(T);
    const unsigned inv_tt = (unsigned)(((1ull << 32) + taps - 1) / taps);
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&adamw_pack_kernel<T>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL((adamw_pack_kernel<T>), dim3((B + 31) / 32, (A + 31) / 32), dim3(256), lds, st, p, grad, exp_avg, exp_avg_sq, clip, aa,
                       A, B, taps, inv_tt, (T*)same, (T*)swp);
  });
  RX_CHECK_LAUNCH("rx_adamw_pack");
  return RX_OK;
}

extern "C" int rx_adamw_flat(float* p, const float* grad, float* exp_avg, float* exp_avg_sq, const float* clip, double lr, double beta1,
                             double beta2, double eps, double weight_decay, int step, long n, void* stream) {
  if (!p || !grad || !exp_avg || !exp_avg_sq || n < 1 || step < 1) RX_FAIL(RX_EINVAL, "rx_adamw_flat: bad arguments");
  const AdamArgs aa = adam_args(lr, beta1, beta2, eps, weight_decay, step);
  long blocks = (n + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(adamw_flat_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, p, grad, exp_avg, exp_avg_sq, clip, aa, n);
  RX_CHECK_LAUNCH("rx_adamw_flat");
  return RX_OK;
}

// the same update for a LIST of tensors that share hyper-parameters and step count (one optimizer param group): one call from
// the host language instead of one per parameter, and ONE launch per 48 tensors instead of one each.  cfg2 has 69 un-packed
// ... and, with RX_ENGINE_ADAMW=2, every conv weight too: 102 M parameters x 28 B (read p, g, m, v; write p, m, v) = 2.9 GB,
// 0.36 ms at 8 TB/s.  One scalar-load launch per tensor took 1.29 ms per step (18.7 us average over 69 launches: the small
// ones are launch-bound, the large ones ran 4-byte loads); the table kernel below runs 4 x 16-byte loads per array per thread,
// all 16 issued before the first use.  Pointer arrays are HOST arrays.
#define RX_AM_MAX 48
#define RX_AM_CHUNK 4096          // elements per workgroup: 256 threads x 4 float4
struct AdamMulti {
  float* p[RX_AM_MAX];
  const float* g[RX_AM_MAX];
  float* m[RX_AM_MAX];
  float* v[RX_AM_MAX];
  long n[RX_AM_MAX];
  int start[RX_AM_MAX + 1];       // first workgroup of tensor i; start[count] = grid size
  int count;
};

__global__ __launch_bounds__(256) void adamw_multi_kernel(const AdamMulti t, const float* __restrict__ clip, const AdamArgs aa) {
  const int b = blockIdx.x;
  int lo = 0, hi = t.count;       // start[lo] <= b < start[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (t.start[mid] <= b) lo = mid; else hi = mid;
  }
  const long base = (long)(b - t.start[lo]) * RX_AM_CHUNK;
  const long n = t.n[lo];
  float* __restrict__ w = t.p[lo];
  const float* __restrict__ grad = t.g[lo];
  float* __restrict__ m = t.m[lo];
  float* __restrict__ v = t.v[lo];
  const float cs = clip ? *clip : 1.f;
  const bool vec = (((uintptr_t)w | (uintptr_t)grad | (uintptr_t)m | (uintptr_t)v) & 15) == 0;
  if (vec && base + RX_AM_CHUNK <= n) {
    f32x4 pw[4], pg[4], pm[4], pv[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const long i = base + (long)(j * 256 + threadIdx.x) * 4;
      pw[j] = *reinterpret_cast<const f32x4*>(w + i);
      pg[j] = *reinterpret_cast<const f32x4*>(grad + i);
      pm[j] = *reinterpret_cast<const f32x4*>(m + i);
      pv[j] = *reinterpret_cast<const f32x4*>(v + i);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const long i = base + (long)(j * 256 + threadIdx.x) * 4;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        float mj = pm[j][k], vj = pv[j][k];
        pw[j][k] = adamw_update(pw[j][k], pg[j][k] * cs, mj, vj, aa);
        pm[j][k] = mj, pv[j][k] = vj;
      }
      *reinterpret_cast<f32x4*>(w + i) = pw[j];
      *reinterpret_cast<f32x4*>(m + i) = pm[j];
      *reinterpret_cast<f32x4*>(v + i) = pv[j];
    }
    return;
  }
  const long end = base + RX_AM_CHUNK < n ? base + RX_AM_CHUNK : n;
  for (long i = base + threadIdx.x; i < end; i += 256) {
    float mj = m[i], vj = v[i];
    w[i] = adamw_update(w[i], grad[i] * cs, mj, vj, aa);
    m[i] = mj, v[i] = vj;
  }
}

extern "C" int rx_adamw_flat_multi(int count, float* const* p, const float* const* grad, float* const* exp_avg, float* const* exp_avg_sq,
                                   const long* numel, const float* clip, double lr, double beta1, double beta2, double eps,
                                   double weight_decay, int step, void* stream) {
  if (count < 0 || (count > 0 && (!p || !grad || !exp_avg || !exp_avg_sq || !numel)) || step < 1) RX_FAIL(RX_EINVAL, "rx_adamw_flat_multi: bad arguments");
  const AdamArgs aa = adam_args(lr, beta1, beta2, eps, weight_decay, step);
  for (int i = 0; i < count; ++i)
    if (!p[i] || !grad[i] || !exp_avg[i] || !exp_avg_sq[i] || numel[i] < 1) RX_FAIL(RX_EINVAL, "rx_adamw_flat_multi: bad tensor %d", i);
  for (int i0 = 0; i0 < count;) {
    AdamMulti t;
    int k = 0;
    long blocks = 0;
    for (; i0 + k < count && k < RX_AM_MAX; ++k) {
      const long nb = (numel[i0 + k] + RX_AM_CHUNK - 1) / RX_AM_CHUNK;
      if (blocks + nb > 0x3fffffffL) break;           // keep the grid inside int range
      t.p[k] = p[i0 + k], t.g[k] = grad[i0 + k], t.m[k] = exp_avg[i0 + k], t.v[k] = exp_avg_sq[i0 + k], t.n[k] = numel[i0 + k];
      t.start[k] = (int)blocks;
      blocks += nb;
    }
    if (k == 0) RX_FAIL(RX_EINVAL, "rx_adamw_flat_multi: tensor %d too large", i0);
    for (int q = k; q <= RX_AM_MAX; ++q) t.start[q] = (int)blocks;
    for (int q = k; q < RX_AM_MAX; ++q) t.p[q] = nullptr, t.g[q] = nullptr, t.m[q] = nullptr, t.v[q] = nullptr, t.n[q] = 0;
    t.count = k;
    hipLaunchKernelGGL(adamw_multi_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, t, clip, aa);
    i0 += k;
  }
  RX_CHECK_LAUNCH("rx_adamw_flat_multi");
  return RX_OK;
}

// ---- SGD with momentum / Nesterov (torch.optim.SGD arithmetic, `_single_tensor_sgd`) -----------------------------------------
// The reference's other optimizer (train.py:70-77: SGD(momentum=0.9, nesterov=True)).  Same two shapes as AdamW above: a table
// kernel over the un-packed parameters and a tile-walk kernel that also rewrites both packed copies of a conv / convT weight.
//   g' = g * clip;  d = wd != 0 ? g' + wd * p : g';  buf = first ? d : mu * buf + (1 - dampening) * d;
//   u = nesterov ? d + mu * buf : buf  (mu == 0: u = d, no buffer);  p -= lr * u
// 16 bytes per parameter with momentum (read p, g, buf; write p, buf; 12 on a first step, which only writes buf), 12 without.
struct SgdArgs {
  float lr, mu, omd, wd;          // omd = 1 - dampening, formed in double and cast once
  int nesterov, first;            // first: no momentum buffer yet -- buf is written, never read
};

template <bool MOM>
__device__ inline float sgd_update(float p, float g, float& buf, const SgdArgs a) {
  const float d = a.wd != 0.f ? g + a.wd * p : g;
  float u = d;
  if (MOM) {
    buf = a.first ? d : a.mu * buf + a.omd * d;
    u = a.nesterov ? d + a.mu * buf : buf;
  }
  return p - a.lr * u;
}

static SgdArgs sgd_args(double lr, double momentum, double dampening, double wd, int nesterov, int first) {
  SgdArgs a;
  a.lr = (float)lr, a.mu = (float)momentum, a.omd = (float)(1.0 - dampening), a.wd = (float)wd;
  a.nesterov = nesterov != 0, a.first = first != 0;
  return a;
}

static bool sgd_hypers_bad(double momentum, double dampening, int nesterov) {
  return nesterov && (momentum <= 0.0 || dampening != 0.0);
}

// the store half of the pack tile walk for a tile that is already in LDS as [t][32 a][RX_PACK_PB] (what adamw_pack_kernel does
// after its barrier), for any thread count
template <typename T, int THREADS>
__device__ __forceinline__ void pack_tile_store(const T* __restrict__ L, int A, int B, int TT, int a0, int b0, bool full,
                                                T* __restrict__ same, T* __restrict__ swp) {
  if (full) {
    for (int vv = threadIdx.x; vv < TT * 128; vv += THREADS) {
      const int t = vv >> 7, rem = vv & 127, row = rem >> 2, c8 = (rem & 3) * 8;
      if (same) {
        const u32x4 x = *reinterpret_cast<const u32x4*>(L + (t * 32 + row) * RX_PACK_PB + c8);
        *reinterpret_cast<u32x4*>(same + ((size_t)t * A + a0 + row) * B + b0 + c8) = x;
      }
      if (swp) {
        T vals[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) vals[j] = L[(t * 32 + c8 + j) * RX_PACK_PB + row];
        *reinterpret_cast<u32x4*>(swp + ((size_t)t * B + b0 + row) * A + a0 + c8) = *reinterpret_cast<u32x4*>(vals);
      }
    }
    return;
  }
  for (int i = threadIdx.x; i < TT * 32 * 32; i += THREADS) {
    const int t = i / 1024, r = i - t * 1024;
    {
      const int a = r >> 5, b = r & 31;
      if (same && a0 + a < A && b0 + b < B) same[((size_t)t * A + a0 + a) * B + b0 + b] = L[(t * 32 + a) * RX_PACK_PB + b];
    }
    {
      const int b = r >> 5, a = r & 31;
      if (swp && a0 + a < A && b0 + b < B) swp[((size_t)t * B + b0 + b) * A + a0 + a] = L[(t * 32 + a) * RX_PACK_PB + b];
    }
  }
}

// (the packed values are the cast of stored_f32(p'): the last multiply-subtract of sgd_update has the same f16 tie hazard as AdamW's)
template <typename T, bool MOM>
__global__ __launch_bounds__(256) void sgd_pack_kernel(float* __restrict__ w, const float* __restrict__ grad, float* __restrict__ buf,
                                                       const float* __restrict__ clip, const SgdArgs aa, int A, int B, int TT,
                                                       unsigned inv_tt, T* __restrict__ same, T* __restrict__ swp) {
  extern __shared__ __attribute__((aligned(16))) unsigned char pack_smem[];
  T* L = reinterpret_cast<T*>(pack_smem);               // [TT][32 a][RX_PACK_PB]
  const int a0 = blockIdx.y * 32, b0 = blockIdx.x * 32;
  const int rowlen = 32 * TT;
  const float cs = clip ? *clip : 1.f;
  const bool rd = MOM && !aa.first;
  const bool full = a0 + 32 <= A && b0 + 32 <= B && sizeof(T) == 2 && (B & 7) == 0 && (A & 7) == 0;
  if (full && TT > 1 && (rowlen & 3) == 0 && ((size_t)B * TT & 3) == 0) {
    const int q4 = rowlen >> 2;
    for (int q = threadIdx.x; q < 32 * q4; q += 256) {
      const int a = q / q4, c = q - a * q4;
      const size_t off = ((size_t)(a0 + a) * B + b0) * TT + 4 * c;
      f32x4 pw = *reinterpret_cast<const f32x4*>(w + off);
      const f32x4 pg = *reinterpret_cast<const f32x4*>(grad + off);
      f32x4 pb = f32x4{0.f, 0.f, 0.f, 0.f};
      if (rd) pb = *reinterpret_cast<const f32x4*>(buf + off);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float bj = pb[j];
        pw[j] = stored_f32(sgd_update<MOM>(pw[j], pg[j] * cs, bj, aa));
        pb[j] = bj;
      }
      *reinterpret_cast<f32x4*>(w + off) = pw;
      if (MOM) *reinterpret_cast<f32x4*>(buf + off) = pb;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const unsigned r = 4 * c + j;
        const unsigned b = __umulhi(r, inv_tt), t = r - b * TT;
        L[((int)t * 32 + a) * RX_PACK_PB + (int)b] = Elem<T>::from_f(pw[j]);
      }
    }
  } else {
    for (int i = threadIdx.x; i < 32 * rowlen; i += 256) {
      const int a = i / rowlen, r = i - a * rowlen;
      const int b = r / TT, t = r - b * TT;
      float nw = 0.f;
      if (a0 + a < A && b0 + b < B) {
        const size_t off = ((size_t)(a0 + a) * B + b0) * TT + r;
        float bj = rd ? buf[off] : 0.f;
        nw = stored_f32(sgd_update<MOM>(w[off], grad[off] * cs, bj, aa));
        w[off] = nw;
        if (MOM) buf[off] = bj;
      }
      L[(t * 32 + a) * RX_PACK_PB + b] = Elem<T>::from_f(nw);
    }
  }
  __syncthreads();
  pack_tile_store<T, 256>(L, A, B, TT, a0, b0, full, same, swp);
}

// p (A,B,T), kind, w_fwd / w_bwd as in rx_adamw_pack.  `buf` = momentum buffer (NULL iff momentum == 0); `first` != 0: the
// buffer does not exist yet and is written with d (torch: clone of the first gradient), never read.
extern "C" int rx_sgd_pack(rx_dtype dt, float* p, const float* grad, float* buf, const float* clip, double lr, double momentum,
                           double dampening, double weight_decay, int nesterov, int first, int kind, int A, int B, int taps,
                           void* w_fwd, void* w_bwd, void* stream) {
  const bool mom = momentum != 0.0;
  if (!p || !grad || (mom && !buf) || A < 1 || B < 1 || taps < 1 || taps > 27 || sgd_hypers_bad(momentum, dampening, nesterov))
    RX_FAIL(RX_EINVAL, "rx_sgd_pack: bad arguments");
  hipStream_t st = (hipStream_t)stream;
  const SgdArgs aa = sgd_args(lr, momentum, dampening, weight_decay, nesterov, first);
  void* same = kind == 0 ? w_fwd : w_bwd;
  void* swp = kind == 0 ? w_bwd : w_fwd;
  RX_DISPATCH_DTYPE(dt, T, {
    size_t lds = (size_t)taps * 32 * RX_PACK_PB * sizeof(T);
    const unsigned inv_tt = (unsigned)(((1ull << 32) + taps - 1) / taps);
    if (mom) {
      (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&sgd_pack_kernel<T, true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
      hipLaunchKernelGGL((sgd_pack_kernel<T, true>), dim3((B + 31) / 32, (A + 31) / 32), dim3(256), lds, st, p, grad, buf, clip, aa, A, B,
                         taps, inv_tt, (T*)same, (T*)swp);
    } else {
      (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&sgd_pack_kernel<T, false>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
      hipLaunchKernelGGL((sgd_pack_kernel<T, false>), dim3((B + 31) / 32, (A + 31) / 32), dim3(256), lds, st, p, grad, (float*)nullptr, clip,
                         aa, A, B, taps, inv_tt, (T*)same, (T*)swp);
    }
  });
  RX_CHECK_LAUNCH("rx_sgd_pack");
  return RX_OK;
}

// the AdamMulti table shape for SGD: 48 tensors per launch, one workgroup per 4096 elements, four 16-byte loads per array per
// thread, all issued before the first use; scalar path for a misaligned pointer or a tail chunk
struct SgdMulti {
  float* p[RX_AM_MAX];
  const float* g[RX_AM_MAX];
  float* buf[RX_AM_MAX];
  long n[RX_AM_MAX];
  int start[RX_AM_MAX + 1];       // first workgroup of tensor i; start[count] = grid size
  int count;
};

template <bool MOM>
__global__ __launch_bounds__(256) void sgd_multi_kernel(const SgdMulti t, const float* __restrict__ clip, const SgdArgs aa) {
  const int b = blockIdx.x;
  int lo = 0, hi = t.count;       // start[lo] <= b < start[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (t.start[mid] <= b) lo = mid; else hi = mid;
  }
  const long base = (long)(b - t.start[lo]) * RX_AM_CHUNK;
  const long n = t.n[lo];
  float* __restrict__ w = t.p[lo];
  const float* __restrict__ grad = t.g[lo];
  float* __restrict__ buf = MOM ? t.buf[lo] : nullptr;
  const float cs = clip ? *clip : 1.f;
  const bool rd = MOM && !aa.first;
  const bool vec = (((uintptr_t)w | (uintptr_t)grad | (uintptr_t)buf) & 15) == 0;
  if (vec && base + RX_AM_CHUNK <= n) {
    f32x4 pw[4], pg[4], pb[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const long i = base + (long)(j * 256 + threadIdx.x) * 4;
      pw[j] = *reinterpret_cast<const f32x4*>(w + i);
      pg[j] = *reinterpret_cast<const f32x4*>(grad + i);
      pb[j] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (rd) pb[j] = *reinterpret_cast<const f32x4*>(buf + i);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const long i = base + (long)(j * 256 + threadIdx.x) * 4;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        float bj = pb[j][k];
        pw[j][k] = sgd_update<MOM>(pw[j][k], pg[j][k] * cs, bj, aa);
        pb[j][k] = bj;
      }
      *reinterpret_cast<f32x4*>(w + i) = pw[j];
      if (MOM) *reinterpret_cast<f32x4*>(buf + i) = pb[j];
    }
    return;
  }
  const long end = base + RX_AM_CHUNK < n ? base + RX_AM_CHUNK : n;
  for (long i = base + threadIdx.x; i < end; i += 256) {
    float bj = rd ? buf[i] : 0.f;
    w[i] = sgd_update<MOM>(w[i], grad[i] * cs, bj, aa);
    if (MOM) buf[i] = bj;
  }
}

// `count` tensors of one param group that share `first` (all have a momentum buffer, or none has one yet).  `buf` is NULL
// iff momentum == 0.  Pointer arrays are HOST arrays.
extern "C" int rx_sgd_flat_multi(int count, float* const* p, const float* const* grad, float* const* buf, const long* numel,
                                 const float* clip, double lr, double momentum, double dampening, double weight_decay, int nesterov,
                                 int first, void* stream) {
  const bool mom = momentum != 0.0;
  if (count < 0 || (count > 0 && (!p || !grad || !numel || (mom && !buf))) || sgd_hypers_bad(momentum, dampening, nesterov))
    RX_FAIL(RX_EINVAL, "rx_sgd_flat_multi: bad arguments");
  const SgdArgs aa = sgd_args(lr, momentum, dampening, weight_decay, nesterov, first);
  for (int i = 0; i < count; ++i)
    if (!p[i] || !grad[i] || (mom && !buf[i]) || numel[i] < 1) RX_FAIL(RX_EINVAL, "rx_sgd_flat_multi: bad tensor %d", i);
  for (int i0 = 0; i0 < count;) {
    SgdMulti t;
    int k = 0;
    long blocks = 0;
    for (; i0 + k < count && k < RX_AM_MAX; ++k) {
      const long nb = (numel[i0 + k] + RX_AM_CHUNK - 1) / RX_AM_CHUNK;
      if (blocks + nb > 0x3fffffffL) break;           // keep the grid inside int range
      t.p[k] = p[i0 + k], t.g[k] = grad[i0 + k], t.buf[k] = mom ? buf[i0 + k] : nullptr, t.n[k] = numel[i0 + k];
      t.start[k] = (int)blocks;
      blocks += nb;
    }
    if (k == 0) RX_FAIL(RX_EINVAL, "rx_sgd_flat_multi: tensor %d too large", i0);
    for (int q = k; q <= RX_AM_MAX; ++q) t.start[q] = (int)blocks;
    for (int q = k; q < RX_AM_MAX; ++q) t.p[q] = nullptr, t.g[q] = nullptr, t.buf[q] = nullptr, t.n[q] = 0;
    t.count = k;
    if (mom)
      hipLaunchKernelGGL(sgd_multi_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, t, clip, aa);
    else
      hipLaunchKernelGGL(sgd_multi_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, t, clip, aa);
    i0 += k;
  }
  RX_CHECK_LAUNCH("rx_sgd_flat_multi");
  return RX_OK;
}

// ---- global gradient norm + clip coefficient (torch.nn.utils.clip_grad_norm_, train.py:227) as two launches ---------------
// torch's path is _foreach_norm (one multi-tensor launch per ~20 tensors: 10 launches of 24 us at cfg2) + stack + vector_norm +
// the scalar arithmetic of the coefficient: ~20 launches at the serial end of a step.  Here: the AdamW table layout (48 tensors
// per launch, one workgroup per 4096 elements) writes one fp32 sum of squares per workgroup, and a single workgroup adds them
// in fp64 in a fixed order (deterministic) and leaves (norm, min(1, max_norm / (norm + 1e-6))) behind.
struct SqnormMulti {
  const float* g[RX_AM_MAX];
  long n[RX_AM_MAX];
  int start[RX_AM_MAX + 1];
  int count;
};

__global__ __launch_bounds__(256) void sqnorm_multi_kernel(const SqnormMulti t, float* __restrict__ partial) {
  __shared__ float red[4];
  const int b = blockIdx.x;
  int lo = 0, hi = t.count;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (t.start[mid] <= b) lo = mid; else hi = mid;
  }
  const long base = (long)(b - t.start[lo]) * RX_AM_CHUNK;
  const long n = t.n[lo];
  const float* __restrict__ g = t.g[lo];
  float s = 0.f;
  if ((((uintptr_t)g) & 15) == 0 && base + RX_AM_CHUNK <= n) {
    f32x4 v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = *reinterpret_cast<const f32x4*>(g + base + (long)(j * 256 + threadIdx.x) * 4);
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int k = 0; k < 4; ++k) s += v[j][k] * v[j][k];
  } else {
    const long end = base + RX_AM_CHUNK < n ? base + RX_AM_CHUNK : n;
    for (long i = base + threadIdx.x; i < end; i += 256) s += g[i] * g[i];
  }
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) partial[b] = (red[0] + red[1]) + (red[2] + red[3]);
}

// (one workgroup of 1024 threads, eight loads in flight per thread: the 52 K partials of cfg2 took 64 us as a 256-thread serial
// load chain at the serial end of the step; the summation order stays fixed)
__global__ __launch_bounds__(1024) void sqnorm_finalize_kernel(const float* __restrict__ partial, int nblocks, float max_norm,
                                                               float* __restrict__ out /* [2]: norm, clip coefficient */) {
  __shared__ double red[1024];
  double s[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  int i = threadIdx.x;
  for (; i + 7 * 1024 < nblocks; i += 8 * 1024) {
    float v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = partial[i + u * 1024];
#pragma unroll
    for (int u = 0; u < 8; ++u) s[u] += (double)v[u];
  }
  for (; i < nblocks; i += 1024) s[0] += (double)partial[i];
  red[threadIdx.x] = ((s[0] + s[1]) + (s[2] + s[3])) + ((s[4] + s[5]) + (s[6] + s[7]));
  __syncthreads();
  for (int o = 512; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const float norm = (float)sqrt(red[0]);
    const float coef = max_norm / (norm + 1e-6f);
    out[0] = norm;
    out[1] = coef < 1.f ? coef : 1.f;
  }
}

// number of fp32 partials rx_grad_norm_clip needs for these tensor sizes
extern "C" long rx_grad_norm_clip_partials(int count, const long* numel) {
  long blocks = 0;
  for (int i = 0; i < count; ++i) blocks += (numel[i] + RX_AM_CHUNK - 1) / RX_AM_CHUNK;
  return blocks;
}

// out[0] = || (g_0, ..., g_{count-1}) ||_2, out[1] = min(1, max_norm / (out[0] + 1e-6)).  `partial`: device scratch of
// rx_grad_norm_clip_partials() floats.  Pointer arrays are HOST arrays.
extern "C" int rx_grad_norm_clip(int count, const float* const* grad, const long* numel, float max_norm, float* partial, long partial_len,
                                 float* out, void* stream) {
  if (count < 1 || !grad || !numel || !partial || !out) RX_FAIL(RX_EINVAL, "rx_grad_norm_clip: bad arguments");
  const long need = rx_grad_norm_clip_partials(count, numel);
  if (need > partial_len || need > 0x3fffffffL) RX_FAIL(RX_EWORKSPACE, "rx_grad_norm_clip: %ld partials needed, %ld given", need, partial_len);
  long done = 0;
  for (int i0 = 0; i0 < count;) {
    SqnormMulti t;
    int k = 0;
    long blocks = 0;
    for (; i0 + k < count && k < RX_AM_MAX; ++k) {
      if (!grad[i0 + k] || numel[i0 + k] < 1) RX_FAIL(RX_EINVAL, "rx_grad_norm_clip: bad tensor %d", i0 + k);
      t.g[k] = grad[i0 + k], t.n[k] = numel[i0 + k];
      t.start[k] = (int)blocks;
      blocks += (numel[i0 + k] + RX_AM_CHUNK - 1) / RX_AM_CHUNK;
    }
    for (int q = k; q <= RX_AM_MAX; ++q) t.start[q] = (int)blocks;
    for (int q = k; q < RX_AM_MAX; ++q) t.g[q] = nullptr, t.n[q] = 0;
    t.count = k;
    hipLaunchKernelGGL(sqnorm_multi_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, t, partial + done);
    done += blocks;
    i0 += k;
  }
  hipLaunchKernelGGL(sqnorm_finalize_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, (const float*)partial, (int)done, max_norm, out);
  RX_CHECK_LAUNCH("rx_grad_norm_clip");
  return RX_OK;
}
