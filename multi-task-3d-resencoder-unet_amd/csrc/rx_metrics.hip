// rx_metrics.hip -- validation metrics on the device: the counts and sums behind Dice / IoU / precision / recall and the angular error
// of a normals head, each from ONE read of the prediction and the target (host side training/metrics/metrics.py, whose
// seg_counts_numpy, class_counts_numpy and normal_stats_numpy are the statements).  Operands are contiguous (N, C, V): the
// prediction fp32, bf16 or fp16, the target fp32 (or int64 class indices).  Every entry point ADDS into the caller's buffers, so
// an epoch of validation batches accumulates with no extra kernel and no synchronisation.
//
//   seg_counts_kernel<T>     a row = one (sample, channel); counts (TP, FP, FN) of pred > thr_pred against target > thr_target.
//   class_counts_kernel<T>   a row group = one sample; per voxel the arg-max over C channel rows V apart, of the prediction and of
//                            the label; per-class (TP, FP, FN) in LDS (RX_MET_REP copies, picked by lane, so the lanes of a wave
//                            that meet on one class spread over several words), then one atomic per workgroup and output word.
//   normal_stats_kernel<T>   3-channel fields; the masked voxels (integer atomic) and the fp64 sums of cos and of the angle in
//                            degrees, written as per-workgroup partials; normal_stats_finalize_kernel adds a sample's partials in
//                            index order in fp64 and adds the result into `sums`.
//
// Reading a row: a scalar head up to the first 16-byte boundary of the PREDICTION row, then `units` of 16 prediction bytes (P = 4
// or 8 voxels), then a scalar tail.  The prediction's units are aligned 16-byte loads.  Everything else that belongs to the same
// voxels -- the target, and in the channel kernels the other channel rows, which start V elements further on -- is loaded through a
// struct that promises only its element's alignment (MetRun): for 4- and 8-byte elements that is still one 16-byte load
// instruction (multi-dword global loads need dword alignment only), aligned whenever the rows share the head's alignment; for
// 16-bit channel rows that do not (V % 8 != 0) the compiler splits it into narrower loads, behind a launch-uniform branch.
// Nothing outside [0, V) of a row is read; every offset is 64-bit.
// Integer reductions: lane, wave (xor shuffles), workgroup (LDS), then one 64-bit atomic add per workgroup and output word --
// order-free, so the counts are bit-reproducible.  No float ever goes through an atomic.
// Contraction is off: every fp32 product and sum of the normals formula rounds once, as the float32 evaluation the tests bound
// the kernel with.
#include "rx_common.h"

#pragma clang fp contract(off)

#define RX_MET_BLOCK 256
#define RX_MET_WAVES (RX_MET_BLOCK / 64)
#define RX_MET_TARGET_BLOCKS 4096      // large calls are cut into about this many chunks (16 per CU)
#define RX_MET_MIN_UNITS 1024          // ... and no chunk of a row kernel is below this many 16-byte units (16 KiB of prediction)
#define RX_MET_REP 16                  // copies of the per-class counters in LDS
#define RX_MET_MAXC 64
#define RX_NS_MAX_CHUNKS 512           // partials per sample of rx_normal_stats

// P elements that promise only the alignment of one element
template <typename E, int P>
struct MetRun {
  E v[P];
};

// one unit of the prediction; `al16` (launch-uniform): the address is known to be 16-byte aligned
template <typename T>
__device__ inline void met_load_pred(const T* __restrict__ p, bool al16, float (&o)[Elem<T>::PER16]) {
  constexpr int P = Elem<T>::PER16;
  if (al16) {
    const Vec16<T> r = ld16(p);
#pragma unroll
    for (int j = 0; j < P; ++j) o[j] = Elem<T>::to_f(r.v[j]);
  } else {
    const MetRun<T, P> r = *reinterpret_cast<const MetRun<T, P>*>(p);
#pragma unroll
    for (int j = 0; j < P; ++j) o[j] = Elem<T>::to_f(r.v[j]);
  }
}
template <int P>
__device__ inline void met_load_f32(const float* __restrict__ p, float (&o)[P]) {
  const MetRun<float, P> r = *reinterpret_cast<const MetRun<float, P>*>(p);
#pragma unroll
  for (int j = 0; j < P; ++j) o[j] = r.v[j];
}

// voxels of a row before the first 16-byte boundary (at most V)
template <typename T>
__device__ inline long met_head(const T* row, long V) {
  const long h = (long)(((16u - (unsigned)((uintptr_t)row & 15u)) & 15u) / (unsigned)sizeof(T));
  return h < V ? h : V;
}

// NW integer words of every thread -> out[w] in thread 0 (all threads must call)
template <int NW>
__device__ inline void met_block_sum(unsigned (&c)[NW], unsigned long long (&out)[NW]) {
  __shared__ unsigned s_red[RX_MET_WAVES][NW];
#pragma unroll
  for (int w = 0; w < NW; ++w)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c[w] += __shfl_xor(c[w], o, 64);
  if ((threadIdx.x & 63) == 0)
#pragma unroll
    for (int w = 0; w < NW; ++w) s_red[threadIdx.x >> 6][w] = c[w];
  __syncthreads();
  if (threadIdx.x == 0)
#pragma unroll
    for (int w = 0; w < NW; ++w) {
      out[w] = 0ull;
#pragma unroll
      for (int k = 0; k < RX_MET_WAVES; ++k) out[w] += s_red[k][w];
    }
}

// ---- binary confusion: workgroup b works on chunk b % cpr (U units) of row b / cpr -------------------------------------------------
template <typename T>
__global__ __launch_bounds__(RX_MET_BLOCK) void seg_counts_kernel(const T* __restrict__ pred, const float* __restrict__ target, long V,
                                                                  int cpr, long U, float thr_p, float thr_t,
                                                                  unsigned long long* __restrict__ counts) {
  constexpr int P = Elem<T>::PER16;
  const long row = (long)(blockIdx.x / (unsigned)cpr);
  const int chunk = (int)(blockIdx.x - (unsigned)row * (unsigned)cpr);
  const T* __restrict__ p = pred + row * V;
  const float* __restrict__ t = target + row * V;
  const long h = met_head(p, V), nvec = (V - h) / P;
  const long u0 = (long)chunk * U, u1 = u0 + U < nvec ? u0 + U : nvec;
  unsigned c[3] = {0u, 0u, 0u};      // TP, FP, FN
  auto one = [&](float x, float y) {
    const bool a = x > thr_p, b = y > thr_t;      // IEEE: a NaN is negative
    c[0] += (a && b) ? 1u : 0u, c[1] += (a && !b) ? 1u : 0u, c[2] += (!a && b) ? 1u : 0u;
  };
#pragma unroll 2
  for (long u = u0 + threadIdx.x; u < u1; u += RX_MET_BLOCK) {
    const long off = h + u * P;
    float x[P], y[P];
    met_load_pred<T>(p + off, true, x);
    met_load_f32<P>(t + off, y);
#pragma unroll
    for (int j = 0; j < P; ++j) one(x[j], y[j]);
  }
  if (chunk == 0) {      // head and tail: fewer than P voxels each
    const long tail = h + nvec * P;
    if ((long)threadIdx.x < h) one(Elem<T>::to_f(p[threadIdx.x]), t[threadIdx.x]);
    if (tail + threadIdx.x < V) one(Elem<T>::to_f(p[tail + threadIdx.x]), t[tail + threadIdx.x]);
  }
  unsigned long long s[3];
  met_block_sum<3>(c, s);
  if (threadIdx.x == 0)
#pragma unroll
    for (int w = 0; w < 3; ++w)
      if (s[w]) atomicAdd(counts + row * 3 + w, s[w]);
}

// ---- multi-class confusion: workgroup b works on chunk b % cps of sample b / cps ---------------------------------------------------
// the arg-max rule: the first maximum wins and a NaN never displaces or outlasts a number (all NaN: class 0)
__device__ inline bool met_better(float x, float best) { return !(x <= best) && x == x; }

template <typename T>
__global__ __launch_bounds__(RX_MET_BLOCK) void class_counts_kernel(const T* __restrict__ pred, const float* __restrict__ tprob,
                                                                    const long long* __restrict__ tindex, long long ignore_index, int C,
                                                                    long V, int cps, long U, unsigned long long* __restrict__ counts) {
  constexpr int P = Elem<T>::PER16;
  extern __shared__ __attribute__((aligned(16))) unsigned s_cls[];      // [RX_MET_REP][C * 3]
  const int n = (int)(blockIdx.x / (unsigned)cps), chunk = (int)(blockIdx.x - (unsigned)n * (unsigned)cps);
  const int words = C * 3;
  for (int i = threadIdx.x; i < RX_MET_REP * words; i += RX_MET_BLOCK) s_cls[i] = 0u;
  __syncthreads();
  unsigned* __restrict__ mine = s_cls + (threadIdx.x & (RX_MET_REP - 1)) * words;
  const T* __restrict__ p = pred + (long)n * C * V;
  const float* __restrict__ tp = tprob ? tprob + (long)n * C * V : nullptr;
  const long long* __restrict__ ti = tindex ? tindex + (long)n * V : nullptr;
  const long h = met_head(p, V), nvec = (V - h) / P;
  const bool al16 = (V % P) == 0;      // every channel row then shares the head of channel 0
  const long u0 = (long)chunk * U, u1 = u0 + U < nvec ? u0 + U : nvec;
  auto tally = [&](int pc, long long lab) {
    if (lab < 0 || lab >= C) return;      // ignore_index (mapped to -1 below), and any label that is no class
    if (pc == (int)lab) {
      atomicAdd(mine + pc * 3, 1u);
    } else {
      atomicAdd(mine + pc * 3 + 1, 1u);
      atomicAdd(mine + (int)lab * 3 + 2, 1u);
    }
  };
  for (long u = u0 + threadIdx.x; u < u1; u += RX_MET_BLOCK) {
    const long off = h + u * P;
    float bv[P], x[P];
    int bi[P];
    met_load_pred<T>(p + off, al16, bv);
#pragma unroll
    for (int j = 0; j < P; ++j) bi[j] = 0;
#pragma unroll 4
    for (int k = 1; k < C; ++k) {
      met_load_pred<T>(p + (long)k * V + off, al16, x);
#pragma unroll
      for (int j = 0; j < P; ++j)
        if (met_better(x[j], bv[j])) bv[j] = x[j], bi[j] = k;
    }
    long long lab[P];
    if (ti) {
      const MetRun<long long, P> r = *reinterpret_cast<const MetRun<long long, P>*>(ti + off);
#pragma unroll
      for (int j = 0; j < P; ++j) lab[j] = r.v[j] == ignore_index ? -1ll : r.v[j];
    } else {
      float lv[P];
      met_load_f32<P>(tp + off, lv);
#pragma unroll
      for (int j = 0; j < P; ++j) lab[j] = 0;
#pragma unroll 4
      for (int k = 1; k < C; ++k) {
        met_load_f32<P>(tp + (long)k * V + off, x);
#pragma unroll
        for (int j = 0; j < P; ++j)
          if (met_better(x[j], lv[j])) lv[j] = x[j], lab[j] = k;
      }
    }
#pragma unroll
    for (int j = 0; j < P; ++j) tally(bi[j], lab[j]);
  }
  if (chunk == 0) {      // head and tail voxels, one lane each
    const long tail = h + nvec * P;
    long i = -1;
    if ((long)threadIdx.x < h) i = threadIdx.x;
    else if ((long)threadIdx.x >= 64 && tail + (threadIdx.x - 64) < V) i = tail + (threadIdx.x - 64);
    if (i >= 0) {
      float bv = Elem<T>::to_f(p[i]);
      int bi = 0;
      for (int k = 1; k < C; ++k) {
        const float x = Elem<T>::to_f(p[(long)k * V + i]);
        if (met_better(x, bv)) bv = x, bi = k;
      }
      long long lab;
      if (ti) {
        lab = ti[i] == ignore_index ? -1ll : ti[i];
      } else {
        float lv = tp[i];
        lab = 0;
        for (int k = 1; k < C; ++k) {
          const float x = tp[(long)k * V + i];
          if (met_better(x, lv)) lv = x, lab = k;
        }
      }
      tally(bi, lab);
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < words; i += RX_MET_BLOCK) {
    unsigned long long s = 0ull;
#pragma unroll
    for (int r = 0; r < RX_MET_REP; ++r) s += s_cls[r * words + i];
    if (s) atomicAdd(counts + (long)n * words + i, s);
  }
}

// ---- normals: workgroup b works on chunk b % cps of sample b / cps and writes partial b --------------------------------------------
struct NormalAcc {
  double cs, dg;
  unsigned cnt;
};
__device__ inline void normal_one(float px, float py, float pz, float tx, float ty, float tz, NormalAcc& a) {
  const float tt = (tx * tx + ty * ty) + tz * tz;
  const float tn = sqrtf(tt);
  if (tn > 1e-6f) {
    const float pp = (px * px + py * py) + pz * pz;
    const float dot = (px * tx + py * ty) + pz * tz;
    float c = dot / (fmaxf(sqrtf(pp), 1e-8f) * fmaxf(tn, 1e-8f));
    c = fminf(fmaxf(c, -1.f), 1.f);      // (a NaN from a non-finite prediction goes through both and stays in the sums)
    a.cs += (double)c;
    a.dg += (double)(acosf(c) * 57.29577951308232f);
    a.cnt += 1u;
  }
}

template <typename T>
__global__ __launch_bounds__(RX_MET_BLOCK) void normal_stats_kernel(const T* __restrict__ pred, const float* __restrict__ target, long V,
                                                                    int cps, long U, unsigned long long* __restrict__ count,
                                                                    double* __restrict__ partial) {
  constexpr int P = Elem<T>::PER16;
  __shared__ double s_sum[RX_MET_WAVES][2];
  const int n = (int)(blockIdx.x / (unsigned)cps), chunk = (int)(blockIdx.x - (unsigned)n * (unsigned)cps);
  const T* __restrict__ p = pred + (long)n * 3 * V;
  const float* __restrict__ t = target + (long)n * 3 * V;
  const long h = met_head(p, V), nvec = (V - h) / P;
  const bool al16 = (V % P) == 0;
  const long u0 = (long)chunk * U, u1 = u0 + U < nvec ? u0 + U : nvec;
  NormalAcc a{0.0, 0.0, 0u};
  for (long u = u0 + threadIdx.x; u < u1; u += RX_MET_BLOCK) {
    const long off = h + u * P;
    float px[P], py[P], pz[P], tx[P], ty[P], tz[P];
    met_load_pred<T>(p + off, al16, px);
    met_load_pred<T>(p + V + off, al16, py);
    met_load_pred<T>(p + 2 * V + off, al16, pz);
    met_load_f32<P>(t + off, tx);
    met_load_f32<P>(t + V + off, ty);
    met_load_f32<P>(t + 2 * V + off, tz);
#pragma unroll
    for (int j = 0; j < P; ++j) normal_one(px[j], py[j], pz[j], tx[j], ty[j], tz[j], a);
  }
  if (chunk == 0) {
    const long tail = h + nvec * P;
    long i = -1;
    if ((long)threadIdx.x < h) i = threadIdx.x;
    else if ((long)threadIdx.x >= 64 && tail + (threadIdx.x - 64) < V) i = tail + (threadIdx.x - 64);
    if (i >= 0)
      normal_one(Elem<T>::to_f(p[i]), Elem<T>::to_f(p[V + i]), Elem<T>::to_f(p[2 * V + i]), t[i], t[V + i], t[2 * V + i], a);
  }
  // fixed order: the lanes of a wave by xor shuffles, the four waves in order
  const double cs = wave_sum_d(a.cs), dg = wave_sum_d(a.dg);
  if ((threadIdx.x & 63) == 0) s_sum[threadIdx.x >> 6][0] = cs, s_sum[threadIdx.x >> 6][1] = dg;
  unsigned c[1] = {a.cnt};
  unsigned long long s[1];
  met_block_sum<1>(c, s);      // (its barrier also publishes s_sum)
  if (threadIdx.x == 0) {
    if (s[0]) atomicAdd(count + n, s[0]);
    double* o = partial + (long)blockIdx.x * 2;
    o[0] = ((s_sum[0][0] + s_sum[1][0]) + s_sum[2][0]) + s_sum[3][0];
    o[1] = ((s_sum[0][1] + s_sum[1][1]) + s_sum[2][1]) + s_sum[3][1];
  }
}

// one lane per (sample, sum): its cps partials in index order, eight loads in flight at a time
__global__ __launch_bounds__(RX_MET_BLOCK) void normal_stats_finalize_kernel(const double* __restrict__ partial, int N, int cps,
                                                                             double* __restrict__ sums) {
  for (int i = threadIdx.x; i < 2 * N; i += RX_MET_BLOCK) {
    const double* __restrict__ q = partial + (long)(i >> 1) * cps * 2 + (i & 1);
    double s = 0.0;
    int k = 0;
    for (; k + 8 <= cps; k += 8) {
      double v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = q[(long)(k + j) * 2];
#pragma unroll
      for (int j = 0; j < 8; ++j) s += v[j];
    }
    for (; k < cps; ++k) s += q[(long)k * 2];
    sums[i] += s;
  }
}

// ---- host side -------------------------------------------------------------------------------------------------------------------
// units per chunk and chunks per row: about RX_MET_TARGET_BLOCKS chunks in the call, none below `min_units`, at most `max_chunks`
// per row (0: no limit), the grid below 2^31
struct MetPlan {
  long U;
  int chunks;
};
static inline MetPlan met_plan(long rows, long units, long min_units, long max_chunks) {
  long U = (rows * units + RX_MET_TARGET_BLOCKS - 1) / RX_MET_TARGET_BLOCKS;
  U = U > min_units ? U : min_units;
  if (max_chunks && (units + U - 1) / U > max_chunks) U = (units + max_chunks - 1) / max_chunks;
  U = (U + RX_MET_BLOCK - 1) / RX_MET_BLOCK * RX_MET_BLOCK;
  while ((units + U - 1) / U * rows > 0x7fffffffL) U *= 2;
  long ch = (units + U - 1) / U;
  return MetPlan{U, (int)(ch > 0 ? ch : 1)};
}

static inline int met_pred_ok(const char* fn, const void* pred, int dtype) {
  if (dtype != RX_F32 && dtype != RX_BF16 && dtype != RX_F16) RX_FAIL(RX_EINVAL, "%s: unknown prediction dtype %d (RX_F32, RX_BF16 or RX_F16)", fn, dtype);
  if (((uintptr_t)pred & (uintptr_t)(rx_dtype_size(dtype) - 1)) != 0)
    RX_FAIL(RX_EINVAL, "%s: the prediction must be aligned to its %zu-byte element", fn, rx_dtype_size(dtype));
  return RX_OK;
}

extern "C" int rx_seg_counts(const void* pred, int pred_dtype, const float* target, int n, int c, long v, float thr_pred, float thr_target,
                             int64_t* counts, void* stream) {
  if (!pred || !target) RX_FAIL(RX_EINVAL, "rx_seg_counts: null input pointer");
  if (!counts) RX_FAIL(RX_EINVAL, "rx_seg_counts: null output pointer");
  if (n <= 0 || c <= 0 || v <= 0) RX_FAIL(RX_EINVAL, "rx_seg_counts: sizes must be positive (got n=%d c=%d v=%ld)", n, c, v);
  if (int rc = met_pred_ok("rx_seg_counts", pred, pred_dtype)) return rc;
  if (((uintptr_t)target & 3) != 0 || ((uintptr_t)counts & 7) != 0)
    RX_FAIL(RX_EINVAL, "rx_seg_counts: target must be 4-byte and counts 8-byte aligned");
  if (thr_pred != thr_pred || thr_target != thr_target) RX_FAIL(RX_EINVAL, "rx_seg_counts: a threshold is NaN");
  const long rows = (long)n * c;
  const int per16 = pred_dtype == RX_F32 ? 4 : 8;
  const MetPlan pl = met_plan(rows, v / per16, RX_MET_MIN_UNITS, 0);
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)(rows * pl.chunks)), block(RX_MET_BLOCK);
  RX_DISPATCH_DTYPE(pred_dtype, T,
                    hipLaunchKernelGGL(seg_counts_kernel<T>, grid, block, 0, st, (const T*)pred, target, v, pl.chunks, pl.U, thr_pred,
                                       thr_target, (unsigned long long*)counts));
  RX_CHECK_LAUNCH("rx_seg_counts");
  return RX_OK;
}

extern "C" int rx_class_counts(const void* pred, int pred_dtype, const float* target_prob, const int64_t* target_index, int64_t ignore_index,
                               int n, int c, long v, int64_t* counts, void* stream) {
  if (!pred) RX_FAIL(RX_EINVAL, "rx_class_counts: null prediction pointer");
  if ((target_prob != nullptr) == (target_index != nullptr))
    RX_FAIL(RX_EINVAL, "rx_class_counts: exactly one of target_prob and target_index must be given");
  if (!counts) RX_FAIL(RX_EINVAL, "rx_class_counts: null output pointer");
  if (n <= 0 || v <= 0) RX_FAIL(RX_EINVAL, "rx_class_counts: sizes must be positive (got n=%d v=%ld)", n, v);
  if (c < 2 || c > RX_MET_MAXC) RX_FAIL(RX_EINVAL, "rx_class_counts: 2 to %d classes (got %d)", RX_MET_MAXC, c);
  if (int rc = met_pred_ok("rx_class_counts", pred, pred_dtype)) return rc;
  if (((uintptr_t)target_prob & 3) != 0 || ((uintptr_t)target_index & 7) != 0 || ((uintptr_t)counts & 7) != 0)
    RX_FAIL(RX_EINVAL, "rx_class_counts: target_prob must be 4-byte, target_index and counts 8-byte aligned");
  const int per16 = pred_dtype == RX_F32 ? 4 : 8;
  const MetPlan pl = met_plan(n, v / per16, RX_MET_BLOCK, 0);
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)((long)n * pl.chunks)), block(RX_MET_BLOCK);
  const size_t lds = (size_t)RX_MET_REP * c * 3 * sizeof(unsigned);
  RX_DISPATCH_DTYPE(pred_dtype, T,
                    hipLaunchKernelGGL(class_counts_kernel<T>, grid, block, lds, st, (const T*)pred, target_prob, (const long long*)target_index,
                                       (long long)ignore_index, c, v, pl.chunks, pl.U, (unsigned long long*)counts));
  RX_CHECK_LAUNCH("rx_class_counts");
  return RX_OK;
}

extern "C" size_t rx_normal_stats_workspace(int n, long v) {
  if (n <= 0 || v <= 0) return 0;
  return (size_t)n * RX_NS_MAX_CHUNKS * 2 * sizeof(double);
}

extern "C" int rx_normal_stats(const void* pred, int pred_dtype, const float* target, int n, long v, int64_t* count, double* sums, void* ws,
                               size_t ws_bytes, void* stream) {
  if (!pred || !target) RX_FAIL(RX_EINVAL, "rx_normal_stats: null input pointer");
  if (!count || !sums) RX_FAIL(RX_EINVAL, "rx_normal_stats: null output pointer");
  if (!ws) RX_FAIL(RX_EINVAL, "rx_normal_stats: null workspace pointer");
  if (n <= 0 || v <= 0) RX_FAIL(RX_EINVAL, "rx_normal_stats: sizes must be positive (got n=%d v=%ld)", n, v);
  if (int rc = met_pred_ok("rx_normal_stats", pred, pred_dtype)) return rc;
  if (((uintptr_t)target & 3) != 0 || ((uintptr_t)count & 7) != 0 || ((uintptr_t)sums & 7) != 0 || ((uintptr_t)ws & 7) != 0)
    RX_FAIL(RX_EINVAL, "rx_normal_stats: target must be 4-byte, count, sums and the workspace 8-byte aligned");
  if (ws_bytes < rx_normal_stats_workspace(n, v))
    RX_FAIL(RX_EWORKSPACE, "rx_normal_stats: workspace of %zu bytes, rx_normal_stats_workspace says %zu", ws_bytes,
            rx_normal_stats_workspace(n, v));
  const int per16 = pred_dtype == RX_F32 ? 4 : 8;
  const MetPlan pl = met_plan(n, v / per16, RX_MET_BLOCK, RX_NS_MAX_CHUNKS);
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)((long)n * pl.chunks)), block(RX_MET_BLOCK);
  RX_DISPATCH_DTYPE(pred_dtype, T,
                    hipLaunchKernelGGL(normal_stats_kernel<T>, grid, block, 0, st, (const T*)pred, target, v, pl.chunks, pl.U,
                                       (unsigned long long*)count, (double*)ws));
  RX_CHECK_LAUNCH("rx_normal_stats");
  hipLaunchKernelGGL(normal_stats_finalize_kernel, dim3(1), dim3(RX_MET_BLOCK), 0, st, (const double*)ws, n, pl.chunks, sums);
  RX_CHECK_LAUNCH("rx_normal_stats");
  return RX_OK;
}
