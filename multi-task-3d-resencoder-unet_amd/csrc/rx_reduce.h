// rx_reduce.h -- what the channels-last elementwise files (rx_instnorm.hip, rx_head.hip, rx_stem.hip, rx_se.hip) share: the
// deterministic two-stage column reduction, the activation view its operators read through, and the host-side descriptor checks.
#pragma once
#include <initializer_list>

#include "rx_common.h"

// ---------------------------------------------------------------------------------------------
// column (per-(n,c)) reductions: shared machinery
// ---------------------------------------------------------------------------------------------
// Work split: grid = (nchunks, N).  A block owns voxels [chunk*chunk_vox, ...) of sample n.
// thread -> (vl = tid / CV, cv = tid % CV): channel vector cv of voxels vl, vl+VP, ...
// Partials: partial[((n*nchunks + chunk)*NACC + a)*C + c].
struct ReducePlan {
  int nchunks, chunk_vox;
};
static inline ReducePlan rx_reduce_plan(long V, int C, int per16) {
  int CV = C / per16;
  int VP = 256 / CV;
  if (VP < 1) VP = 1;
  // ~1024 blocks per launch keep 256 CUs streaming; a block should own >= 8 passes of VP voxels
  long nch = V / ((long)VP * 8);
  if (nch < 1) nch = 1;
  if (nch > 512) nch = 512;
  long cvx = (V + nch - 1) / nch;
  cvx = (cvx + VP - 1) / VP * VP;
  nch = (V + cvx - 1) / cvx;
  ReducePlan p;
  p.nchunks = (int)nch;
  p.chunk_vox = (int)cvx;
  return p;
}
static inline size_t rx_reduce_ws_bytes(int N, long V, int C, int nacc) {
  // sized for the finest element type (per16 = 4 gives the most chunks)
  ReducePlan p = rx_reduce_plan(V, C, 4);
  ReducePlan q = rx_reduce_plan(V, C, 8);
  int nch = p.nchunks > q.nchunks ? p.nchunks : q.nchunks;
  return (size_t)N * nch * nacc * C * sizeof(float) + 256;
}

template <typename T, int NACC, typename Op>
__global__ __launch_bounds__(256) void colreduce_kernel(Op op, int V, int C, int chunk_vox, float* __restrict__ partial) {
  constexpr int P = Elem<T>::PER16;
  extern __shared__ __attribute__((aligned(16))) float sm[];  // [NACC][rows][C], rows = 4 (shuffle path) or VP
  const int CV = C / P;
  const int VP = 256 / CV > 0 ? 256 / CV : 1;
  const int tid = threadIdx.x;
  const int n = blockIdx.y, chunk = blockIdx.x;
  float acc[NACC][P];
#pragma unroll
  for (int a = 0; a < NACC; ++a)
#pragma unroll
    for (int j = 0; j < P; ++j) acc[a][j] = 0.f;
  const int v_begin = chunk * chunk_vox;
  const int v_end = min(V, v_begin + chunk_vox);
  const int vl = tid / CV, cv = tid - vl * CV;
  if (vl < VP) {
    op.prepare(n, cv * P);
#pragma unroll 4
    for (int v = v_begin + vl; v < v_end; v += VP) op.accumulate(n, v, cv * P, acc);
  }
  const bool shuffle_path = (64 % CV) == 0;  // lanes of one wave with equal cv are CV apart
  int rows;
  if (shuffle_path) {
    for (int o = CV; o < 64; o <<= 1) {
#pragma unroll
      for (int a = 0; a < NACC; ++a)
#pragma unroll
        for (int j = 0; j < P; ++j) acc[a][j] += __shfl_xor(acc[a][j], o, 64);
    }
    rows = 4;
    const int lane = tid & 63, wave = tid >> 6;
    if (lane < CV) {
#pragma unroll
      for (int a = 0; a < NACC; ++a)
#pragma unroll
        for (int j = 0; j < P; ++j) sm[(a * 4 + wave) * C + lane * P + j] = acc[a][j];
    }
  } else {
    rows = VP;
    if (vl < VP) {
#pragma unroll
      for (int a = 0; a < NACC; ++a)
#pragma unroll
        for (int j = 0; j < P; ++j) sm[(a * VP + vl) * C + cv * P + j] = acc[a][j];
    }
  }
  __syncthreads();
  for (int i = tid; i < NACC * C; i += 256) {
    int a = i / C, c = i - a * C;
    float s = 0.f;
    for (int r = 0; r < rows; ++r) s += sm[(a * rows + r) * C + c];
    partial[((size_t)(n * gridDim.x + chunk) * NACC + a) * C + c] = s;
  }
}

// finalize modes
enum { FIN_STATS = 0, FIN_MEAN2 = 1, FIN_SUM_OVER_N = 2 };
// FIN_STATS: out[n][c] = (mean, rstd) from (sum, sumsq);  FIN_MEAN2: out[n][c] = (s0/V, s1/V);
// FIN_SUM_OVER_N: out[a][c] = sum over n and chunks (NACC planes)
// one WORKGROUP per output element: the 256 threads stride over the chunks with up to four independent loads each in flight
// (a wave per element walked 512 chunks in 8 dependent round trips: 6.4 us per launch on average, 30 at worst, 71 launches per
// cfg2 step, every one of them between two kernels that depend on it), fp64 xor-shuffle combine, the four waves added in order.
__device__ inline void fin_gather(const float* __restrict__ base, size_t row_stride, int rows, int second, double& s0, double& s1) {
  const int tid = threadIdx.x;
  for (int k0 = tid; k0 < rows; k0 += 1024) {
    float v0[4], v1[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int k = k0 + 256 * u;
      const bool ok = k < rows;
      const float* p = base + (size_t)(ok ? k : 0) * row_stride;
      v0[u] = ok ? p[0] : 0.f;
      v1[u] = (ok && second) ? p[second] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) s0 += (double)v0[u], s1 += (double)v1[u];
  }
  __shared__ double red[2][4];
  s0 = wave_sum_d(s0);
  s1 = wave_sum_d(s1);
  if ((tid & 63) == 0) red[0][tid >> 6] = s0, red[1][tid >> 6] = s1;
  __syncthreads();
  s0 = ((red[0][0] + red[0][1]) + red[0][2]) + red[0][3];
  s1 = ((red[1][0] + red[1][1]) + red[1][2]) + red[1][3];
}

template <typename T>
struct ActView {
  const T* ptr;
  long sample_stride;  // elements
  int ld;
  __device__ inline const T* at(int n, long v, int c) const { return ptr + n * sample_stride + v * ld + c; }
};
template <typename T>
static inline ActView<T> make_view(const rx_act* a) {   // a == NULL: the null view (ptr == nullptr)
  if (!a) return ActView<T>{nullptr, 0, 0};
  return ActView<T>{(const T*)a->ptr, rx_act_voxels(a) * (long)a->ld, a->ld};
}

// ---- one host path for the two-stage reductions ------------------------------------------------
// Workspace of a backward entry point: the colreduce partials, then the (m1, m2) table of N*C pairs.  rx_reduce_ws_bytes is
// payload + 256 spare bytes; m12 starts at the payload rounded up to 256 (hence `- 256`: at most 255 bytes past the payload,
// inside the spare), so partial and m12 never overlap and `need` = partials + table covers both.
struct ReduceWs {
  float* partial;
  float* m12;
  size_t need;
};
static inline ReduceWs reduce_ws(void* ws, int N, long V, int C, int nacc) {
  const size_t part = rx_reduce_ws_bytes(N, V, C, nacc);
  return ReduceWs{(float*)ws, (float*)((char*)ws + rx_align_up(part - 256, 256)), part + (size_t)N * C * 2 * sizeof(float)};
}

// first stage of a column reduction: plan, LDS rows (4 on the shuffle path, VP otherwise) and launch
template <typename T, int NACC, typename Op>
static inline ReducePlan launch_colreduce(const Op& op, int N, long V, int C, float* partial, hipStream_t st) {
  constexpr int P = Elem<T>::PER16;
  const ReducePlan p = rx_reduce_plan(V, C, P);
  const int VP = 256 / (C / P);
  const size_t lds = (size_t)NACC * (VP > 4 ? VP : 4) * C * sizeof(float);
  hipLaunchKernelGGL((colreduce_kernel<T, NACC, Op>), dim3(p.nchunks, N), dim3(256), lds, st, op, (int)V, C, p.chunk_vox, partial);
  return p;
}

// ---- descriptor checks and sweep geometry (host) ---------------------------------------------
// max_c: most channels the caller's kernels take; 0 = the 256 16-byte vectors a column-reduction workgroup covers (1024
// channels in fp32, 2048 in the 16-bit types)
static inline int check_vec_channels(const rx_act* a, int dt, const char* who, int max_c = 0) {
  int per16 = dt == RX_F32 ? 4 : 8;
  if (!rx_act_ok(a)) RX_FAIL(RX_EINVAL, "%s: bad activation descriptor", who);
  if (a->c % per16 || a->ld % per16 || ((uintptr_t)a->ptr & 15)) RX_FAIL(RX_EUNSUPPORTED, "%s: channels/ld/ptr must be 16-byte multiples (c=%d ld=%d)", who, a->c, a->ld);
  if (max_c ? a->c > max_c : a->c / per16 > 256) RX_FAIL(RX_EUNSUPPORTED, "%s: too many channels (%d)", who, a->c);
  return RX_OK;
}

static inline int sweep_grid(long total_vec, int CV) {
  // number of blocks G with (G*256) % CV == 0, so that every thread keeps one channel vector
  int g = CV, d = 256;
  while (g % 2 == 0 && d > 1) {
    g /= 2;
    d /= 2;
  }
  long want = (total_vec + 256 * 8 - 1) / (256 * 8);
  if (want < 1) want = 1;
  if (want > 2048) want = 2048;
  long G = (want + g - 1) / g * g;
  return (int)G;
}

static inline int same_geom(const rx_act* a, const rx_act* b) {
  return a->n == b->n && a->z == b->z && a->y == b->y && a->x == b->x && a->c == b->c;
}

// The validation preamble of an entry point `fn`: every listed activation passes check_vec_channels and has the geometry of
// `ref` (list `ref` itself first, so it is validated before it is compared against).  An absent optional one is skipped.
struct ActArg {
  const char* name;
  const rx_act* act;
  bool required;
};
static inline int check_acts(int dt, const char* fn, const rx_act* ref, std::initializer_list<ActArg> acts, int max_c = 0) {
  for (const ActArg& a : acts) {
    if (!a.act && !a.required) continue;
    char who[96];
    snprintf(who, sizeof who, "%s(%s)", fn, a.name);
    int rc = check_vec_channels(a.act, dt, who, max_c);
    if (rc) return rc;
    if (!same_geom(ref, a.act)) RX_FAIL(RX_EINVAL, "%s: %s geometry mismatch", fn, a.name);
  }
  return RX_OK;
}

static inline int check_pool(const rx_act* big, const rx_act* small, const int32_t f[3], const char* who) {
  for (int i = 0; i < 3; ++i)
    if (f[i] < 1 || f[i] > RX_MAX_STRIDE) RX_FAIL(RX_EUNSUPPORTED, "%s: pool factor must be 1..%d per axis", who, RX_MAX_STRIDE);
  if (big->n != small->n || big->c != small->c || big->z != small->z * f[0] || big->y != small->y * f[1] || big->x != small->x * f[2])
    RX_FAIL(RX_EINVAL, "%s: geometry mismatch (%d,%d,%d)/(%d,%d,%d)", who, big->z, big->y, big->x, small->z, small->y, small->x);
  return RX_OK;
}
