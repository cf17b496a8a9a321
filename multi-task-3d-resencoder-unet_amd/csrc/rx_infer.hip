// rx_infer.hip -- the per-patch work of streaming sliding-window inference around the network forward (reference
// inference.py:115-157 patch loop, :166-210 overlap processing, :251-263 cast; dataloading/inference_dataset.py:60-71 input
// normalisation).  Volumes live on the device as RING SLABS: a (C, R, Y, X) array whose ring row r holds absolute volume row z
// with z % R == r.  Three entry points:
//   rx_sw_gather      input slab (uint8 / uint16 / fp32) -> B patches, contiguous fp32 (B, Cin, pz, py, px), /255 or /65535
//                     ("scale") and optionally the per-patch standardisation ("zscore")
//   rx_sw_accumulate  one task's logits (B, c, pz, py, px) -> activation -> sum += w * p and wsum += w on the ring accumulators
//   rx_sw_finalize    finished rows -> blended fp32 + uint8 / uint16 final (+ the weight sum), accumulators reset for reuse
// Gather and accumulate each take an optional table of records for test-time augmentation (one flip / 90-degree rotation record,
// `rx_geom_sample`, per patch slot; checked and lowered by rx_geom_core.h):
//   rx_sw_gather_geom      rx_sw_gather of the TRANSFORMED patch: output voxel o of slot b reads slab voxel origin_b + i(o)
//   rx_sw_accumulate_geom  rx_sw_accumulate of the TRANSFORMED prediction: destination voxel l of slot b adds the activated logit
//                          at i(l), a 3-vector task with the record's component permutation and signs
// both with the gather form of rx_geom_apply, out[o] = in[i(o)], i[src_axis[d]] = flip[d] ? n_d - 1 - o_d : o_d.  Each pair is ONE
// host path (sw_gather_impl, sw_accumulate_impl) and ONE kernel body with a template flag GEOM: without a table (GEOM = false) the
// table is not among the kernel's arguments and nothing that reads it is compiled in; with identity records both forms load the
// same values and run the same arithmetic on them, so they agree bit for bit.
// For empty-patch skipping, rx_sw_occupancy counts per patch the raw slab voxels above a threshold (integer atomics: exact).
// The entry points above are deterministic without atomics.  rx_sw_accumulate runs one thread per 4 destination voxels of the batch's bounding box, each adding
// the batch's patches in patch order -- the same additions, in the same order, as one launch per patch, with every destination
// read and written once per batch instead of once per covering patch (patches of one batch overlap by design).
// Floating-point contraction is off in this file: every product and sum rounds like the numpy / torch statement it restates.
#include <type_traits>

#include "rx_common.h"
#include "rx_geom_core.h"

#pragma clang fp contract(off)

#define RX_SW_MAXB 32        // patches per call (kernel-argument table)
#define RX_SW_BLOCK 256
#define RX_SW_STAT_CHUNKS 64 // blocks per patch of the zscore partial sums

struct SwPatches {
  int32_t oz[RX_SW_MAXB], oy[RX_SW_MAXB], ox[RX_SW_MAXB];
};

static int sw_patches(const int32_t* origins, int batch, int R, int Y, int X, int pz, int py, int px, SwPatches& p,
                      const char* who) {
  if (!origins || batch < 1 || batch > RX_SW_MAXB) RX_FAIL(RX_EINVAL, "%s: batch must be 1..%d", who, RX_SW_MAXB);
  if (pz < 1 || py < 1 || px < 1 || pz > R || py > Y || px > X)
    RX_FAIL(RX_EINVAL, "%s: patch (%d,%d,%d) does not fit the slab (ring %d, %d, %d)", who, pz, py, px, R, Y, X);
  for (int b = 0; b < batch; ++b) {
    const int z = origins[3 * b], y = origins[3 * b + 1], x = origins[3 * b + 2];
    if (z < 0 || y < 0 || x < 0 || y + py > Y || x + px > X)
      RX_FAIL(RX_EINVAL, "%s: patch %d at (%d,%d,%d) leaves the slab (%d, %d)", who, b, z, y, x, Y, X);
    p.oz[b] = z, p.oy[b] = y, p.ox[b] = x;
  }
  return RX_OK;
}

// the records of a call with a table: every one passes rx_geom_check over the patch extents
static int sw_records(const rx_geom_sample* ops, int batch, int pz, int py, int px, const char* who) {
  if (!ops) RX_FAIL(RX_EINVAL, "%s: null record table", who);
  for (int b = 0; b < batch; ++b)
    if (const int verdict = rx_geom_check(ops, pz, py, px, b)) {
      char text[160];
      rx_geom_refusal(text, sizeof(text), verdict, ops, pz, py, px, b, "slot", "patch shape");
      RX_FAIL(RX_EINVAL, "%s: %s", who, text);
    }
  return RX_OK;
}

// the per-slot table among a kernel's arguments: V with records (GEOM), nothing without
struct SwNone {};
template <bool GEOM, typename V>
using SwTable = std::conditional_t<GEOM, V, SwNone>;

// f(the slab as a pointer to its element type): the launches that are templates on SwElem<decltype(pointer)>
template <typename P>
using SwElem = std::remove_cv_t<std::remove_pointer_t<P>>;
template <typename F>
static void sw_typed(int in_dtype, const void* slab, F&& f) {
  if (in_dtype == RX_SW_U8) f((const uint8_t*)slab);
  else if (in_dtype == RX_SW_U16) f((const uint16_t*)slab);
  else f((const float*)slab);
}

// a quad of 4 consecutive floats: one 16-byte access (VEC), or its first n voxels one by one, the others reading as 0
template <bool VEC>
__device__ inline void sw_load_quad(const float* p, int n, float (&a)[4]) {
  if (VEC) {
    const f32x4 t = *reinterpret_cast<const f32x4*>(p);
#pragma unroll
    for (int i = 0; i < 4; ++i) a[i] = t[i];
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i) a[i] = i < n ? p[i] : 0.f;
  }
}
template <bool VEC>
__device__ inline void sw_store_quad(float* p, int n, const float (&a)[4]) {
  if (VEC) {
    *reinterpret_cast<f32x4*>(p) = f32x4{a[0], a[1], a[2], a[3]};
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (i < n) p[i] = a[i];
  }
}

// ---- gather ---------------------------------------------------------------------------------------------------------
struct GatherGeom {
  int cin, R, Y, X, pz, py, px, pxq;   // pxq: quads of 4 outputs per patch row
  float div;                           // 0: fp32 input as is; otherwise the divisor 255 / 65535
  long total;                          // B * cin * pz * py * pxq
};
// GEOM: slot b, source axis a (z, y, x of the slab patch) takes the output coordinate of axis from[b][a], mirrored where flip[b][a]
// (the slot's RxGeomInverse)
struct SwViews {
  uint8_t from[RX_SW_MAXB][3], flip[RX_SW_MAXB][3];
};

template <typename T>
__device__ inline float sw_scale(T v, float div) {
  return div == 0.f ? (float)v : (float)v / div;   // true division: bit-exact against numpy's float32 `img /= 255.0`
}

__device__ inline int sw_pick(int axis, int oz, int oy, int ox) { return axis == 0 ? oz : axis == 1 ? oy : ox; }

template <typename T, bool GEOM>
__global__ __launch_bounds__(RX_SW_BLOCK) void sw_gather_kernel(const T* __restrict__ slab, float* __restrict__ out, GatherGeom g,
                                                                SwPatches p, SwTable<GEOM, SwViews> v) {
  const long q = (long)blockIdx.x * RX_SW_BLOCK + threadIdx.x;
  if (q >= g.total) return;
  long r = q;
  const int xq = (int)(r % g.pxq);
  r /= g.pxq;
  const int ly = (int)(r % g.py);
  r /= g.py;
  const int lz = (int)(r % g.pz);
  r /= g.pz;
  const int ci = (int)(r % g.cin);
  const int b = (int)(r / g.cin);
  float* dst = out + (((long)(b * g.cin + ci) * g.pz + lz) * g.py + ly) * g.px;
  const int x0 = xq * 4;
  const bool quad = (g.px & 3) == 0;      // whole quads: one 16-byte store
  if constexpr (GEOM) {
    const int fz = v.from[b][0], fy = v.from[b][1], fx = v.from[b][2];
    const int mz = v.flip[b][0], my = v.flip[b][1], mx = v.flip[b][2];
    const T* src = slab + (long)ci * g.R * g.Y * g.X;
    float val[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int lx = x0 + i;
      if (lx >= g.px) continue;
      // the three source coordinates: z is taken modulo the ring, so one linear stride along output x is not enough
      int sz = sw_pick(fz, lz, ly, lx), sy = sw_pick(fy, lz, ly, lx), sx = sw_pick(fx, lz, ly, lx);
      if (mz) sz = g.pz - 1 - sz;
      if (my) sy = g.py - 1 - sy;
      if (mx) sx = g.px - 1 - sx;
      const int zr = (p.oz[b] + sz) % g.R;
      val[i] = sw_scale(src[((long)zr * g.Y + p.oy[b] + sy) * g.X + p.ox[b] + sx], g.div);
    }
    if (quad) sw_store_quad<true>(dst + x0, 4, val);
    else sw_store_quad<false>(dst + x0, g.px - x0, val);
  } else {
    const int zr = (p.oz[b] + lz) % g.R;
    const T* src = slab + (((long)ci * g.R + zr) * g.Y + p.oy[b] + ly) * g.X + p.ox[b];
    if (quad) {
      // patch origins put the source row at any alignment: four coalesced scalar loads, one 16-byte store
      float val[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) val[i] = sw_scale(src[x0 + i], g.div);
      sw_store_quad<true>(dst + x0, 4, val);
    } else {
      for (int i = 0; i < 4 && x0 + i < g.px; ++i) dst[x0 + i] = sw_scale(src[x0 + i], g.div);
    }
  }
}

// zscore: per-patch (sum, sum of squares) in fp64, fixed order (thread-strided loop, xor-shuffle, waves in index order), then
// one block per patch slice sums the chunk partials in index order and applies (x - mean) / max(std, 1e-10) in place
__global__ __launch_bounds__(RX_SW_BLOCK) void sw_stat_partial_kernel(const float* __restrict__ x, long n, double* __restrict__ part) {
  const int b = blockIdx.y, chunk = blockIdx.x;
  const long per = (n + gridDim.x - 1) / gridDim.x;
  const long lo = chunk * per, hi = lo + per < n ? lo + per : n;
  const float* xb = x + (long)b * n;
  double s = 0.0, s2 = 0.0;
  for (long i = lo + threadIdx.x; i < hi; i += RX_SW_BLOCK) {
    const double v = xb[i];
    s += v;
    s2 += v * v;
  }
  s = wave_sum_d(s);
  s2 = wave_sum_d(s2);
  __shared__ double red[2][RX_SW_BLOCK / RX_WAVE];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) red[0][wave] = s, red[1][wave] = s2;
  __syncthreads();
  if (threadIdx.x == 0) {
    double a = 0.0, a2 = 0.0;
    for (int w = 0; w < RX_SW_BLOCK / RX_WAVE; ++w) a += red[0][w], a2 += red[1][w];
    part[((long)b * gridDim.x + chunk) * 2] = a;
    part[((long)b * gridDim.x + chunk) * 2 + 1] = a2;
  }
}

__global__ __launch_bounds__(RX_SW_BLOCK) void sw_standardize_kernel(float* __restrict__ x, long n, const double* __restrict__ part,
                                                                      int chunks) {
  const int b = blockIdx.y;
  __shared__ float ms[2];
  if (threadIdx.x == 0) {
    double s = 0.0, s2 = 0.0;
    for (int c = 0; c < chunks; ++c) s += part[((long)b * chunks + c) * 2], s2 += part[((long)b * chunks + c) * 2 + 1];
    const double mean = s / (double)n;
    double var = s2 / (double)n - mean * mean;
    if (var < 0.0) var = 0.0;
    const float sd = (float)sqrt(var);
    ms[0] = (float)mean;
    ms[1] = sd > 1e-10f ? sd : 1e-10f;
  }
  __syncthreads();
  const float mean = ms[0], sd = ms[1];
  float* xb = x + (long)b * n;
  const long nq = n / 4;
  if ((n & 3) == 0) {       // each patch starts 16-byte aligned
    for (long i = (long)blockIdx.x * RX_SW_BLOCK + threadIdx.x; i < nq; i += (long)gridDim.x * RX_SW_BLOCK) {
      f32x4 v = *reinterpret_cast<const f32x4*>(xb + 4 * i);
#pragma unroll
      for (int k = 0; k < 4; ++k) v[k] = (v[k] - mean) / sd;
      *reinterpret_cast<f32x4*>(xb + 4 * i) = v;
    }
  } else {
    for (long i = (long)blockIdx.x * RX_SW_BLOCK + threadIdx.x; i < n; i += (long)gridDim.x * RX_SW_BLOCK) xb[i] = (xb[i] - mean) / sd;
  }
}

static int sw_stat_chunks(long n) {
  long c = (n + 4 * RX_SW_BLOCK - 1) / (4 * RX_SW_BLOCK);
  return (int)(c < 1 ? 1 : c > RX_SW_STAT_CHUNKS ? RX_SW_STAT_CHUNKS : c);
}

extern "C" size_t rx_sw_gather_workspace(int batch, int cin, int pz, int py, int px) {
  if (batch < 1 || cin < 1 || pz < 1 || py < 1 || px < 1) return 0;
  return (size_t)batch * sw_stat_chunks((long)cin * pz * py * px) * 2 * sizeof(double);
}

// `geom`: the call has a record table (`ops`, refused when null); `who`: the entry point that was called, for its messages
static int sw_gather_impl(int in_dtype, const void* slab, int cin, int ring, int y, int x, int batch, const int32_t* origins, int pz,
                          int py, int px, int norm, float* out, void* ws, size_t ws_bytes, void* stream, bool geom,
                          const rx_geom_sample* ops, const char* who) {
  if (!slab || !out || cin < 1 || ring < 1 || y < 1 || x < 1) RX_FAIL(RX_EINVAL, "%s: bad arguments", who);
  if (in_dtype < RX_SW_U8 || in_dtype > RX_SW_F32) RX_FAIL(RX_EINVAL, "%s: unknown input dtype %d", who, in_dtype);
  if (norm != RX_SW_SCALE && norm != RX_SW_ZSCORE) RX_FAIL(RX_EINVAL, "%s: unknown normalization %d", who, norm);
  if ((uintptr_t)out & 15) RX_FAIL(RX_EINVAL, "%s: output must be 16-byte aligned", who);
  SwPatches p;
  if (int rc = sw_patches(origins, batch, ring, y, x, pz, py, px, p, who)) return rc;
  SwViews v;
  memset(&v, 0, sizeof(v));
  if (geom) {
    if (int rc = sw_records(ops, batch, pz, py, px, who)) return rc;
    for (int b = 0; b < batch; ++b) {
      const RxGeomInverse r = rx_geom_inverse(ops[b]);
      for (int a = 0; a < 3; ++a) v.from[b][a] = r.from[a], v.flip[b][a] = r.flip[a];
    }
  }
  const long n = (long)cin * pz * py * px;
  if (norm == RX_SW_ZSCORE && (!ws || ws_bytes < rx_sw_gather_workspace(batch, cin, pz, py, px)))
    RX_FAIL(RX_EWORKSPACE, "%s: zscore needs rx_sw_gather_workspace() bytes of workspace", who);
  hipStream_t st = (hipStream_t)stream;
  GatherGeom g;
  g.cin = cin, g.R = ring, g.Y = y, g.X = x, g.pz = pz, g.py = py, g.px = px, g.pxq = (px + 3) / 4;
  g.div = in_dtype == RX_SW_U8 ? 255.f : in_dtype == RX_SW_U16 ? 65535.f : 0.f;
  g.total = (long)batch * cin * pz * py * g.pxq;
  const dim3 grid((unsigned)((g.total + RX_SW_BLOCK - 1) / RX_SW_BLOCK));
  sw_typed(in_dtype, slab, [&](auto* s) {
    using T = SwElem<decltype(s)>;
    if (geom) hipLaunchKernelGGL(HIP_KERNEL_NAME(sw_gather_kernel<T, true>), grid, dim3(RX_SW_BLOCK), 0, st, s, out, g, p, v);
    else hipLaunchKernelGGL(HIP_KERNEL_NAME(sw_gather_kernel<T, false>), grid, dim3(RX_SW_BLOCK), 0, st, s, out, g, p, SwNone{});
  });
  if (norm == RX_SW_ZSCORE) {      // of the patch as gathered: a transformed patch holds the same multiset of values
    const int chunks = sw_stat_chunks(n);
    hipLaunchKernelGGL(sw_stat_partial_kernel, dim3(chunks, batch), dim3(RX_SW_BLOCK), 0, st, (const float*)out, n, (double*)ws);
    long gx = (n / 4 + RX_SW_BLOCK - 1) / RX_SW_BLOCK;
    gx = gx < 1 ? 1 : gx > 1024 ? 1024 : gx;
    hipLaunchKernelGGL(sw_standardize_kernel, dim3((unsigned)gx, batch), dim3(RX_SW_BLOCK), 0, st, out, n, (const double*)ws, chunks);
  }
  RX_CHECK_LAUNCH(who);
  return RX_OK;
}

extern "C" int rx_sw_gather(int in_dtype, const void* slab, int cin, int ring, int y, int x, int batch, const int32_t* origins,
                            int pz, int py, int px, int norm, float* out, void* ws, size_t ws_bytes, void* stream) {
  return sw_gather_impl(in_dtype, slab, cin, ring, y, x, batch, origins, pz, py, px, norm, out, ws, ws_bytes, stream, false, nullptr, "rx_sw_gather");
}

extern "C" int rx_sw_gather_geom(int in_dtype, const void* slab, int cin, int ring, int y, int x, int batch, const int32_t* origins,
                                 const rx_geom_sample* ops, int pz, int py, int px, int norm, float* out, void* ws, size_t ws_bytes,
                                 void* stream) {
  return sw_gather_impl(in_dtype, slab, cin, ring, y, x, batch, origins, pz, py, px, norm, out, ws, ws_bytes, stream, true, ops, "rx_sw_gather_geom");
}

// ---- accumulate -----------------------------------------------------------------------------------------------------
struct AccGeom {
  int c, pz, py, px, R, Y, X, act, npatch;
  int bz0, by0, bx0;        // bounding box origin (bx0 rounded down to a multiple of 4 on the vector path)
  int bny, bnq;             // rows and x-quads of the box
  int bx1;                  // exclusive x end of the box
  long total;               // box rows * bny * bnq
};
// GEOM: slot b's destination local voxel (lz, ly, lx) reads the logit at base + lz * sz + ly * sy + lx * sx of one channel volume;
// destination channel ch of a `vector` task takes the ACTIVATED view-frame channel ch[ch], its sign bit flipped where bit ch of neg is
// set.  The weight stays in the destination frame.
struct SwAccViews {
  RxGeomView s[RX_SW_MAXB];
  int vector;
};

__device__ inline float sw_sigmoid(float v) { return 1.f / (1.f + expf(-v)); }

// offset (lz*py + ly)*px + lx of voxel (z, y, x) in patch b, or -1 outside it.  b is wave-uniform: the origins are scalar loads.
__device__ inline int sw_local(const AccGeom& g, const SwPatches& p, int b, int z, int y, int x) {
  const int lz = z - p.oz[b], ly = y - p.oy[b], lx = x - p.ox[b];
  return (lz >= 0 && lz < g.pz && ly >= 0 && ly < g.py && lx >= 0 && lx < g.px) ? (lz * g.py + ly) * g.px + lx : -1;
}

// channel ch of one patch's logits `lb` (c channel volumes of pvol) at offset l, activated over the channels of that voxel
__device__ inline float sw_activate(const float* __restrict__ lb, long pvol, int c, int act, int ch, int l) {
  float pr = lb[ch * pvol + l];
  if (act == RX_ACT_SIGMOID) {
    pr = sw_sigmoid(pr);
  } else if (act == RX_ACT_SOFTMAX) {   // torch.softmax over the channels: exp(x - max) / sum exp(x - max)
    float mx = lb[l];
    for (int k = 1; k < c; ++k) mx = fmaxf(mx, lb[k * pvol + l]);
    float den = 0.f;
    for (int k = 0; k < c; ++k) den = den + expf(lb[k * pvol + l] - mx);
    pr = expf(pr - mx) / den;
  }
  return pr;
}

template <bool VEC, bool GEOM>
__global__ __launch_bounds__(RX_SW_BLOCK) void sw_accumulate_kernel(const float* __restrict__ logits, const float* __restrict__ w,
                                                                    float* __restrict__ sum, float* __restrict__ wsum, AccGeom g,
                                                                    SwPatches p, SwTable<GEOM, SwAccViews> v) {
  const long q = (long)blockIdx.x * RX_SW_BLOCK + threadIdx.x;
  if (q >= g.total) return;
  const int xq = (int)(q % g.bnq);
  const int yy = (int)((q / g.bnq) % g.bny);
  const int z = g.bz0 + (int)(q / ((long)g.bnq * g.bny));
  const int y = g.by0 + yy, x0 = g.bx0 + 4 * xq;
  const long plane = (long)g.Y * g.X, cstride = (long)g.R * plane;
  const long base = (long)(z % g.R) * plane + (long)y * g.X + x0;
  const long pvol = (long)g.pz * g.py * g.px;
  // quads that straddle the box edge: only voxels inside [bx0, bx1) are read and written on the scalar path; on the vector path
  // the whole quad is inside the row (X % 4 == 0) and voxels no patch covers are written back unchanged
  const int nx = g.bx1 - x0;
  float a[4];
  if (wsum) {
    sw_load_quad<VEC>(wsum + base, nx, a);
    for (int b = 0; b < g.npatch; ++b)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int l = sw_local(g, p, b, z, y, x0 + i);
        if (l >= 0) a[i] = a[i] + w[l];
      }
    sw_store_quad<VEC>(wsum + base, nx, a);
  }
  for (int ch = 0; ch < g.c; ++ch) {
    float* sp = sum + ch * cstride + base;
    sw_load_quad<VEC>(sp, nx, a);
    for (int b = 0; b < g.npatch; ++b) {
      const float* lb = logits + (long)b * g.c * pvol;
      // the logit of a destination voxel: without records at the weight's offset, channel ch, as it is
      int chs = ch, row = 0, sx = 0;
      uint32_t sign = 0u;
      if constexpr (GEOM) {
        const RxGeomView& s = v.s[b];
        if (v.vector) {
          chs = ch == 0 ? s.ch[0] : ch == 1 ? s.ch[1] : s.ch[2];
          sign = ((s.neg >> ch) & 1u) << 31;
        }
        row = s.base + (z - p.oz[b]) * s.sz + (y - p.oy[b]) * s.sy, sx = s.sx;      // offset of destination x = ox[b], step along x
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int l = sw_local(g, p, b, z, y, x0 + i);
        if (l < 0) continue;
        int li = l;
        if constexpr (GEOM) li = row + (x0 + i - p.ox[b]) * sx;
        float pr = sw_activate(lb, pvol, g.c, g.act, chs, li);
        if constexpr (GEOM) pr = __uint_as_float(__float_as_uint(pr) ^ sign);   // IEEE negation: 0.0 becomes -0.0
        a[i] = a[i] + w[l] * pr;
      }
    }
    sw_store_quad<VEC>(sp, nx, a);
  }
}

// the least and the greatest origin per axis of the first `valid` patches
struct SwBox {
  int z0, z1, y0, y1, x0, x1;
};
static SwBox sw_bbox(const SwPatches& p, int valid) {
  SwBox k = {p.oz[0], p.oz[0], p.oy[0], p.oy[0], p.ox[0], p.ox[0]};
  for (int b = 1; b < valid; ++b) {
    k.z0 = p.oz[b] < k.z0 ? p.oz[b] : k.z0, k.z1 = p.oz[b] > k.z1 ? p.oz[b] : k.z1;
    k.y0 = p.oy[b] < k.y0 ? p.oy[b] : k.y0, k.y1 = p.oy[b] > k.y1 ? p.oy[b] : k.y1;
    k.x0 = p.ox[b] < k.x0 ? p.ox[b] : k.x0, k.x1 = p.ox[b] > k.x1 ? p.ox[b] : k.x1;
  }
  return k;
}

// `geom`, `who`: as sw_gather_impl.  All `batch` records are checked, the first `valid` are lowered.
static int sw_accumulate_impl(const float* logits, int batch, int valid, int c, int pz, int py, int px, const int32_t* origins, int act,
                              const float* weight, float* sum, float* wsum, int ring, int y, int x, void* stream, bool geom,
                              const rx_geom_sample* ops, int vector, const char* who) {
  if (!logits || !weight || !sum || c < 1 || ring < 1 || y < 1 || x < 1 || valid < 0 || valid > batch)
    RX_FAIL(RX_EINVAL, "%s: bad arguments", who);
  if (act != RX_ACT_NONE && act != RX_ACT_SIGMOID && act != RX_ACT_SOFTMAX) RX_FAIL(RX_EINVAL, "%s: unknown activation %d", who, act);
  if (geom && vector && c != 3) RX_FAIL(RX_EINVAL, "%s: a vector task has 3 channels, not %d", who, c);
  SwPatches p;
  if (int rc = sw_patches(origins, batch, ring, y, x, pz, py, px, p, who)) return rc;
  if (geom) {
    if (int rc = sw_records(ops, batch, pz, py, px, who)) return rc;
    if ((long)c * pz * py * px > 0x7fffffffL) RX_FAIL(RX_EINVAL, "%s: c * pz * py * px must stay below 2^31", who);
  }
  if (valid == 0) return RX_OK;
  const SwBox k = sw_bbox(p, valid);
  // every row of the box must own a ring row of its own: rows [z0, z1 + pz) are live together
  if (k.z1 + pz - k.z0 > ring) RX_FAIL(RX_EINVAL, "%s: patches span %d rows, the ring holds %d", who, k.z1 + pz - k.z0, ring);
  const bool vec = (x & 3) == 0 && ((uintptr_t)sum & 15) == 0 && (!wsum || ((uintptr_t)wsum & 15) == 0);
  AccGeom g;
  g.c = c, g.pz = pz, g.py = py, g.px = px, g.R = ring, g.Y = y, g.X = x, g.act = act, g.npatch = valid;
  g.bz0 = k.z0, g.by0 = k.y0, g.bx0 = vec ? (k.x0 & ~3) : k.x0, g.bx1 = k.x1 + px;
  g.bny = k.y1 + py - k.y0, g.bnq = (g.bx1 - g.bx0 + 3) / 4;
  g.total = (long)(k.z1 + pz - k.z0) * g.bny * g.bnq;
  const dim3 grid((unsigned)((g.total + RX_SW_BLOCK - 1) / RX_SW_BLOCK));
  hipStream_t st = (hipStream_t)stream;
  auto launch = [&](auto kernel, const auto& table) {
    hipLaunchKernelGGL(kernel, grid, dim3(RX_SW_BLOCK), 0, st, logits, weight, sum, wsum, g, p, table);
  };
  if (geom) {
    SwAccViews v;
    memset(&v, 0, sizeof(v));
    for (int b = 0; b < valid; ++b) v.s[b] = rx_geom_lower(ops[b], pz, py, px);
    v.vector = vector ? 1 : 0;
    if (vec) launch(sw_accumulate_kernel<true, true>, v);
    else launch(sw_accumulate_kernel<false, true>, v);
  } else {
    if (vec) launch(sw_accumulate_kernel<true, false>, SwNone{});
    else launch(sw_accumulate_kernel<false, false>, SwNone{});
  }
  RX_CHECK_LAUNCH(who);
  return RX_OK;
}

extern "C" int rx_sw_accumulate(const float* logits, int batch, int valid, int c, int pz, int py, int px, const int32_t* origins,
                                int act, const float* weight, float* sum, float* wsum, int ring, int y, int x, void* stream) {
  return sw_accumulate_impl(logits, batch, valid, c, pz, py, px, origins, act, weight, sum, wsum, ring, y, x, stream, false, nullptr, 0, "rx_sw_accumulate");
}

extern "C" int rx_sw_accumulate_geom(const float* logits, int batch, int valid, int c, int pz, int py, int px, const int32_t* origins,
                                     const rx_geom_sample* ops, int vector, int act, const float* weight, float* sum, float* wsum,
                                     int ring, int y, int x, void* stream) {
  return sw_accumulate_impl(logits, batch, valid, c, pz, py, px, origins, act, weight, sum, wsum, ring, y, x, stream, true, ops, vector, "rx_sw_accumulate_geom");
}

// ---- finalize -------------------------------------------------------------------------------------------------------
struct FinGeom {
  int c, R, z0, rows, blend, cast, reset;
  long plane, qpr, nq;      // voxels per row; quads per row; quads per launch
};

__device__ inline float sw_cast_val(float v, int cast) {
  if (cast == RX_SW_CAST_U16) {
    const float t = (v + 1.0f) / 2.0f * 65535.0f;
    return fminf(fmaxf(t, 0.f), 65535.f);
  }
  return fminf(fmaxf(v * 255.0f, 0.f), 255.f);
}

template <bool VEC>
__global__ __launch_bounds__(RX_SW_BLOCK) void sw_finalize_kernel(float* __restrict__ sum, float* __restrict__ wsum,
                                                                  float* __restrict__ blended, void* __restrict__ final_out,
                                                                  float* __restrict__ wsum_out, FinGeom g) {
  const long q = (long)blockIdx.x * RX_SW_BLOCK + threadIdx.x;
  if (q >= g.nq) return;
  const int row = (int)(q / g.qpr);
  const long v0 = (q % g.qpr) * 4;
  const long src = (long)((g.z0 + row) % g.R) * g.plane + v0, dst = (long)row * g.plane + v0;
  const long cs = (long)g.R * g.plane, os = (long)g.rows * g.plane;
  const int nv = g.plane - v0 < 4 ? (int)(g.plane - v0) : 4;
  float wv[4];
  sw_load_quad<VEC>(wsum + src, nv, wv);
  float mag[4] = {1.f, 1.f, 1.f, 1.f};
  if (g.blend == RX_SW_BLEND_UNIT) {   // sqrt(s0^2 + s1^2 + s2^2) + 1e-8, the oracle's order of operations
    for (int i = 0; i < nv; ++i) {
      const float a = sum[src + i], b = sum[cs + src + i], c = sum[2 * cs + src + i];
      mag[i] = sqrtf(a * a + b * b + c * c) + 1e-8f;
    }
  }
  for (int ch = 0; ch < g.c; ++ch) {
    float s[4];
    float* sp = sum + ch * cs + src;
    sw_load_quad<VEC>(sp, nv, s);
    float o[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float v = s[i];
      if (wv[i] > 0.f) {
        if (g.blend == RX_SW_BLEND_AVERAGE) v = v / wv[i];
        else if (g.blend == RX_SW_BLEND_UNIT) v = v / mag[i];
      }
      o[i] = v;
    }
    float* bp = blended + ch * os + dst;
    if (VEC) {
      *reinterpret_cast<f32x4*>(bp) = f32x4{o[0], o[1], o[2], o[3]};
      if (g.reset) *reinterpret_cast<f32x4*>(sp) = f32x4{0.f, 0.f, 0.f, 0.f};
    } else {
      for (int i = 0; i < nv; ++i) {
        bp[i] = o[i];
        if (g.reset) sp[i] = 0.f;
      }
    }
    if (g.cast == RX_SW_CAST_U16) {   // clip, then truncation toward zero as numpy's astype
      uint16_t* fp = (uint16_t*)final_out + ch * os + dst;
      uint32_t u[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) u[i] = (uint32_t)(int)sw_cast_val(o[i], g.cast);
      if (VEC) *reinterpret_cast<u32x2*>(fp) = u32x2{u[0] | (u[1] << 16), u[2] | (u[3] << 16)};
      else for (int i = 0; i < nv; ++i) fp[i] = (uint16_t)u[i];
    } else {
      uint8_t* fp = (uint8_t*)final_out + ch * os + dst;
      uint32_t u[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) u[i] = (uint32_t)(int)sw_cast_val(o[i], g.cast);
      if (VEC) *reinterpret_cast<uint32_t*>(fp) = u[0] | (u[1] << 8) | (u[2] << 16) | (u[3] << 24);
      else for (int i = 0; i < nv; ++i) fp[i] = (uint8_t)u[i];
    }
  }
  if (wsum_out) sw_store_quad<VEC>(wsum_out + dst, nv, wv);
  if (g.reset == 2) {
    if (VEC) *reinterpret_cast<f32x4*>(wsum + src) = f32x4{0.f, 0.f, 0.f, 0.f};
    else for (int i = 0; i < nv; ++i) wsum[src + i] = 0.f;
  }
}

extern "C" int rx_sw_finalize(float* sum, float* wsum, int c, int ring, int y, int x, int z0, int rows, int blend, int cast,
                              int reset, float* blended, void* final_out, float* wsum_out, void* stream) {
  if (!sum || !wsum || !blended || !final_out || c < 1 || ring < 1 || y < 1 || x < 1 || z0 < 0 || rows < 0 || rows > ring)
    RX_FAIL(RX_EINVAL, "rx_sw_finalize: bad arguments");
  if (blend < RX_SW_BLEND_AVERAGE || blend > RX_SW_BLEND_NONE) RX_FAIL(RX_EINVAL, "rx_sw_finalize: unknown blend %d", blend);
  if (blend == RX_SW_BLEND_UNIT && c != 3) RX_FAIL(RX_EINVAL, "rx_sw_finalize: unit-length blending needs 3 channels (got %d)", c);
  if (cast != RX_SW_CAST_U8 && cast != RX_SW_CAST_U16) RX_FAIL(RX_EINVAL, "rx_sw_finalize: unknown cast %d", cast);
  if (reset < 0 || reset > 2) RX_FAIL(RX_EINVAL, "rx_sw_finalize: reset must be 0, 1 or 2");
  if (rows == 0) return RX_OK;
  FinGeom g;
  g.c = c, g.R = ring, g.z0 = z0, g.rows = rows, g.blend = blend, g.cast = cast, g.reset = reset;
  g.plane = (long)y * x;
  g.qpr = (g.plane + 3) / 4;
  g.nq = g.qpr * rows;
  const uintptr_t al = (uintptr_t)sum | (uintptr_t)wsum | (uintptr_t)blended | (uintptr_t)(wsum_out ? wsum_out : blended);
  const bool vec = (g.plane & 3) == 0 && (al & 15) == 0 && ((uintptr_t)final_out & 7) == 0;
  const dim3 grid((unsigned)((g.nq + RX_SW_BLOCK - 1) / RX_SW_BLOCK));
  hipStream_t st = (hipStream_t)stream;
  if (vec)
    hipLaunchKernelGGL(sw_finalize_kernel<true>, grid, dim3(RX_SW_BLOCK), 0, st, sum, wsum, blended, final_out, wsum_out, g);
  else
    hipLaunchKernelGGL(sw_finalize_kernel<false>, grid, dim3(RX_SW_BLOCK), 0, st, sum, wsum, blended, final_out, wsum_out, g);
  RX_CHECK_LAUNCH("rx_sw_finalize");
  return RX_OK;
}

// ---- occupancy (empty-patch skipping) -------------------------------------------------------------------------------------------
// counts[p] = the raw voxels v of patch p, over all channels, with float(v) > value (a float compare: a NaN never counts; uint8 and
// uint16 are exact in fp32).  Host statement: inference.occupancy_numpy.  A patch is cin * pz * py x-runs of px voxels; a run is cut
// at the 16-byte boundaries of its own address, so a unit of work is one aligned 16-byte window: a window that lies inside the run
// is one vector load, the partial windows at its two ends (the scalar head and tail) are read voxel by voxel -- nothing outside
// a run is read.  Workgroup (chunk, p) strides over the units of patch p; lane -> wave (xor shuffles) -> workgroup (LDS) -> ONE
// 64-bit integer atomicAdd per workgroup: integer adds are order-free, so the counts are exact and reproducible.  The origins
// travel by value, RX_OCC_MAXP patches per launch: no device table, copy, allocation or synchronisation.
#define RX_OCC_MAXP 256
#define RX_OCC_CHUNKS 64      // at most this many workgroups per patch
#define RX_OCC_UNITS 8        // units per lane before a patch is cut into another chunk

struct OccPatches {
  int32_t oz[RX_OCC_MAXP], oy[RX_OCC_MAXP], ox[RX_OCC_MAXP];
};
struct OccGeom {
  int cin, R, Y, X, pz, py, px;
  int seg;          // aligned 16-byte windows a run can touch
  long rows, units; // cin * pz * py; rows * seg
  float value;
};

template <typename T>
__device__ inline unsigned occ_vec(const u32x4& v, float value);
template <>
__device__ inline unsigned occ_vec<uint8_t>(const u32x4& v, float value) {
  unsigned c = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int k = 0; k < 4; ++k) c += (float)((v[j] >> (8 * k)) & 0xffu) > value ? 1u : 0u;
  return c;
}
template <>
__device__ inline unsigned occ_vec<uint16_t>(const u32x4& v, float value) {
  unsigned c = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) c += ((float)(v[j] & 0xffffu) > value ? 1u : 0u) + ((float)(v[j] >> 16) > value ? 1u : 0u);
  return c;
}
template <>
__device__ inline unsigned occ_vec<float>(const u32x4& v, float value) {
  unsigned c = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) c += __uint_as_float(v[j]) > value ? 1u : 0u;
  return c;
}

template <typename T>
__global__ __launch_bounds__(RX_SW_BLOCK) void sw_occupancy_kernel(const T* __restrict__ slab, OccGeom g, OccPatches p,
                                                                   unsigned long long* __restrict__ counts) {
  __shared__ unsigned long long s_cnt[RX_SW_BLOCK / RX_WAVE];
  const int b = blockIdx.y;
  const int oz = p.oz[b], oy = p.oy[b], ox = p.ox[b];
  unsigned long long cnt = 0;
  for (long u = (long)blockIdx.x * RX_SW_BLOCK + threadIdx.x; u < g.units; u += (long)gridDim.x * RX_SW_BLOCK) {
    long r = u / g.seg;
    const int s = (int)(u - r * g.seg);
    const int ly = (int)(r % g.py);
    r /= g.py;
    const int lz = (int)(r % g.pz);
    const int ci = (int)(r / g.pz);
    const T* row = slab + (((long)ci * g.R + (oz + lz) % g.R) * g.Y + oy + ly) * g.X + ox;
    const uintptr_t a0 = (uintptr_t)row, a1 = a0 + (uintptr_t)g.px * sizeof(T);
    const uintptr_t w0 = (a0 & ~(uintptr_t)15) + (uintptr_t)16 * s, w1 = w0 + 16;
    const uintptr_t lo = w0 > a0 ? w0 : a0, hi = w1 < a1 ? w1 : a1;
    if (lo >= hi) continue;
    if (hi - lo == 16) {
      cnt += occ_vec<T>(*reinterpret_cast<const u32x4*>(lo), g.value);
    } else {
      for (const T* q = reinterpret_cast<const T*>(lo); q < reinterpret_cast<const T*>(hi); ++q) cnt += (float)*q > g.value ? 1u : 0u;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) s_cnt[wave] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 1; w < RX_SW_BLOCK / RX_WAVE; ++w) cnt += s_cnt[w];
    if (cnt) atomicAdd(counts + b, cnt);
  }
}

extern "C" int rx_sw_occupancy(int in_dtype, const void* slab, int cin, int ring, int y, int x, int n_pos, const int32_t* origins,
                               int pz, int py, int px, float value, uint64_t* counts, void* stream) {
  if (!slab || !counts || cin < 1 || ring < 1 || y < 1 || x < 1) RX_FAIL(RX_EINVAL, "rx_sw_occupancy: bad arguments");
  if (in_dtype < RX_SW_U8 || in_dtype > RX_SW_F32) RX_FAIL(RX_EINVAL, "rx_sw_occupancy: unknown input dtype %d", in_dtype);
  if (n_pos < 0 || (n_pos > 0 && !origins)) RX_FAIL(RX_EINVAL, "rx_sw_occupancy: n_pos must be >= 0 and the origin table non-null");
  if (pz < 1 || py < 1 || px < 1 || pz > ring || py > y || px > x)
    RX_FAIL(RX_EINVAL, "rx_sw_occupancy: patch (%d,%d,%d) does not fit the slab (ring %d, %d, %d)", pz, py, px, ring, y, x);
  const int esize = in_dtype == RX_SW_U8 ? 1 : in_dtype == RX_SW_U16 ? 2 : 4;
  if ((uintptr_t)slab & (uintptr_t)(esize - 1)) RX_FAIL(RX_EINVAL, "rx_sw_occupancy: the slab must be aligned to its %d-byte element", esize);
  if ((uintptr_t)counts & 7) RX_FAIL(RX_EINVAL, "rx_sw_occupancy: counts must be 8-byte aligned");
  if (n_pos == 0) return RX_OK;
  int zmin = origins[0], zmax = origins[0];
  for (int i = 0; i < n_pos; ++i) {
    const int z = origins[3 * i], yy = origins[3 * i + 1], xx = origins[3 * i + 2];
    if (z < 0 || yy < 0 || xx < 0 || yy > y - py || xx > x - px)
      RX_FAIL(RX_EINVAL, "rx_sw_occupancy: patch %d at (%d,%d,%d) leaves the slab (%d, %d)", i, z, yy, xx, y, x);
    zmin = z < zmin ? z : zmin, zmax = z > zmax ? z : zmax;
  }
  // the rows [min z, max z + pz) of the call are live together: each needs a ring row of its own
  if ((long)zmax + pz - zmin > ring)
    RX_FAIL(RX_EINVAL, "rx_sw_occupancy: patches span %ld rows, the ring holds %d", (long)zmax + pz - zmin, ring);
  hipStream_t st = (hipStream_t)stream;
  hipError_t e = hipMemsetAsync(counts, 0, (size_t)n_pos * sizeof(uint64_t), st);
  if (e != hipSuccess) RX_FAIL(RX_ELAUNCH, "rx_sw_occupancy: zeroing the counts: %s", hipGetErrorString(e));
  OccGeom g;
  g.cin = cin, g.R = ring, g.Y = y, g.X = x, g.pz = pz, g.py = py, g.px = px, g.value = value;
  g.seg = (int)(((long)px * esize + 15) / 16) + 1;      // a run of n bytes at any alignment touches at most ceil(n / 16) + 1 windows
  g.rows = (long)cin * pz * py;
  g.units = g.rows * g.seg;
  long chunks = (g.units + (long)RX_SW_BLOCK * RX_OCC_UNITS - 1) / ((long)RX_SW_BLOCK * RX_OCC_UNITS);
  chunks = chunks < 1 ? 1 : chunks > RX_OCC_CHUNKS ? RX_OCC_CHUNKS : chunks;
  for (int i0 = 0; i0 < n_pos; i0 += RX_OCC_MAXP) {
    const int n = n_pos - i0 < RX_OCC_MAXP ? n_pos - i0 : RX_OCC_MAXP;
    OccPatches p;
    memset(&p, 0, sizeof(p));
    for (int i = 0; i < n; ++i) p.oz[i] = origins[3 * (i0 + i)], p.oy[i] = origins[3 * (i0 + i) + 1], p.ox[i] = origins[3 * (i0 + i) + 2];
    const dim3 grid((unsigned)chunks, (unsigned)n);
    unsigned long long* out = (unsigned long long*)counts + i0;
    sw_typed(in_dtype, slab, [&](auto* s) {
      hipLaunchKernelGGL(sw_occupancy_kernel<SwElem<decltype(s)>>, grid, dim3(RX_SW_BLOCK), 0, st, s, g, p, out);
    });
  }
  RX_CHECK_LAUNCH("rx_sw_occupancy");
  return RX_OK;
}
