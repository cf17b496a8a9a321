// rx_pointwise.hip -- the convolutions WITHOUT a spatial footprint on one streaming kernel (16-bit types):
//   * nn.ConvTranspose3d with kernel == stride (decoder.py:110-113,146):   y[s*v + t][co] = sum_ci x[v][ci] W[t][co][ci] + b[co]
//   * 1x1x1 nn.Conv3d forward (skip projections, resblocks.py:89-104) and its data gradient (the same form on the swapped pack).
// The generic gather kernel (rx_igemm.hip) runs them as up to 8 single-tap GEMMs with a 64-byte K tile per barrier pair: at
// K = Ci = 64 that is two K steps per workgroup, and the 64 -> 32 transposed conv that writes the full-resolution concat half
// (268 MB) ran at 2.3 TB/s.  Here a wave owns 32 consecutive input voxels: their Ci channels are loaded ONCE, straight from
// global memory into the MFMA B fragments (16 bytes per lane and K step, no LDS), and stay in registers while the wave walks the
// taps; the weights of a 32-channel output block -- all taps, all Ci -- sit in LDS for the workgroup's whole life (rows padded
// by 16 bytes: 16 consecutive rows hit 16 distinct 4-bank groups).  Per tap: Ci/16 MFMAs 32x32x16, then the 32 x 32 tile leaves
// as 16-byte stores (rx_pair16).  Persistent over voxel tiles; HBM traffic = x once + y once.
#include "rx_common.h"
#include "rx_internal.h"

// PwGeom, RX_PW_MAXKS and which calls take this kernel (rx_pw_choose): rx_gather_plan.h

template <typename T>
__global__ __launch_bounds__(256) void pointwise_kernel(const T* __restrict__ in, const T* __restrict__ w, const float* __restrict__ bias,
                                                        T* __restrict__ out, const PwGeom g) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];      // [taps][32 co][Ci * 2 + 16 bytes]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int fr = lane & 31, fh = lane >> 5;
  const int ntaps = g.sz * g.sy * g.sx;
  const int pitch = g.Ci * 2 + 16;
  const int n0 = blockIdx.y * 32;
  const int cpr = g.Ci / 8;                           // 16-byte chunks per weight row
  for (int i = tid; i < ntaps * 32 * cpr; i += 256) {
    const int c = i % cpr, row = i / cpr;             // row = t * 32 + co
    const int t = row >> 5, co = row & 31;
    *reinterpret_cast<u32x4*>(smem + row * pitch + c * 16) =
        *reinterpret_cast<const u32x4*>(w + ((long)t * g.Co + n0 + co) * g.Ci + c * 8);
  }
  __syncthreads();
  const int KS = g.Ci >> 4;
  const long V = (long)g.Zi * g.Yi * g.Xi, NV = (long)g.N * V;
  float bv[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) bv[r] = bias ? bias[n0 + 8 * (r >> 2) + 4 * fh + (r & 3)] : 0.f;
  const unsigned char* wrow = smem + fr * pitch + fh * 16;
  for (int tile = blockIdx.x; tile < g.ntiles; tile += gridDim.x) {
    const long q = (long)tile * 128 + wave * 32 + fr;
    const bool ok = q < NV;
    const int n = ok ? (int)(q / V) : 0;
    const long v = ok ? q - (long)n * V : 0;
    const int x = (int)(v % g.Xi), y = (int)((v / g.Xi) % g.Yi), z = (int)(v / ((long)g.Xi * g.Yi));
    u32x4 bq[RX_PW_MAXKS];
    const T* ip = in + (long)n * g.in_ss + v * g.ldi + fh * 8;
#pragma unroll
    for (int ks = 0; ks < RX_PW_MAXKS; ++ks)
      if (ks < KS) bq[ks] = ok ? *reinterpret_cast<const u32x4*>(ip + ks * 16) : u32x4{0u, 0u, 0u, 0u};
    T* on = out + (long)n * g.out_ss + n0;
    for (int t = 0; t < ntaps; ++t) {
      const int c = t % g.sx, b = (t / g.sx) % g.sy, a = t / (g.sx * g.sy);
      const long ov = ((long)(z * g.sz + a) * g.Yo + (y * g.sy + b)) * g.Xo + (x * g.sx + c);
      T* op = on + ov * g.ldo;
      u32x2 oldv[4];
      if (g.accumulate && ok) {
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) oldv[g4] = *reinterpret_cast<const u32x2*>(op + 8 * g4 + 4 * fh);
      }
      f32x16 acc;
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[r] = 0.f;
      const unsigned char* wt = wrow + t * 32 * pitch;
#pragma unroll
      for (int ks = 0; ks < RX_PW_MAXKS; ++ks)
        if (ks < KS) Mma<T>::run(acc, *reinterpret_cast<const u32x4*>(wt + ks * 32), bq[ks]);
      u32x2 piece[4];
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4) {
        T vals[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          float f = acc[4 * g4 + i] + bv[4 * g4 + i];
          if (g.accumulate) f += Elem<T>::to_f(reinterpret_cast<const T*>(&oldv[g4])[i]);
          vals[i] = Elem<T>::from_f(f);
        }
        piece[g4] = *reinterpret_cast<u32x2*>(vals);
      }
      // lanes l and l + 32 hold the same voxel (both pass `ok` together): pair their 8-byte pieces into 16-byte stores
#pragma unroll
      for (int pr = 0; pr < 2; ++pr) {
        const u32x4 o16 = rx_pair16(piece[2 * pr], piece[2 * pr + 1]);
        if (ok) *reinterpret_cast<u32x4*>(op + 16 * pr + 8 * fh) = o16;
      }
    }
  }
}

int rx_pointwise_launch(const RxPwChoice& c, rx_dtype dt, const void* in, const void* w, const float* bias, void* out, hipStream_t st,
                        const char* who) {
  rx_note_kernel("pointwise_kernel");
#define RX_PW_ROW(TT)                                                                                                                  \
  {                                                                                                                                    \
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&pointwise_kernel<TT>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024); \
    hipLaunchKernelGGL((pointwise_kernel<TT>), dim3(c.grid[0], c.grid[1]), dim3(256), c.lds, st, (const TT*)in, (const TT*)w, bias, (TT*)out, c.g); \
  }
  if (dt == RX_BF16) RX_PW_ROW(bf16_t) else RX_PW_ROW(f16_t)
#undef RX_PW_ROW
  RX_CHECK_LAUNCH(who);
  return RX_OK;
}
