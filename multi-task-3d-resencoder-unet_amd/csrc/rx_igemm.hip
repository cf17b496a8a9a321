// rx_igemm.hip -- tap-table implicit GEMM on MFMA for every "forward-shaped" contraction of the
// hot path:  Conv3d forward (stride 1/2), Conv3d backward-data (stride 1: one launch; stride 2:
// one launch per output parity class), ConvTranspose3d(k=s) forward (one launch per phase) and
// backward-data.
//
//   D[co][q] = sum_{tap} sum_{ci} W[tap.w][co][ci] * In[ q*is + tap.d ][ci]      (zero outside)
//   Out[ q*os + op ][co] (+)= D[co][q] (+ bias[co])
//
// MFMA orientation: the WEIGHTS are the A operand (rows = output channels) and the gathered
// ACTIVATIONS the B operand (columns = voxels), so a lane of the 32x32 accumulator holds 4 runs of
// 4 consecutive output channels of ONE voxel -> channels-last stores of 8/16 bytes.
// fp32 mode uses v_mfma_f32_32x32x2_f32 (exact fp32 fma chain), bf16/f16 modes 32x32x16.
//
// Tiling: 256 threads = 4 waves; block tile BM voxels x BN channels; K tile = 64 bytes of input
// channels of one tap; LDS tiles are [row][64 B] with the 16-byte chunk index XOR-swizzled by
// (row>>2)&3 (conflict-free ds_read_b128 for the 32x32 operand fetch); register-staged double
// buffering (global loads of tile k+1 in flight under the MFMAs of tile k).
// Optional split-K (deep 4^3/8^3 layers: few voxels, 14 MB of weights): fp32 slabs + a
// deterministic reduce kernel.
#include <stdlib.h>

#include "rx_common.h"
#include "rx_internal.h"


// IgemmPhase / IgemmGeom, the geometry builders and the choice of kernel and split: rx_gather_plan.h

__device__ inline int swz(int row, int chunk) { return row * 4 + (chunk ^ ((row >> 2) & 3)); }

template <typename T, int BM, int BN>
__global__ __launch_bounds__(256) void igemm_kernel(const T* __restrict__ in, const T* __restrict__ w, const float* __restrict__ bias,
                                                    T* __restrict__ out, float* __restrict__ slab, const IgemmGeom g) {
  constexpr int P = Elem<T>::PER16;  // elements per 16 B
  constexpr int KB = 4 * P;          // input channels per K tile (64 B)
  constexpr int NB = BN / 32;        // channel blocks per wave
  constexpr int MV = BM / 128;       // voxel blocks per wave
  constexpr int XP = BM / 64;        // activation pieces per thread
  constexpr int WP = (BN + 63) / 64; // weight pieces per thread
  __shared__ u32x4 sX[2][BM * 4];
  __shared__ u32x4 sW[2][BN * 4];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int mt_all = blockIdx.x % g.total_mtiles, split = blockIdx.x / g.total_mtiles;
  int phase = 0;
  for (int i = 1; i < g.nph; ++i)
    if (mt_all >= g.ph[i].mtile0) phase = i;
  const IgemmPhase P_ = g.ph[phase];
  const int mtile = mt_all - P_.mtile0;
  const int m0 = mtile * BM, n0 = blockIdx.y * BN, n = blockIdx.z;
  const T* in_n = in + (long)n * g.in_ss;

  // ---- per-thread row geometry for the activation gather (fixed for the whole K loop)
  const int chunk = tid & 3;
  int rz[XP], ry[XP], rx[XP];
  bool rok[XP];
#pragma unroll
  for (int p = 0; p < XP; ++p) {
    int q = m0 + (tid >> 2) + 64 * p;
    rok[p] = q < P_.Vq;
    int qx = q % P_.Qx, t = q / P_.Qx;
    int qy = t % P_.Qy, qz = t / P_.Qy;
    rz[p] = qz * g.isz;
    ry[p] = qy * g.isy;
    rx[p] = qx * g.isx;
  }
  const int nkc = g.Ci / KB;
  const int nkt_all = P_.ntaps * nkc;
  const int kt_begin = (int)((long)nkt_all * split / g.ksplit);
  const int kt_end = (int)((long)nkt_all * (split + 1) / g.ksplit);

  u32x4 xr[XP], wr[WP];
  auto load_tile = [&](int kt) {
    const int tap = kt / nkc, cc = kt - tap * nkc;
    const RxTap tp = g.taps[P_.tap0 + tap];
#pragma unroll
    for (int p = 0; p < XP; ++p) {
      int z = rz[p] + tp.dz, y = ry[p] + tp.dy, x = rx[p] + tp.dx;
      bool ok = rok[p] && (unsigned)z < (unsigned)g.Zi && (unsigned)y < (unsigned)g.Yi && (unsigned)x < (unsigned)g.Xi;
      u32x4 v = u32x4{0u, 0u, 0u, 0u};
      if (ok) v = *reinterpret_cast<const u32x4*>(in_n + ((long)(z * g.Yi + y) * g.Xi + x) * g.ldi + cc * KB + chunk * P);
      xr[p] = v;
    }
#pragma unroll
    for (int p = 0; p < WP; ++p) {
      int row = (tid >> 2) + 64 * p;
      u32x4 v = u32x4{0u, 0u, 0u, 0u};
      if (row < BN) v = *reinterpret_cast<const u32x4*>(w + ((long)tp.w * g.Co + n0 + row) * g.Ci + cc * KB + chunk * P);
      wr[p] = v;
    }
  };
  auto store_tile = [&](int buf) {
#pragma unroll
    for (int p = 0; p < XP; ++p) sX[buf][swz((tid >> 2) + 64 * p, chunk)] = xr[p];
#pragma unroll
    for (int p = 0; p < WP; ++p) {
      int row = (tid >> 2) + 64 * p;
      if (row < BN) sW[buf][swz(row, chunk)] = wr[p];
    }
  };

  f32x16 acc[NB][MV];
#pragma unroll
  for (int a = 0; a < NB; ++a)
#pragma unroll
    for (int b = 0; b < MV; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;

  if (kt_begin < kt_end) {
    load_tile(kt_begin);
    store_tile(0);
  }
  __syncthreads();
  const int fr = lane & 31, fh = lane >> 5;
  for (int kt = kt_begin; kt < kt_end; ++kt) {
    const int buf = (kt - kt_begin) & 1;
    if (kt + 1 < kt_end) load_tile(kt + 1);
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      u32x4 af[NB], bf[MV];
#pragma unroll
      for (int a = 0; a < NB; ++a) af[a] = sW[buf][swz(a * 32 + fr, ks * 2 + fh)];
#pragma unroll
      for (int b = 0; b < MV; ++b) bf[b] = sX[buf][swz(wave * (BM / 4) + b * 32 + fr, ks * 2 + fh)];
#pragma unroll
      for (int a = 0; a < NB; ++a)
#pragma unroll
        for (int b = 0; b < MV; ++b) Mma<T>::run(acc[a][b], af[a], bf[b]);
    }
    if (kt + 1 < kt_end) store_tile(buf ^ 1);
    __syncthreads();
  }

  // ---- epilogue: lane holds voxel (lane&31) of each voxel block, channel runs 8*g4 + 4*fh + (0..3)
#pragma unroll
  for (int b = 0; b < MV; ++b) {
    const int q = m0 + wave * (BM / 4) + b * 32 + fr;
    if (q >= P_.Vq) continue;
    if (g.ksplit > 1) {
      float* sp = slab + P_.slab_off + (((long)split * gridDim.z + n) * P_.Vq + q) * g.Co + n0;
#pragma unroll
      for (int a = 0; a < NB; ++a)
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
          f32x4 v = {acc[a][b][4 * g4], acc[a][b][4 * g4 + 1], acc[a][b][4 * g4 + 2], acc[a][b][4 * g4 + 3]};
          *reinterpret_cast<f32x4*>(sp + a * 32 + 8 * g4 + 4 * fh) = v;
        }
      continue;
    }
    int qx = q % P_.Qx, t = q / P_.Qx;
    int qy = t % P_.Qy, qz = t / P_.Qy;
    long ov = ((long)(qz * g.osz + P_.opz) * g.Yo + (qy * g.osy + P_.opy)) * g.Xo + (qx * g.osx + P_.opx);
    T* op = out + (long)n * g.out_ss + ov * g.ldo + n0;
    auto epi = [&](auto HB, auto RA) {       // bias / accumulate as compile-time flags behind one uniform branch (RX_EPI_DISPATCH)
#pragma unroll
      for (int a = 0; a < NB; ++a)
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
          const int co = a * 32 + 8 * g4 + 4 * fh;
          f32x4 bv = {0.f, 0.f, 0.f, 0.f};
          if (decltype(HB)::value) bv = *reinterpret_cast<const f32x4*>(bias + n0 + co);
          T old4[4];
          if (decltype(RA)::value) {
            if (sizeof(T) == 2) *reinterpret_cast<u32x2*>(old4) = *reinterpret_cast<const u32x2*>(op + co);
            else *reinterpret_cast<u32x4*>(old4) = *reinterpret_cast<const u32x4*>(op + co);
          }
          T vals[4];
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            float f = acc[a][b][4 * g4 + i] + bv[i];
            if (decltype(RA)::value) f += Elem<T>::to_f(old4[i]);
            vals[i] = Elem<T>::from_f(f);
          }
          if (sizeof(T) == 2)
            *reinterpret_cast<u32x2*>(op + co) = *reinterpret_cast<u32x2*>(vals);
          else
            *reinterpret_cast<u32x4*>(op + co) = *reinterpret_cast<u32x4*>(vals);
        }
    };
    RX_EPI_DISPATCH(bias != nullptr, g.accumulate != 0, epi);
  }
}

// split-K reduce: out[q*os+op][c] (+)= sum_s slab[s][n][q][c] (+ bias); blockIdx.y = phase
template <typename T>
__global__ __launch_bounds__(256) void igemm_splitk_reduce(const float* __restrict__ slab, const float* __restrict__ bias, T* __restrict__ out,
                                                           const IgemmGeom g, int N) {
  const IgemmPhase P_ = g.ph[blockIdx.y];
  const int CV = g.Co / 4;
  const long total = (long)N * P_.Vq * CV;
  const float* sl = slab + P_.slab_off;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    int cv = (int)(i % CV);
    long nq = i / CV;
    int q = (int)(nq % P_.Vq), n = (int)(nq / P_.Vq);
    f32x4 s = {0.f, 0.f, 0.f, 0.f};
    for (int k = 0; k < g.ksplit; ++k) s += *reinterpret_cast<const f32x4*>(sl + (((long)k * N + n) * P_.Vq + q) * g.Co + cv * 4);
    int qx = q % P_.Qx, t = q / P_.Qx;
    int qy = t % P_.Qy, qz = t / P_.Qy;
    long ov = ((long)(qz * g.osz + P_.opz) * g.Yo + (qy * g.osy + P_.opy)) * g.Xo + (qx * g.osx + P_.opx);
    T* op = out + (long)n * g.out_ss + ov * g.ldo + cv * 4;
    T vals[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float f = s[j];
      if (bias) f += bias[cv * 4 + j];
      if (g.accumulate) f += Elem<T>::to_f(op[j]);
      vals[j] = Elem<T>::from_f(f);
    }
    if (sizeof(T) == 2)
      *reinterpret_cast<u32x2*>(op) = *reinterpret_cast<u32x2*>(vals);
    else
      *reinterpret_cast<u32x4*>(op) = *reinterpret_cast<u32x4*>(vals);
  }
}

// ---------------------------------------------------------------------------------------------
// Low-resolution layers (8^3 / 4^3: N*V <= 2048 voxels, 512 channels, 14 MB of weights per layer).  The kernel above
// is latency bound there: a 64-byte K tile is only 4 MFMAs per wave between two barriers (~1.5 us per K step), half of a
// 128-voxel tile is padding at 4^3 (one sample = 64 voxels), and every sample re-reads the weights.  This variant
//   * folds the batch into M (row Q = n*V + v), so a weight slice is read once per M tile instead of once per sample;
//   * takes 256-byte K tiles (128 channels of one tap): 16 MFMAs per wave per barrier pair, 4x fewer steps, 4x the
//     bytes in flight per step; rows are 256 B with the 16-byte chunk index XOR-ed with (row & 15) (conflict free for
//     the ds_read_b128 lane groups: both operands' 16-lane groups cover 16 distinct row residues, see lane_voxel);
//   * always splits K (taps x channel groups) so that >= 512 workgroups exist; fp32 slabs + the reduce below.
// ---------------------------------------------------------------------------------------------
__device__ inline int lane_voxel_ig(int l) { return l < 4 ? l : l < 12 ? l + 12 : l < 16 ? l - 8 : l < 20 ? l + 8 : l < 28 ? l - 12 : l; }

template <typename T, int ABL = 0>      // ABL: timing ablations (-DRX_ABLATION=1 builds only): 1 no global loads, 2 no MFMAs, 4 no LDS traffic
__global__ __launch_bounds__(256, 2) void igemm_fat_kernel(const T* __restrict__ in, const T* __restrict__ w, float* __restrict__ slab,
                                                           const IgemmGeom g, int NV /* N * Vq */, int nsteps_total) {
  constexpr int P = Elem<T>::PER16;
  constexpr int KC = 16;             // 16-byte chunks per K row (256 B)
  constexpr int KE = KC * P;         // input channels per K step
  constexpr int BM = 128, BN = 64;
  constexpr int XP = BM * KC / 256;  // 8 pieces per thread
  constexpr int WP = BN * KC / 256;  // 4
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_f[];
  u32x4* sX = reinterpret_cast<u32x4*>(smem_f);          // [BM][KC]
  u32x4* sW = sX + BM * KC;                              // [BN][KC]

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int mtiles = (NV + BM - 1) / BM;
  // the M tiles of one (channel block, K split) read the SAME weight slice: keep them on one XCD (one L2) so that the
  // slice comes from HBM once, not once per M tile
  const int lid = rx_xcd_remap(blockIdx.y * gridDim.x + blockIdx.x, gridDim.x * gridDim.y);
  const int mtile = lid % mtiles, rest = lid / mtiles;
  const int split = rest % g.ksplit, n0 = (rest / g.ksplit) * BN;
  const IgemmPhase P_ = g.ph[0];
  const int chunk = tid & 15, rbase = tid >> 4;          // 16 rows per pass

  // ---- per-thread gather geometry: rows rbase + 16p of the M tile
  int gz[XP], gy[XP], gx[XP];
  long gbase[XP];
  bool rok[XP];
#pragma unroll
  for (int p = 0; p < XP; ++p) {
    const int Q = mtile * BM + rbase + 16 * p;
    rok[p] = Q < NV;
    const int n = Q / P_.Vq, q = Q - n * P_.Vq;
    const int qx = q % P_.Qx, t = q / P_.Qx;
    const int qy = t % P_.Qy, qz = t / P_.Qy;
    gz[p] = qz * g.isz, gy[p] = qy * g.isy, gx[p] = qx * g.isx;
    gbase[p] = (long)n * g.in_ss + chunk * P;
  }
  const int nkc = g.Ci / KE;
  const int st_begin = (int)((long)nsteps_total * split / g.ksplit);
  const int st_end = (int)((long)nsteps_total * (split + 1) / g.ksplit);

  // SQ counters of this kernel: 39 % of the wave cycles issuing (VALU 21 %, two waves per SIMD), MFMA busy 14 % -- it was bound by
  // the instruction stream of the gather, ~20 VALU + a branch per activation row and K step against 16 MFMAs per wave.  The row
  // offsets only change with the TAP, not with the channel chunk: they are recomputed when the tap changes (every Ci/128 steps) and
  // kept as one 32-bit element offset per row (-1 = zero padding).
  u32x4 xr[XP], wr[WP];
  int xo[XP], wo = 0, cur_tap = -1;
  auto load_step = [&](int st) {
    const int tap = st / nkc, cc = st - tap * nkc;
    if (tap != cur_tap) {                     // uniform
      cur_tap = tap;
      const RxTap tp = g.taps[P_.tap0 + tap];
#pragma unroll
      for (int p = 0; p < XP; ++p) {
        const int z = gz[p] + tp.dz, y = gy[p] + tp.dy, x = gx[p] + tp.dx;
        const bool ok = rok[p] & ((unsigned)z < (unsigned)g.Zi) & ((unsigned)y < (unsigned)g.Yi) & ((unsigned)x < (unsigned)g.Xi);
        xo[p] = ok ? (int)(gbase[p] + ((long)(z * g.Yi + y) * g.Xi + x) * g.ldi) : -1;
      }
      wo = (int)(((long)tp.w * g.Co + n0 + rbase) * g.Ci + chunk * P);
    }
    const int ko = cc * KE;
    if (ABL & 1) {
#pragma unroll
      for (int p = 0; p < XP; ++p) xr[p] = u32x4{(unsigned)(xo[p] + ko), 1u, 2u, 3u};
#pragma unroll
      for (int p = 0; p < WP; ++p) wr[p] = u32x4{(unsigned)(wo + ko), 1u, 2u, 3u};
      return;
    }
#pragma unroll
    for (int p = 0; p < XP; ++p) {
      const int o = xo[p] < 0 ? 0 : xo[p] + ko;           // always a valid address: the load is unconditional, the select zeroes padding
      const u32x4 v = *reinterpret_cast<const u32x4*>(in + o);
      xr[p] = xo[p] < 0 ? u32x4{0u, 0u, 0u, 0u} : v;
    }
#pragma unroll
    for (int p = 0; p < WP; ++p) wr[p] = *reinterpret_cast<const u32x4*>(w + wo + (long)(16 * p) * g.Ci + ko);
  };
  auto store_step = [&]() {
    if (ABL & 4) {          // keep the values alive without touching LDS
      if (xr[0][0] == 0x7fffffffu && wr[0][0] == 0x7ffffffeu) sX[0] = xr[1];
      return;
    }
#pragma unroll
    for (int p = 0; p < XP; ++p) {
      const int row = rbase + 16 * p;
      sX[row * KC + (chunk ^ (row & 15))] = xr[p];
    }
#pragma unroll
    for (int p = 0; p < WP; ++p) {
      const int row = rbase + 16 * p;
      sW[row * KC + (chunk ^ (row & 15))] = wr[p];
    }
  };

  f32x16 acc[2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[a][r] = 0.f;

  const int fr = lane & 31, fh = lane >> 5;
  const int vrow = wave * 32 + lane_voxel_ig(fr);         // this lane's voxel row of the M tile
  const u32x4* xrow = sX + vrow * KC;
  const u32x4* wrow0 = sW + fr * KC;
  const u32x4* wrow1 = sW + (32 + fr) * KC;
  const int xm = vrow & 15, wm = fr & 15;                  // (32 + fr) & 15 == fr & 15

  if (st_begin < st_end) load_step(st_begin);
  for (int st = st_begin; st < st_end; ++st) {
    __syncthreads();
    store_step();
    __syncthreads();
    if (st + 1 < st_end) load_step(st + 1);
#pragma unroll
    for (int ks = 0; ks < KC / 2; ++ks) {
      const int c = ks * 2 + fh;
      u32x4 b, a0, a1;
      if (ABL & 4) {
        b = u32x4{(unsigned)c, (unsigned)st, 2u, 3u}, a0 = b, a1 = b;
      } else {
        b = xrow[c ^ xm];
        a0 = wrow0[c ^ wm], a1 = wrow1[c ^ wm];
      }
      if (ABL & 2) {
        acc[0][ks] += __builtin_bit_cast(float, a0[0] ^ b[1]);
        acc[1][ks] += __builtin_bit_cast(float, a1[2] ^ b[3]);
      } else {
        Mma<T>::run(acc[0], a0, b);
        Mma<T>::run(acc[1], a1, b);
      }
    }
  }

  // ---- fp32 partial sums: slab[split][Q][Co]
  const int Q = mtile * BM + vrow;
  if (Q < NV) {
    float* sp = slab + ((long)split * NV + Q) * g.Co + n0;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4) {
        f32x4 v = {acc[a][4 * g4], acc[a][4 * g4 + 1], acc[a][4 * g4 + 2], acc[a][4 * g4 + 3]};
        *reinterpret_cast<f32x4*>(sp + a * 32 + 8 * g4 + 4 * fh) = v;
      }
  }
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------

// launches what rx_gather_choose chose for `g`: one table row per instantiation
template <typename T>
static void igemm_launch_as(const RxGatherChoice& c, hipStream_t st, const void* in, const void* w, const float* bias, void* out, void* ws,
                            const IgemmGeom& g, int N) {
  const dim3 grid(c.grid[0], c.grid[1], c.grid[2]), rgrid(c.rgrid[0], c.rgrid[1]);
#define RX_IG_ROW(BM_, BN_) \
  if (c.kind == RX_GA_TILE && c.BM == BM_ && c.BN == BN_) \
    hipLaunchKernelGGL((igemm_kernel<T, BM_, BN_>), grid, dim3(256), 0, st, (const T*)in, (const T*)w, bias, (T*)out, (float*)ws, g);
  RX_IG_ROW(256, 64) RX_IG_ROW(256, 32) RX_IG_ROW(128, 64) RX_IG_ROW(128, 32)
#undef RX_IG_ROW
  if constexpr (!std::is_same<T, float>::value) {
#define RX_FAT_ROW(KERNEL)                                                                                                          \
  {                                                                                                                                 \
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&KERNEL), hipFuncAttributeMaxDynamicSharedMemorySize, (int)c.lds);      \
    hipLaunchKernelGGL(KERNEL, grid, dim3(256), c.lds, st, (const T*)in, (const T*)w, (float*)ws, g, c.NV, c.nsteps);               \
  }
    if (c.kind == RX_GA_FAT) {
#if RX_ABLATION
      static const int abl = rx_env_mask("RX_FAT_ABL");
#define RX_FAT_ABL(A) case A: RX_FAT_ROW((igemm_fat_kernel<T, A>)) break;
      if constexpr (std::is_same<T, bf16_t>::value) {
        switch (abl) {
          RX_FAT_ABL(1) RX_FAT_ABL(2) RX_FAT_ABL(3) RX_FAT_ABL(4) RX_FAT_ABL(5) RX_FAT_ABL(6) RX_FAT_ABL(7)
          default: RX_FAT_ROW((igemm_fat_kernel<T>))
        }
      } else
#undef RX_FAT_ABL
#endif
        RX_FAT_ROW((igemm_fat_kernel<T>))
    }
#undef RX_FAT_ROW
  }
  if (c.rgrid[0]) hipLaunchKernelGGL((igemm_splitk_reduce<T>), rgrid, dim3(256), 0, st, (const float*)ws, bias, (T*)out, g, N);
}

static int igemm_launch(rx_dtype dt, const void* in, const void* w, const float* bias, void* out, IgemmGeom& g, int N, void* ws,
                        size_t ws_bytes, hipStream_t st) {
  const RxGatherChoice c = rx_gather_choose(dt, g, N, ws != nullptr, ws_bytes, rx_lo4(in), rx_lo4(out), rx_lo4(w));
  if (c.kind == RX_GA_REFUSE) RX_FAIL(RX_EUNSUPPORTED, "%s", c.message);
  if (c.kind == RX_GA_NOTHING) return RX_OK;
  rx_note_kernel(c.name);
  RX_DISPATCH_DTYPE(dt, T, igemm_launch_as<T>(c, st, in, w, bias, out, ws, g, N));
  RX_CHECK_LAUNCH(c.kind == RX_GA_FAT ? "igemm_fat" : "igemm");
  return RX_OK;
}

// the legs of a route that other files launch; RX_RT_GATHER stays with the caller
static int route_launch(const RxConvRoute& r, rx_dtype dt, const rx_act* in, const void* w, const float* bias, const rx_act* out, int flip,
                        int accumulate, hipStream_t st, float* stat_part, const RxBwdStat* bs, const char* who) {
  switch (r.kind) {
    case RX_RT_REFUSE: RX_FAIL(r.code, "%s", r.message);
    case RX_RT_HALO: return rx_conv_halo_launch(r.halo, dt, in, w, bias, out, flip, accumulate, st, stat_part, bs);
    case RX_RT_POINTWISE: return rx_pointwise_launch(r.pw, dt, in->ptr, w, bias, out->ptr, st, who);
    case RX_RT_DS2: return rx_dgrad_s2_launch(r.ds2, dt, in->ptr, w, out->ptr, st);
    default: return RX_OK;
  }
}

extern "C" int rx_conv3d_fwd(rx_dtype dt, const rx_act* x, const void* w_fwd, const float* bias, const rx_act* y,
                             const int32_t kernel[3], const int32_t stride[3], void* ws, size_t wsb, void* stream) {
  RX_RECORD(stream, [=, x_ = RxActV(x), y_ = RxActV(y), kernel_ = RxI3V(kernel), stride_ = RxI3V(stride)](void* s) { return rx_conv3d_fwd(dt, x_.p(), w_fwd, bias, y_.p(), kernel_.v, stride_.v, ws, wsb, s); });
  if (!rx_act_ok_planar(x) || !rx_act_ok(y) || !w_fwd) RX_FAIL(RX_EINVAL, "rx_conv3d_fwd: bad arguments");
  const RxConvRoute r = rx_route_conv(dt, x, rx_lo4(w_fwd), y, kernel, stride, 0, 0);
  if (r.kind != RX_RT_GATHER) return route_launch(r, dt, x, w_fwd, bias, y, 0, 0, (hipStream_t)stream, nullptr, nullptr, "rx_conv3d_fwd(pointwise)");
  IgemmGeom g;
  rx_gather_fwd(g, x, y, kernel, stride);
  return igemm_launch(dt, x->ptr, w_fwd, bias, y->ptr, g, x->n, ws, wsb, (hipStream_t)stream);
}

// backward-data + the two sums of the InstanceNorm backward of the layer whose output gradient this launch COMPLETES (dx =
// dL/d(out of that layer); the layer has no residual, its LeakyReLU mask is the sign of the normalised value).  *fused = 1 and
// m12[n][c] = (mean g', mean g'*xhat) when the launch ran on the persistent 32-channel kernel (continue with
// rx_instnorm_act_bwd_apply); otherwise *fused = 0, m12 untouched (continue with rx_instnorm_act_bwd).  The caller guarantees
// that nothing adds to dx afterwards.
extern "C" int rx_conv3d_bwd_data_instats(rx_dtype dt, const rx_act* dy, const void* w_bwd, const rx_act* dx, const int32_t kernel[3],
                                          const int32_t stride[3], int accumulate, const rx_act* in_y, const float* in_stats, float slope,
                                          float* m12, int* fused, void* ws, size_t wsb, void* stream) {
  RX_RECORD(stream, [=, dy_ = RxActV(dy), dx_ = RxActV(dx), kernel_ = RxI3V(kernel), stride_ = RxI3V(stride), in_y_ = RxActV(in_y)](void* s) { int fused_dummy = 0; return rx_conv3d_bwd_data_instats(dt, dy_.p(), w_bwd, dx_.p(), kernel_.v, stride_.v, accumulate, in_y_.p(), in_stats, slope, m12, &fused_dummy, ws, wsb, s); });
  if (!fused || !m12 || !in_stats || !rx_act_ok(in_y) || !ws) RX_FAIL(RX_EINVAL, "rx_conv3d_bwd_data_instats: bad arguments");
  *fused = 0;
  if (!rx_act_ok(dy) || !rx_act_ok(dx) || !w_bwd) RX_FAIL(RX_EINVAL, "rx_conv3d_bwd_data_instats: bad arguments");
  const RxConvRoute r = rx_route_conv_stats(dt, dy, rx_lo4(w_bwd), dx, kernel, stride, accumulate, in_y, wsb);
  if (r.kind == RX_RT_PLAIN) return rx_conv3d_bwd_data(dt, dy, w_bwd, dx, kernel, stride, accumulate, ws, wsb, stream);
  const RxBwdStat bs{in_y, in_stats, slope};
  const int rc = route_launch(r, dt, dy, w_bwd, nullptr, dx, 1, accumulate, (hipStream_t)stream, (float*)ws, &bs, "");
  if (rc || r.halo.stat_chunks <= 0) return rc;
  rx_inbwd_fused_finalize_launch((const float*)ws, dx->n, r.halo.stat_chunks, dx->c, (double)rx_act_voxels(dx), in_stats, m12, (hipStream_t)stream);
  RX_CHECK_LAUNCH("rx_conv3d_bwd_data_instats(finalize)");
  *fused = 1;
  return RX_OK;
}

// conv + InstanceNorm statistics of its output in one call.  When the layer runs on a persistent halo kernel the sums of y and
// y^2 come out of the conv epilogue (no extra pass over y); otherwise this is rx_conv3d_fwd followed by rx_instnorm_stats.
extern "C" int rx_conv3d_fwd_stats(rx_dtype dt, const rx_act* x, const void* w_fwd, const float* bias, const rx_act* y,
                                   const int32_t kernel[3], const int32_t stride[3], float eps, float* stats, void* ws, size_t wsb,
                                   void* stream) {
  RX_RECORD(stream, [=, x_ = RxActV(x), y_ = RxActV(y), kernel_ = RxI3V(kernel), stride_ = RxI3V(stride)](void* s) { return rx_conv3d_fwd_stats(dt, x_.p(), w_fwd, bias, y_.p(), kernel_.v, stride_.v, eps, stats, ws, wsb, s); });
  if (!rx_act_ok_planar(x) || !rx_act_ok(y) || !w_fwd || !stats || !ws) RX_FAIL(RX_EINVAL, "rx_conv3d_fwd_stats: bad arguments");
  const RxConvRoute r = rx_route_conv_stats(dt, x, rx_lo4(w_fwd), y, kernel, stride, 0, nullptr, wsb);
  const int rc = r.kind == RX_RT_PLAIN ? rx_conv3d_fwd(dt, x, w_fwd, bias, y, kernel, stride, ws, wsb, stream)
                                       : route_launch(r, dt, x, w_fwd, bias, y, 0, 0, (hipStream_t)stream, (float*)ws, nullptr, "");
  if (rc) return rc;
  if (r.kind == RX_RT_PLAIN || r.halo.stat_chunks <= 0) return rx_instnorm_stats(dt, y, eps, stats, ws, wsb, stream);
  rx_stats_finalize_launch((const float*)ws, y->n, r.halo.stat_chunks, y->c, (double)rx_act_voxels(y), eps, stats, (hipStream_t)stream);
  RX_CHECK_LAUNCH("rx_conv3d_fwd_stats(finalize)");
  return RX_OK;
}

extern "C" int rx_conv3d_bwd_data(rx_dtype dt, const rx_act* dy, const void* w_bwd, const rx_act* dx, const int32_t kernel[3],
                                  const int32_t stride[3], int accumulate, void* ws, size_t wsb, void* stream) {
  RX_RECORD(stream, [=, dy_ = RxActV(dy), dx_ = RxActV(dx), kernel_ = RxI3V(kernel), stride_ = RxI3V(stride)](void* s) { return rx_conv3d_bwd_data(dt, dy_.p(), w_bwd, dx_.p(), kernel_.v, stride_.v, accumulate, ws, wsb, s); });
  if (!rx_act_ok(dy) || !rx_act_ok_planar(dx) || !w_bwd) RX_FAIL(RX_EINVAL, "rx_conv3d_bwd_data: bad arguments");
  const RxConvRoute r = rx_route_conv(dt, dy, rx_lo4(w_bwd), dx, kernel, stride, 1, accumulate);
  if (r.kind != RX_RT_GATHER)
    return route_launch(r, dt, dy, w_bwd, nullptr, dx, 1, accumulate, (hipStream_t)stream, nullptr, nullptr, "rx_conv3d_bwd_data(pointwise)");
  IgemmGeom g;
  for (int cls = 0; rx_gather_bwd_data_next(g, dy, dx, kernel, stride, accumulate, &cls);) {
    const int rc = igemm_launch(dt, dy->ptr, w_bwd, nullptr, dx->ptr, g, dx->n, ws, wsb, (hipStream_t)stream);
    if (rc) return rc;
  }
  return RX_OK;
}

extern "C" int rx_convT3d_fwd(rx_dtype dt, const rx_act* x, const void* w_fwd, const float* bias, const rx_act* y,
                              const int32_t stride[3], void* ws, size_t wsb, void* stream) {
  RX_RECORD(stream, [=, x_ = RxActV(x), y_ = RxActV(y), stride_ = RxI3V(stride)](void* s) { return rx_convT3d_fwd(dt, x_.p(), w_fwd, bias, y_.p(), stride_.v, ws, wsb, s); });
  if (!rx_act_ok(x) || !rx_act_ok(y) || !w_fwd) RX_FAIL(RX_EINVAL, "rx_convT3d_fwd: bad arguments");
  const RxConvRoute r = rx_route_convT(dt, x, rx_lo4(w_fwd), y, stride, true);
  if (r.kind != RX_RT_GATHER) return route_launch(r, dt, x, w_fwd, bias, y, 0, 0, (hipStream_t)stream, nullptr, nullptr, "rx_convT3d_fwd(pointwise)");
  IgemmGeom g;
  for (int pos = 0; rx_gather_convT_fwd_next(g, x, y, stride, &pos);) {
    const int rc = igemm_launch(dt, x->ptr, w_fwd, bias, y->ptr, g, x->n, ws, wsb, (hipStream_t)stream);
    if (rc) return rc;
  }
  return RX_OK;
}

extern "C" int rx_convT3d_bwd_data(rx_dtype dt, const rx_act* dy, const void* w_bwd, const rx_act* dx, const int32_t stride[3],
                                   int accumulate, void* ws, size_t wsb, void* stream) {
  RX_RECORD(stream, [=, dy_ = RxActV(dy), dx_ = RxActV(dx), stride_ = RxI3V(stride)](void* s) { return rx_convT3d_bwd_data(dt, dy_.p(), w_bwd, dx_.p(), stride_.v, accumulate, ws, wsb, s); });
  if (!rx_act_ok(dy) || !rx_act_ok(dx) || !w_bwd) RX_FAIL(RX_EINVAL, "rx_convT3d_bwd_data: bad arguments");
  const RxConvRoute r = rx_route_convT(dt, dx, rx_lo4(w_bwd), dy, stride, false);
  if (r.kind != RX_RT_GATHER) return route_launch(r, dt, dy, w_bwd, nullptr, dx, 1, accumulate, (hipStream_t)stream, nullptr, nullptr, "");
  IgemmGeom g;
  rx_gather_convT_bwd_data(g, dy, dx, stride, accumulate);
  return igemm_launch(dt, dy->ptr, w_bwd, nullptr, dx->ptr, g, dx->n, ws, wsb, (hipStream_t)stream);
}

extern "C" size_t rx_conv_workspace_hint(void) { return (size_t)96 << 20; }
