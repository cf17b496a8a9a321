// rx_dgrad_s2.hip -- backward-data of the stride-2 3x3x3 convolution that opens an encoder stage (resblocks.py:71-74 with
// stride 2), 16-bit compute types, 64 dY channels (two 64-byte chunks) -- the 32 -> 64 layer at 128^3 -> 64^3, whose data
// gradient is the largest launch of the generic gather kernel (igemm<256,32>: 8 parity phases, one 64-byte K step = 2 MFMAs
// per wave between two barriers; 297 us isolated, 195 TF/s).
//
//   dx[2q + r] = sum_{t : (r + 1 - t) even} W[t]^T dy[q + (r + 1 - t)/2]        per axis:   r = 0: t = 1 (offset 0)
//                                                                                              r = 1: t = 0 (offset +1), t = 2 (0)
// so each of the 8 output parity classes is a stride-1 convolution over the dY grid with 1, 2, 4 or 8 taps (27 in total)
// whose offsets are 0 / +1.  A workgroup owns a 4x4x16 tile of dY voxels and 32 output channels: the (5 x 5 x 17)-row dY
// halo of BOTH channel chunks is staged in LDS once and serves all 27 taps of all 8 classes (the gather kernel re-reads a
// dY row from L2 for every tap: 27/8 times per output voxel).
//
// Persistent and weight-stationary.  All 27 weight slices of a 32-channel block are 108 KB and the dY halo of both chunks
// 53 KB: together 1.1 KB MORE than the 160 KB of LDS -- so the single tap of class (0,0,0) lives in registers as ready-made
// A fragments and the other 26 (104 KB) stay in LDS for the workgroup's whole life; one workgroup per CU walks a contiguous
// range of tiles, the next tile's halo waits in registers while the current tile's 216 MFMAs per wave run barrier-free
// (class structure, tap offsets and weight slots are compile-time).  290 us (gather kernel) -> 192 us (a non-persistent
// kernel with one phase per (class, chunk), since retired) -> 140 us; -0.35 ms per cfg2 step.  Ablation (-DRX_ABLATION=1,
// RX_DBG): without halo loads 128 us, without MFMAs 144, without stores 111, with none of the three 99 us -- the floor is
// the LDS operand traffic (every one of the 8 waves reads every weight fragment: 1.7 MB per tile) plus the weight staging.
// Tried: one parity class per wave with its weights as register-resident A fragments (LDS then holds only the halo): 128
// fragment registers + halo prefetch + accumulators do not fit 256 VGPRs (the compiler spilled ~200 registers, 271 us) --
// it needs the weight fragments in AGPRs by hand, not attempted.
#include "rx_common.h"
#include "rx_internal.h"

// DS2_H*, DS2P_*_BYTES, DgradS2Geom and which calls take this kernel (rx_ds2_choose): rx_gather_plan.h

__device__ inline int ds2_lane_voxel(int l) { return l < 4 ? l : l < 12 ? l + 12 : l < 16 ? l - 8 : l < 20 ? l + 8 : l < 28 ? l - 12 : l; }

__device__ constexpr int DS2_SLOT_K[26] = {12, 14, 10, 16, 9, 11, 15, 17, 4, 22, 3, 5, 21, 23, 1, 7, 19, 25, 0, 2, 6, 8, 18, 20, 24, 26};
__device__ constexpr int DS2_SLOT_OFF[26] = {1, 0, 17, 0, 18, 17, 1, 0, 85, 0, 86, 85, 1, 0, 102, 85, 17, 0, 103, 102, 86, 85, 18, 17, 1, 0};
__device__ constexpr int DS2_CLS_BASE[8] = {0, 0, 2, 4, 8, 10, 14, 18};
__device__ constexpr int DS2_CLS_NT[8] = {1, 2, 2, 4, 2, 4, 4, 8};
#define DS2P_HP ((2 * DS2_HV * 4 + 511) / 512)  // halo pieces per thread: 7

template <typename T, bool ACC>
__global__ __launch_bounds__(512, 1) void dgrad_s2p_kernel(const T* __restrict__ dy, const T* __restrict__ w, T* __restrict__ dx,
                                                           const DgradS2Geom g, int tiles_per_wg) {
  constexpr int P = Elem<T>::PER16;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  unsigned char* sW = smem;                          // [26 slots][2 chunks][32 rows][64 B], piece XOR (row>>2)&3
  unsigned char* sX = smem + DS2P_W_BYTES;           // [2 chunks][425 rows][64 B], same swizzle
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int vb = rx_xcd_remap(blockIdx.x, gridDim.x);
  const int c0 = blockIdx.y * 32;
  const int t_begin = vb * tiles_per_wg, t_end = min(g.NT, t_begin + tiles_per_wg);
  if (t_begin >= t_end) return;
  const int fr = lane & 31, fh = lane >> 5;

  // ---- weights: 26 slices into LDS, the centre tap (class 0) into registers
  for (int i = tid; i < 26 * 2 * 32 * 4; i += 512) {
    const int c4 = i & 3, r = (i >> 2) & 31, cc = (i >> 7) & 1, slot = i >> 8;
    const u32x4 v = *reinterpret_cast<const u32x4*>(w + ((long)DS2_SLOT_K[slot] * g.Ci + c0 + r) * g.Co + cc * 32 + c4 * P);
    const int row = (slot * 2 + cc) * 32 + r;
    *reinterpret_cast<u32x4*>(sW + row * 64 + ((c4 ^ ((row >> 2) & 3)) << 4)) = v;
  }
  u32x4 wc0[4];                                      // [cc*2 + ks]
#pragma unroll
  for (int j = 0; j < 4; ++j)
    wc0[j] = *reinterpret_cast<const u32x4*>(w + ((long)13 * g.Ci + c0 + fr) * g.Co + (j >> 1) * 32 + ((j & 1) * 2 + fh) * P);

  // ---- halo pieces of this thread: (chunk-of-64B cc, row, piece) decoded once
  int hcoord[DS2P_HP], hdst[DS2P_HP];
#pragma unroll
  for (int p = 0; p < DS2P_HP; ++p) {
    const int i = tid + 512 * p;
    hcoord[p] = -1, hdst[p] = 0;
    if (i < 2 * DS2_HV * 4) {
      const int cc = i / (DS2_HV * 4), rem = i - cc * (DS2_HV * 4), row = rem >> 2, c4 = rem & 3;
      const int hx = row % DS2_HX, t = row / DS2_HX, hy = t % DS2_HY, hz = t / DS2_HY;
      hcoord[p] = (hz << 16) | (hy << 8) | hx;
      hdst[p] = (cc * DS2_HV + row) * 64 + ((c4 ^ ((row >> 2) & 3)) << 4) | (cc << 30) | (c4 << 28);
    }
  }
  u32x4 hq[DS2P_HP];
  auto prefetch_halo = [&](int tile) {
    int tx, ty, tz, n;
    rx_tile_coords(tile, g.tx_n, g.ty_n, g.tz_n, 1, n, tz, ty, tx);
    const int z0 = tz * 4, y0 = ty * 4, x0 = tx * 16;
    const T* dyn = dy + (long)n * g.dy_ss;
#pragma unroll
    for (int p = 0; p < DS2P_HP; ++p) {
      u32x4 v = u32x4{0u, 0u, 0u, 0u};
      if (hcoord[p] >= 0) {
        const int z = z0 + (hcoord[p] >> 16), y = y0 + ((hcoord[p] >> 8) & 255), x = x0 + (hcoord[p] & 255);
        const int cc = (hdst[p] >> 30) & 1, c4 = (hdst[p] >> 28) & 3;
        if (z < g.Zo && y < g.Yo && x < g.Xo && !RX_ABLATE(g, 1)) v = *reinterpret_cast<const u32x4*>(dyn + ((long)(z * g.Yo + y) * g.Xo + x) * g.ldy + cc * 32 + c4 * P);
      }
      hq[p] = v;
    }
  };
  const int fv = ds2_lane_voxel(fr);
  // 8 waves, one 32-voxel block each: two waves per SIMD hide each other's LDS latency (4 waves x 2 blocks: 145 us)
  constexpr int NB = 1;
  int hrow[NB];
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    const int v = (wave * NB + b) * 32 + fv;
    hrow[b] = (((v >> 6) * DS2_HY) + ((v >> 4) & 3)) * DS2_HX + (v & 15);
  }
  const int wsw = (fr >> 2) & 3;
  prefetch_halo(t_begin);
  for (int tile = t_begin; tile < t_end; ++tile) {
    __syncthreads();                                 // the previous tile's operand reads are done (first tile: nothing)
#pragma unroll
    for (int p = 0; p < DS2P_HP; ++p)
      if (hcoord[p] >= 0) *reinterpret_cast<u32x4*>(sX + (hdst[p] & 0x0fffffff)) = hq[p];
    __syncthreads();                                 // (also publishes the weights before the first tile)
    if (tile + 1 < t_end) prefetch_halo(tile + 1);
    int tx, ty, tz, n;
    rx_tile_coords(tile, g.tx_n, g.ty_n, g.tz_n, 1, n, tz, ty, tx);
    const int z0 = tz * 4, y0 = ty * 4, x0 = tx * 16;
    T* dxn = dx + (long)n * g.dx_ss + c0 + 4 * fh;
#pragma unroll
    for (int cls = 0; cls < 8; ++cls) {
      const int rz = cls >> 2, ry = (cls >> 1) & 1, rx = cls & 1;
      // output addresses of this lane's two voxels for this class (and, ACC, their old values: fetched before the MFMAs)
      T* op[NB];
      bool ok[NB];
      u32x2 oldv[NB][4];
#pragma unroll
      for (int b = 0; b < NB; ++b) {
        const int v = (wave * NB + b) * 32 + fv;
        const int qz = z0 + (v >> 6), qy = y0 + ((v >> 4) & 3), qx = x0 + (v & 15);
        ok[b] = qz < g.Zo && qy < g.Yo && qx < g.Xo;
        op[b] = dxn + ((long)((2 * qz + rz) * g.Y + 2 * qy + ry) * g.X + 2 * qx + rx) * g.ldx;
        if (ACC) {
#pragma unroll
          for (int g4 = 0; g4 < 4; ++g4) oldv[b][g4] = ok[b] ? *reinterpret_cast<const u32x2*>(op[b] + 8 * g4) : u32x2{0u, 0u};
        }
      }
      f32x16 acc[NB];
#pragma unroll
      for (int b = 0; b < NB; ++b)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[b][r] = 0.f;
      __builtin_amdgcn_sched_barrier(0);             // keep the 8 classes apart: left alone the scheduler hoists every fragment read
#pragma unroll                                       // of the tile (512 registers + spills)
      for (int cc = 0; cc < 2; ++cc)
#pragma unroll
        for (int tl = 0; tl < DS2_CLS_NT[cls]; ++tl) {
          const int slot = DS2_CLS_BASE[cls] + tl;
          const int off = cls == 0 ? 0 : DS2_SLOT_OFF[slot];
#pragma unroll
          for (int ks = 0; ks < 2; ++ks) {
            u32x4 af;
            if (cls == 0)
              af = wc0[cc * 2 + ks];
            else
              af = *reinterpret_cast<const u32x4*>(sW + ((slot * 2 + cc) * 32 + fr) * 64 + (((ks * 2 + fh) ^ wsw) << 4));
#pragma unroll
            for (int b = 0; b < NB; ++b) {
              const int row = hrow[b] + off;
              const u32x4 bf = *reinterpret_cast<const u32x4*>(sX + (cc * DS2_HV + row) * 64 + (((ks * 2 + fh) ^ ((row >> 2) & 3)) << 4));
              if (!RX_ABLATE(g, 4)) Mma<T>::run(acc[b], af, bf);
              else acc[b][0] += __builtin_bit_cast(float, af[0] ^ bf[0]);
            }
          }
        }
#pragma unroll
      for (int b = 0; b < NB; ++b) {
        if (!ok[b] || RX_ABLATE(g, 8)) continue;
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
          T vals[4];
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            float f = acc[b][4 * g4 + i];
            if (ACC) f += Elem<T>::to_f(reinterpret_cast<const T*>(&oldv[b][g4])[i]);
            vals[i] = Elem<T>::from_f(f);
          }
          *reinterpret_cast<u32x2*>(op[b] + 8 * g4) = *reinterpret_cast<u32x2*>(vals);
        }
      }
      __builtin_amdgcn_sched_barrier(0);
    }
  }
}

int rx_dgrad_s2_launch(const RxDs2Choice& c, rx_dtype dt, const void* dy, const void* w_bwd, void* dx, hipStream_t st) {
  DgradS2Geom g = c.g;
  static const int dbg = rx_env_mask("RX_DBG");
  g.dbg = dbg;
  rx_note_kernel("dgrad_s2p_kernel");
#define RX_DS2P_ROW(TT, A)                                                                                                             \
  if ((dt == RX_BF16) == std::is_same<TT, bf16_t>::value && (g.accumulate != 0) == A) {                                                 \
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&dgrad_s2p_kernel<TT, A>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)c.lds); \
    hipLaunchKernelGGL((dgrad_s2p_kernel<TT, A>), dim3(c.grid[0], c.grid[1]), dim3(512), c.lds, st, (const TT*)dy, (const TT*)w_bwd, (TT*)dx, g, c.per); \
  }
  RX_DS2P_ROW(bf16_t, false) RX_DS2P_ROW(bf16_t, true) RX_DS2P_ROW(f16_t, false) RX_DS2P_ROW(f16_t, true)
#undef RX_DS2P_ROW
  RX_CHECK_LAUNCH("dgrad_s2p");
  return RX_OK;
}
