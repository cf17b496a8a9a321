// rx_conv_halo_plan.h -- which halo kernel a stride-1 3x3x3 convolution (forward or backward-data) runs on, and with what grid.
// No HIP in here: rx_ch_choose is a pure function of a query, so every branch of it -- the ones that need operands past 2 GiB
// included -- is executed on the CPU by tools/conv_halo_plan_check.cpp.  rx_conv_halo.hip launches exactly what the choice says.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/rxunet.h"

// what the decision reads of a call (in / out have the same N, Z, Y, X: stride 1, padding 1)
struct RxChQuery {
  rx_dtype dt;
  int N, Z, Y, X;
  int Ci, Co, ldi, ldo;
  long in_cs, out_cs;                    // rx_act.cs of in / out (0: interleaved channels)
  unsigned in_lo, out_lo, w_lo, bsy_lo;  // low 4 address bits of in, out, w and of the backward sums' y
  int bs_ldy;                            // ld of that y
  int flip, accumulate;                  // flip = 1: backward-data
  bool stat_offered;                     // the caller passed a partial-sum buffer (and somewhere to put the chunk count) ...
  size_t stat_bytes;                     // ... of this many bytes
  bool want_bs;                          // the caller asks for the InstanceNorm backward sums (RxBwdStat)
};

enum RxChKind { RX_CH_FALLTHROUGH = 0, RX_CH_REFUSE, RX_CH_LAUNCH };   // the route goes on to the gather kernels / fails with RX_EUNSUPPORTED / launches
enum RxChFamily { RX_CH_GENERIC32, RX_CH_GENERIC64, RX_CH_HALO32, RX_CH_HALO32P, RX_CH_HALO32WS, RX_CH_HALO64WS };

struct RxChChoice {
  RxChKind kind;
  const char* message;                   // RX_CH_REFUSE: the error text
  RxChFamily family;
  const char* name;                      // for rx_note_kernel
  bool FLIP, XDMA, STATS, ACC, BS;       // template flags of the instantiation (BS: conv_halo32p's BS, conv_halo64ws's BSP)
  int TZ, TY, TX, lTX, lTY, HY, HX, HV;  // tile and halo geometry
  int tz_n, ty_n, tx_n, NT;
  int order;                             // tile walk order (rx_tile_coords)
  long in_ss, out_ss, in_cs, out_cs;     // element strides (cs: between 32-channel groups, the dense value when not planar)
  unsigned grid_x, grid_y, block;
  size_t lds;                            // dynamic LDS bytes
  int per, wgs_s;                        // persistent families: tiles per workgroup, workgroups per sample; else 0
  bool take_stats, take_bs;              // the launch gets the partial-sum buffer / the backward-sum operands
  int stat_chunks;                       // partial rows per sample it leaves there (0: the caller reduces in a pass of its own)
};

#define RX_CH_PLAN_MAX_HV 656
#define RX_CH_LDS_GENERIC(BN) ((size_t)(RX_CH_PLAN_MAX_HV * 4 + 9 * (BN)*4) * 16)
#define RX_CH_LDS_HALO32 ((size_t)648 * 80 + (size_t)9 * 32 * 64)
#define RX_CH_LDS_HALO32P ((size_t)27 * 32 * 64 + 2 * (size_t)(648 * 80))
#define RX_CH_LDS_HALO32WS ((size_t)2 * (9 * 32 * 64 + 648 * 64))
#define RX_CH_LDS_HALO64WS ((size_t)2 * (9 * 64 * 64 + 648 * 64))

inline int rx_ch_p2ceil(int v) {
  int p = 1;
  while (p < v) p <<= 1;
  return p;
}
inline int rx_ch_ilog2(int v) {
  int l = 0;
  while ((1 << l) < v) ++l;
  return l;
}

// Persistent families: at most `cap` workgroups (one per CU in total), each walking `per` consecutive tiles of ONE sample -- a
// workgroup's tile range never straddles samples (the fused InstanceNorm sums are per (n, c)).
inline void rx_ch_persistent_grid(RxChChoice& c, int cap, int N, unsigned blocks) {
  int wgs = cap < 1 ? 1 : cap;
  if (wgs > c.NT) wgs = c.NT;
  const int NTs = c.NT / N;
  int wgs_s = wgs / N > 0 ? wgs / N : 1;
  c.per = (NTs + wgs_s - 1) / wgs_s;
  c.wgs_s = (NTs + c.per - 1) / c.per;
  c.grid_x = (unsigned)(c.wgs_s * N), c.grid_y = blocks, c.block = 512;
}

inline RxChChoice rx_ch_refuse(RxChChoice c, const char* message) {
  c.kind = RX_CH_REFUSE, c.message = message;
  return c;
}
inline RxChChoice rx_ch_launch(RxChChoice c, RxChFamily family, const char* name, size_t lds) {
  c.kind = RX_CH_LAUNCH, c.family = family, c.name = name, c.lds = lds;
  return c;
}

inline unsigned rx_lo4(const void* p) { return (unsigned)((uintptr_t)p & 15); }
// the query of a call: in / out of the launch (backward-data: dy / dx), bs_y: the y of the backward sums the caller asks for, or null
inline RxChQuery rx_ch_query(rx_dtype dt, const rx_act* in, unsigned w_lo, const rx_act* out, int flip, int accumulate, bool stat_offered,
                             size_t stat_bytes, const rx_act* bs_y) {
  RxChQuery q = {};
  q.dt = dt;
  q.N = in->n, q.Z = in->z, q.Y = in->y, q.X = in->x;
  q.Ci = in->c, q.Co = out->c, q.ldi = in->ld, q.ldo = out->ld;
  q.in_cs = in->cs, q.out_cs = out->cs;
  q.in_lo = rx_lo4(in->ptr), q.out_lo = rx_lo4(out->ptr), q.w_lo = w_lo;
  q.flip = flip, q.accumulate = accumulate;
  q.stat_offered = stat_offered, q.stat_bytes = stat_bytes;
  q.want_bs = bs_y != nullptr;
  if (bs_y) q.bsy_lo = rx_lo4(bs_y->ptr), q.bs_ldy = bs_y->ld;
  return q;
}

inline RxChChoice rx_ch_choose(const RxChQuery& q) {
  RxChChoice c = {};                                     // RX_CH_FALLTHROUGH
  const rx_dtype dt = q.dt;
  if (dt != RX_F32 && dt != RX_BF16 && dt != RX_F16) return c;
  const int per16 = dt == RX_F32 ? 4 : 8;
  const int KB = 4 * per16;
  if (q.Ci % KB || q.Co % 32 || q.ldi % per16 || q.ldo % 4) return c;
  if ((q.in_lo & 15) || (q.out_lo & 7) || (q.w_lo & 15)) return c;
  const long voxels = (long)q.Z * q.Y * q.X;
  if (voxels * (long)q.ldi >= (1L << 31)) return c;      // 32-bit halo offsets
  const int N = q.N, Ci = q.Ci, Co = q.Co;
  const bool flip = q.flip != 0, accumulate = q.accumulate != 0, bs = q.want_bs;
  c.in_ss = voxels * (long)q.ldi, c.out_ss = voxels * (long)q.ldo;
  c.in_cs = q.in_cs ? q.in_cs : KB, c.out_cs = q.out_cs ? q.out_cs : 32;
  const bool planar = q.in_cs || q.out_cs;
  if (planar && dt == RX_F32) return c;
  int TX = rx_ch_p2ceil(q.X);
  TX = TX < 4 ? 4 : (TX > 16 ? 16 : TX);
  const int rem = 256 / TX;
  int TY = rx_ch_p2ceil(q.Y);
  const int capy = TX == 16 ? 4 : 8;
  if (TY > capy) TY = capy;
  if (TY > rem) TY = rem;
  int TZ = rx_ch_p2ceil(q.Z);
  if (TZ > rem / TY) TZ = rem / TY;
  if (TZ * TY * TX != 256) return c;                     // the kernels are written for full 256-voxel tiles
  c.TZ = TZ, c.TY = TY, c.TX = TX, c.lTX = rx_ch_ilog2(TX), c.lTY = rx_ch_ilog2(TY);
  c.HY = TY + 2, c.HX = TX + 2, c.HV = (TZ + 2) * c.HY * c.HX;
  if (c.HV > RX_CH_PLAN_MAX_HV) return c;
  c.tz_n = (q.Z + TZ - 1) / TZ, c.ty_n = (q.Y + TY - 1) / TY, c.tx_n = (q.X + TX - 1) / TX;
  c.NT = N * c.tz_n * c.ty_n * c.tx_n;
  c.order = 1;               // persistent kernels: z-fastest columns; one-tile grids: 4x4x4 bricks where the tile grid allows
  int BN = (Co % 64 == 0) ? 64 : 32;
  if (BN == 64 && (long)c.NT * (Co / 64) < 256) BN = 32;  // under-filled grid: twice the workgroups, half the work each
  if (planar && (long)c.NT * (Co / BN) < 192) return rx_ch_refuse(c, "conv_halo: planar-concat operand on a layer too small for the halo kernels");
  // Too few (tile, channel block) pairs to fill 256 CUs (128 pairs -- the 1024-channel data gradient of the first decoder conv
  // at 8^3 -- measured 93 us here, ~60 us on igemm_fat): the split-K gather kernel takes them.  A split-K variant of this kernel
  // (input channels over blockIdx.z, fp32 slabs + a fixed-order reduce) measured no gain against it, 35.7 + 5.5 us against 36 +
  // 5 us inside the cfg2 step: with 3-6 phases per workgroup it is a chain of cold weight-slice fetches, not an L2-bandwidth
  // problem.
  if ((long)c.NT * (Co / BN) < 192) return c;
  const bool tile4416 = TZ == 4 && TY == 4 && TX == 16;
  // room for the persistent families' partial sums: [n][<= 1024 chunks][2][Co] floats
  const bool room = q.stat_offered && (size_t)N * 1024 * 2 * Co * sizeof(float) <= q.stat_bytes;
  c.FLIP = flip;

  if (BN == 32 && tile4416 && dt != RX_F32 && Ci == 32 && Co == 32 && c.NT >= 512) {
    // 32 -> 32 channels: persistent, weights stationary in LDS
    if (planar) return rx_ch_refuse(c, "conv_halo32p: planar-concat operand");
    const bool fuse32 = room && ((!flip && !accumulate && !bs) || (flip && bs));
    c.take_stats = fuse32, c.take_bs = fuse32 && bs;
    c.BS = c.take_bs, c.STATS = fuse32 && !bs, c.ACC = accumulate;
    rx_ch_persistent_grid(c, 256, N, 1);
    c.stat_chunks = fuse32 ? c.wgs_s * 4 : 0;
    return rx_ch_launch(c, RX_CH_HALO32P, "conv_halo32p_kernel", RX_CH_LDS_HALO32P);
  }
  // 32-channel blocks on the wave-specialised DMA pipeline (the 256-channel layers at 16^3: 32 tiles x 8 blocks = one workgroup
  // per CU; alone 43 -> ~30 us against conv_halo32_kernel's one tile per workgroup).  LDS-DMA only: an input past the
  // buffer-descriptor range (out-of-range offsets must stay out of range of the descriptor; planar concat input: the planes lie
  // in_cs apart) takes conv_halo32_kernel as before.
  if (BN == 32 && tile4416 && dt != RX_F32 && !q.out_cs && Ci >= 64 && (long)c.NT * (Co / 32) >= 256 && !(accumulate && !flip) &&
      ((long)N * c.in_ss + (c.in_cs == 32 ? 0L : (long)(Ci / 32 - 1) * c.in_cs)) * 2 < 0x7fffff00L) {
    const bool fuse = room && !flip && !accumulate;
    c.take_stats = c.STATS = fuse;
    c.XDMA = true, c.ACC = flip && accumulate;
    rx_ch_persistent_grid(c, 256 / (Co / 32), N, (unsigned)(Co / 32));
    c.stat_chunks = fuse ? c.wgs_s * 4 : 0;
    return rx_ch_launch(c, RX_CH_HALO32WS, "conv_halo32ws_kernel", RX_CH_LDS_HALO32WS);
  }
  // one tile per workgroup: bricks of tiles where the tile grid allows
  const int order1 = (c.tx_n % 4 == 0 && c.ty_n % 4 == 0 && c.tz_n % 4 == 0) ? 2 : 1;
  if (BN == 32 && tile4416) {                            // full-resolution layers: compile-time tile, padded rows
    if (q.out_cs) return rx_ch_refuse(c, "conv_halo32: planar-concat output");
    // statistics in the epilogue only for DEEP layers (>= 4 input-channel chunks: >= 432 MFMAs per wave behind the one wavefront
    // reduction) with few tiles per sample (the finalize reads 4 partial rows per tile): the 16^3 layers
    const int NTs32 = c.NT / N;
    const bool fuse32n = q.stat_offered && !flip && !accumulate && dt != RX_F32 && Ci / KB >= 4 && NTs32 * 4 <= 1024 &&
                         (size_t)N * NTs32 * 4 * 2 * Co * sizeof(float) <= q.stat_bytes;
    c.take_stats = c.STATS = fuse32n;
    c.stat_chunks = fuse32n ? NTs32 * 4 : 0;
    c.order = order1;
    c.grid_x = (unsigned)c.NT, c.grid_y = (unsigned)(Co / 32), c.block = 256;
    return rx_ch_launch(c, RX_CH_HALO32, "conv_halo32_kernel", RX_CH_LDS_HALO32);
  }
  if (Co % 64 == 0 && tile4416 && dt != RX_F32 && (long)c.NT * (Co / 64) >= 256) {
    if (q.in_cs) return rx_ch_refuse(c, "conv_halo64ws: planar-concat input");
    // the weight planes always go by LDS-DMA; the halo too unless the input is past the buffer-descriptor range (out-of-range
    // offsets must stay out of range of the descriptor)
    const bool dma_ok = (long)N * c.in_ss * 2 < 0x7fffff00L;
    // only the DMA instantiations accumulate sums; backward sums run on the producer waves with whole-row 16-byte stores / loads.
    // Not taken: the caller runs the separate reduce pass.
    c.take_stats = room && dma_ok && !flip && !accumulate && !bs;
    c.take_bs = room && dma_ok && flip && bs && !(q.out_lo & 15) && q.ldo % 8 == 0 && c.out_cs % 8 == 0 && !(q.bsy_lo & 15) && q.bs_ldy % 8 == 0;
    c.STATS = c.take_stats, c.BS = c.take_bs, c.XDMA = dma_ok;
    c.ACC = dma_ok && flip && accumulate;                // dx +=: old values prefetched (else the epilogue reads them)
    c.take_stats = c.take_stats || c.take_bs;            // the backward sums leave their partial rows in the same buffer
    rx_ch_persistent_grid(c, 256 / (Co / 64), N, (unsigned)(Co / 64));
    c.stat_chunks = c.take_stats ? c.wgs_s * 4 : 0;
    return rx_ch_launch(c, RX_CH_HALO64WS, "conv_halo64ws_kernel", RX_CH_LDS_HALO64WS);
  }
  if (planar) return rx_ch_refuse(c, "conv_halo: planar-concat operand on the generic halo kernel");
  c.order = order1;
  c.grid_x = (unsigned)c.NT, c.grid_y = (unsigned)(Co / BN), c.block = 256;
  c.FLIP = false;                                        // (run-time in the generic kernel: one instantiation per block width)
  return BN == 64 ? rx_ch_launch(c, RX_CH_GENERIC64, "conv_halo_kernel<64>", RX_CH_LDS_GENERIC(64))
                  : rx_ch_launch(c, RX_CH_GENERIC32, "conv_halo_kernel<32>", RX_CH_LDS_GENERIC(32));
}
