// rx_wgrad_plan.h -- what the weight-gradient entry points (rx_wgrad.hip, rx_wgrad_halo.hip) launch: tile widths, split counts,
// the DMA flag of the wave-specialised kernel, the reduce form, and the workspace sizes that bound the planners' needs.  No HIP in
// here (see rx_gather_plan.h): tools/conv_plan_check.cpp runs every branch on the CPU, the .hip files launch what a choice says.
#pragma once
#include "rx_gather_plan.h"

// ---- wgrad_kernel<BR,BC> -------------------------------------------------------------------------------------------------------
struct WgradGeom {
  int Qz, Qy, Qx, Vq, NQ;
  int R, ldg;
  long g_ss;
  int Zx, Yx, Xx, Cc, ldx;
  long x_ss;
  int isz, isy, isx;
  int ntaps, ksplit, q_per_split, tiles_c;
  RxTap taps[RX_MAX_TAPS];
};

// rows from `gt` (its grid is the iteration grid), columns from `xt`, read with step `s`; transposed: the taps of a kernel == stride
// transposed conv, dW[ci][co][t] = sum_i x[i][ci] * dy[i*s + t][co], else those of the centred kernel `k`
inline void rx_wgrad_geom(WgradGeom& g, const rx_act* gt, const rx_act* xt, const int32_t* k, const int32_t s[3]) {
  memset(&g, 0, sizeof(g));
  g.Qz = gt->z, g.Qy = gt->y, g.Qx = gt->x, g.Vq = (int)rx_act_voxels(gt), g.NQ = gt->n * g.Vq;
  g.R = gt->c, g.ldg = gt->ld, g.g_ss = (long)g.Vq * gt->ld;
  g.Zx = xt->z, g.Yx = xt->y, g.Xx = xt->x, g.Cc = xt->c, g.ldx = xt->ld, g.x_ss = rx_act_voxels(xt) * (long)xt->ld;
  g.isz = s[0], g.isy = s[1], g.isx = s[2];
  g.ntaps = k ? rx_taps_centred(g.taps, k) : rx_taps_transposed(g.taps, s);
}

// the split of BR x BC tiles: RX_EWORKSPACE when not even one slab fits
inline int rx_wgrad_split(int R, int Cc, int ntaps, long NQ, int BR, int BC, size_t ws_bytes, int* ksplit, int* qps) {
  const long tiles = (long)(R / BR) * (Cc / BC) * ntaps;
  const long ktiles = (NQ + 63) / 64;
  long S = (1024 + tiles - 1) / tiles;
  if (S > ktiles / 4) S = ktiles / 4;
  if (S < 1) S = 1;
  const size_t slab1 = (size_t)ntaps * R * Cc * sizeof(float);
  while (S > 1 && S * slab1 > ws_bytes) --S;
  if (slab1 > ws_bytes) return RX_EWORKSPACE;
  long per = (ktiles + S - 1) / S;
  S = (ktiles + per - 1) / per;
  *ksplit = (int)S;
  *qps = (int)(per * 64);
  return RX_OK;
}

struct RxWgradChoice {
  int code;                // RX_OK, or the refusal's code and text
  char message[96];
  const char* name;
  int BR, BC;
  unsigned grid[3];
  size_t lds;
};
// fills g.tiles_c, g.ksplit, g.q_per_split
inline RxWgradChoice rx_wgrad_choose(rx_dtype dt, WgradGeom& g, unsigned g_lo, unsigned x_lo, bool ws, bool dw, size_t ws_bytes) {
  RxWgradChoice c = {};
  const int per16 = dt == RX_F32 ? 4 : 8;
  c.code = RX_EUNSUPPORTED;
  if (g.R % 32 || g.Cc % 32) return snprintf(c.message, sizeof(c.message), "wgrad: channel counts must be multiples of 32 (R=%d C=%d)", g.R, g.Cc), c;
  if (g.ldg % per16 || g.ldx % per16 || (g_lo & 15) || (x_lo & 15)) return snprintf(c.message, sizeof(c.message), "wgrad: misaligned operand"), c;
  c.code = RX_EINVAL;
  if (!ws || !dw) return snprintf(c.message, sizeof(c.message), "wgrad: null workspace / output"), c;
  c.BR = g.R % 64 == 0 ? 64 : 32, c.BC = g.Cc % 64 == 0 ? 64 : 32;
  g.tiles_c = g.Cc / c.BC;
  c.code = rx_wgrad_split(g.R, g.Cc, g.ntaps, g.NQ, c.BR, c.BC, ws_bytes, &g.ksplit, &g.q_per_split);
  if (c.code) return snprintf(c.message, sizeof(c.message), "wgrad: workspace too small (%zu bytes)", ws_bytes), c;
  c.grid[0] = (unsigned)((g.R / c.BR) * (g.Cc / c.BC)), c.grid[1] = (unsigned)g.ntaps, c.grid[2] = (unsigned)g.ksplit;
  c.lds = 65536;
  c.name = c.BR == 64 ? (c.BC == 64 ? "wgrad_kernel<64,64>" : "wgrad_kernel<64,32>") : (c.BC == 64 ? "wgrad_kernel<32,64>" : "wgrad_kernel<32,32>");
  return c;
}
// what rx_wgrad_choose needs at most
inline size_t rx_wgrad_ws_bytes(int R, int C, int taps, long NQ) {
  const size_t slab1 = (size_t)taps * R * C * sizeof(float);
  const long tiles = (long)((R + 63) / 64) * ((C + 63) / 64) * taps;
  long S = (1024 + tiles - 1) / tiles;
  long ktiles = (NQ + 63) / 64;
  if (S > ktiles / 4) S = ktiles / 4;
  if (S < 1) S = 1;
  // BR/BC may fall back to 32 (4x the tiles) -> S only shrinks; this bound is safe
  if (R % 64 || C % 64) {
    const long t32 = (long)(R / 32) * (C / 32) * taps;
    long S2 = (1024 + t32 - 1) / t32;
    if (S2 > S) S = S2;
  }
  return S * slab1 + 256;
}

// the reduce both weight-gradient files end with: many splits or many taps take wgrad_reduce_manysplits
// (wgrad_reduce transposes a [256][T <= 27] tile through LDS)
inline bool rx_wgrad_reduce_manysplits(int S, int T_) { return S >= 8 || T_ > 27; }

// ---- wgrad_halo_kernel / wgrad_halo16ws_kernel (3x3x3, 16-bit types) ------------------------------------------------------------
struct WgHaloGeom {
  int N, Z, Y, X;
  int R, Cc, ldg, ldx;
  long g_ss, x_ss;
  long x_cs;             // planar concat x (rx_act.cs): element offset of 32-channel group j = j * x_cs; 0 = contiguous channels
  int TZ, TY, TX, lTX, lTY;
  int HY, HX, HV, VT;
  int tz_n, ty_n, tx_n, NT;
  int S, tiles_per_split, panels_c;
  int sz, sy, sx;        // conv stride per axis (1 or 2); the X halo of a TZ x TY x TX tile of dY is (s*(T-1)+3) per axis
  int Zi, Yi, Xi;        // extent of X (the conv INPUT); Z, Y, X above are the extent of dY
  int order; // tile walk order (rx_tile_coords)
  int dbg;   // ablation mask (RX_DBG env): 1 stage only the first tile, 2 no MFMA loop
};
#define RX_WGH_MAX_HV 768
#define RX_WGH_MAX_VT 256
#define WGH16_HV 648
#define WGH16_BUF_BYTES ((256 + WGH16_HV) * 64)   // one (dY tile, X halo tile) pair: 57,856 bytes

struct RxWghChoice {
  bool ok;               // false: the call falls through to wgrad_kernel
  WgHaloGeom g;
  bool ws16, DMA;        // the wave-specialised 4x4x16 kernel; its producers stage by LDS-DMA
  const char* name;
  unsigned grid[2], block;
  size_t lds;
};
inline RxWghChoice rx_wgh_choose(rx_dtype dt, const rx_act* x, const rx_act* dy, const int32_t stride[3], size_t ws_bytes) {
  RxWghChoice c = {};
  if (dt == RX_F32) return c;
  if (x->c % 32 || dy->c % 32 || x->ld % 8 || dy->ld % 8 || rx_lo4(x->ptr) || rx_lo4(dy->ptr)) return c;
  WgHaloGeom* g = &c.g;
  g->N = dy->n, g->Z = dy->z, g->Y = dy->y, g->X = dy->x;
  g->Zi = x->z, g->Yi = x->y, g->Xi = x->x;
  g->sz = stride[0], g->sy = stride[1], g->sx = stride[2];
  g->R = dy->c, g->Cc = x->c, g->ldg = dy->ld, g->ldx = x->ld;
  g->g_ss = rx_act_voxels(dy) * (long)dy->ld;
  g->x_ss = rx_act_voxels(x) * (long)x->ld;
  g->x_cs = x->cs;
  const bool strided = stride[0] > 1 || stride[1] > 1 || stride[2] > 1;
  int TX = rx_ch_p2ceil(g->X);
  TX = TX < 4 ? 4 : (TX > 16 ? 16 : TX);
  if (strided && TX > 8) TX = 8;               // the X halo grows with the stride: 64-voxel tiles (2 x 4 x 8) keep it in LDS
  int budget = strided ? 64 : 256;
  int rem = budget / TX;
  int TY = rx_ch_p2ceil(g->Y);
  int capy = TX == 16 ? 4 : (strided ? 4 : 8);
  if (TY > capy) TY = capy;
  if (TY > rem) TY = rem;
  int TZ = rx_ch_p2ceil(g->Z);
  if (TZ > rem / TY) TZ = rem / TY;
  g->TZ = TZ, g->TY = TY, g->TX = TX, g->lTX = rx_ch_ilog2(TX), g->lTY = rx_ch_ilog2(TY);
  g->VT = TZ * TY * TX;
  const int HZ = g->sz * (TZ - 1) + 3;
  g->HY = g->sy * (TY - 1) + 3, g->HX = g->sx * (TX - 1) + 3, g->HV = HZ * g->HY * g->HX;
  if (g->VT < 16 || g->VT > RX_WGH_MAX_VT || g->HV > RX_WGH_MAX_HV || HZ > 255 || g->HY > 255 || g->HX > 255) return c;
  g->tz_n = (g->Z + TZ - 1) / TZ, g->ty_n = (g->Y + TY - 1) / TY, g->tx_n = (g->X + TX - 1) / TX;
  g->NT = g->N * g->tz_n * g->ty_n * g->tx_n;
  g->panels_c = g->Cc / 32;
  const long PP = (long)(g->R / 32) * g->panels_c;
  c.ws16 = !strided && TZ == 4 && TY == 4 && TX == 16;   // compile-time tile
  // the wave-specialised 4x4x16 kernel runs ONE workgroup per CU: 256 workgroups are one full wave of the chip (half the
  // slab traffic and reduce work of 512); the generic kernel runs two per CU
  long target = c.ws16 ? 256 : 512;
  if (target == 256 && g->NT * PP < 16 * 256) target = 512;   // few tiles (16^3 layers): shorter per-workgroup chains win
  long S = (target + PP - 1) / PP;
  if (PP >= 256) S = 1;  // the panel pairs alone fill the chip: accumulate every tile in registers, write dw directly
  if (S > g->NT) S = g->NT;
  if (S < 1) S = 1;
  const size_t slab1 = (size_t)27 * g->R * g->Cc * sizeof(float);
  while (S > 1 && S * slab1 > ws_bytes) --S;
  if (S > 1 && slab1 > ws_bytes) return c;
  g->tiles_per_split = (int)((g->NT + S - 1) / S);
  g->S = (g->NT + g->tiles_per_split - 1) / g->tiles_per_split;
  g->order = 1;   // z-fastest walk of each split's tile range (rx_tile_coords)
  c.grid[0] = (unsigned)((g->R / 32) * g->panels_c), c.grid[1] = (unsigned)g->S;
  if (c.ws16) {
    // the DMA producers address both tensors through 32-bit buffer offsets; larger tensors take the register-staged producers
    c.DMA = (long)g->N * g->g_ss * 2 < 0x7fffff00L &&
            ((long)g->N * g->x_ss + (g->x_cs ? (long)(g->Cc / 32 - 1) * g->x_cs : 0)) * 2 < 0x7fffff00L;
    c.name = "wgrad_halo16ws_kernel", c.block = 512, c.lds = (size_t)2 * WGH16_BUF_BYTES;
  } else {
    c.name = "wgrad_halo_kernel", c.block = 256, c.lds = (size_t)(RX_WGH_MAX_VT + RX_WGH_MAX_HV) * 64;
  }
  c.ok = true;
  return c;
}
// what rx_wgh_choose needs at most
inline size_t rx_wgh_ws_bytes(const rx_act* x, const rx_act* dy) {
  const long PP = (long)(dy->c / 32) * (x->c / 32);
  long S = PP > 0 ? (512 + PP - 1) / PP : 1;
  return (size_t)S * 27 * dy->c * x->c * sizeof(float) + 256;
}

// ---- convT_wgrad_kernel<NR,NC> (16-bit types, taps <= 8) -----------------------------------------------------------------------
struct ConvTWgGeom {
  int Vq, NQ, Qy, Qx;         // coarse voxels per sample / in total, coarse Y, X
  int R, ldr;                 // coarse channels (rows of dW)
  long r_ss;
  int Yf, Xf, Cc, ldc;        // fine tensor
  long c_ss;
  int sz, sy, sx, ntaps;
  int q_per_split;
};
inline int rx_ctw_splits(long NQ, size_t slab1) {
  long ktiles = (NQ + 63) / 64;
  long S = ktiles / 8;                    // >= 8 tiles per workgroup
  if (S > 256) S = 256;
  while (S > 32 && (size_t)S * slab1 > ((size_t)32 << 20)) S /= 2;      // slabs stay within ~32 MB (MALL-resident round trip)
  if (S < 1) S = 1;
  return (int)S;
}
struct RxCtwChoice {
  bool ok;                    // false: not applicable, the call falls through to wgrad_kernel
  ConvTWgGeom g;
  int NR, NC, S2;
  size_t lds;
};
inline RxCtwChoice rx_ctw_choose(rx_dtype dt, const rx_act* x, const rx_act* dy, const int32_t stride[3], size_t ws_bytes) {
  RxCtwChoice c = {};
  const int taps = stride[0] * stride[1] * stride[2];
  const int R = x->c, C = dy->c;
  if (dt == RX_F32 || taps > 8 || R % 32 || C % 32 || x->ld % 8 || dy->ld % 8 || rx_lo4(x->ptr) || rx_lo4(dy->ptr)) return c;
  c.NR = R / 32, c.NC = C / 32;
  if (!((c.NR == 2 && c.NC == 1) || (c.NR == 4 && c.NC == 2) || (c.NR == 1 && c.NC == 1) || (c.NR == 2 && c.NC == 2))) return c;
  const long NQ = (long)x->n * rx_act_voxels(x);
  if (NQ < 32768) return c;               // the low-resolution layers: too few tiles to split, the generic kernel is fine there
  const size_t slab1 = (size_t)taps * R * C * sizeof(float);
  const int S = rx_ctw_splits(NQ, slab1);
  if ((size_t)S * slab1 > ws_bytes) return c;
  ConvTWgGeom& g = c.g;
  g.Vq = (int)rx_act_voxels(x), g.NQ = (int)NQ, g.Qy = x->y, g.Qx = x->x;
  g.R = R, g.ldr = x->ld, g.r_ss = (long)g.Vq * x->ld;
  g.Yf = dy->y, g.Xf = dy->x, g.Cc = C, g.ldc = dy->ld, g.c_ss = rx_act_voxels(dy) * (long)dy->ld;
  g.sz = stride[0], g.sy = stride[1], g.sx = stride[2], g.ntaps = taps;
  const long ktiles = (NQ + 63) / 64;
  g.q_per_split = (int)(((ktiles + S - 1) / S) * 64);
  c.S2 = (int)((NQ + g.q_per_split - 1) / g.q_per_split);
  c.lds = (size_t)64 * (R + taps * C) * 2;
  c.ok = true;
  return c;
}

// ---- the two workspace sizes of include/rxunet.h --------------------------------------------------------------------------------
inline size_t rx_conv_bwd_weight_ws_bytes(const rx_act* x, const rx_act* dy, const int32_t kernel[3]) {
  size_t a = rx_wgrad_ws_bytes(dy->c, x->c, kernel[0] * kernel[1] * kernel[2], (long)dy->n * rx_act_voxels(dy));
  size_t b = rx_is_all(kernel, 3) ? rx_wgh_ws_bytes(x, dy) : 0;
  return a > b ? a : b;
}
inline size_t rx_convT_bwd_weight_ws_bytes(const rx_act* x, const rx_act* dy, const int32_t stride[3]) {
  const int taps = stride[0] * stride[1] * stride[2];
  const long NQ = (long)x->n * rx_act_voxels(x);
  const size_t slab1 = (size_t)taps * x->c * dy->c * sizeof(float);
  const size_t a = rx_wgrad_ws_bytes(x->c, dy->c, taps, NQ);
  const size_t b = (size_t)rx_ctw_splits(NQ, slab1) * slab1 + 256;
  return a > b ? a : b;
}

// ---- routes ----------------------------------------------------------------------------------------------------------------------
enum RxWRouteKind { RX_WR_REFUSE = 0, RX_WR_HALO, RX_WR_CONVT, RX_WR_GENERIC };
struct RxWgradRoute {
  int kind, code;          // RxWRouteKind; the code of a refusal
  char message[128];
  RxWghChoice halo;
  RxCtwChoice ctw;
};
// rx_conv3d_bwd_weight: the halo kernels (3x3x3, stride 1 or 2), planar refusal, wgrad_kernel; rx_convT3d_bwd_weight (k null):
// convT_wgrad_kernel (every operand byte once), wgrad_kernel
inline RxWgradRoute rx_route_bwd_weight(rx_dtype dt, const rx_act* x, const rx_act* dy, const int32_t* k, const int32_t s[3], bool ws, bool dw,
                                        size_t ws_bytes) {
  RxWgradRoute r = {};
  const char* who = k ? "rx_conv3d_bwd_weight" : "rx_convT3d_bwd_weight";
  int bad = 0;
  if (const int which = rx_conv_range(k, s, &bad)) return rx_route_range(r, who, which, bad, false);
  if (!(k ? rx_conv_dims_match(x, dy, k, s) : rx_convT_dims_match(x, dy, s))) return rx_route_refuse(r, RX_EINVAL, who, ": geometry mismatch");
  if (ws && dw && k && rx_is_all(k, 3) && (r.halo = rx_wgh_choose(dt, x, dy, s, ws_bytes)).ok) return r.kind = RX_WR_HALO, r;
  if (ws && dw && !k && (r.ctw = rx_ctw_choose(dt, x, dy, s, ws_bytes)).ok) return r.kind = RX_WR_CONVT, r;
  if (x->cs) return rx_route_refuse(r, RX_EUNSUPPORTED, who, ": a planar-concat x needs the LDS-halo weight-gradient kernels");
  return r.kind = RX_WR_GENERIC, r;
}
