// rx_gather_plan.h -- what the conv entry points of rx_igemm.hip launch: the geometry of every gather launch, which kernel runs it
// with what split, whether the streaming 1x1x1 kernel or the stride-2 parity-plane kernel takes the call instead, and in which
// order these are tried.  No HIP in here: every function is a pure function of descriptors (an rx_act's pointer is only looked at
// for its low bits), so every branch runs on the CPU in tools/conv_plan_check.cpp.  rx_igemm.hip, rx_pointwise.hip and
// rx_dgrad_s2.hip launch exactly what a choice says.  The structs the kernels take by value live here too; their layout is part
// of the kernels' argument layout.
#pragma once
#include <stdio.h>
#include <string.h>

#include "rx_conv_halo_plan.h"

static inline long rx_act_voxels(const rx_act* a) { return (long)a->z * a->y * a->x; }

// ---- tap tables shared by the implicit-GEMM and weight-gradient kernels ------------------------------------------------------
// kernel sizes 1..7 and strides 1..4 per axis (the reference passes any `kernel_sizes` / `strides` of a manual model_config
// straight to Conv(k, stride, pad = (k-1)//2), build_network_from_config.py:85-148): up to 7^3 = 343 taps per launch, so the
// weight index needs 9 bits and the tables live in the kernel arguments (RX_MAX_TAPS x 8 bytes, within the 4 KB kernarg limit)
#define RX_MAX_TAPS 344
#define RX_MAX_KERNEL 7
#define RX_MAX_STRIDE 4
struct RxTap {
  int8_t dz, dy, dx, pad_;
  uint16_t w, pad2_;
};

inline int rx_conv_out_dim(int in, int k, int s) { return (in + 2 * ((k - 1) / 2) - k) / s + 1; }
inline bool rx_conv_dims_match(const rx_act* in, const rx_act* out, const int32_t k[3], const int32_t s[3]) {
  return out->n == in->n && out->z == rx_conv_out_dim(in->z, k[0], s[0]) && out->y == rx_conv_out_dim(in->y, k[1], s[1]) &&
         out->x == rx_conv_out_dim(in->x, k[2], s[2]);
}
inline bool rx_convT_dims_match(const rx_act* small, const rx_act* big, const int32_t s[3]) {
  return small->n == big->n && big->z == small->z * s[0] && big->y == small->y * s[1] && big->x == small->x * s[2];
}
// the one range check: 0 in range, 1 a kernel size outside 1..RX_MAX_KERNEL (kernel may be null: transposed conv), 2 a stride
// outside 1..RX_MAX_STRIDE; *bad = the first offending value
inline int rx_conv_range(const int32_t* kernel, const int32_t stride[3], int* bad) {
  for (int i = 0; i < 3; ++i) {
    if (kernel && (kernel[i] < 1 || kernel[i] > RX_MAX_KERNEL)) return *bad = kernel[i], 1;
    if (stride[i] < 1 || stride[i] > RX_MAX_STRIDE) return *bad = stride[i], 2;
  }
  return 0;
}
inline bool rx_is_all(const int32_t v[3], int a) { return v[0] == a && v[1] == a && v[2] == a; }

// the taps of a kernel centred with pad (k-1)/2, weight index = position in the kernel; returns their number
inline int rx_taps_centred(RxTap* t, const int32_t k[3]) {
  int n = 0;
  const int pz = (k[0] - 1) / 2, py = (k[1] - 1) / 2, px = (k[2] - 1) / 2;
  for (int a = 0; a < k[0]; ++a)
    for (int b = 0; b < k[1]; ++b)
      for (int c = 0; c < k[2]; ++c, ++n) t[n].dz = (int8_t)(a - pz), t[n].dy = (int8_t)(b - py), t[n].dx = (int8_t)(c - px), t[n].w = (uint16_t)n;
  return n;
}
// the taps of a transposed conv with kernel == stride: offsets 0..s-1 inside a coarse voxel
inline int rx_taps_transposed(RxTap* t, const int32_t s[3]) {
  int n = 0;
  for (int a = 0; a < s[0]; ++a)
    for (int b = 0; b < s[1]; ++b)
      for (int c = 0; c < s[2]; ++c, ++n) t[n].dz = (int8_t)a, t[n].dy = (int8_t)b, t[n].dx = (int8_t)c, t[n].w = (uint16_t)n;
  return n;
}

// ---- the gather kernels (rx_igemm.hip) -----------------------------------------------------------------------------------------
// One launch covers up to 8 PHASES that share input / output / weights but differ in iteration grid, output
// phase offset and tap list: the 8 output parity classes of a stride-2 backward-data, or the 8 kernel positions
// of a k=s=2 transposed convolution (previously 8 launches of ~10 us each).
struct IgemmPhase {
  int Qz, Qy, Qx, Vq;
  int opz, opy, opx;
  int tap0, ntaps;
  int mtile0, mtiles;
  long slab_off;  // element offset of this phase's split-K slabs
};

struct IgemmGeom {
  int Zi, Yi, Xi, Ci, ldi;
  long in_ss;
  int isz, isy, isx;
  int Zo, Yo, Xo, Co, ldo;
  long out_ss;
  int osz, osy, osx;
  int accumulate, ksplit, nph, total_mtiles;
  IgemmPhase ph[8];
  RxTap taps[RX_MAX_TAPS];
};

// a zeroed geometry reading `in` with step `is` and writing `out` with step `os`
inline void rx_gather_reset(IgemmGeom& g, const rx_act* in, const rx_act* out, const int32_t* is, const int32_t* os, int accumulate) {
  memset(&g, 0, sizeof(g));
  g.Zi = in->z, g.Yi = in->y, g.Xi = in->x, g.Ci = in->c, g.ldi = in->ld, g.in_ss = rx_act_voxels(in) * (long)in->ld;
  g.Zo = out->z, g.Yo = out->y, g.Xo = out->x, g.Co = out->c, g.ldo = out->ld, g.out_ss = rx_act_voxels(out) * (long)out->ld;
  g.isz = is ? is[0] : 1, g.isy = is ? is[1] : 1, g.isx = is ? is[2] : 1;
  g.osz = os ? os[0] : 1, g.osy = os ? os[1] : 1, g.osx = os ? os[2] : 1;
  g.accumulate = accumulate;
}
// one phase over the whole grid of `q`, every tap of the table
inline void rx_gather_one_phase(IgemmGeom& g, const rx_act* q, int ntaps) {
  g.nph = 1;
  g.ph[0].Qz = q->z, g.ph[0].Qy = q->y, g.ph[0].Qx = q->x, g.ph[0].Vq = (int)rx_act_voxels(q), g.ph[0].ntaps = ntaps;
}
// forward: y[q] = sum_t x[q*s + t] W[t]
inline void rx_gather_fwd(IgemmGeom& g, const rx_act* x, const rx_act* y, const int32_t k[3], const int32_t s[3]) {
  rx_gather_reset(g, x, y, s, nullptr, 0);
  rx_gather_one_phase(g, y, rx_taps_centred(g.taps, k));
}
// transposed backward-data: dx[i] = sum_t dy[i*s + t] W[t]^T
inline void rx_gather_convT_bwd_data(IgemmGeom& g, const rx_act* dy, const rx_act* dx, const int32_t s[3], int accumulate) {
  rx_gather_reset(g, dy, dx, s, nullptr, accumulate);
  rx_gather_one_phase(g, dx, rx_taps_transposed(g.taps, s));
}
// backward-data: dx[s*q + r] = sum_{t : (r+p-t) % s == 0} dy[q + (r+p-t)/s] * W[t]^T      per axis; one PHASE per parity class r.
// Up to 8 phases and RX_MAX_TAPS taps per launch: stride 2 is one launch (8 classes, 27 taps), strides 3 / 4 or 5..7-wide
// kernels take a few (the classes write disjoint voxels, so the launches are independent).  Fills the next launch from class
// *cls on (start at 0) and advances *cls; false: no class is left.
inline bool rx_gather_bwd_data_next(IgemmGeom& g, const rx_act* dy, const rx_act* dx, const int32_t k[3], const int32_t s[3], int accumulate,
                                    int* cls) {
  rx_gather_reset(g, dy, dx, nullptr, s, accumulate);
  const int p[3] = {(k[0] - 1) / 2, (k[1] - 1) / 2, (k[2] - 1) / 2}, din[3] = {dx->z, dx->y, dx->x};
  int ntap_total = 0;
  for (; *cls < s[0] * s[1] * s[2]; ++*cls) {
    const int r[3] = {*cls / (s[1] * s[2]), *cls / s[2] % s[1], *cls % s[2]};
    int Q[3];
    for (int a = 0; a < 3; ++a) Q[a] = (din[a] - r[a] + s[a] - 1) / s[a];
    if (Q[0] * Q[1] * Q[2] <= 0) continue;
    // a class without any tap (kernel narrower than the stride) still has to WRITE its voxels: zeros (or keep dx when accumulating)
    RxTap mine[RX_MAX_TAPS];
    int cnt = 0;
    for (int a = 0; a < k[0]; ++a) {
      if ((r[0] + p[0] - a) % s[0]) continue;
      for (int b = 0; b < k[1]; ++b) {
        if ((r[1] + p[1] - b) % s[1]) continue;
        for (int c = 0; c < k[2]; ++c) {
          if ((r[2] + p[2] - c) % s[2]) continue;
          RxTap& t = mine[cnt++];
          memset(&t, 0, sizeof(t));
          t.dz = (int8_t)((r[0] + p[0] - a) / s[0]), t.dy = (int8_t)((r[1] + p[1] - b) / s[1]), t.dx = (int8_t)((r[2] + p[2] - c) / s[2]);
          t.w = (uint16_t)((a * k[1] + b) * k[2] + c);
        }
      }
    }
    if (g.nph == 8 || ntap_total + cnt > RX_MAX_TAPS) break;
    IgemmPhase& P = g.ph[g.nph++];
    P.Qz = Q[0], P.Qy = Q[1], P.Qx = Q[2], P.Vq = Q[0] * Q[1] * Q[2];
    P.opz = r[0], P.opy = r[1], P.opx = r[2];
    P.tap0 = ntap_total, P.ntaps = cnt;
    memcpy(g.taps + ntap_total, mine, cnt * sizeof(RxTap));
    ntap_total += cnt;
  }
  return g.nph > 0;
}
// transposed forward: y[i*s + t] = sum_ci x[i] W[ci][co][t] + b : one single-tap PHASE per kernel position t, up to 8 per launch;
// *pos as *cls above
inline bool rx_gather_convT_fwd_next(IgemmGeom& g, const rx_act* x, const rx_act* y, const int32_t s[3], int* pos) {
  rx_gather_reset(g, x, y, nullptr, s, 0);
  for (; *pos < s[0] * s[1] * s[2] && g.nph < 8; ++*pos, ++g.nph) {
    IgemmPhase& P = g.ph[g.nph];
    P.Qz = x->z, P.Qy = x->y, P.Qx = x->x, P.Vq = (int)rx_act_voxels(x);
    P.opz = *pos / (s[1] * s[2]), P.opy = *pos / s[2] % s[1], P.opx = *pos % s[2];
    P.tap0 = g.nph, P.ntaps = 1;
    g.taps[g.nph].w = (uint16_t)*pos;
  }
  return g.nph > 0;
}

// the grid of igemm_splitk_reduce over `total` 4-channel pieces
inline unsigned rx_gather_reduce_grid(long total) { return (unsigned)((total + 255) / 256 > 2048 ? 2048 : (total + 255) / 256); }
enum RxGatherKind { RX_GA_NOTHING = 0, RX_GA_REFUSE, RX_GA_FAT, RX_GA_TILE };   // NOTHING: no voxel to compute, RX_OK
struct RxGatherChoice {
  RxGatherKind kind;
  char message[96];            // RX_GA_REFUSE: the error text (RX_EUNSUPPORTED)
  const char* name;            // for rx_note_kernel
  int BM, BN, ks;
  unsigned grid[3];
  size_t lds;
  unsigned rgrid[2];           // the split-K reduce (0: none)
  int NV, nsteps;              // RX_GA_FAT: rows and K steps
};

// Which gather kernel runs the geometry `g` of N samples; fills g.ksplit, g.total_mtiles and each phase's mtile0 / mtiles /
// slab_off.  ws / ws_bytes: whether the caller passed a workspace and its size; *_lo: the low address bits of the operands.
inline RxGatherChoice rx_gather_choose(rx_dtype dt, IgemmGeom& g, int N, bool ws, size_t ws_bytes, unsigned in_lo, unsigned out_lo, unsigned w_lo) {
  RxGatherChoice c = {};
  const int per16 = dt == RX_F32 ? 4 : 8;
  const int KB = 4 * per16;
  c.kind = RX_GA_REFUSE;
  if (g.Ci % KB) return snprintf(c.message, sizeof(c.message), "igemm: input channels must be a multiple of %d (got %d)", KB, g.Ci), c;
  if (g.Co % 32) return snprintf(c.message, sizeof(c.message), "igemm: output channels must be a multiple of 32 (got %d)", g.Co), c;
  if (g.ldi % per16 || g.ldo % 4 || (in_lo & 15) || (out_lo & 7) || (w_lo & 15))
    return snprintf(c.message, sizeof(c.message), "igemm: misaligned operand (ldi=%d ldo=%d)", g.ldi, g.ldo), c;
  int vmax = 0, nkt_max = 0;
  for (int i = 0; i < g.nph; ++i) {
    vmax = g.ph[i].Vq > vmax ? g.ph[i].Vq : vmax;
    nkt_max = g.ph[i].ntaps > nkt_max ? g.ph[i].ntaps : nkt_max;
  }
  nkt_max *= g.Ci / KB;
  c.kind = RX_GA_NOTHING;
  if (vmax <= 0 || g.nph <= 0) return c;
  // low-resolution layers: fat K steps, batch folded into M (see igemm_fat_kernel)
  const int KE = 16 * per16;
  const long NV = (long)N * g.ph[0].Vq;
  if (dt != RX_F32 && g.nph == 1 && g.Ci % KE == 0 && g.Co % 64 == 0 && NV <= 2048 && ws &&
      g.ph[0].ntaps * (g.Ci / KE) >= 8 && g.ph[0].opz == 0 && g.ph[0].opy == 0 && g.ph[0].opx == 0 && g.osz == 1 && g.osy == 1 &&
      g.osx == 1) {
    const int mtiles = (int)((NV + 127) / 128);
    const int nsteps = g.ph[0].ntaps * (g.Ci / KE);
    const long base_wgs = (long)mtiles * (g.Co / 64);
    int ks = (int)((512 + base_wgs - 1) / base_wgs);      // aim at 512 workgroups
    if (ks > nsteps / 4) ks = nsteps / 4;   // >= 4 K steps per workgroup; also bounds the serial sum of the reduce
    if (ks < 1) ks = 1;
    while (ks > 1 && (size_t)ks * NV * g.Co * sizeof(float) > ws_bytes) --ks;
    if ((size_t)ks * NV * g.Co * sizeof(float) <= ws_bytes) {
      g.ksplit = ks;
      g.total_mtiles = mtiles;
      g.ph[0].mtile0 = 0, g.ph[0].mtiles = mtiles, g.ph[0].slab_off = 0;
      c.kind = RX_GA_FAT, c.name = "igemm_fat_kernel", c.ks = ks, c.NV = (int)NV, c.nsteps = nsteps;
      c.lds = (size_t)(128 + 64) * 256;
      c.grid[0] = (unsigned)(mtiles * ks), c.grid[1] = (unsigned)(g.Co / 64), c.grid[2] = 1;
      // the reduce always runs here (even for ks == 1 the kernel only writes fp32 slabs): force its split path
      c.rgrid[0] = rx_gather_reduce_grid(NV * (g.Co / 4)), c.rgrid[1] = 1;
      return c;
    }
  }
  const int BN = (g.Co % 64 == 0) ? 64 : 32;
  const int BM = (vmax <= 128) ? 128 : 256;
  g.total_mtiles = 0;
  long vsum = 0;
  for (int i = 0; i < g.nph; ++i) {
    g.ph[i].mtile0 = g.total_mtiles;
    g.ph[i].mtiles = (g.ph[i].Vq + BM - 1) / BM;
    g.total_mtiles += g.ph[i].mtiles;
    vsum += g.ph[i].Vq;
  }
  // split-K when the natural grid cannot fill the chip and K is deep
  const long wgs = (long)g.total_mtiles * (g.Co / BN) * N;
  int ks = 1;
  if (wgs < 192 && nkt_max >= 16 && ws) {
    ks = (int)((512 + wgs - 1) / wgs);
    if (ks > nkt_max / 4) ks = nkt_max / 4;
    if (ks > 32) ks = 32;
    size_t need = (size_t)ks * N * vsum * g.Co * sizeof(float);
    while (ks > 1 && need > ws_bytes) {
      --ks;
      need = (size_t)ks * N * vsum * g.Co * sizeof(float);
    }
    if (ks < 1) ks = 1;
  }
  long off = 0;
  for (int i = 0; i < g.nph; ++i) {
    g.ph[i].slab_off = off;
    off += (long)ks * N * g.ph[i].Vq * g.Co;
  }
  g.ksplit = ks;
  c.kind = RX_GA_TILE, c.BM = BM, c.BN = BN, c.ks = ks;
  c.name = BM == 256 ? (BN == 64 ? "igemm_kernel<256,64>" : "igemm_kernel<256,32>") : (BN == 64 ? "igemm_kernel<128,64>" : "igemm_kernel<128,32>");
  c.grid[0] = (unsigned)(g.total_mtiles * ks), c.grid[1] = (unsigned)(g.Co / BN), c.grid[2] = (unsigned)N;
  if (ks > 1) c.rgrid[0] = rx_gather_reduce_grid((long)N * vmax * (g.Co / 4)), c.rgrid[1] = (unsigned)g.nph;
  return c;
}

// ---- pointwise_kernel (rx_pointwise.hip) ---------------------------------------------------------------------------------------
struct PwGeom {
  int N, Zi, Yi, Xi, Ci, ldi;
  long in_ss;
  int Yo, Xo, Co, ldo;
  long out_ss;
  int sz, sy, sx;      // output voxel = s * input voxel + tap (1 or 2 per axis); taps = sz * sy * sx
  int accumulate;
  int ntiles;          // tiles of 128 rows (n, z, y, x flattened)
};
#define RX_PW_MAXKS 16   // Ci <= 256: 16 B-fragment registers of 16 bytes per lane

struct RxPwChoice {
  bool ok;             // false: the call is not for this kernel
  PwGeom g;
  unsigned grid[2];
  size_t lds;
};
// in: the tensor on the small grid (Zi, Yi, Xi); out voxel = s * in voxel + tap; w = [taps][Co][Ci] packed weights.
inline RxPwChoice rx_pw_choose(rx_dtype dt, const rx_act* in, unsigned w_lo, const rx_act* out, const int32_t stride[3], int accumulate) {
  RxPwChoice c = {};
  if (dt == RX_F32 || in->cs || out->cs) return c;
  const int taps = stride[0] * stride[1] * stride[2];
  const int Ci = in->c, Co = out->c;
  if (Ci % 16 || Ci > 16 * RX_PW_MAXKS || Co % 32 || in->ld % 8 || out->ld % 8 || rx_lo4(in->ptr) || rx_lo4(out->ptr) || (w_lo & 15)) return c;
  c.lds = (size_t)taps * 32 * (Ci * 2 + 16);
  if (c.lds > 150 * 1024) return c;
  if (taps > 1 && c.lds > 80 * 1024) return c;          // one workgroup per CU: the 256 -> 128 transposed conv measured 20.7 vs 19.1 us on the gather kernel
  const long NV = (long)in->n * rx_act_voxels(in);
  if (NV < 4096) return c;                              // the low-resolution layers stay on the split-K kernels
  PwGeom& g = c.g;
  g.N = in->n, g.Zi = in->z, g.Yi = in->y, g.Xi = in->x, g.Ci = Ci, g.ldi = in->ld;
  g.in_ss = rx_act_voxels(in) * (long)in->ld;
  g.Yo = out->y, g.Xo = out->x, g.Co = Co, g.ldo = out->ld;
  g.out_ss = rx_act_voxels(out) * (long)out->ld;
  g.sz = stride[0], g.sy = stride[1], g.sx = stride[2];
  g.accumulate = accumulate;
  g.ntiles = (int)((NV + 127) / 128);
  // persistent: as many workgroups as stay resident (LDS-limited), each walking tiles with stride gridDim.x
  int per_cu = (int)((160 * 1024) / (c.lds + 1024));
  if (per_cu > 8) per_cu = 8;
  if (per_cu < 1) per_cu = 1;
  int gx = 256 * per_cu / (Co / 32);
  if (gx < 1) gx = 1;
  if (gx > g.ntiles) gx = g.ntiles;
  c.grid[0] = (unsigned)gx, c.grid[1] = (unsigned)(Co / 32);
  c.ok = true;
  return c;
}

// ---- dgrad_s2p_kernel (rx_dgrad_s2.hip) ----------------------------------------------------------------------------------------
#define DS2_HZ 5
#define DS2_HY 5
#define DS2_HX 17
#define DS2_HV (DS2_HZ * DS2_HY * DS2_HX)   // 425 rows per chunk
#define DS2P_W_BYTES (26 * 2 * 32 * 64)       // 106,496
#define DS2P_X_BYTES (2 * DS2_HV * 64)        // 54,400
struct DgradS2Geom {
  int N, Zo, Yo, Xo;       // dY grid
  int Z, Y, X;             // dX grid (= 2 * dY grid)
  int Ci, Co;              // dX channels (conv input), dY channels (conv output, == 64)
  int ldy, ldx;
  long dy_ss, dx_ss;
  int tz_n, ty_n, tx_n, NT;
  int accumulate, dbg;
};
struct RxDs2Choice {
  bool ok;
  DgradS2Geom g;
  int per;                 // tiles per workgroup
  unsigned grid[2];
  size_t lds;
};
inline RxDs2Choice rx_ds2_choose(rx_dtype dt, const rx_act* dy, unsigned w_lo, const rx_act* dx, int accumulate) {
  RxDs2Choice c = {};
  if (dt == RX_F32 || dy->c != 64 || dx->c % 32 || dy->ld % 8 || dx->ld % 4 || rx_lo4(dy->ptr) || (rx_lo4(dx->ptr) & 7) || (w_lo & 15)) return c;
  if (dx->z != 2 * dy->z || dx->y != 2 * dy->y || dx->x != 2 * dy->x) return c;     // even input extents only
  if (rx_act_voxels(dx) * (long)dx->ld >= (1L << 31) || rx_act_voxels(dy) * (long)dy->ld >= (1L << 31)) return c;
  DgradS2Geom& g = c.g;
  g.N = dy->n, g.Zo = dy->z, g.Yo = dy->y, g.Xo = dy->x;
  g.Z = dx->z, g.Y = dx->y, g.X = dx->x;
  g.Ci = dx->c, g.Co = dy->c, g.ldy = dy->ld, g.ldx = dx->ld;
  g.dy_ss = rx_act_voxels(dy) * (long)dy->ld, g.dx_ss = rx_act_voxels(dx) * (long)dx->ld;
  g.tz_n = (g.Zo + 3) / 4, g.ty_n = (g.Yo + 3) / 4, g.tx_n = (g.Xo + 15) / 16;
  g.NT = g.N * g.tz_n * g.ty_n * g.tx_n;
  g.accumulate = accumulate;
  if ((long)g.NT * (g.Ci / 32) < 256) return c;                 // small layers: the gather kernel's split-K fills the chip better
  c.lds = (size_t)DS2P_W_BYTES + DS2P_X_BYTES;                  // 160,896 B
  int wgs = 256 / (g.Ci / 32);
  if (wgs < 1) wgs = 1;
  if (wgs > g.NT) wgs = g.NT;
  c.per = (g.NT + wgs - 1) / wgs;
  wgs = (g.NT + c.per - 1) / c.per;
  c.grid[0] = (unsigned)wgs, c.grid[1] = (unsigned)(g.Ci / 32);
  c.ok = true;
  return c;
}

// ---- routes: the ordered outcome of an entry point ---------------------------------------------------------------------------
// RX_RT_PLAIN: the statistics entry points hand the call to the plain entry point (and its route)
enum RxRouteKind { RX_RT_REFUSE = 0, RX_RT_HALO, RX_RT_POINTWISE, RX_RT_DS2, RX_RT_GATHER, RX_RT_PLAIN };
struct RxConvRoute {
  int kind, code;          // RxRouteKind; the code of a refusal
  char message[128];
  RxChChoice halo;         // RX_RT_HALO
  RxPwChoice pw;           // RX_RT_POINTWISE
  RxDs2Choice ds2;         // RX_RT_DS2
};
// a refusal (kind 0 of either route type), and the one of rx_conv_range; got: the text names the offending value
template <typename R>
inline R rx_route_refuse(R r, int code, const char* who, const char* what, int a = 0, int b = 0) {
  r.kind = 0, r.code = code;
  const int n = snprintf(r.message, sizeof(r.message), "%s", who);
  snprintf(r.message + n, sizeof(r.message) - n, what, a, b);
  return r;
}
template <typename R>
inline R rx_route_range(R r, const char* who, int which, int bad, bool got = true) {
  const char* what = which == 1 ? (got ? ": kernel sizes must be 1..%d per axis (got %d)" : ": kernel sizes must be 1..%d per axis")
                                : (got ? ": strides must be 1..%d per axis (got %d)" : ": strides must be 1..%d per axis");
  return rx_route_refuse(r, RX_EUNSUPPORTED, who, what, which == 1 ? RX_MAX_KERNEL : RX_MAX_STRIDE, bad);
}
// the halo leg of a route: true when it settles the call (a launch or a refusal)
inline bool rx_route_halo(RxConvRoute& r, const RxChQuery& q) {
  r.halo = rx_ch_choose(q);
  if (r.halo.kind == RX_CH_REFUSE) r = rx_route_refuse(r, RX_EUNSUPPORTED, r.halo.message, "");
  else if (r.halo.kind == RX_CH_LAUNCH) r.kind = RX_RT_HALO;
  return r.halo.kind != RX_CH_FALLTHROUGH;
}

// rx_conv3d_fwd (in = x, out = y) and rx_conv3d_bwd_data (flip: in = dy, out = dx): halo, planar refusal, pointwise, stride-2 halo
// (backward only), gather
inline RxConvRoute rx_route_conv(rx_dtype dt, const rx_act* in, unsigned w_lo, const rx_act* out, const int32_t k[3], const int32_t s[3], int flip,
                                 int accumulate) {
  RxConvRoute r = {};
  const char* who = flip ? "rx_conv3d_bwd_data" : "rx_conv3d_fwd";
  int bad = 0;
  if (const int which = rx_conv_range(k, s, &bad)) return rx_route_range(r, who, which, bad);
  if (!(flip ? rx_conv_dims_match(out, in, k, s) : rx_conv_dims_match(in, out, k, s)))
    return rx_route_refuse(r, RX_EINVAL, who, flip ? ": geometry mismatch" : ": output geometry mismatch");
  if (rx_is_all(k, 3) && rx_is_all(s, 1) && rx_route_halo(r, rx_ch_query(dt, in, w_lo, out, flip, accumulate, false, 0, nullptr))) return r;  // LDS-halo kernel
  if (flip ? out->cs : in->cs)
    return rx_route_refuse(r, RX_EUNSUPPORTED, who, flip ? ": a planar-concat dx needs the wave-specialised 64-channel halo kernel"
                                                         : ": a planar-concat input needs the 3x3x3 stride-1 halo kernel (Co = 32, X >= 16)");
  if (rx_is_all(k, 1) && rx_is_all(s, 1) && (r.pw = rx_pw_choose(dt, in, w_lo, out, s, accumulate)).ok) return r.kind = RX_RT_POINTWISE, r;  // streaming kernel, no spatial footprint
  if (flip && rx_is_all(k, 3) && rx_is_all(s, 2) && (r.ds2 = rx_ds2_choose(dt, in, w_lo, out, accumulate)).ok) return r.kind = RX_RT_DS2, r;  // LDS-halo kernel, all 8 parity classes
  return r.kind = RX_RT_GATHER, r;
}
// rx_conv3d_fwd_stats (in_y null) and rx_conv3d_bwd_data_instats (flip; in_y: the saved output of the layer whose gradient dx
// completes): the halo kernels with the partial-sum buffer, else the plain entry point (and a statistics pass / *fused = 0)
inline RxConvRoute rx_route_conv_stats(rx_dtype dt, const rx_act* in, unsigned w_lo, const rx_act* out, const int32_t k[3], const int32_t s[3],
                                       int accumulate, const rx_act* in_y, size_t stat_bytes) {
  RxConvRoute r = {};
  int bad = 0;
  if (const int which = rx_conv_range(k, s, &bad)) return rx_route_range(r, in_y ? "rx_conv3d_bwd_data_instats" : "rx_conv3d_fwd_stats", which, bad);
  bool fits = out->z == in->z && out->y == in->y && out->x == in->x;
  if (in_y) fits = fits && in_y->n == out->n && in_y->z == out->z && in_y->y == out->y && in_y->x == out->x && in_y->c == out->c && in_y->ld % 4 == 0 && !(rx_lo4(in_y->ptr) & 7);
  else fits = fits && out->n == in->n;
  if (fits && rx_is_all(k, 3) && rx_is_all(s, 1) && rx_route_halo(r, rx_ch_query(dt, in, w_lo, out, in_y != nullptr, accumulate, true, stat_bytes, in_y))) return r;
  return r.kind = RX_RT_PLAIN, r;
}
// rx_convT3d_fwd: pointwise (x once, y once), gather; rx_convT3d_bwd_data: gather
inline RxConvRoute rx_route_convT(rx_dtype dt, const rx_act* small, unsigned w_lo, const rx_act* big, const int32_t s[3], bool fwd) {
  RxConvRoute r = {};
  const char* who = fwd ? "rx_convT3d_fwd" : "rx_convT3d_bwd_data";
  int bad = 0;
  if (rx_conv_range(nullptr, s, &bad)) return rx_route_range(r, who, 2, bad, false);
  if (!rx_convT_dims_match(small, big, s)) return rx_route_refuse(r, RX_EINVAL, who, ": geometry mismatch");
  if (fwd && (r.pw = rx_pw_choose(dt, small, w_lo, big, s, 0)).ok) return r.kind = RX_RT_POINTWISE, r;
  return r.kind = RX_RT_GATHER, r;
}
