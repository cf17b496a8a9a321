// rx_isosurface_core.h -- the per-cell and per-edge arithmetic of the surface-nets pass (rx_isosurface.hip), written so that it
// compiles for the host as well: csrc/tools/isosurface_host_check.cpp runs exactly these functions serially, row by row, against a
// direct restatement, under the address and undefined-behaviour sanitizers.  postprocess/isosurface.py (surface_nets_numpy) is the
// statement; every float32 operation here is one rounding (contraction is off, denormals are kept, / is correctly rounded).
//
// Geometry: a volume of (Z, Y, X) voxels, padded with 0, has (Z+1, Y+1, X+1) cells; cell (k, j, i) has corner 0 at voxel
// (k-1, j-1, i-1).  A cell ROW is (k, j); its cells are handled 64 at a time (a CHUNK, one wave along x), and everything that is one
// bit per cell -- inside flags of a voxel row, the active flags, the three crossing flags -- is one 64-bit word per chunk.
#ifndef RX_ISOSURFACE_CORE_H
#define RX_ISOSURFACE_CORE_H
#include <stdint.h>

#pragma clang fp contract(off)

#if defined(__HIPCC__)
#define RX_ISO_HD __host__ __device__ __forceinline__
#else
#define RX_ISO_HD inline
#endif

#define RX_ISO_BK 4      // a workgroup's band: 4 cell planes x 8 cell rows, which read 5 x 9 voxel rows
#define RX_ISO_BJ 8
#define RX_ISO_BAND (RX_ISO_BK * RX_ISO_BJ)
#define RX_ISO_VROWS ((RX_ISO_BK + 1) * (RX_ISO_BJ + 1))
#ifndef RX_ISO_MAX_EXTENT
#define RX_ISO_MAX_EXTENT 16777213      // 2^24 - 3: an extent of 2^24 - 2 or more is refused (include/rxunet.h says the same)
#define RX_ISO_MAX_CELLS 2147483646L    // 2^31 - 2
#endif
#define RX_ISO_MAX_BANDS 16777215L      // 2^24 - 1 workgroups of 256 threads: a launch holds fewer than 2^32 threads

RX_ISO_HD int iso_popc(uint64_t w) { return __builtin_popcountll(w); }
// the number of set bits of `w` below bit `lane` (0 .. 63)
RX_ISO_HD int iso_prefix(uint64_t w, int lane) { return iso_popc(w & ((1ull << lane) - 1ull)); }

// One chunk of a cell row.  b[dz*2 + dy] holds the inside flags of voxel row (k-1+dz, j-1+dy) at x = i0 .. i0+63 (bit l: x = i0 + l;
// 0 outside the volume) and bit q of `halo` the flag at x = i0 - 1.  Cell i0 + l has its dx = 0 corners at x = i0 + l - 1.
// -> the active cells, and the cells whose edge from corner 0 along z / y / x crosses (the quads they own)
RX_ISO_HD void iso_chunk_flags(const uint64_t b[4], unsigned halo, uint64_t* active, uint64_t* qz, uint64_t* qy, uint64_t* qx) {
  uint64_t a[4], all = ~0ull, any = 0ull;
  for (int q = 0; q < 4; ++q) {
    a[q] = (b[q] << 1) | (uint64_t)((halo >> q) & 1u);
    all &= a[q] & b[q];
    any |= a[q] | b[q];
  }
  *active = any & ~all;
  *qz = a[0] ^ a[2];
  *qy = a[0] ^ a[1];
  *qx = a[0] ^ b[0];
}

// The vertex of an active cell: c[dz*4 + dy*2 + dx] its corner values, (cz, cy, cx) the voxel coordinate of corner 0 (>= -1, exact
// in float32).  out = (x, y, z).
RX_ISO_HD void iso_vertex(const uint8_t c[8], int level, int cz, int cy, int cx, float out[3]) {
  const float iso = (float)level + 0.5f;      // exact
  float s[3] = {0.0f, 0.0f, 0.0f}, n = 0.0f;
  for (int d = 0; d < 3; ++d) {               // axis 0 z, 1 y, 2 x: the corner index has strides 4, 2, 1
    const int sd = 4 >> d, s0 = d == 0 ? 2 : 4, s1 = d == 2 ? 2 : 1;      // the other two axes, in z, y, x order
    const int ax0 = d == 0 ? 1 : 0, ax1 = d == 2 ? 1 : 2;
    for (int o0 = 0; o0 < 2; ++o0)
      for (int o1 = 0; o1 < 2; ++o1) {
        const int ia = o0 * s0 + o1 * s1, ib = ia + sd;
        const int va = c[ia], vb = c[ib];
        if ((va > level) == (vb > level)) continue;
        const float t = (iso - (float)va) / ((float)vb - (float)va);
        s[d] = s[d] + t;
        s[ax0] = s[ax0] + (float)o0;
        s[ax1] = s[ax1] + (float)o1;
        n = n + 1.0f;
      }
  }
  out[0] = (float)cx + s[2] / n;
  out[1] = (float)cy + s[1] / n;
  out[2] = (float)cz + s[0] / n;
}

// The two triangles of the quad that cell C = (k, j, i) owns in axis slot 0 z / 1 y / 2 x.  pC, pJ, pK, pKJ: the vertex ids of
// the cells at column i of rows (k, j), (k, j-1), (k-1, j), (k-1, j-1); the cell at column i - 1 of a row is active whenever it is
// needed, so its id is one less.  `inside`: corner 0 of C is inside.  t[0..2], t[3..5].
RX_ISO_HD void iso_quad(int slot, bool inside, int64_t pC, int64_t pJ, int64_t pK, int64_t pKJ, int64_t t[6]) {
  int64_t A, B, D;
  if (slot == 0) A = pJ - 1, B = pJ, D = pC - 1;            // z edge, (u, v) = (x, y): A = C - ex - ey, B = C - ey, D = C - ex
  else if (slot == 1) A = pK - 1, B = pC - 1, D = pK;       // y edge, (u, v) = (z, x): A = C - ez - ex, B = C - ex, D = C - ez
  else A = pKJ, B = pK, D = pJ;                             // x edge, (u, v) = (y, z): A = C - ey - ez, B = C - ez, D = C - ey
  t[0] = A, t[3] = A;
  if (inside) t[1] = B, t[2] = pC, t[4] = pC, t[5] = D;
  else t[1] = D, t[2] = pC, t[4] = pC, t[5] = B;
}
#endif
