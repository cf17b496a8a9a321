// rx_geom_core.h -- one `rx_geom_sample` (a flip / 90-degree rotation record, include/rxunet.h), checked and lowered once for
// everything that runs one: rx_geom_apply (rx_geometry.hip) and the test-time-augmentation forms of streaming inference
// (rx_sw_gather_geom / rx_sw_accumulate_geom, rx_infer.hip).  The record is the gather form
//   out[o] = in[i(o)],   i[src_axis[d]] = flip[d] ? n_d - 1 - o_d : o_d   (d = 0, 1, 2 = z, y, x)
// No HIP in here: tools/geom_core_check.cpp runs every function below on the CPU over all 48 signed axis permutations.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/rxunet.h"

// the verdict on one record; a shape-changing output axis d answers RX_GEOM_SHAPE + d
enum { RX_GEOM_OK = 0, RX_GEOM_BAD_SRC_AXIS = 1, RX_GEOM_BAD_CH_SRC = 2, RX_GEOM_SHAPE = 3 };

inline bool rx_geom_is_perm(const int32_t* p) {
  unsigned seen = 0;
  for (int i = 0; i < 3; ++i) {
    if (p[i] < 0 || p[i] > 2) return false;
    seen |= 1u << p[i];
  }
  return seen == 7u;
}

// record i of a table over extents (z, y, x): permutations, and none that would change the shape
inline int rx_geom_check(const rx_geom_sample* table, int z, int y, int x, int i) {
  const rx_geom_sample& s = table[i];
  if (!rx_geom_is_perm(s.src_axis)) return RX_GEOM_BAD_SRC_AXIS;
  if (!rx_geom_is_perm(s.ch_src)) return RX_GEOM_BAD_CH_SRC;
  const int ext[3] = {z, y, x};
  for (int d = 0; d < 3; ++d)
    if (ext[s.src_axis[d]] != ext[d]) return RX_GEOM_SHAPE + d;
  return RX_GEOM_OK;
}

// the text of a refusal, to follow the entry point's name: `noun` is what the caller calls a record ("sample", "slot"), `what` what
// it calls the extents ("shape", "patch shape")
inline void rx_geom_refusal(char* buf, size_t n, int verdict, const rx_geom_sample* table, int z, int y, int x, int i, const char* noun,
                            const char* what) {
  const rx_geom_sample& s = table[i];
  if (verdict >= RX_GEOM_SHAPE)
    snprintf(buf, n, "%s %d: output axis %d reads input axis %d, which would change the %s (%d x %d x %d)", noun, i, verdict - RX_GEOM_SHAPE,
             s.src_axis[verdict - RX_GEOM_SHAPE], what, z, y, x);
  else {
    const int32_t* p = verdict == RX_GEOM_BAD_SRC_AXIS ? s.src_axis : s.ch_src;
    snprintf(buf, n, "%s %d: %s (%d, %d, %d) is not a permutation of 0..2", noun, i, verdict == RX_GEOM_BAD_SRC_AXIS ? "src_axis" : "ch_src", p[0],
             p[1], p[2]);
  }
}

// the record turned round per INPUT axis a (z, y, x): it takes the output coordinate of axis from[a], mirrored where flip[a]
struct RxGeomInverse {
  uint8_t from[3], flip[3];
};
inline RxGeomInverse rx_geom_inverse(const rx_geom_sample& s) {
  RxGeomInverse r = {};
  for (int d = 0; d < 3; ++d) {
    const int a = s.src_axis[d];
    r.from[a] = (uint8_t)d, r.flip[a] = s.flip[d] ? 1 : 0;
  }
  return r;
}

// a checked record as the kernels index with it, in element units of ONE contiguous (z, y, x) channel volume: output voxel o reads
// base + oz * sz + oy * sy + ox * sx; output channel c of a vector tensor reads channel ch[c], its sign bit flipped where bit c of neg
struct RxGeomView {
  int32_t base, sz, sy, sx;
  int32_t ch[3];
  uint32_t neg;
  int32_t feeds;            // the output axis input x feeds: 2 = x stays innermost, 0 or 1 = x moves
};
inline RxGeomView rx_geom_lower(const rx_geom_sample& s, int z, int y, int x) {
  const int ext[3] = {z, y, x};
  const int stride[3] = {y * x, x, 1};
  RxGeomView v = {};
  int32_t sd[3];
  for (int ax = 0; ax < 3; ++ax) {
    const int st_in = stride[s.src_axis[ax]];
    sd[ax] = s.flip[ax] ? -st_in : st_in;
    if (s.flip[ax]) v.base += (ext[ax] - 1) * st_in;
  }
  v.sz = sd[0], v.sy = sd[1], v.sx = sd[2];
  for (int k = 0; k < 3; ++k) {
    v.ch[k] = s.ch_src[k];
    if (s.ch_neg[k]) v.neg |= 1u << k;
  }
  v.feeds = rx_geom_inverse(s).from[2];
  return v;
}
