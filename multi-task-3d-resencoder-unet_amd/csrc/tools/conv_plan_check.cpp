// conv_plan_check.cpp -- runs the routes and planners of ../rx_gather_plan.h and ../rx_wgrad_plan.h (what the conv entry points of
// rx_igemm.hip and rx_wgrad.hip launch by) on the CPU.  Built by tests/test_conv_dispatch_cpu.py with -fsanitize=address,undefined.
//
//   stdin:  one query per line, 29 integers: entry dt | A: n z y x c ld cs lo | B: n z y x c ld cs lo | w_lo k0 k1 k2 s0 s1 s2
//           accumulate ws ws_bytes dw.  entry: 0 conv3d_fwd, 1 conv3d_fwd_stats, 2 conv3d_bwd_data, 3 conv3d_bwd_data_instats,
//           4 convT3d_fwd, 5 convT3d_bwd_data, 6 conv3d_bwd_weight, 7 convT3d_bwd_weight.  A, B: the entry point's two activations in
//           its own argument order (x y / dy dx / x dy), lo = the low four address bits; ws, dw: whether the pointer was passed.
//   stdout: one outcome per line, `key=value` fields separated by single spaces; the message of a refusal comes last
#include <stdio.h>

#include <vector>

#include "../rx_wgrad_plan.h"

static rx_act act(const long long* v) {
  rx_act a = {};
  a.ptr = (void*)(uintptr_t)(4096 + v[7]);      // never dereferenced: the planners read its low bits
  a.n = (int32_t)v[0], a.z = (int32_t)v[1], a.y = (int32_t)v[2], a.x = (int32_t)v[3], a.c = (int32_t)v[4], a.ld = (int32_t)v[5];
  a.cs = v[6];
  return a;
}

// every launch of a gather sequence: the last kernel name (what rx_last_conv_kernel reports), the largest phase / tap / slab
// figures, and whether the phases of the whole sequence write every output voxel exactly once
struct Seq {
  int launches = 0, phases = 0, taps = 0, ks = 0, grid_ok = 1;
  size_t slab_bytes = 0, lds = 0;
  const char* name = "";
  std::vector<unsigned char> hit;
  RxGatherChoice refused = {};
};
static bool seq_add(Seq& q, rx_dtype dt, IgemmGeom& g, const rx_act* in, const rx_act* out, unsigned w_lo, bool ws, size_t ws_bytes) {
  const RxGatherChoice c = rx_gather_choose(dt, g, in->n, ws, ws_bytes, rx_lo4(in->ptr), rx_lo4(out->ptr), w_lo);
  if (c.kind == RX_GA_REFUSE) return q.refused = c, false;
  ++q.launches;
  int taps = 0;
  long vsum = 0;
  for (int i = 0; i < g.nph; ++i) {
    const IgemmPhase& P = g.ph[i];
    taps += P.ntaps, vsum += P.Vq;
    for (int z = 0; z < P.Qz; ++z)
      for (int y = 0; y < P.Qy; ++y)
        for (int x = 0; x < P.Qx; ++x) {
          const long o = ((long)(z * g.osz + P.opz) * g.Yo + (y * g.osy + P.opy)) * g.Xo + (x * g.osx + P.opx);
          if (o < 0 || o >= (long)q.hit.size() || q.hit[o] == 255) return q.grid_ok = 0, true;
          ++q.hit[o];
        }
  }
  q.phases = g.nph > q.phases ? g.nph : q.phases, q.taps = taps > q.taps ? taps : q.taps;
  if (c.kind == RX_GA_NOTHING) return true;
  q.name = c.name, q.ks = c.ks, q.lds = c.lds > q.lds ? c.lds : q.lds;
  const size_t slab = (c.kind == RX_GA_FAT || c.ks > 1) ? (size_t)c.ks * in->n * vsum * g.Co * sizeof(float) : 0;
  q.slab_bytes = slab > q.slab_bytes ? slab : q.slab_bytes;
  if (!c.grid[0] || !c.grid[1] || !c.grid[2] || ((c.kind == RX_GA_FAT || c.ks > 1) && !(c.rgrid[0] && c.rgrid[1]))) q.grid_ok = 0;
  return true;
}

static void print_seq(const Seq& q) {
  if (q.refused.kind == RX_GA_REFUSE) {
    printf("path=refuse code=%d message=%s\n", RX_EUNSUPPORTED, q.refused.message);
    return;
  }
  int once = 1;
  for (unsigned char h : q.hit) once &= h == 1;
  printf("path=gather name=%s ks=%d launches=%d phases=%d taps=%d slab_bytes=%zu lds=%zu grid_ok=%d once=%d\n", q.name, q.ks, q.launches,
         q.phases, q.taps, q.slab_bytes, q.lds, q.grid_ok, once);
}

static void print_wgrad(rx_dtype dt, const rx_act* gt, const rx_act* xt, const int32_t* k, const int32_t* s, bool ws, bool dw, size_t ws_bytes,
                        size_t fn_bytes) {
  WgradGeom g;
  rx_wgrad_geom(g, gt, xt, k, s);
  const RxWgradChoice c = rx_wgrad_choose(dt, g, rx_lo4(gt->ptr), rx_lo4(xt->ptr), ws, dw, ws_bytes);
  if (c.code) {
    printf("path=refuse code=%d message=%s\n", c.code, c.message);
    return;
  }
  const int S = g.ksplit, qps = g.q_per_split;
  rx_wgrad_choose(dt, g, rx_lo4(gt->ptr), rx_lo4(xt->ptr), ws, dw, fn_bytes);
  const int S_fn = g.ksplit;
  rx_wgrad_choose(dt, g, rx_lo4(gt->ptr), rx_lo4(xt->ptr), ws, dw, (size_t)1 << 60);
  printf("path=generic name=%s S=%d S_fn=%d S_unl=%d per=%d NT=%ld taps=%d slab_bytes=%zu lds=%zu grid_ok=%d manysplits=%d\n", c.name, S, S_fn,
         g.ksplit, qps / 64, ((long)g.NQ + 63) / 64, g.ntaps, (size_t)S * g.ntaps * g.R * g.Cc * sizeof(float), c.lds,
         c.grid[0] && c.grid[1] && c.grid[2], rx_wgrad_reduce_manysplits(S, g.ntaps));
}

int main() {
  long long v[29];
  for (;;) {
    int got = 0;
    while (got < 29 && scanf("%lld", &v[got]) == 1) ++got;
    if (got == 0) return 0;
    if (got != 29) return fprintf(stderr, "short query: %d of 29 fields\n", got), 2;
    int entry = (int)v[0];
    const rx_dtype dt = (rx_dtype)v[1];
    const rx_act A = act(v + 2), B = act(v + 10);
    const unsigned w_lo = (unsigned)v[18];
    const int32_t k[3] = {(int32_t)v[19], (int32_t)v[20], (int32_t)v[21]}, s[3] = {(int32_t)v[22], (int32_t)v[23], (int32_t)v[24]};
    const int acc = (int)v[25];
    const bool ws = v[26] != 0, dw = v[28] != 0;
    const size_t wsb = (size_t)v[27];
    if (entry >= 6) {
      const size_t fn = entry == 6 ? rx_conv_bwd_weight_ws_bytes(&A, &B, k) : rx_convT_bwd_weight_ws_bytes(&A, &B, s);
      const RxWgradRoute r = rx_route_bwd_weight(dt, &A, &B, entry == 6 ? k : nullptr, s, ws, dw, wsb);
      if (r.kind == RX_WR_REFUSE) {
        printf("path=refuse code=%d message=%s\n", r.code, r.message);
      } else if (r.kind == RX_WR_HALO) {
        const RxWghChoice &h = r.halo, f = rx_wgh_choose(dt, &A, &B, s, fn), u = rx_wgh_choose(dt, &A, &B, s, (size_t)1 << 60);
        printf("path=halo name=%s S=%d S_fn=%d S_unl=%d per=%d NT=%d taps=27 DMA=%d tile=%dx%dx%d slab_bytes=%zu lds=%zu grid_ok=%d manysplits=%d\n",
               h.name, h.g.S, f.ok ? f.g.S : -1, u.g.S, h.g.tiles_per_split, h.g.NT, h.DMA, h.g.TZ, h.g.TY, h.g.TX,
               h.g.S > 1 ? (size_t)h.g.S * 27 * h.g.R * h.g.Cc * sizeof(float) : 0, h.lds, h.grid[0] && h.grid[1] && h.block,
               rx_wgrad_reduce_manysplits(h.g.S, 27));
      } else if (r.kind == RX_WR_CONVT) {
        const RxCtwChoice &t = r.ctw, f = rx_ctw_choose(dt, &A, &B, s, fn), u = rx_ctw_choose(dt, &A, &B, s, (size_t)1 << 60);
        printf("path=convT name=convT_wgrad_kernel S=%d S_fn=%d S_unl=%d per=%d NT=%d taps=%d slab_bytes=%zu lds=%zu grid_ok=%d manysplits=%d\n", t.S2,
               f.ok ? f.S2 : -1, u.S2, t.g.q_per_split / 64, (t.g.NQ + 63) / 64, t.g.ntaps, (size_t)t.S2 * t.g.ntaps * t.g.R * t.g.Cc * sizeof(float),
               t.lds, t.S2 > 0, rx_wgrad_reduce_manysplits(t.S2, t.g.ntaps));
      } else if (entry == 6) {
        print_wgrad(dt, &B, &A, k, s, ws, dw, wsb, fn);
      } else {
        print_wgrad(dt, &A, &B, nullptr, s, ws, dw, wsb, fn);
      }
      continue;
    }
    RxConvRoute r;
    const rx_act in_y = {B.ptr, B.n, B.z, B.y, B.x, B.c, B.c, 0};      // the saved output of the layer whose gradient dx completes: dense
    if (entry == 1) r = rx_route_conv_stats(dt, &A, w_lo, &B, k, s, 0, nullptr, wsb);
    if (entry == 3) r = rx_route_conv_stats(dt, &A, w_lo, &B, k, s, acc, &in_y, wsb);
    const bool plain = (entry == 1 || entry == 3) && r.kind == RX_RT_PLAIN;
    if (plain) --entry;
    if (entry == 0) r = rx_route_conv(dt, &A, w_lo, &B, k, s, 0, 0);
    if (entry == 2) r = rx_route_conv(dt, &A, w_lo, &B, k, s, 1, acc);
    if (entry == 4) r = rx_route_convT(dt, &A, w_lo, &B, s, true);
    if (entry == 5) r = rx_route_convT(dt, &B, w_lo, &A, s, false);
    if (plain) printf("plain=1 ");
    if (r.kind == RX_RT_REFUSE) {
      printf("path=refuse code=%d message=%s\n", r.code, r.message);
    } else if (r.kind == RX_RT_HALO) {
      const RxChChoice& c = r.halo;
      printf("path=halo name=%s FLIP=%d XDMA=%d STATS=%d ACC=%d BS=%d take_bs=%d stat_chunks=%d lds=%zu grid_ok=%d\n", c.name, c.FLIP, c.XDMA, c.STATS,
             c.ACC, c.BS, c.take_bs, c.stat_chunks, c.lds, c.grid_x && c.grid_y);
    } else if (r.kind == RX_RT_POINTWISE) {
      printf("path=pointwise name=pointwise_kernel lds=%zu grid_ok=%d ntiles=%d\n", r.pw.lds, r.pw.grid[0] && r.pw.grid[1], r.pw.g.ntiles);
    } else if (r.kind == RX_RT_DS2) {
      printf("path=ds2 name=dgrad_s2p_kernel lds=%zu grid_ok=%d per=%d NT=%d wgs=%u\n", r.ds2.lds, r.ds2.grid[0] && r.ds2.grid[1], r.ds2.per, r.ds2.g.NT,
             r.ds2.grid[0]);
    } else {
      Seq q;
      IgemmGeom g;
      q.hit.assign((size_t)rx_act_voxels(&B), 0);      // B is the output of all four gather entry points
      if (entry == 0) {
        rx_gather_fwd(g, &A, &B, k, s);
        seq_add(q, dt, g, &A, &B, w_lo, ws, wsb);
      } else if (entry == 2) {
        for (int cls = 0; rx_gather_bwd_data_next(g, &A, &B, k, s, acc, &cls);)
          if (!seq_add(q, dt, g, &A, &B, w_lo, ws, wsb)) break;
      } else if (entry == 4) {
        for (int pos = 0; rx_gather_convT_fwd_next(g, &A, &B, s, &pos);)
          if (!seq_add(q, dt, g, &A, &B, w_lo, ws, wsb)) break;
      } else {
        rx_gather_convT_bwd_data(g, &A, &B, s, acc);
        seq_add(q, dt, g, &A, &B, w_lo, ws, wsb);
      }
      print_seq(q);
    }
  }
}
