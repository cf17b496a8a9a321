// conv_halo_plan_check.cpp -- runs rx_ch_choose (../rx_conv_halo_plan.h, the function rx_conv_halo_launch launches by) on the CPU.
// Built by tests/test_conv_halo_plan_cpu.py with -fsanitize=address,undefined.
//
//   stdin:  one query per line, 21 integers: dt N Z Y X Ci Co ldi ldo in_cs out_cs in_lo out_lo w_lo bsy_lo bs_ldy flip accumulate
//           stat_offered stat_bytes want_bs
//   stdout: one choice per line, `key=value` fields separated by single spaces; the message of a refusal comes last
#include <stdio.h>

#include "../rx_conv_halo_plan.h"

int main() {
  long long v[21];
  for (;;) {
    int got = 0;
    while (got < 21 && scanf("%lld", &v[got]) == 1) ++got;
    if (got == 0) return 0;
    if (got != 21) return fprintf(stderr, "short query: %d of 21 fields\n", got), 2;
    RxChQuery q = {};
    q.dt = (rx_dtype)v[0];
    q.N = (int)v[1], q.Z = (int)v[2], q.Y = (int)v[3], q.X = (int)v[4];
    q.Ci = (int)v[5], q.Co = (int)v[6], q.ldi = (int)v[7], q.ldo = (int)v[8];
    q.in_cs = (long)v[9], q.out_cs = (long)v[10];
    q.in_lo = (unsigned)v[11], q.out_lo = (unsigned)v[12], q.w_lo = (unsigned)v[13], q.bsy_lo = (unsigned)v[14];
    q.bs_ldy = (int)v[15], q.flip = (int)v[16], q.accumulate = (int)v[17];
    q.stat_offered = v[18] != 0, q.stat_bytes = (size_t)v[19], q.want_bs = v[20] != 0;
    const RxChChoice c = rx_ch_choose(q);
    if (c.kind == RX_CH_FALLTHROUGH) {
      printf("kind=fallthrough\n");
    } else if (c.kind == RX_CH_REFUSE) {
      printf("kind=refuse code=%d message=%s\n", RX_EUNSUPPORTED, c.message);
    } else {
      printf("kind=launch name=%s family=%d FLIP=%d XDMA=%d STATS=%d ACC=%d BS=%d tile=%dx%dx%d order=%d NT=%d grid_x=%u grid_y=%u block=%u "
             "lds=%zu per=%d wgs_s=%d take_stats=%d take_bs=%d stat_chunks=%d\n",
             c.name, (int)c.family, c.FLIP, c.XDMA, c.STATS, c.ACC, c.BS, c.TZ, c.TY, c.TX, c.order, c.NT, c.grid_x, c.grid_y, c.block,
             c.lds, c.per, c.wgs_s, c.take_stats, c.take_bs, c.stat_chunks);
    }
  }
}
