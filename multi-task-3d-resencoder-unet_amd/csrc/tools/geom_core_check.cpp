// geom_core_check.cpp -- runs ../rx_geom_core.h (the check, the lowering and the inverse table that rx_geom_apply, rx_sw_gather_geom and
// rx_sw_accumulate_geom share) on the CPU against the definition of a record in include/rxunet.h:
//   out[o] = in[i(o)],   i[src_axis[d]] = flip[d] ? n_d - 1 - o_d : o_d
// Built by tests/test_geometry_cpu.py with -fsanitize=address,undefined.  Prints one summary line; exit status 1 and a line on
// stderr per expectation that fails.
#include <stdio.h>
#include <string.h>

#include "../rx_geom_core.h"

static int failures = 0;
#define EXPECT(cond, ...)                         \
  do {                                            \
    if (!(cond)) {                                \
      ++failures;                                 \
      fprintf(stderr, "FAILED %s: ", #cond);      \
      fprintf(stderr, __VA_ARGS__);               \
      fprintf(stderr, "\n");                      \
    }                                             \
  } while (0)

static const int PERMS[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};

static rx_geom_sample record(int perm, int flips) {
  rx_geom_sample s = {};
  for (int d = 0; d < 3; ++d) s.src_axis[d] = PERMS[perm][d], s.flip[d] = (flips >> d) & 1, s.ch_src[d] = d;
  return s;
}

// all 48 records over one shape: how many the check accepts; each accepted one against the definition, voxel by voxel
static int sweep(const int ext[3]) {
  int accepted = 0;
  for (int perm = 0; perm < 6; ++perm)
    for (int flips = 0; flips < 8; ++flips) {
      const rx_geom_sample s = record(perm, flips);
      bool keeps = true;
      for (int d = 0; d < 3; ++d) keeps = keeps && ext[s.src_axis[d]] == ext[d];
      const int verdict = rx_geom_check(&s, ext[0], ext[1], ext[2], 0);
      EXPECT((verdict == RX_GEOM_OK) == keeps, "perm %d flips %d over %d x %d x %d: verdict %d", perm, flips, ext[0], ext[1], ext[2], verdict);
      if (verdict >= RX_GEOM_SHAPE) {
        const int d = verdict - RX_GEOM_SHAPE;
        EXPECT(d < 3 && ext[s.src_axis[d]] != ext[d], "perm %d: axis %d is named but keeps its extent", perm, d);
      }
      if (verdict != RX_GEOM_OK) continue;
      ++accepted;
      const RxGeomView v = rx_geom_lower(s, ext[0], ext[1], ext[2]);
      const RxGeomInverse inv = rx_geom_inverse(s);
      EXPECT(v.feeds == inv.from[2] && s.src_axis[v.feeds] == 2, "perm %d: feeds %d", perm, v.feeds);
      for (int oz = 0; oz < ext[0]; ++oz)
        for (int oy = 0; oy < ext[1]; ++oy)
          for (int ox = 0; ox < ext[2]; ++ox) {
            const int o[3] = {oz, oy, ox};
            int i[3] = {-1, -1, -1};
            for (int d = 0; d < 3; ++d) i[s.src_axis[d]] = s.flip[d] ? ext[d] - 1 - o[d] : o[d];
            const int want = (i[0] * ext[1] + i[1]) * ext[2] + i[2];
            const int got = v.base + oz * v.sz + oy * v.sy + ox * v.sx;
            EXPECT(got == want, "perm %d flips %d: o (%d,%d,%d) lowers to %d, the definition says %d", perm, flips, oz, oy, ox, got, want);
            for (int a = 0; a < 3; ++a) {      // the gather's way: per input axis, the output coordinate that feeds it
              const int c = inv.flip[a] ? ext[a] - 1 - o[inv.from[a]] : o[inv.from[a]];
              EXPECT(c == i[a], "perm %d flips %d: o (%d,%d,%d), input axis %d: inverse table %d, definition %d", perm, flips, oz, oy, ox, a, c, i[a]);
            }
          }
    }
  return accepted;
}

int main() {
  const int shapes[3][3] = {{4, 4, 4}, {3, 5, 5}, {3, 4, 5}};
  const int expected[3] = {48, 16, 8};
  int counts[3];
  for (int k = 0; k < 3; ++k) {
    counts[k] = sweep(shapes[k]);
    EXPECT(counts[k] == expected[k], "%d x %d x %d: %d records accepted, %d keep the shape", shapes[k][0], shapes[k][1], shapes[k][2], counts[k], expected[k]);
  }

  // malformed records, at an index other than 0, with the text of each refusal
  rx_geom_sample t[2] = {record(0, 0), record(0, 0)};
  char text[160];
  t[1].src_axis[1] = 0;      // (0, 0, 2)
  int verdict = rx_geom_check(t, 4, 4, 4, 1);
  EXPECT(rx_geom_check(t, 4, 4, 4, 0) == RX_GEOM_OK && verdict == RX_GEOM_BAD_SRC_AXIS, "repeated src_axis entry: verdict %d", verdict);
  rx_geom_refusal(text, sizeof(text), verdict, t, 4, 4, 4, 1, "slot", "patch shape");
  EXPECT(!strcmp(text, "slot 1: src_axis (0, 0, 2) is not a permutation of 0..2"), "%s", text);
  t[1] = record(0, 0), t[1].ch_src[2] = 1;      // (0, 1, 1)
  verdict = rx_geom_check(t, 4, 4, 4, 1);
  EXPECT(verdict == RX_GEOM_BAD_CH_SRC, "repeated ch_src entry: verdict %d", verdict);
  rx_geom_refusal(text, sizeof(text), verdict, t, 4, 4, 4, 1, "sample", "shape");
  EXPECT(!strcmp(text, "sample 1: ch_src (0, 1, 1) is not a permutation of 0..2"), "%s", text);
  t[1] = record(0, 0), t[1].ch_src[0] = 3;
  EXPECT(rx_geom_check(t, 4, 4, 4, 1) == RX_GEOM_BAD_CH_SRC, "ch_src entry out of range");
  t[1].ch_src[0] = -1;
  EXPECT(rx_geom_check(t, 4, 4, 4, 1) == RX_GEOM_BAD_CH_SRC, "negative ch_src entry");
  t[1] = record(0, 0), t[1].src_axis[0] = 7;
  EXPECT(rx_geom_check(t, 4, 4, 4, 1) == RX_GEOM_BAD_SRC_AXIS, "src_axis entry out of range");
  t[1] = record(1, 0);      // (0, 2, 1) over 8 x 8 x 12: y would read x
  verdict = rx_geom_check(t, 8, 8, 12, 1);
  EXPECT(verdict == RX_GEOM_SHAPE + 1, "shape-changing permutation: verdict %d", verdict);
  rx_geom_refusal(text, sizeof(text), verdict, t, 8, 8, 12, 1, "slot", "patch shape");
  EXPECT(!strcmp(text, "slot 1: output axis 1 reads input axis 2, which would change the patch shape (8 x 8 x 12)"), "%s", text);
  rx_geom_refusal(text, sizeof(text), verdict, t, 8, 8, 12, 1, "sample", "shape");
  EXPECT(!strcmp(text, "sample 1: output axis 1 reads input axis 2, which would change the shape (8 x 8 x 12)"), "%s", text);

  // channels and signs of a record with mixed ch_neg
  rx_geom_sample m = record(2, 5);
  m.ch_src[0] = 1, m.ch_src[1] = 0, m.ch_src[2] = 2;
  m.ch_neg[0] = 1, m.ch_neg[1] = 0, m.ch_neg[2] = 7;      // any non-zero value negates
  EXPECT(rx_geom_check(&m, 4, 4, 4, 0) == RX_GEOM_OK, "mixed record refused");
  const RxGeomView mv = rx_geom_lower(m, 4, 4, 4);
  EXPECT(mv.ch[0] == 1 && mv.ch[1] == 0 && mv.ch[2] == 2 && mv.neg == 5u, "ch (%d, %d, %d) neg %u", mv.ch[0], mv.ch[1], mv.ch[2], mv.neg);
  const RxGeomView iv = rx_geom_lower(record(0, 0), 3, 4, 5);
  EXPECT(iv.base == 0 && iv.sz == 20 && iv.sy == 5 && iv.sx == 1 && iv.neg == 0u && iv.feeds == 2, "identity lowers to %d + (%d, %d, %d)", iv.base, iv.sz, iv.sy, iv.sx);

  printf("accepted %d %d %d of 48, %d expectations failed\n", counts[0], counts[1], counts[2], failures);
  return failures ? 1 : 0;
}
