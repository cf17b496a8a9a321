// check_util.h -- what the stand-alone host-check programs of this directory share: one seeded generator (every program starts
// from the same state, so its case list and its printed counts are the same from run to run), the three visiting orders a pass is
// run in, and the comparison of floats by their bits.
#pragma once
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

static uint64_t g_rng = 0x9e3779b97f4a7c15ull;
static inline uint32_t rnd() {
  g_rng = g_rng * 6364136223846793005ull + 1442695040888963407ull;
  return (uint32_t)(g_rng >> 33);
}
static inline float rndf() { return (float)(rnd() % 20001) / 100.0f - 100.0f; }      // -100 .. 100 in steps of 0.01

template <typename I>
static inline void order(std::vector<I>& idx, int how) {      // 0 raster, 1 reverse, 2 shuffled
  if (how == 1) std::reverse(idx.begin(), idx.end());
  if (how == 2)
    for (size_t i = idx.size(); i > 1; --i) std::swap(idx[i - 1], idx[rnd() % i]);
}

static inline bool same_bits(float a, float b) { return memcmp(&a, &b, 4) == 0; }
static inline bool same_bits(const std::vector<float>& a, const std::vector<float>& b) {
  return a.size() == b.size() && (a.empty() || memcmp(a.data(), b.data(), a.size() * sizeof(float)) == 0);
}
