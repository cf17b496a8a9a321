// rx_meshdecimate_core.h -- the per-vertex, per-cluster and per-triangle work of mesh decimation by vertex clustering
// (rx_meshdecimate.hip), written so that it compiles for the host as well: csrc/tools/meshdecimate_host_check.cpp runs exactly these
// functions serially against a direct restatement, under the address and undefined-behaviour sanitizers.  postprocess/decimate.py
// (decimate_numpy) is the statement; every float32 operation here is one rounding (contraction is off, denormals are kept, / is
// correctly rounded: IEEE on the host, hipcc's default on the device).
//
// The hash table: `capacity` slots, a power of two above the number of vertices, so it never fills.  Slot s holds a cell key in
// table_keys[s] (MD_EMPTY until claimed) and the smallest vertex id that carries the key in table_min[s].  Which slot a key gets
// depends on arrival; the key and the smallest id do not, and every later number comes from those two.
#ifndef RX_MESHDECIMATE_CORE_H
#define RX_MESHDECIMATE_CORE_H
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "rx_meshrefine_core.h"

#pragma clang fp contract(off)

#define MD_KEY_RANGE 1048576      // 2^20: a cell index k has |k| < 2^20 per component
#define MD_EMPTY (-1LL)           // a key is below 2^63
#define MD_NO_MIN 0xffffffffu      // above every vertex id; the smallest ids are held unsigned

// the cell key of position p; false when a cell index is outside (-2^20, 2^20) (an infinity from a tiny cell included)
RX_MR_HD bool md_key(const float p[3], float cell, int64_t* key) {
  int64_t k[3];
  for (int c = 0; c < 3; ++c) {
    const float q = p[c] / cell;
    const float f = floorf(q);
    if (!(fabsf(f) < (float)MD_KEY_RANGE)) return false;      // a NaN compares false
    k[c] = (int64_t)f + MD_KEY_RANGE;
  }
  *key = (k[0] << 42) | (k[1] << 21) | k[2];
  return true;
}

RX_MR_HD int64_t md_hash(int64_t key, int64_t mask) {
  uint64_t x = (uint64_t)key;
  x ^= x >> 33;
  x *= 0xff51afd7ed558ccdULL;
  x ^= x >> 33;
  x *= 0xc4ceb9fe1a85ec53ULL;
  x ^= x >> 33;
  return (int64_t)(x & (uint64_t)mask);
}

// Vertex v with cell key `key` finds or claims the key's slot by linear probing and lowers the slot's smallest id to v -> the slot,
// or -1 after `capacity` probes without one (a table that was not cleared, or is not of this mesh).  On the device the claim is a
// 64-bit compare-and-swap and the minimum an integer atomic; on the host the same steps are plain.
RX_MR_HD int32_t md_insert(int64_t key, int32_t v, int64_t capacity, int64_t* table_keys, uint32_t* table_min) {
  const int64_t mask = capacity - 1;
  int64_t s = md_hash(key, mask);
  for (int64_t probe = 0; probe < capacity; ++probe, s = (s + 1) & mask) {
#if defined(__HIP_DEVICE_COMPILE__)
    long long seen = __hip_atomic_load((long long*)&table_keys[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (seen == MD_EMPTY)
      seen = (long long)atomicCAS((unsigned long long*)&table_keys[s], (unsigned long long)MD_EMPTY, (unsigned long long)key);
    if (seen == MD_EMPTY || seen == key) {
      atomicMin(&table_min[s], (uint32_t)v);
      return (int32_t)s;
    }
#else
    if (table_keys[s] == MD_EMPTY) table_keys[s] = key;
    if (table_keys[s] == key) {
      if ((uint32_t)v < table_min[s]) table_min[s] = (uint32_t)v;
      return (int32_t)s;
    }
#endif
  }
  return -1;
}

// the smallest member id of vertex v's cluster, or -1 where the vertex has no slot
RX_MR_HD int32_t md_smallest(int32_t slot, int64_t capacity, const uint32_t* table_min, int64_t V) {
  if (slot < 0 || slot >= capacity) return -1;
  const uint32_t m = table_min[slot];
  return (int64_t)m < V ? (int32_t)m : -1;
}

// "mean": the members of one cluster, sorted ascending in place, summed in that order from 0 and divided by float(n)
RX_MR_HD void md_mean(int32_t* members, int64_t n, const float* pos, int64_t V, float out[3]) {
  mr_heapsort(members, n);
  float s[3] = {0.0f, 0.0f, 0.0f};
  for (int64_t i = 0; i < n; ++i) {
    const int64_t m = members[i];
    if ((uint64_t)m >= (uint64_t)V) continue;
    s[0] = s[0] + pos[3 * m], s[1] = s[1] + pos[3 * m + 1], s[2] = s[2] + pos[3 * m + 2];
  }
  const float d = (float)n;
  out[0] = s[0] / d, out[1] = s[1] / d, out[2] = s[2] / d;
}

// "nearest": (bits of d) << 32 | v with d the squared distance of p to the centre of its cell; d >= 0, so its bits order as integers
RX_MR_HD uint64_t md_nearest_pack(const float p[3], int64_t key, float cell, int32_t v) {
  float d = 0.0f;
  for (int c = 0; c < 3; ++c) {
    const int64_t k = ((key >> (21 * (2 - c))) & 0x1fffff) - MD_KEY_RANGE;
    const float h = (float)k + 0.5f;
    const float centre = h * cell;
    const float dx = p[c] - centre;
    const float sq = dx * dx;
    d = c == 0 ? sq : d + sq;
  }
  uint32_t bits;
  memcpy(&bits, &d, 4);
  return ((uint64_t)bits << 32) | (uint32_t)v;
}

// the clusters of triangle t's corners -> true when the ids name vertices and the three clusters differ; lo < mid < hi are they sorted
RX_MR_HD bool md_remap(const int64_t t[3], int64_t V, const int64_t* cluster_of, int64_t C, int64_t c[3], int32_t* lo, int32_t* mid, int32_t* hi) {
  if (!mr_triangle_ok(t, V)) return false;
  c[0] = cluster_of[t[0]], c[1] = cluster_of[t[1]], c[2] = cluster_of[t[2]];
  if ((uint64_t)c[0] >= (uint64_t)C || (uint64_t)c[1] >= (uint64_t)C || (uint64_t)c[2] >= (uint64_t)C) return false;
  if (c[0] == c[1] || c[1] == c[2] || c[0] == c[2]) return false;
  const int64_t a = c[0] < c[1] ? c[0] : c[1], b = c[0] < c[1] ? c[1] : c[0];
  *lo = (int32_t)(a < c[2] ? a : c[2]);
  *hi = (int32_t)(b > c[2] ? b : c[2]);
  *mid = (int32_t)(c[0] + c[1] + c[2] - *lo - *hi);
  return true;
}

// entries are (middle, largest, triangle) triples of int32, compared in that order
RX_MR_HD bool md_less3(const int32_t* a, const int32_t* b) {
  if (a[0] != b[0]) return a[0] < b[0];
  if (a[1] != b[1]) return a[1] < b[1];
  return a[2] < b[2];
}

RX_MR_HD void md_sift3(int32_t* a, int64_t root, int64_t n) {
  const int32_t x[3] = {a[3 * root], a[3 * root + 1], a[3 * root + 2]};
  int64_t i = root;
  for (;;) {
    int64_t c = 2 * i + 1;
    if (c >= n) break;
    if (c + 1 < n && md_less3(a + 3 * c, a + 3 * (c + 1))) ++c;
    if (!md_less3(x, a + 3 * c)) break;
    a[3 * i] = a[3 * c], a[3 * i + 1] = a[3 * c + 1], a[3 * i + 2] = a[3 * c + 2];
    i = c;
  }
  a[3 * i] = x[0], a[3 * i + 1] = x[1], a[3 * i + 2] = x[2];
}

// The n entries of one cluster (the triangles whose smallest cluster it is), heap-sorted ascending in place; then keep[triangle] = 1
// for every entry that does not repeat the (middle, largest) of the one before it: the lowest triangle index of each unordered triple.
RX_MR_HD void md_unique(int32_t* entries, int64_t n, int64_t T, int32_t* keep) {
  for (int64_t r = n / 2 - 1; r >= 0; --r) md_sift3(entries, r, n);
  for (int64_t m = n - 1; m > 0; --m) {
    for (int k = 0; k < 3; ++k) {
      const int32_t top = entries[k];
      entries[k] = entries[3 * m + k];
      entries[3 * m + k] = top;
    }
    md_sift3(entries, 0, m);
  }
  for (int64_t i = 0; i < n; ++i) {
    const int32_t* e = entries + 3 * i;
    if ((uint64_t)e[2] >= (uint64_t)T) continue;
    if (i == 0 || e[0] != e[-3] || e[1] != e[-2]) keep[e[2]] = 1;
  }
}
#endif
