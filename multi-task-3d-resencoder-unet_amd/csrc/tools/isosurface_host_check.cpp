// isosurface_host_check.cpp -- runs csrc/rx_isosurface_core.h, the per-cell and per-edge arithmetic of rx_isosurface.hip, serially on the
// host: every cell row classified chunk by chunk from the inside words of its four voxel rows (iso_chunk_flags), the row counts
// scanned, every row emitted (iso_vertex, iso_quad, ids from the popcounts of the active words) -- the three passes of the kernels,
// with plain arrays where they have LDS.  The rows of the classify and the emit pass are visited in raster order, in reverse and
// in a shuffled order: the arrays must be the same each time and equal to a direct restatement of surface nets written here, cell
// by cell with a table of vertex ids.  Build with
//     g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all isosurface_host_check.cpp
// so that an index outside a row's words, the offsets or the outputs is an error, not a wrong mesh.
// The cases restate tests/isosurface_cases.py: the same shapes, levels and kinds of volume (the random ones from this program's
// own generator).
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../rx_isosurface_core.h"
#include "check_util.h"

struct Shape { int z, y, x; };
static const Shape SHAPES[] = {{1, 1, 1}, {1, 1, 70}, {1, 70, 1}, {5, 1, 3}, {9, 10, 12}, {33, 17, 70}, {3, 130, 5}, {130, 3, 5}, {2, 3, 257}, {40, 40, 130}};
static const int LEVELS[] = {0, 127, 254};



struct Mesh {
  std::vector<float> v;        // 3 per vertex: x, y, z
  std::vector<int64_t> t;      // 3 per triangle
};

struct Vol {
  const std::vector<uint8_t>& d;
  Shape s;
  int at(int z, int y, int x) const {      // 0 outside: the padding
    if (z < 0 || z >= s.z || y < 0 || y >= s.y || x < 0 || x >= s.x) return 0;
    return d.at(((size_t)z * s.y + y) * s.x + x);
  }
};

// ---- the three passes, through the core header ------------------------------------------------------------------------------------------
static uint64_t inside_word(const Vol& v, int level, int z, int y, int i0) {
  uint64_t w = 0;
  for (int l = 0; l < 64; ++l)
    if (v.at(z, y, i0 + l) > level) w |= 1ull << l;
  return w;
}

static Mesh mesh_core(const Vol& v, int level, int how) {
  const int CZ = v.s.z + 1, CY = v.s.y + 1, CX = v.s.x + 1, W = (CX + 63) / 64;
  const long rows = (long)CZ * CY;
  std::vector<uint64_t> bits((size_t)rows * W, 0xdeadbeefull);
  std::vector<int> counts((size_t)rows * 2, -1);
  std::vector<long> idx;
  for (long r = 0; r < rows; ++r) idx.push_back(r);
  order(idx, how);
  for (long row : idx) {      // classify
    const int k = (int)(row / CY), j = (int)(row % CY);
    int nact = 0, nquad = 0;
    for (int ch = 0; ch < W; ++ch) {
      uint64_t b[4], act, qz, qy, qx;
      unsigned halo = 0;
      for (int q = 0; q < 4; ++q) {
        b[q] = inside_word(v, level, k - 1 + (q >> 1), j - 1 + (q & 1), ch * 64);
        halo |= (unsigned)(v.at(k - 1 + (q >> 1), j - 1 + (q & 1), ch * 64 - 1) > level) << q;
      }
      iso_chunk_flags(b, halo, &act, &qz, &qy, &qx);
      bits.at((size_t)row * W + ch) = act;
      nact += iso_popc(act), nquad += iso_popc(qz) + iso_popc(qy) + iso_popc(qx);
    }
    counts.at(row * 2) = nact, counts.at(row * 2 + 1) = nquad;
  }
  std::vector<int64_t> offs((size_t)rows * 2);      // scan
  int64_t nv = 0, nq = 0;
  for (long r = 0; r < rows; ++r) offs[r * 2] = nv, offs[r * 2 + 1] = nq, nv += counts[r * 2], nq += counts[r * 2 + 1];
  Mesh m;
  m.v.assign((size_t)nv * 3, NAN);
  m.t.assign((size_t)nq * 6, -1);
  auto id_at = [&](long row, int ch, int lane) -> int64_t {      // offset + active cells of the row before column 64 ch + lane
    if (row < 0) return -1;                                      // a neighbour row outside the grid: never used
    int64_t p = offs.at(row * 2);
    for (int c = 0; c < ch; ++c) p += iso_popc(bits.at((size_t)row * W + c));
    return p + iso_prefix(bits.at((size_t)row * W + ch), lane);
  };
  order(idx, how);
  for (long row : idx) {      // emit
    const int k = (int)(row / CY), j = (int)(row % CY);
    int64_t qrun = offs.at(row * 2 + 1);
    for (int ch = 0; ch < W; ++ch) {
      const uint64_t word = bits.at((size_t)row * W + ch);
      for (int lane = 0; lane < 64; ++lane) {
        if (!((word >> lane) & 1ull)) continue;
        const int i = ch * 64 + lane;
        uint8_t c[8];
        for (int q = 0; q < 8; ++q) c[q] = (uint8_t)v.at(k - 1 + (q >> 2), j - 1 + ((q >> 1) & 1), i - 1 + (q & 1));
        const int64_t pC = id_at(row, ch, lane);
        iso_vertex(c, level, k - 1, j - 1, i - 1, &m.v.at((size_t)pC * 3));
        const bool in0 = c[0] > level;
        const bool cross[3] = {(c[4] > level) != in0, (c[2] > level) != in0, (c[1] > level) != in0};
        if (!(cross[0] || cross[1] || cross[2])) continue;
        const int64_t pJ = id_at(j > 0 ? row - 1 : -1, ch, lane), pK = id_at(k > 0 ? row - CY : -1, ch, lane);
        const int64_t pKJ = id_at(k > 0 && j > 0 ? row - CY - 1 : -1, ch, lane);
        for (int slot = 0; slot < 3; ++slot)
          if (cross[slot]) iso_quad(slot, in0, pC, pJ, pK, pKJ, &m.t.at((size_t)qrun * 6)), ++qrun;
      }
    }
    if (qrun != offs.at(row * 2 + 1) + counts.at(row * 2 + 1)) printf("ROW %ld: emitted quads differ from the classified count\n", row), m.t.push_back(-9);
  }
  return m;
}

// ---- the direct restatement: surface nets cell by cell, with a table of vertex ids ----------------------------------------------------------
static Mesh mesh_direct(const Vol& v, int level) {
  const int CZ = v.s.z + 1, CY = v.s.y + 1, CX = v.s.x + 1;
  std::vector<int64_t> vid((size_t)CZ * CY * CX, -1);
  auto cell = [&](int k, int j, int i) -> int64_t& { return vid.at(((size_t)k * CY + j) * CX + i); };
  Mesh m;
  const float iso = (float)(level + 0.5);
  for (int k = 0; k < CZ; ++k)
    for (int j = 0; j < CY; ++j)
      for (int i = 0; i < CX; ++i) {
        int nin = 0;
        for (int q = 0; q < 8; ++q) nin += v.at(k - 1 + (q >> 2), j - 1 + ((q >> 1) & 1), i - 1 + (q & 1)) > level;
        if (nin == 0 || nin == 8) continue;
        cell(k, j, i) = (int64_t)(m.v.size() / 3);
        float sum[3] = {0, 0, 0}, n = 0;      // indexed z, y, x
        for (int d = 0; d < 3; ++d)
          for (int o0 = 0; o0 < 2; ++o0)
            for (int o1 = 0; o1 < 2; ++o1) {
              int a[3], b[3], o[2] = {o0, o1}, w = 0;
              for (int ax = 0; ax < 3; ++ax) a[ax] = ax == d ? 0 : o[w++];
              memcpy(b, a, sizeof a);
              b[d] = 1;
              const int va = v.at(k - 1 + a[0], j - 1 + a[1], i - 1 + a[2]), vb = v.at(k - 1 + b[0], j - 1 + b[1], i - 1 + b[2]);
              if ((va > level) == (vb > level)) continue;
              const float t = (iso - (float)va) / ((float)vb - (float)va);
              for (int ax = 0; ax < 3; ++ax) sum[ax] = sum[ax] + (ax == d ? t : (float)a[ax]);
              n = n + 1.0f;
            }
        m.v.push_back((float)(i - 1) + sum[2] / n);
        m.v.push_back((float)(j - 1) + sum[1] / n);
        m.v.push_back((float)(k - 1) + sum[0] / n);
      }
  const int cyc[3][2] = {{2, 1}, {0, 2}, {1, 0}};      // edge axis (0 z, 1 y, 2 x) -> (u, v): z -> (x, y), y -> (z, x), x -> (y, z)
  for (int k = 0; k < CZ; ++k)
    for (int j = 0; j < CY; ++j)
      for (int i = 0; i < CX; ++i)
        for (int d = 0; d < 3; ++d) {
          int p[3] = {k, j, i}, e[3] = {0, 0, 0};
          e[d] = 1;
          const bool lo = v.at(k - 1, j - 1, i - 1) > level, hi = v.at(k - 1 + e[0], j - 1 + e[1], i - 1 + e[2]) > level;
          if (lo == hi) continue;
          auto at = [&](int du, int dv) -> int64_t {
            int q[3] = {p[0], p[1], p[2]};
            q[cyc[d][0]] += du, q[cyc[d][1]] += dv;
            return cell(q[0], q[1], q[2]);
          };
          const int64_t A = at(-1, -1), B = at(0, -1), C = at(0, 0), D = at(-1, 0);
          if (A < 0 || B < 0 || C < 0 || D < 0) printf("a cell around a crossing edge is not active\n");
          const int64_t t[6] = {A, lo ? B : D, C, A, C, lo ? D : B};
          m.t.insert(m.t.end(), t, t + 6);
        }
  return m;
}

// ---- the volumes of tests/isosurface_cases.py ----------------------------------------------------------------------------------------------
struct Case { std::string name; std::vector<uint8_t> d; };

static std::vector<Case> cases_of(Shape s, int level) {
  const long XY = (long)s.y * s.x, V = s.z * XY;
  std::vector<Case> out;
  out.push_back({"zero", std::vector<uint8_t>(V, 0)});
  out.push_back({"full", std::vector<uint8_t>(V, 255)});
  { std::vector<uint8_t> d(V);
    for (long i = 0; i < V; ++i) d[i] = ((i / XY + i % XY / s.x + i % s.x) & 1) == 0 ? 255 : 0;
    out.push_back({"checkerboard", d}); }
  for (int pc : {10, 50, 90}) {
    std::vector<uint8_t> d(V);
    for (auto& b : d) b = (uint8_t)(rnd() % 100 < (uint32_t)pc ? level + 1 + rnd() % (255 - level) : rnd() % (level + 1));
    out.push_back({"random" + std::to_string(pc), d});
  }
  { std::vector<uint8_t> d(V);
    const double R = 0.4 * std::min(s.z, std::min(s.y, s.x)), c[3] = {(s.z - 1) / 2.0 + 0.2, (s.y - 1) / 2.0 + 0.2, (s.x - 1) / 2.0 + 0.2};
    for (long i = 0; i < V; ++i) {
      const double dz = i / XY - c[0], dy = i % XY / s.x - c[1], dx = i % s.x - c[2];
      d[i] = (uint8_t)std::min(255.0, std::max(0.0, nearbyint(127.5 + 32 * (R - sqrt(dz * dz + dy * dy + dx * dx)))));
    }
    out.push_back({"ball", d}); }
  { std::vector<uint8_t> d(V, 0);
    for (long i = 0; i < V; ++i) {
      const int z = (int)(i / XY), y = (int)(i % XY / s.x), x = (int)(i % s.x);
      if (y >= s.y / 2 && y < s.y / 2 + 2) d[i] = 200;
      if (z == s.z / 2) d[i] = 255;
      if (x == s.x / 2) d[i] = 129;
    }
    out.push_back({"slab", d}); }
  return out;
}

int main() {
  long ncases = 0, bad = 0;
  for (const Shape& s : SHAPES)
    for (int level : LEVELS)
      for (const Case& c : cases_of(s, level)) {
        const Vol v{c.d, s};
        const Mesh want = mesh_direct(v, level);
        for (int how = 0; how < 3; ++how) {
          const Mesh got = mesh_core(v, level, how);
          ++ncases;
          const bool same = got.t == want.t && got.v.size() == want.v.size() &&
                            same_bits(got.v, want.v);
          if (!same) {
            ++bad;
            printf("DIFFER %dx%dx%d %s level %d order %d: %zu / %zu vertices, %zu / %zu triangles\n", s.z, s.y, s.x, c.name.c_str(), level, how,
                   got.v.size() / 3, want.v.size() / 3, got.t.size() / 3, want.t.size() / 3);
          }
        }
      }
  printf("%ld cases, %ld differ from the direct restatement\n", ncases, bad);
  return bad ? 1 : 0;
}
