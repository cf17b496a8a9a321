// components_host_check.cpp -- runs csrc/rx_components_core.h, the find / union / tile-merge logic of rx_components.hip, serially on
// the host: every tile seeded from its row masks and merged (cc_tile_voxel), every tile face joined (cc_seam_voxel), every label
// flattened (cc_flatten_voxel), exactly the three passes of rx_cc_label, with plain arrays where the kernels have LDS and the label
// volume.  The voxels of each pass are visited in raster order, in reverse and in a shuffled order: the labels must be the same
// each time (1 + the component's smallest linear index) and equal to a breadth-first search written here.  Build with
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all components_host_check.cpp -o components_host_check
// so that an index outside a tile's forest, its masks or the volume is an error, not a wrong label.
// The cases restate tests/components_cases.py: the same shapes and the same kinds of mask (the random ones from this program's own
// generator).
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <queue>
#include <string>
#include <vector>

#include "../rx_components_core.h"
#include "check_util.h"

struct Shape { int z, y, x; };
static const Shape SHAPES[] = {{1, 1, 1}, {1, 1, 70}, {1, 70, 1}, {5, 1, 3}, {9, 10, 12}, {33, 17, 70}, {3, 130, 5}, {130, 3, 5}, {2, 3, 257}, {40, 40, 130}};


struct TileForest {      // a tile's forest: what the kernel keeps in LDS
  std::vector<int> p;
  int parent(int i) { return p.at(i); }
  int parent_min(int i, int v) { const int old = p.at(i); p.at(i) = std::min(old, v); return old; }
};

struct VolForest {      // the label volume: label = parent + 1
  std::vector<int>& l;
  int label(int i) { return l.at(i); }
  int parent(int i) { return l.at(i) - 1; }
  int parent_min(int i, int v) { const int old = l.at(i); l.at(i) = std::min(old, v + 1); return old - 1; }
  void set_parent(int i, int v) { l.at(i) = v + 1; }
};


static std::vector<int> label_core(const std::vector<uint8_t>& m, Shape s, int conn, int how) {
  const int Z = s.z, Y = s.y, X = s.x, steps = cc_max_steps(conn);
  const long XY = (long)Y * X;
  std::vector<int> labels((size_t)Z * XY, -7);
  const int ntx = (X + RX_CC_TX - 1) / RX_CC_TX, nty = (Y + RX_CC_TY - 1) / RX_CC_TY, ntz = (Z + RX_CC_TZ - 1) / RX_CC_TZ;
  for (int tiz = 0; tiz < ntz; ++tiz)
    for (int tiy = 0; tiy < nty; ++tiy)
      for (int tix = 0; tix < ntx; ++tix) {
        const int z0 = tiz * RX_CC_TZ, y0 = tiy * RX_CC_TY, x0 = tix * RX_CC_TX;
        std::vector<uint64_t> masks(RX_CC_ROWS, 0);
        TileForest lds{std::vector<int>(RX_CC_TILE, -1)};
        for (int row = 0; row < RX_CC_ROWS; ++row) {
          const int z = z0 + row / RX_CC_TY, y = y0 + row % RX_CC_TY;
          for (int t = 0; t < RX_CC_TX; ++t)
            if (z < Z && y < Y && x0 + t < X && m[z * XY + (long)y * X + x0 + t]) masks[row] |= 1ull << t;
          for (int t = 0; t < RX_CC_TX; ++t)
            if ((masks[row] >> t) & 1ull) lds.p[row * RX_CC_TX + t] = row * RX_CC_TX + cc_run_start(masks[row], t);
        }
        std::vector<long> idx;
        for (long l = 0; l < RX_CC_TILE; ++l)
          if ((masks[l / RX_CC_TX] >> (l % RX_CC_TX)) & 1ull) idx.push_back(l);
        order(idx, how);
        for (long l : idx) cc_tile_voxel(lds, masks.data(), (int)(l / RX_CC_TX) / RX_CC_TY, (int)(l / RX_CC_TX) % RX_CC_TY, (int)(l % RX_CC_TX), steps);
        for (int row = 0; row < RX_CC_ROWS; ++row) {
          const int z = z0 + row / RX_CC_TY, y = y0 + row % RX_CC_TY;
          for (int t = 0; t < RX_CC_TX; ++t) {
            if (!(z < Z && y < Y && x0 + t < X)) continue;
            int lab = 0;
            if ((masks[row] >> t) & 1ull) {
              const int r = cc_find(lds, row * RX_CC_TX + t), rrow = r / RX_CC_TX;
              lab = (int)((z0 + rrow / RX_CC_TY) * XY + (long)(y0 + rrow % RX_CC_TY) * X + x0 + r % RX_CC_TX) + 1;
            }
            labels.at(z * XY + (long)y * X + x0 + t) = lab;
          }
        }
      }
  VolForest vol{labels};
  for (int axis = 0; axis < 3; ++axis) {
    const int tile = axis == 0 ? RX_CC_TZ : axis == 1 ? RX_CC_TY : RX_CC_TX;
    std::vector<long> idx;
    for (int z = 0; z < Z; ++z)
      for (int y = 0; y < Y; ++y)
        for (int x = 0; x < X; ++x) {
          const int c = axis == 0 ? z : axis == 1 ? y : x;
          if (c > 0 && c % tile == 0) idx.push_back(z * XY + (long)y * X + x);
        }
    order(idx, how);
    for (long i : idx) cc_seam_voxel(vol, axis, (int)(i / XY), (int)(i % XY / X), (int)(i % X), Z, Y, X, steps);
  }
  std::vector<long> idx;
  for (long i = 0; i < (long)labels.size(); ++i) idx.push_back(i);
  order(idx, how);
  for (long i : idx) cc_flatten_voxel(vol, (int)i);
  return labels;
}

static std::vector<int> label_bfs(const std::vector<uint8_t>& m, Shape s, int conn) {
  const int Z = s.z, Y = s.y, X = s.x, steps = conn == 6 ? 1 : conn == 18 ? 2 : 3;
  const long XY = (long)Y * X;
  std::vector<int> labels((size_t)Z * XY, 0);
  for (long i = 0; i < (long)labels.size(); ++i) {      // raster order: the first voxel of a component is its smallest index
    if (!m[i] || labels[i]) continue;
    std::queue<long> q;
    q.push(i), labels[i] = (int)i + 1;
    while (!q.empty()) {
      const long v = q.front();
      q.pop();
      const int z = (int)(v / XY), y = (int)(v % XY / X), x = (int)(v % X);
      for (int dz = -1; dz <= 1; ++dz)
        for (int dy = -1; dy <= 1; ++dy)
          for (int dx = -1; dx <= 1; ++dx) {
            const int n = (dz != 0) + (dy != 0) + (dx != 0);
            if (n == 0 || n > steps) continue;
            const int z2 = z + dz, y2 = y + dy, x2 = x + dx;
            if (z2 < 0 || z2 >= Z || y2 < 0 || y2 >= Y || x2 < 0 || x2 >= X) continue;
            const long u = z2 * XY + (long)y2 * X + x2;
            if (m[u] && !labels[u]) labels[u] = (int)i + 1, q.push(u);
          }
    }
  }
  return labels;
}

// ---- the masks of tests/components_cases.py ----------------------------------------------------------------------------------------------
struct Case { std::string name; std::vector<uint8_t> m; };

static std::vector<Case> cases_of(Shape s) {
  const int Z = s.z, Y = s.y, X = s.x;
  const long XY = (long)Y * X, V = Z * XY;
  auto at = [&](std::vector<uint8_t>& m, int z, int y, int x) -> uint8_t& { return m.at(z * XY + (long)y * X + x); };
  auto box = [&](std::vector<uint8_t>& m, int z0, int z1, int y0, int y1, int x0, int x1) {      // clipped to the volume
    for (int z = std::max(z0, 0); z < std::min(z1, Z); ++z)
      for (int y = std::max(y0, 0); y < std::min(y1, Y); ++y)
        for (int x = std::max(x0, 0); x < std::min(x1, X); ++x) at(m, z, y, x) = 1;
  };
  std::vector<Case> out;
  out.push_back({"empty", std::vector<uint8_t>(V, 0)});
  out.push_back({"full", std::vector<uint8_t>(V, 1)});
  { std::vector<uint8_t> m(V, 0); m.front() = 1, m.back() = 1; out.push_back({"corners", m}); }
  for (int pc : {10, 30, 60}) {
    std::vector<uint8_t> m(V);
    for (auto& b : m) b = rnd() % 100 < (uint32_t)pc;
    out.push_back({"random" + std::to_string(pc), m});
  }
  { std::vector<uint8_t> m(V);
    for (long i = 0; i < V; ++i) m[i] = ((i / XY + i % XY / X + i % X) & 1) == 0;
    out.push_back({"checkerboard", m}); }
  { std::vector<uint8_t> m(V, 0);      // full-x rows on every second y, joined alternately at x = 0 and x = X - 1, on every z
    for (int z = 0; z < Z; ++z)
      for (int y = 0; y < Y; ++y)
        if (y % 2 == 0) { for (int x = 0; x < X; ++x) at(m, z, y, x) = 1; }
        else at(m, z, y, (y / 2) % 2 == 0 ? X - 1 : 0) = 1;
    out.push_back({"serpentine", m}); }
  // two slabs that meet in one voxel pair, diagonally across the tile corner / across the tile edge at (cz, cy, cx), the first
  // tile boundary of every axis that has one (else the middle of the axis)
  const int cz = Z > RX_CC_TZ ? RX_CC_TZ : (Z + 1) / 2, cy = Y > RX_CC_TY ? RX_CC_TY : (Y + 1) / 2, cx = X > RX_CC_TX ? RX_CC_TX : (X + 1) / 2;
  { std::vector<uint8_t> m(V, 0);
    box(m, cz - 3, cz, cy - 3, cy, cx - 3, cx), box(m, cz, cz + 3, cy, cy + 3, cx, cx + 3);
    out.push_back({"corner_pair", m}); }
  { std::vector<uint8_t> m(V, 0);
    box(m, cz - 3, cz, cy - 3, cy, 0, X), box(m, cz, cz + 3, cy, cy + 3, 0, X);
    out.push_back({"edge_pair", m}); }
  { std::vector<uint8_t> m(V, 0);      // one path from voxel (0, 0, 1) along x, then y, then z to the last voxel: every other tile's root is linked back to the first tile's
    for (int z = 0; z < Z; ++z) at(m, z, Y - 1, X - 1) = 1;
    for (int y = 0; y < Y; ++y) at(m, 0, y, X - 1) = 1;
    for (int x = 0; x < X; ++x) at(m, 0, 0, x) = 1;
    at(m, 0, 0, 0) = X > 1 || Y > 1 || Z > 1 ? 0 : 1;
    out.push_back({"backward_root", m}); }
  return out;
}

int main() {
  long ncases = 0, bad = 0;
  for (const Shape& s : SHAPES)
    for (const Case& c : cases_of(s))
      for (int conn : {6, 18, 26}) {
        const std::vector<int> want = label_bfs(c.m, s, conn);
        for (int how = 0; how < 3; ++how) {
          const std::vector<int> got = label_core(c.m, s, conn, how);
          long diff = 0;
          for (size_t i = 0; i < want.size(); ++i) diff += got[i] != want[i];
          ++ncases;
          if (diff) {
            ++bad;
            printf("DIFFER %dx%dx%d %s connectivity %d order %d: %ld voxels\n", s.z, s.y, s.x, c.name.c_str(), conn, how, diff);
          }
        }
      }
  printf("%ld cases, %ld differ from the breadth-first search\n", ncases, bad);
  return bad ? 1 : 0;
}
