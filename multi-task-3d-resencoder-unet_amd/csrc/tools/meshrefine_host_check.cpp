// meshrefine_host_check.cpp -- runs csrc/rx_meshrefine_core.h, the per-corner, per-vertex and per-face work of rx_meshrefine.hip, serially
// on the host: the corners counted, the counts scanned, every corner filled at its vertex's cursor (mr_fill_corner), every vertex
// canonicalised (mr_canonical), the degrees scanned and the neighbours compacted, then Taubin passes over ping-pong buffers
// (mr_smooth_vertex), face vectors (mr_face_vector) and vertex normals (mr_vertex_normal) -- the passes of the kernels, with plain
// loops where they have threads.  The corners take their slots in raster, reverse and shuffled order (on the device arrival decides),
// and every mesh is run once more with its triangles shuffled and the ids rotated within each: the adjacency must be the same each
// time, and everything must equal a direct restatement written here with std::set and std::map.  Build with
//     g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all meshrefine_host_check.cpp
// so that an index outside a vertex's slots, the lists or the outputs is an error, not a wrong mesh.
// The cases restate tests/mesh_refine_cases.py: the grid patch, the vertex counts, the awkward topology, the fans (the closed meshes
// are an octahedron and random triangle soups from this program's own generator).
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <set>
#include <string>
#include <utility>
#include <vector>

#include "../rx_meshrefine_core.h"
#include "check_util.h"


struct Mesh {
  std::string name;
  std::vector<float> v;        // 3 per vertex
  std::vector<int64_t> t;      // 3 per triangle
  int64_t V() const { return (int64_t)v.size() / 3; }
  int64_t T() const { return (int64_t)t.size() / 3; }
};

struct Adjacency {
  std::vector<int64_t> offsets, foff;
  std::vector<int32_t> nbr, faces;
  std::vector<uint8_t> boundary;
  bool operator==(const Adjacency& o) const {
    return offsets == o.offsets && foff == o.foff && nbr == o.nbr && faces == o.faces && boundary == o.boundary;
  }
};


// ---- the passes, through the core header --------------------------------------------------------------------------------------------------
static Adjacency adjacency_core(const Mesh& m, int how) {
  const int64_t V = m.V(), T = m.T();
  Adjacency a;
  std::vector<int32_t> counts(V, 0), cursor(V, 0), degrees(V, -1);
  for (int64_t t = 0; t < T; ++t)
    if (mr_triangle_ok(&m.t[3 * t], V))
      for (int k = 0; k < 3; ++k) ++counts.at(m.t[3 * t + k]);
  a.foff.assign(V + 1, 0);
  for (int64_t v = 0; v < V; ++v) a.foff[v + 1] = a.foff[v] + counts[v];
  const int64_t cap = a.foff[V];
  a.faces.assign(cap, -7);
  std::vector<int32_t> raw(2 * cap, -7);
  std::vector<int64_t> corners;
  for (int64_t c = 0; c < 3 * T; ++c) corners.push_back(c);
  order(corners, how);
  for (int64_t c : corners) {      // fill: the order of the corners stands for the arrival order of the atomics
    const int64_t t = c / 3;
    const int k = (int)(c % 3);
    if (!mr_triangle_ok(&m.t[3 * t], V)) continue;
    const int64_t v = m.t[3 * t + k], at = a.foff[v] + cursor.at(v)++;
    if (at >= a.foff[v + 1]) printf("%s: more corners than counted at vertex %ld\n", m.name.c_str(), (long)v);
    mr_fill_corner(&m.t[3 * t], k, t, at, cap, a.faces.data(), raw.data());
  }
  a.boundary.assign(V, 9);
  std::vector<int64_t> verts;
  for (int64_t v = 0; v < V; ++v) verts.push_back(v);
  order(verts, how);
  for (int64_t v : verts)
    degrees.at(v) = mr_canonical((int32_t)v, a.faces.data() + a.foff[v], raw.data() + 2 * a.foff[v], a.foff[v + 1] - a.foff[v], &a.boundary.at(v));
  a.offsets.assign(V + 1, 0);
  for (int64_t v = 0; v < V; ++v) a.offsets[v + 1] = a.offsets[v] + degrees[v];
  a.nbr.assign(a.offsets[V], -7);
  for (int64_t v : verts)
    for (int64_t r = 0; r < degrees[v]; ++r) a.nbr.at(a.offsets[v] + r) = raw.at(2 * a.foff[v] + r);
  return a;
}

static std::vector<float> smooth_core(const Mesh& m, const Adjacency& a, int iterations, float lam, const float* mu, const float* clamp, bool pin) {
  const int64_t V = m.V();
  std::vector<float> buf[2] = {std::vector<float>(3 * V, NAN), std::vector<float>(3 * V, NAN)};
  const std::vector<float>* src = &m.v;
  int pass = 0;
  for (int it = 0; it < iterations; ++it)
    for (int h = 0; h < (mu ? 2 : 1); ++h, ++pass) {
      std::vector<float>& dst = buf[pass % 2];
      for (int64_t v = 0; v < V; ++v)
        mr_smooth_vertex(v, src->data(), clamp ? m.v.data() : nullptr, V, a.offsets.data(), a.nbr.data(), (int64_t)a.nbr.size(), pin && a.boundary[v],
                         h ? *mu : lam, clamp ? *clamp : 0.0f, &dst.at(3 * v));
      src = &dst;
    }
  return *src;
}

static std::vector<float> normals_core(const Mesh& m, const std::vector<float>& pos, const Adjacency& a) {
  const int64_t V = m.V(), T = m.T();
  std::vector<float> fvec(3 * T, NAN), out(3 * V, NAN);
  for (int64_t t = 0; t < T; ++t) {
    float n[3] = {0, 0, 0};
    if (mr_triangle_ok(&m.t[3 * t], V)) mr_face_vector(&pos.at(3 * m.t[3 * t]), &pos.at(3 * m.t[3 * t + 1]), &pos.at(3 * m.t[3 * t + 2]), n);
    memcpy(&fvec.at(3 * t), n, sizeof n);
  }
  for (int64_t v = 0; v < V; ++v) mr_vertex_normal(v, a.foff.data(), a.faces.data(), (int64_t)a.faces.size(), fvec.data(), T, &out.at(3 * v));
  return out;
}

// ---- the direct restatement ------------------------------------------------------------------------------------------------------------------
struct Direct {
  std::vector<std::set<int64_t>> nbr;
  std::vector<uint8_t> boundary;
  std::vector<std::vector<int64_t>> faces;      // per vertex, ascending by construction
};

static Direct direct_adjacency(const Mesh& m) {
  Direct d;
  d.nbr.resize(m.V());
  d.boundary.assign(m.V(), 0);
  d.faces.resize(m.V());
  std::map<std::pair<int64_t, int64_t>, int> uses;
  for (int64_t t = 0; t < m.T(); ++t)
    for (int k = 0; k < 3; ++k) {
      const int64_t a = m.t[3 * t + k], b = m.t[3 * t + (k + 1) % 3];
      d.faces.at(a).push_back(t);
      if (a == b) continue;
      d.nbr.at(a).insert(b), d.nbr.at(b).insert(a);
      ++uses[{std::min(a, b), std::max(a, b)}];
    }
  for (const auto& u : uses)
    if (u.second == 1) d.boundary.at(u.first.first) = 1, d.boundary.at(u.first.second) = 1;
  return d;
}

static std::vector<float> direct_smooth(const Mesh& m, const Direct& d, int iterations, float lam, const float* mu, const float* clamp, bool pin) {
  std::vector<float> p = m.v;
  for (int it = 0; it < iterations; ++it)
    for (int h = 0; h < (mu ? 2 : 1); ++h) {
      const float f = h ? *mu : lam;
      std::vector<float> q = p;
      for (int64_t v = 0; v < m.V(); ++v) {
        if (d.nbr[v].empty() || (pin && d.boundary[v])) continue;
        for (int k = 0; k < 3; ++k) {
          float s = 0.0f;
          for (int64_t n : d.nbr[v]) s = s + p[3 * n + k];
          const float mean = s / (float)d.nbr[v].size();
          const float diff = mean - p[3 * v + k];
          const float step = f * diff;
          float r = p[3 * v + k] + step;
          if (clamp) {
            const float lo = m.v[3 * v + k] - *clamp, hi = m.v[3 * v + k] + *clamp;
            if (r < lo) r = lo;
            if (r > hi) r = hi;
          }
          q[3 * v + k] = r;
        }
      }
      p = q;
    }
  return p;
}

static std::vector<float> direct_normals(const Mesh& m, const std::vector<float>& p, const Direct& d) {
  std::vector<float> out(3 * m.V(), 0.0f);
  for (int64_t v = 0; v < m.V(); ++v) {
    float acc[3] = {0, 0, 0};
    for (int64_t t : d.faces[v]) {
      const float *a = &p[3 * m.t[3 * t]], *b = &p[3 * m.t[3 * t + 1]], *c = &p[3 * m.t[3 * t + 2]];
      const float u[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]}, w[3] = {c[0] - a[0], c[1] - a[1], c[2] - a[2]};
      const float x0 = u[1] * w[2], x1 = u[2] * w[1], y0 = u[2] * w[0], y1 = u[0] * w[2], z0 = u[0] * w[1], z1 = u[1] * w[0];
      acc[0] = acc[0] + (x0 - x1), acc[1] = acc[1] + (y0 - y1), acc[2] = acc[2] + (z0 - z1);
    }
    const float xx = acc[0] * acc[0], yy = acc[1] * acc[1], zz = acc[2] * acc[2];
    const float len = sqrtf((xx + yy) + zz);
    if (len != 0.0f)
      for (int k = 0; k < 3; ++k) out[3 * v + k] = acc[k] / len;
  }
  return out;
}

// ---- the meshes of tests/mesh_refine_cases.py ---------------------------------------------------------------------------------------------------
static Mesh with_positions(std::string name, int64_t V, std::vector<int64_t> t) {
  Mesh m{std::move(name), {}, std::move(t)};
  for (int64_t i = 0; i < 3 * V; ++i) m.v.push_back(rndf());
  return m;
}

static Mesh grid_patch(int ny, int nx) {
  Mesh m{"grid", {}, {}};
  for (int j = 0; j < ny; ++j)
    for (int i = 0; i < nx; ++i) m.v.push_back((float)i), m.v.push_back((float)j), m.v.push_back(3.0f);
  for (int j = 0; j + 1 < ny; ++j)
    for (int i = 0; i + 1 < nx; ++i) {
      const int64_t a = j * nx + i, b = a + 1, c = a + nx, d = c + 1;
      const int64_t q[6] = {a, b, d, a, d, c};
      m.t.insert(m.t.end(), q, q + 6);
    }
  return m;
}

static Mesh fan(int degree) {
  std::vector<int64_t> t;
  for (int i = 0; i < degree; ++i) {
    const int64_t q[3] = {0, 1 + i, 1 + (i + 1) % degree};
    t.insert(t.end(), q, q + 3);
  }
  return with_positions("fan" + std::to_string(degree), degree + 1, t);
}

static Mesh soup(int64_t V, int64_t T) {
  std::vector<int64_t> t;
  for (int64_t i = 0; i < 3 * T; ++i) t.push_back(rnd() % V);      // repeated ids and repeated triangles happen
  return with_positions("soup" + std::to_string(V), V, t);
}

static std::vector<Mesh> all_cases() {
  std::vector<Mesh> out;
  out.push_back(grid_patch(5, 7));
  out.push_back(with_positions("octahedron", 6, {0, 2, 4, 2, 1, 4, 1, 3, 4, 3, 0, 4, 2, 0, 5, 1, 2, 5, 3, 1, 5, 0, 3, 5}));
  // vertex 3 isolated, 4 only in a degenerate triangle, (5, 5, 6) a repeated id, (0, 1, 2) twice and four triangles on its edge (0, 1),
  // three triangles on edge (7, 8), id V - 1 in use
  out.push_back(with_positions("awkward", 13, {0, 1, 2, 0, 1, 2, 4, 4, 4, 5, 5, 6, 7, 8, 9, 7, 8, 10, 8, 7, 11, 12, 0, 9, 1, 0, 6, 0, 1, 9}));
  for (int64_t V : {1, 63, 64, 65, 257, 2100}) out.push_back(soup(V, V == 1 ? 2 : 2 * V));
  for (int d : {3, 8, 9, 300, 3000}) out.push_back(fan(d));
  out.push_back(with_positions("no-triangles", 5, {}));
  return out;
}

static Mesh shuffled(const Mesh& m) {
  Mesh s{m.name + "-shuffled", m.v, {}};
  std::vector<int64_t> idx;
  for (int64_t t = 0; t < m.T(); ++t) idx.push_back(t);
  order(idx, 2);
  for (int64_t t : idx) {
    const int r = (int)(rnd() % 3);
    for (int k = 0; k < 3; ++k) s.t.push_back(m.t[3 * t + (k + r) % 3]);
  }
  return s;
}


int main() {
  long runs = 0, bad = 0;
  const float mu = -0.53f, clamp = 1.0f;
  for (const Mesh& base : all_cases()) {
    Adjacency first;
    for (int variant = 0; variant < 2; ++variant) {
      const Mesh m = variant ? shuffled(base) : base;
      const Direct d = direct_adjacency(m);
      for (int how = 0; how < 3; ++how) {
        ++runs;
        const Adjacency a = adjacency_core(m, how);
        bool ok = true;
        for (int64_t v = 0; v < m.V() && ok; ++v) {      // against the sets
          std::vector<int64_t> got(a.nbr.begin() + a.offsets[v], a.nbr.begin() + a.offsets[v + 1]);
          std::vector<int64_t> fgot(a.faces.begin() + a.foff[v], a.faces.begin() + a.foff[v + 1]);
          ok = got == std::vector<int64_t>(d.nbr[v].begin(), d.nbr[v].end()) && a.boundary[v] == d.boundary[v] && fgot == d.faces[v];
        }
        if (variant == 0 && how == 0) first = a;
        // the neighbour lists and the boundary do not depend on the triangle order; the triangle lists name shuffled indices
        ok = ok && a.offsets == first.offsets && a.nbr == first.nbr && a.boundary == first.boundary && (variant || a == first);
        const int iters = m.V() > 1000 ? 2 : 5;
        for (int opt = 0; opt < 4 && ok; ++opt) {      // mu set / None, clamp on / off, pinned / free
          const float* pmu = (opt & 1) ? nullptr : &mu;
          const float* pc = (opt & 2) ? nullptr : &clamp;
          const bool pin = opt == 0 || opt == 3;
          const std::vector<float> p = smooth_core(m, a, iters, 0.5f, pmu, pc, pin);
          ok = same_bits(p, direct_smooth(m, d, iters, 0.5f, pmu, pc, pin)) && same_bits(normals_core(m, p, a), direct_normals(m, p, d));
        }
        if (!ok) ++bad, printf("DIFFER %s fill order %d\n", m.name.c_str(), how);
      }
    }
  }
  printf("%ld runs, %ld differ from the direct restatement\n", runs, bad);
  return bad ? 1 : 0;
}
