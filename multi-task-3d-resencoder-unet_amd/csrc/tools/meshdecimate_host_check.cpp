// meshdecimate_host_check.cpp -- runs csrc/rx_meshdecimate_core.h, the per-vertex, per-cluster and per-triangle work of
// rx_meshdecimate.hip, serially on the host: keys (md_key), the hash table (md_insert, md_smallest) at its smallest and at the default
// capacity, the numbering by a scan of the "smallest of its cluster" flags, member lists filled at a cursor and summed (md_mean), the
// packed minimum (md_nearest_pack), triangles remapped (md_remap), attached to their smallest cluster and made unique (md_unique),
// the outputs compacted -- the passes of the kernels, with plain loops where they have threads.  The vertices and the triangles take
// their turns in raster, reverse and shuffled order (on the device arrival decides): every result must be the same each time, and
// must equal a direct restatement written here with std::map and std::set.  Build with
//     g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all meshdecimate_host_check.cpp
// so that an index outside the table, a list or an output is an error, not a wrong mesh.
// The cases restate tests/mesh_decimate_cases.py: the grid patch at integer and at negative coordinates with cells that divide the
// spacing and cells that do not, one cluster, the identity, the fan of 3000 inside one cell and across 64, soups, the awkward
// topology, the two-sided slab, a mesh without triangles and a 300 x 300 grid (positions from this program's own generator).
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <array>
#include <map>
#include <set>
#include <string>
#include <utility>
#include <vector>

#include "../rx_meshdecimate_core.h"
#include "check_util.h"


struct Mesh {
  std::string name;
  std::vector<float> v;        // 3 per vertex
  std::vector<int64_t> t;      // 3 per triangle
  float cell;
  int64_t V() const { return (int64_t)v.size() / 3; }
  int64_t T() const { return (int64_t)t.size() / 3; }
};

struct Result {
  std::vector<float> v;
  std::vector<int64_t> t, cluster_of;
  bool operator==(const Result& o) const {
    return same_bits(v, o.v) && t == o.t && cluster_of == o.cluster_of;
  }
};

static std::vector<int64_t> order(int64_t n, int how) {      // 0 raster, 1 reverse, 2 shuffled
  std::vector<int64_t> idx;
  for (int64_t i = 0; i < n; ++i) idx.push_back(i);
  order(idx, how);
  return idx;
}

static std::vector<int64_t> scan(const std::vector<int32_t>& c) {
  std::vector<int64_t> o(c.size() + 1, 0);
  for (size_t i = 0; i < c.size(); ++i) o[i + 1] = o[i] + c[i];
  return o;
}

// ---- the passes, through the core header --------------------------------------------------------------------------------------------------
static bool decimate_core(const Mesh& m, bool nearest, int how, int64_t capacity, Result* out) {
  const int64_t V = m.V(), T = m.T();
  std::vector<int64_t> keys(V, -7), table_keys(capacity, MD_EMPTY);
  std::vector<uint32_t> table_min(capacity, MD_NO_MIN);
  std::vector<int32_t> slot_of(V, -7), first(V, -7);
  for (int64_t v = 0; v < V; ++v)
    if (!md_key(&m.v[3 * v], m.cell, &keys.at(v))) return false;
  const std::vector<int64_t> vs = order(V, how), ts = order(T, how);
  for (int64_t v : vs) {
    slot_of.at(v) = md_insert(keys[v], (int32_t)v, capacity, table_keys.data(), table_min.data());
    if (slot_of[v] < 0) return false;
  }
  for (int64_t v : vs) first.at(v) = md_smallest(slot_of[v], capacity, table_min.data(), V) == (int32_t)v;
  const std::vector<int64_t> rank = scan(first);
  const int64_t C = rank[V];
  out->cluster_of.assign(V, -7);
  for (int64_t v : vs) out->cluster_of.at(v) = rank.at(md_smallest(slot_of[v], capacity, table_min.data(), V));
  const std::vector<int64_t>& cl = out->cluster_of;
  std::vector<float> reps(3 * C, NAN);
  if (!nearest) {
    std::vector<int32_t> counts(C, 0), cursor(C, 0), members(V, -7);
    for (int64_t v = 0; v < V; ++v) ++counts.at(cl[v]);
    const std::vector<int64_t> moff = scan(counts);
    for (int64_t v : vs) members.at(moff[cl[v]] + cursor.at(cl[v])++) = (int32_t)v;
    for (int64_t c : order(C, how)) md_mean(members.data() + moff[c], moff[c + 1] - moff[c], m.v.data(), V, &reps.at(3 * c));
  } else {
    std::vector<uint64_t> best(C, ~0ull);
    for (int64_t v : vs) best.at(cl[v]) = std::min(best.at(cl[v]), md_nearest_pack(&m.v[3 * v], keys[v], m.cell, (int32_t)v));
    for (int64_t c = 0; c < C; ++c) memcpy(&reps.at(3 * c), &m.v.at(3 * (best[c] & 0xffffffffull)), 12);
  }
  std::vector<int32_t> counts(C, 0), used(C, 0), cursor(C, 0), keep(T, 0), entries(3 * T, -7);
  int64_t c3[3];
  int32_t lo, mid, hi;
  for (int64_t t = 0; t < T; ++t)
    if (md_remap(&m.t[3 * t], V, cl.data(), C, c3, &lo, &mid, &hi)) used.at(lo) = used.at(mid) = used.at(hi) = 1, ++counts.at(lo);
  const std::vector<int64_t> toff = scan(counts), uoff = scan(used);
  for (int64_t t : ts)
    if (md_remap(&m.t[3 * t], V, cl.data(), C, c3, &lo, &mid, &hi)) {
      const int64_t at = toff[lo] + cursor.at(lo)++;
      entries.at(3 * at) = mid, entries.at(3 * at + 1) = hi, entries.at(3 * at + 2) = (int32_t)t;
    }
  for (int64_t c : order(C, how))
    if (toff[c + 1] > toff[c]) md_unique(entries.data() + 3 * toff[c], toff[c + 1] - toff[c], T, keep.data());
  const std::vector<int64_t> koff = scan(keep);
  out->t.assign(3 * koff[T], -7);
  out->v.assign(3 * uoff[C], NAN);
  for (int64_t t = 0; t < T; ++t)
    if (keep[t])
      for (int k = 0; k < 3; ++k) out->t.at(3 * koff[t] + k) = uoff.at(cl.at(m.t[3 * t + k]));
  for (int64_t c = 0; c < C; ++c)
    if (used[c]) memcpy(&out->v.at(3 * uoff[c]), &reps.at(3 * c), 12);
  return true;
}

// ---- the direct restatement ------------------------------------------------------------------------------------------------------------------
static Result decimate_direct(const Mesh& m, bool nearest) {
  const int64_t V = m.V(), T = m.T();
  std::map<std::array<int64_t, 3>, int64_t> number;
  std::vector<std::array<int64_t, 3>> cells;
  std::vector<std::vector<int64_t>> members;
  Result r;
  for (int64_t v = 0; v < V; ++v) {
    std::array<int64_t, 3> k;
    for (int c = 0; c < 3; ++c) {
      const float q = m.v[3 * v + c] / m.cell;
      k[c] = (int64_t)floorf(q);
    }
    if (!number.count(k)) number[k] = (int64_t)cells.size(), cells.push_back(k), members.emplace_back();
    members[number[k]].push_back(v);      // ascending id by construction; clusters in order of their first, so smallest, member
    r.cluster_of.push_back(number[k]);
  }
  std::vector<float> reps;
  for (size_t c = 0; c < cells.size(); ++c) {
    if (!nearest) {
      for (int k = 0; k < 3; ++k) {
        float s = 0.0f;
        for (int64_t v : members[c]) s = s + m.v[3 * v + k];
        reps.push_back(s / (float)members[c].size());
      }
    } else {
      int64_t who = -1;
      float least = 0.0f;
      for (int64_t v : members[c]) {
        float sq[3];
        for (int k = 0; k < 3; ++k) {
          const float half = (float)cells[c][k] + 0.5f;
          const float centre = half * m.cell;
          const float dx = m.v[3 * v + k] - centre;
          sq[k] = dx * dx;
        }
        const float xy = sq[0] + sq[1];
        const float d = xy + sq[2];
        if (who < 0 || d < least) who = v, least = d;
      }
      for (int k = 0; k < 3; ++k) reps.push_back(m.v[3 * who + k]);
    }
  }
  std::set<std::array<int64_t, 3>> seen;
  std::vector<std::array<int64_t, 3>> kept;
  for (int64_t t = 0; t < T; ++t) {
    const std::array<int64_t, 3> c = {r.cluster_of[m.t[3 * t]], r.cluster_of[m.t[3 * t + 1]], r.cluster_of[m.t[3 * t + 2]]};
    if (c[0] == c[1] || c[1] == c[2] || c[0] == c[2]) continue;
    std::array<int64_t, 3> s = c;
    std::sort(s.begin(), s.end());
    if (seen.insert(s).second) kept.push_back(c);
  }
  std::map<int64_t, int64_t> row;
  for (const auto& c : kept)
    for (int64_t x : c) row[x] = 0;
  int64_t n = 0;
  for (auto& e : row) {
    e.second = n++;
    for (int k = 0; k < 3; ++k) r.v.push_back(reps[3 * e.first + k]);
  }
  for (const auto& c : kept)
    for (int64_t x : c) r.t.push_back(row[x]);
  return r;
}

// ---- the cases of tests/mesh_decimate_cases.py -------------------------------------------------------------------------------------------------
static Mesh grid_patch(std::string name, int ny, int nx, float x0, float y0, float z, float cell) {
  Mesh m{std::move(name), {}, {}, cell};
  for (int j = 0; j < ny; ++j)
    for (int i = 0; i < nx; ++i) m.v.push_back(x0 + (float)i), m.v.push_back(y0 + (float)j), m.v.push_back(z);
  for (int j = 0; j + 1 < ny; ++j)
    for (int i = 0; i + 1 < nx; ++i) {
      const int64_t a = (int64_t)j * nx + i, b = a + 1, c = a + nx, d = c + 1;
      const int64_t q[6] = {a, b, d, a, d, c};
      m.t.insert(m.t.end(), q, q + 6);
    }
  return m;
}

static Mesh with_positions(std::string name, int64_t V, std::vector<int64_t> t, float cell, float scale = 1.0f, float shift = 0.0f) {
  Mesh m{std::move(name), {}, std::move(t), cell};
  for (int64_t i = 0; i < 3 * V; ++i) m.v.push_back(rndf() * scale + shift);
  return m;
}

static std::vector<int64_t> fan(int degree) {
  std::vector<int64_t> t;
  for (int i = 0; i < degree; ++i) {
    const int64_t q[3] = {0, 1 + i, 1 + (i + 1) % degree};
    t.insert(t.end(), q, q + 3);
  }
  return t;
}

static std::vector<int64_t> soup(int64_t V, int64_t T) {
  std::vector<int64_t> t;
  for (int64_t i = 0; i < 3 * T; ++i) t.push_back(rnd() % V);      // repeated ids and repeated triangles happen
  return t;
}

static Mesh slab(float cell) {
  Mesh m = grid_patch("slab", 5, 7, 0.0f, 0.0f, 3.0f, cell);
  const Mesh up = grid_patch("", 5, 7, 0.0f, 0.0f, 3.25f, cell);
  const int64_t V = m.V(), T = m.T();
  m.v.insert(m.v.end(), up.v.begin(), up.v.end());
  for (int64_t t = 0; t < T; ++t)
    for (int k = 2; k >= 0; --k) m.t.push_back(up.t[3 * t + k] + V);      // the opposite winding
  return m;
}

static std::vector<Mesh> all_cases() {
  std::vector<Mesh> out;
  for (float cell : {1.0f, 2.0f, 0.75f, 64.0f, 0.25f}) out.push_back(grid_patch("grid", 5, 7, 0.0f, 0.0f, 3.0f, cell));
  for (float cell : {1.0f, 2.0f, 3.5f}) out.push_back(grid_patch("grid-neg", 5, 7, -6.0f, -4.0f, -1.0f, cell));
  out.push_back(with_positions("fan3000-one-cell", 3001, fan(3000), 1.0f, 0.004f, 0.5f));
  out.push_back(with_positions("fan3000", 3001, fan(3000), 50.0f));
  out.push_back(with_positions("soup257", 257, soup(257, 514), 3.5f));
  out.push_back(with_positions("soup257", 257, soup(257, 514), 60.0f));
  out.push_back(with_positions("soup2100", 2100, soup(2100, 4200), 40.0f));
  // vertex 3 isolated, 4 only in a degenerate triangle, (5, 5, 6) a repeated id, (0, 1, 2) twice, id V - 1 in use
  const std::vector<int64_t> awkward = {0, 1, 2, 0, 1, 2, 4, 4, 4, 5, 5, 6, 7, 8, 9, 7, 8, 10, 8, 7, 11, 12, 0, 9, 1, 0, 6, 0, 1, 9};
  out.push_back(with_positions("awkward", 13, awkward, 50.0f));
  out.push_back(with_positions("awkward", 13, awkward, 0.01f));
  out.push_back(slab(1.0f));
  out.push_back(slab(2.0f));
  out.push_back(with_positions("no-triangles", 5, {}, 30.0f));
  out.push_back(grid_patch("big-grid", 300, 300, 0.0f, 0.0f, 3.0f, 2.0f));
  out.push_back(grid_patch("big-grid", 300, 300, 0.0f, 0.0f, 3.0f, 0.5f));
  return out;
}

int main() {
  long runs = 0, bad = 0;
  for (const Mesh& m : all_cases()) {
    int64_t smallest = 1, usual = 1;
    while (smallest <= m.V()) smallest <<= 1;        // the smallest power of two above V
    while (usual < 2 * m.V() + 2) usual <<= 1;       // what the ops layer passes
    for (int nearest = 0; nearest < 2; ++nearest) {
      const Result want = decimate_direct(m, nearest != 0);
      for (int how = 0; how < 3; ++how)
        for (int64_t capacity : {smallest, usual}) {
          ++runs;
          Result got;
          const bool ok = decimate_core(m, nearest != 0, how, capacity, &got) && got == want;
          if (!ok) ++bad, printf("DIFFER %s cell %g %s order %d capacity %ld\n", m.name.c_str(), m.cell, nearest ? "nearest" : "mean", how, (long)capacity);
        }
    }
  }
  // a key outside the range is refused, and a table that is full of other keys ends the probe loop instead of spinning
  const float far[3] = {3.0f, -1048576.0f, 0.0f}, edge[3] = {1048575.5f, -1048575.0f, 0.0f};
  int64_t key = 0;
  if (md_key(far, 0.5f, &key) || !md_key(edge, 1.0f, &key) || md_key(far, 1e-30f, &key)) ++bad, printf("DIFFER key range\n");
  std::vector<int64_t> full(8);
  std::vector<uint32_t> mins(8, MD_NO_MIN);
  for (int i = 0; i < 8; ++i) full[i] = 1000 + i;
  if (md_insert(5, 0, 8, full.data(), mins.data()) != -1) ++bad, printf("DIFFER full table\n");
  printf("%ld runs, %ld differ from the direct restatement\n", runs, bad);
  return bad ? 1 : 0;
}
