// meshsample_host_check.cpp -- runs the per-vertex and per-triangle work of the mesh orientation kernels (../rx_meshsample_core.h)
// serially on the CPU against a direct restatement written here with plain loops, and compares bits.  Meant to be compiled with
// -fsanitize=address,undefined: every volume and every slab is a heap block of exactly its size, so a load that leaves a slab is
// reported.  The kinds of volume, point and mesh are those of tests/mesh_orient_cases.py: every rule, 1 / 3 / 8 channels, odd
// extents and a volume of one voxel, points on the lattice, beyond each border, at +-1e30, NaN and infinities (which the Python
// wrapper refuses, and which must still not leave the slab), slabs of every depth, a degenerate triangle and a zero vector.
//
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all meshsample_host_check.cpp
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../rx_meshsample_core.h"
#include "check_util.h"

static float uniform(float lo, float hi) { return lo + (hi - lo) * (float)(rnd() % 65536) / 65536.0f; }


// ---- the restatement ----------------------------------------------------------------------------------------------------------------------------
template <typename T>
static float ref_decode(int rule, T v) {
  volatile float f = (float)v;
  if (rule == RX_MSP_COPY) return f;
  if (rule == RX_MSP_U8) {
    volatile float q = f / 255.0f;
    return q;
  }
  volatile float q = f / 65535.0f;
  if (rule == RX_MSP_U16) return q;
  volatile float d = q * 2.0f;
  volatile float r = d - 1.0f;
  return r;
}

static void ref_axis(float p, long n, long* i0, long* i1, float* f) {
  const double fl = std::floor((double)p);
  volatile float fr = p - (float)fl;
  *f = fr;
  long i;
  if (std::isnan(p)) i = n;
  else if (fl < -2.0) i = -2;
  else if (fl > (double)n) i = n;
  else i = (long)fl;
  *i0 = i < 0 ? 0 : (i > n - 1 ? n - 1 : i);
  *i1 = i + 1 < 0 ? 0 : (i + 1 > n - 1 ? n - 1 : i + 1);
}

static float ref_lerp(float u, float w, float f) {
  volatile float d = w - u;
  volatile float fd = f * d;
  volatile float r = u + fd;
  return r;
}

// the whole volume (C, Z, Y, X) at p -> out[C]
template <typename T>
static void ref_sample(int rule, const std::vector<T>& vol, int C, long Z, long Y, long X, const float p[3], float* out) {
  long x[2], y[2], z[2];
  float fx, fy, fz;
  ref_axis(p[0], X, &x[0], &x[1], &fx);
  ref_axis(p[1], Y, &y[0], &y[1], &fy);
  ref_axis(p[2], Z, &z[0], &z[1], &fz);
  for (int c = 0; c < C; ++c) {
    float corner[2][2][2];
    for (int a = 0; a < 2; ++a)
      for (int b = 0; b < 2; ++b)
        for (int d = 0; d < 2; ++d) corner[a][b][d] = ref_decode<T>(rule, vol.at((((size_t)c * Z + z[a]) * Y + y[b]) * X + x[d]));
    float zs[2];
    for (int a = 0; a < 2; ++a) zs[a] = ref_lerp(ref_lerp(corner[a][0][0], corner[a][0][1], fx), ref_lerp(corner[a][1][0], corner[a][1][1], fx), fy);
    out[c] = ref_lerp(zs[0], zs[1], fz);
  }
}

static void ref_unit(float v[3]) {
  volatile float a = v[0] * v[0], b = v[1] * v[1], c = v[2] * v[2];
  volatile float ab = a + b;
  volatile float s = ab + c;
  const float len = std::sqrt(s);
  for (int k = 0; k < 3; ++k) {
    volatile float q = v[k] / len;
    v[k] = len > 0.0f ? (float)q : 0.0f;
  }
}

static float ref_dot(const float a[3], const float b[3]) {
  volatile float x = a[0] * b[0], y = a[1] * b[1], z = a[2] * b[2];
  volatile float xy = x + y;
  volatile float r = xy + z;
  return r;
}

static float ref_face_cos(const float* pa, const float* pb, const float* pc, const float* na, const float* nb, const float* nc) {
  float u[3], w[3], g[3], m[3];
  for (int k = 0; k < 3; ++k) {
    volatile float uk = pb[k] - pa[k], wk = pc[k] - pa[k], ab = na[k] + nb[k];
    volatile float mk = ab + nc[k];
    u[k] = uk, w[k] = wk, m[k] = mk;
  }
  for (int k = 0; k < 3; ++k) {
    const int i = (k + 1) % 3, j = (k + 2) % 3;
    volatile float a = u[i] * w[j], b = u[j] * w[i];
    volatile float d = a - b;
    g[k] = d;
  }
  volatile float q = ref_dot(g, g) * ref_dot(m, m);
  volatile float r = ref_dot(g, m) / std::sqrt(q);
  return r;
}

// ---- the runs -----------------------------------------------------------------------------------------------------------------------------------
static long g_runs = 0, g_differ = 0;

static std::vector<float> make_points(long Z, long Y, long X, int n, bool wild) {
  std::vector<float> p;
  const float hi[3] = {(float)(X - 1), (float)(Y - 1), (float)(Z - 1)};
  const float fixed[][3] = {{0, 0, 0}, {hi[0], hi[1], hi[2]}, {hi[0] + 0.5f, hi[1] - 0.5f, hi[2] + 0.25f}, {-0.5f, -0.75f, -3.0f},
                            {(float)X, (float)Y, (float)Z}, {-1e30f, 1e30f, 0.5f}, {0.25f, 0.5f, -1e30f}, {0.25f, 0.5f, 1e30f}};
  for (auto& f : fixed) p.insert(p.end(), f, f + 3);
  if (wild) {
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const float bad[][3] = {{nan, 0, 0}, {0, nan, 0}, {0, 0, nan}, {inf, -inf, 1}, {1, 1, inf}, {1, 1, -inf}, {3e9f, -3e9f, 3e9f}};
    for (auto& f : bad) p.insert(p.end(), f, f + 3);
  }
  for (long z = 0; z < Z; ++z) {      // whole z planes, fractional in the plane
    p.push_back(uniform(-1.5f, X + 0.5f)), p.push_back(uniform(-1.5f, Y + 0.5f)), p.push_back((float)z);
  }
  while ((int)p.size() < 3 * n) {
    p.push_back(uniform(-1.5f, X + 0.5f)), p.push_back(uniform(-1.5f, Y + 0.5f)), p.push_back(uniform(-1.5f, Z + 0.5f));
  }
  return p;
}

template <int RULE, typename T>
static void run_volume(int C, int Z, int Y, int X, bool wild) {
  std::vector<T> vol((size_t)C * Z * Y * X);
  for (auto& v : vol) {
    if (RULE == RX_MSP_COPY) v = (T)uniform(-4.0f, 4.0f);
    else v = (T)(rnd() % (RULE == RX_MSP_U8 ? 256 : 65536));
  }
  if (RULE == RX_MSP_COPY) {      // -0.0 and two denormals
    const uint32_t bits[3] = {0x80000000u, 1u, 0x8000085eu};
    for (int k = 0; k < 3 && k < (int)vol.size(); ++k) std::memcpy(&vol[(size_t)k * (vol.size() / 3)], &bits[k], 4);
  }
  const std::vector<float> pts = make_points(Z, Y, X, 60, wild);
  const long V = (long)pts.size() / 3;
  std::vector<float> want((size_t)V * C), got((size_t)V * C, -77.0f);
  for (long v = 0; v < V; ++v) ref_sample<T>(RULE, vol, C, Z, Y, X, &pts[3 * v], &want[(size_t)v * C]);
  // resident
  for (long v = 0; v < V; ++v)
    if (!msp_sample_point<RULE, T>(vol.data(), C, 0, Z, Z, Y, X, &pts[3 * v], false, &got[(size_t)v * C])) ++g_differ;
  ++g_runs;
  for (size_t i = 0; i < want.size(); ++i)
    if (!same_bits(want[i], got[i])) { ++g_differ; break; }
  // slabs of every depth, each a heap block of its own: [a, min(a + depth + 1, Z)) for a = 0, depth, .. below Z - 1
  for (int depth = 1; depth <= Z; ++depth) {
    std::vector<float> fill((size_t)V * C, -77.0f);
    std::vector<int> times(V, 0);
    for (int a = 0; a == 0 || a < Z - 1; a += depth) {
      const int planes = (a + depth + 1 < Z ? a + depth + 1 : Z) - a;
      std::vector<T> slab((size_t)C * planes * Y * X);
      for (int c = 0; c < C; ++c)
        std::memcpy(&slab[(size_t)c * planes * Y * X], &vol[((size_t)c * Z + a) * Y * X], (size_t)planes * Y * X * sizeof(T));
      for (long v = 0; v < V; ++v) times[v] += msp_sample_point<RULE, T>(slab.data(), C, a, planes, Z, Y, X, &pts[3 * v], false, &fill[(size_t)v * C]);
    }
    ++g_runs;
    bool bad = false;
    for (long v = 0; v < V; ++v) bad = bad || times[v] != 1;
    for (size_t i = 0; i < want.size(); ++i) bad = bad || !same_bits(want[i], fill[i]);
    if (bad) ++g_differ;
  }
  if (C == 3) {      // the unit epilogue
    ++g_runs;
    for (long v = 0; v < V; ++v) {
      float u[3] = {want[3 * v], want[3 * v + 1], want[3 * v + 2]}, o[3] = {-77.0f, -77.0f, -77.0f};
      ref_unit(u);
      msp_sample_point<RULE, T>(vol.data(), C, 0, Z, Z, Y, X, &pts[3 * v], true, o);
      if (!same_bits(u[0], o[0]) || !same_bits(u[1], o[1]) || !same_bits(u[2], o[2])) { ++g_differ; break; }
    }
  }
}

template <int RULE, typename T>
static void run_rule() {
  const int channels[3] = {1, 3, 8};
  for (int C : channels) run_volume<RULE, T>(C, 5, 6, 7, C == 3);
  run_volume<RULE, T>(3, 3, 9, 4, true);
  run_volume<RULE, T>(3, 1, 1, 1, true);
  run_volume<RULE, T>(2, 2, 1, 3, false);
}

static void run_faces() {
  std::vector<float> pos, vec;
  for (int i = 0; i < 64; ++i)
    for (int k = 0; k < 3; ++k) pos.push_back(uniform(-20.0f, 20.0f)), vec.push_back(i % 7 == 0 ? 0.0f : uniform(-1.0f, 1.0f));
  const float thresholds[3] = {0.0f, 0.2f, 0.9f};
  for (float min_cos : thresholds) {
    ++g_runs;
    bool bad = false;
    int seen[3] = {0, 0, 0};
    for (int t = 0; t < 400; ++t) {
      int64_t id[3] = {(int64_t)(rnd() % 64), (int64_t)(rnd() % 64), (int64_t)(rnd() % 64)};
      if (t % 9 == 0) id[2] = id[1];            // degenerate: g = 0
      if (t % 11 == 0) id[0] = id[1] = id[2] = 7 * (rnd() % 9);      // zero vectors at all corners, and degenerate
      if (t % 13 == 0) id[0] = 0, id[1] = 7, id[2] = 14;             // zero vectors, a proper triangle: m = 0
      const float want = ref_face_cos(&pos[3 * id[0]], &pos[3 * id[1]], &pos[3 * id[2]], &vec[3 * id[0]], &vec[3 * id[1]], &vec[3 * id[2]]);
      const float got = msp_face_cos(&pos[3 * id[0]], &pos[3 * id[1]], &pos[3 * id[2]], &vec[3 * id[0]], &vec[3 * id[1]], &vec[3 * id[2]]);
      const int side = want > min_cos ? 1 : (want < -min_cos ? -1 : 0);
      bad = bad || !(same_bits(want, got) || (std::isnan(want) && std::isnan(got))) || side != msp_side(got, min_cos);
      if ((t % 9 == 0 || t % 13 == 0) && !(std::isnan(got) && msp_side(got, min_cos) == 0)) bad = true;      // the rim rule
      ++seen[side + 1];
    }
    if (bad || !seen[0] || !seen[1] || !seen[2]) ++g_differ;
  }
  // the unit rule at its edges
  ++g_runs;
  float z[3] = {0.0f, -0.0f, 0.0f}, tiny[3] = {1e-30f, 0.0f, 0.0f}, v[3] = {3.0f, 0.0f, 4.0f};
  msp_unit(z), msp_unit(tiny), msp_unit(v);
  const float zero = 0.0f;
  if (!same_bits(z[0], zero) || !same_bits(z[1], zero) || !same_bits(tiny[0], zero) || v[0] != 3.0f / 5.0f || v[2] != 4.0f / 5.0f) ++g_differ;
}

int main() {
  run_rule<RX_MSP_COPY, float>();
  run_rule<RX_MSP_U8, uint8_t>();
  run_rule<RX_MSP_U16, uint16_t>();
  run_rule<RX_MSP_NORMAL_U16, uint16_t>();
  run_faces();
  std::printf("%ld runs, %ld differ from the direct restatement\n", g_runs, g_differ);
  return g_differ ? 1 : 0;
}
