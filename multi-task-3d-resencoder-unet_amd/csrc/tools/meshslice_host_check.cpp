// meshslice_host_check.cpp -- runs the arithmetic of the mesh slicing pass (../rx_meshslice_core.h, the functions the kernels of
// ../rx_meshslice.hip call) on the CPU over the cases of a dump written by tests/test_mesh_targets_cpu.py and compares every pixel
// with tasks/normals/mesh_targets.py: slice_normals_numpy (and its viz bytes) and slice_labels_numpy, bit for bit.  Built by that test
// with -fsanitize=address,undefined: vertices, triangles, keys and images sit in heap buffers of exactly their size, so an index
// that left one would be reported.  Each slice is made the way the device makes it -- every triangle scatters its order keys with
// a maximum, then every pixel is resolved from its key alone -- and, for the normals, also painted serially as the statement does.
//
//   dump := int32 n_cases, then per case: int32 nv, nt, w, h, z0, nz; double exp_factor; float vertices[3 nv]; int32 triangles[3 nt];
//           float normals[3 nv]; int32 tri_labels[nt]; uint16 img[nz h w 3]; uint8 viz[nz h w 3]; uint16 lab[nz h w]
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../rx_meshslice_core.h"

static void load_tri(const std::vector<float>& vertices, const std::vector<float>& normals, const std::vector<int>& tris, long t, float v[3][3],
                     float n[3][3]) {
  for (int c = 0; c < 3; ++c)
    for (int k = 0; k < 3; ++k) {
      v[c][k] = vertices.at(3 * (size_t)tris.at(3 * t + c) + k);
      n[c][k] = normals.at(3 * (size_t)tris.at(3 * t + c) + k);
    }
}

int main(int argc, char** argv) {
  if (argc != 2) return fprintf(stderr, "usage: %s dump\n", argv[0]), 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return perror(argv[1]), 2;
  int n_cases = 0;
  if (fread(&n_cases, 4, 1, f) != 1) return fprintf(stderr, "empty dump\n"), 2;
  long bad_total = 0;
  for (int ci = 0; ci < n_cases; ++ci) {
    int hd[6];
    double exp_factor;
    if (fread(hd, 4, 6, f) != 6 || fread(&exp_factor, 8, 1, f) != 1) return fprintf(stderr, "case %d: short header\n", ci), 2;
    const int nv = hd[0], nt = hd[1], w = hd[2], h = hd[3], z0 = hd[4], nz = hd[5];
    if (nv < 1 || nt < 0 || w < 1 || h < 1 || nz < 1) return fprintf(stderr, "case %d: bad sizes\n", ci), 2;
    const size_t npix = (size_t)nz * h * w;
    std::vector<float> vertices(3 * (size_t)nv), normals(3 * (size_t)nv);
    std::vector<int> tris(3 * (size_t)nt), labels((size_t)nt);
    std::vector<uint16_t> want(3 * npix), want_lab(npix), got(3 * npix), serial(3 * npix), got_lab(npix);
    std::vector<uint8_t> want_viz(3 * npix), got_viz(3 * npix);
    if (fread(vertices.data(), 4, vertices.size(), f) != vertices.size() || fread(tris.data(), 4, tris.size(), f) != tris.size() ||
        fread(normals.data(), 4, normals.size(), f) != normals.size() || fread(labels.data(), 4, labels.size(), f) != labels.size() ||
        fread(want.data(), 2, want.size(), f) != want.size() || fread(want_viz.data(), 1, want_viz.size(), f) != want_viz.size() ||
        fread(want_lab.data(), 2, want_lab.size(), f) != want_lab.size())
      return fprintf(stderr, "case %d: short data\n", ci), 2;
    for (int i : tris)
      if (i < 0 || i >= nv) return fprintf(stderr, "case %d: vertex index %d\n", ci, i), 2;
    const double eff = exp_factor * 1.2;
    const int n_exp = (int)(4.0 * eff + 1.0);
    if (n_exp < 2 || n_exp > RX_MS_MAX_SAMPLES) return fprintf(stderr, "case %d: %d samples\n", ci, n_exp), 2;
    std::vector<uint64_t> keys(npix, 0);
    std::vector<uint32_t> lkeys(npix, 0);
    // ---- scatter: what mesh_keys_normals_kernel / mesh_keys_labels_kernel do per triangle -----------------------------------------
    for (long t = 0; t < nt; ++t) {
      float v[3][3], n[3][3];
      load_tri(vertices, normals, tris, t, v, n);
      for (int zi = 0; zi < nz; ++zi) {
        const int z = z0 + zi;
        const size_t plane = (size_t)zi * h * w;
        RxMsPoint pts[3];
        int np = rx_ms_tri_points_normals(v, n, (float)z, pts);
        for (int pair = 0; pair < rx_ms_num_pairs(np); ++pair) {
          int i, j, x0, y0, x1, y1;
          rx_ms_pair(pair, &i, &j);
          if (!rx_ms_segment(&pts[i], &pts[j], w, h, &x0, &y0, &x1, &y1)) continue;
          const int steps = rx_ms_steps(x0, y0, x1, y1);
          if (steps >= RX_MS_MAX_STEPS) return fprintf(stderr, "case %d: %d steps\n", ci, steps), 2;
          for (int step = 0; step < steps; ++step) {
            double x, y;
            float nn[3];
            rx_ms_step_state(x0, y0, x1, y1, pts[i].n, pts[j].n, steps, step, &x, &y, nn);
            for (int e = 0; e < n_exp; ++e) {
              const float off = rx_ms_exp_offset(e, n_exp, eff);
              const int px = rx_ms_exp_pixel(x, off, nn[0]), py = rx_ms_exp_pixel(y, off, nn[1]);
              if (px < 0 || px >= w || py < 0 || py >= h) continue;
              const size_t q = plane + (size_t)py * w + px;
              const uint64_t k = rx_ms_key(t, pair, step, e);
              if (k > keys.at(q)) keys.at(q) = k;
              for (int c = 0; c < 3; ++c) serial.at(3 * q + c) = rx_ms_code(nn[c]);      // the statement's way: the last writer stays
            }
          }
        }
        np = rx_ms_tri_points_labels(v, z, pts);
        for (int pair = 0; pair < rx_ms_num_pairs(np); ++pair) {
          int i, j;
          rx_ms_pair(pair, &i, &j);
          RxMsDda d = rx_ms_dda(pts[i].x, pts[i].y, pts[j].x, pts[j].y);
          for (int s = 0; s <= d.steps; ++s) {
            const int px = rx_ms_rint(d.x), py = rx_ms_rint(d.y);
            rx_ms_dda_next(&d);
            if (px < 0 || px >= w || py < 0 || py >= h) continue;
            const size_t q = plane + (size_t)py * w + px;
            if ((uint32_t)(t + 1) > lkeys.at(q)) lkeys.at(q) = (uint32_t)(t + 1);
          }
        }
      }
    }
    // ---- resolve: what mesh_resolve_normals_kernel / mesh_resolve_labels_kernel do per key ----------------------------------------
    for (size_t q = 0; q < npix; ++q) {
      const uint64_t k = keys[q];
      if (k != 0) {
        const long t = rx_ms_key_tri(k);
        const int z = z0 + (int)(q / ((size_t)h * w)), pair = rx_ms_key_pair(k), step = rx_ms_key_step(k);
        float v[3][3], n[3][3];
        load_tri(vertices, normals, tris, t, v, n);
        RxMsPoint pts[3];
        const int np = rx_ms_tri_points_normals(v, n, (float)z, pts);
        int i, j, x0, y0, x1, y1;
        rx_ms_pair(pair, &i, &j);
        if (pair >= rx_ms_num_pairs(np) || !rx_ms_segment(&pts[i], &pts[j], w, h, &x0, &y0, &x1, &y1))
          return fprintf(stderr, "case %d: key of pixel %zu names no segment\n", ci, q), 2;
        const int steps = rx_ms_steps(x0, y0, x1, y1);
        double x, y;
        float nn[3];
        rx_ms_step_state(x0, y0, x1, y1, pts[i].n, pts[j].n, steps, step, &x, &y, nn);
        for (int c = 0; c < 3; ++c) got.at(3 * q + c) = rx_ms_code(nn[c]);
      }
      for (int c = 0; c < 3; ++c) got_viz.at(3 * q + c) = rx_ms_viz(got.at(3 * q + c));
      got_lab.at(q) = lkeys[q] ? (uint16_t)(labels.at(lkeys[q] - 1) & 0xFFFF) : 0;
    }
    long bad = 0, bad_serial = 0, bad_viz = 0, bad_lab = 0;
    for (size_t q = 0; q < 3 * npix; ++q) bad += got[q] != want[q], bad_serial += serial[q] != want[q], bad_viz += got_viz[q] != want_viz[q];
    for (size_t q = 0; q < npix; ++q) bad_lab += got_lab[q] != want_lab[q];
    if (bad || bad_serial || bad_viz || bad_lab)
      printf("case %d (%d triangles, %d x %d x %d): differ: %ld codes by key, %ld codes painted serially, %ld viz bytes, %ld labels\n", ci, nt, w, h,
             nz, bad, bad_serial, bad_viz, bad_lab);
    bad_total += bad + bad_serial + bad_viz + bad_lab;
  }
  fclose(f);
  printf("%d cases, %ld values differ\n", n_cases, bad_total);
  return bad_total ? 1 : 0;
}
