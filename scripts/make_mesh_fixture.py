"""Regenerate tests/golden/mesh_slices.npz: the slices the REFERENCE's own `process_slice_points`
(tasks/normals/write_face_normals_final.py) and `process_slice_points_label` (tasks/normals/write_mesh_labels.py) paint for small
meshes, pinning tasks/normals/mesh_targets.py: slice_normals_numpy / slice_labels_numpy and, through them, the device pass.

    RX_REFERENCE_ROOT=<reference checkout> python scripts/make_mesh_fixture.py

Both files import `numba`, `open3d` and `tifffile` at module level (and call `set_num_threads`).  All three are stubbed: `jit` is
the identity decorator, so the two functions run as they are, as plain Python under this numpy (its version is recorded: the
contract is the reference's text under numpy, NOT under numba's typing).  The normals z is passed as the reference's `main()` passes
it, an np.int64 from np.arange; so is the labels z.

Recorded per case i: `vertices_i` float32 (n, 3), `triangles_i` int64 (m, 3), `normals_i` float32 (n, 3), `tri_labels_i` uint16 (m,),
`geom_i` int64 (w, h, z_first, n_slices), `img_i` uint16 (n_slices, h, w, 3), `viz_i` uint8 (n_slices, h, w, 3), `lab_i` uint16
(n_slices, h, w); `exp_factor`; `hits` / `hit_names`: how often each condition the cases were built for actually occurs (asserted
here against the minimum, and again by tests/test_mesh_targets_cpu.py).  Every case is at most 96 x 80 pixels, 400 triangles and
12 slices:
  0  a bumpy open sheet of 64 triangles with random unit normals in a 24 x 20 image;
  1  hand-placed triangles: vertices with integer z (the on-plane branch and its duplicate points), a triangle lying in a slice
     plane (3 points, 3 pairs), a flat edge off the plane, t inside the relaxed margins but outside [0, 1], ends that round outside
     the image, x.5 / y.5 coordinates (negative ones too), a one-step segment, opposite normals that cancel at t = 0.5, an empty slice;
  2  two sheets merged with a vertex offset, labels 1 and 2, crossing each other.
Needs the reference tree at generation time only."""
import importlib.util
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "mesh_slices.npz")
EXP_FACTOR = 1.5
MINIMUM = {"on_plane_vertex": 4, "duplicate_point": 2, "in_plane_triangle": 1, "flat_edge_off_plane": 1, "margin_t_normals": 1,
           "margin_t_labels": 1, "segment_dropped_normals": 1, "label_pixel_clipped": 1, "half_coordinate": 4,
           "negative_half_coordinate": 1, "one_step_segment": 1, "zero_norm_pixel": 1, "pixels_two_triangles": 50,
           "pixels_one_triangle_twice": 20, "two_label_values": 1, "empty_slice": 1}


def _load(ref_root, rel, name):
    sys.dont_write_bytecode = True
    numba = types.ModuleType("numba")
    numba.jit = lambda *a, **k: (a[0] if a and callable(a[0]) and not k else (lambda f: f))
    numba.prange = range
    numba.set_num_threads = lambda n: None
    o3d = types.ModuleType("open3d")
    sys.modules.update({"numba": numba, "open3d": o3d, "tifffile": types.ModuleType("tifffile")})
    spec = importlib.util.spec_from_file_location(name, os.path.join(ref_root, rel))
    mod = importlib.util.module_from_spec(spec)
    import contextlib
    import io
    with contextlib.redirect_stdout(io.StringIO()):
        spec.loader.exec_module(mod)
    return mod


def unit(rng, n):
    v = rng.standard_normal((n, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def sheet(rng, nu, nv, x0, x1, y_mid, z0, z1, bump, tilt=0.0):
    """an open (nu x nv)-vertex sheet: x along u, z along v, y wavy -> vertices, triangles"""
    u, v = np.meshgrid(np.arange(nu), np.arange(nv), indexing="ij")
    x = x0 + (x1 - x0) * u / (nu - 1) + rng.uniform(-0.3, 0.3, u.shape)
    y = y_mid + bump * np.sin(0.9 * u + 0.5 * v) + tilt * (u - nu / 2) + rng.uniform(-0.3, 0.3, u.shape)
    z = z0 + (z1 - z0) * v / (nv - 1) + rng.uniform(-0.2, 0.2, u.shape)
    verts = np.stack([x, y, z], axis=-1).reshape(-1, 3).astype(np.float32)
    tris = []
    for i in range(nu - 1):
        for j in range(nv - 1):
            a, b, c, d = i * nv + j, (i + 1) * nv + j, (i + 1) * nv + j + 1, i * nv + j + 1
            tris += [[a, b, c], [a, c, d]]
    return verts, np.asarray(tris, np.int64)


def cases():
    """(vertices, triangles, normals, tri_labels, w, h, z_first, n_slices)"""
    out = []
    rng = np.random.default_rng(20240611)
    v, t = sheet(rng, 9, 5, 2.0, 22.0, 10.0, 0.4, 5.6, 3.0)
    out.append((v, t, unit(rng, len(v)), np.ones(len(t), np.uint16), 24, 20, 0, 7))

    V, T, N = [], [], []

    def tri(p0, p1, p2, n0=None, n1=None, n2=None):
        k = len(V)
        V.extend([p0, p1, p2])
        T.append([k, k + 1, k + 2])
        for n in (n0, n1, n2):
            N.append(unit(rng, 1)[0] if n is None else np.asarray(n, np.float32))
    tri((5, 5, 2), (15, 6, 1.2), (9, 12, 3.7))                       # a vertex on slice 2: the on-plane branch twice, a duplicate point
    tri((30, 5, 1), (36, 9, 3), (31, 12, 2))                         # vertices on slices 1, 2 and 3
    tri((2.5, 3.5, 3), (10.5, 4.5, 3), (-0.5, 8.5, 3))               # lies in slice 3: 3 points, 3 pairs; .5 coordinates, one negative
    tri((20, 20, 1.5), (27, 22, 1.5), (23, 28, 4))                   # a flat edge off the planes
    tri((14, 24, 2.004), (20, 29, 3.5), (12, 30, 1.0))               # slice 2: t = -0.0027 on the first edge (normals margin)
    tri((3, 14, 2.0005), (8, 18, 3.5), (2, 20, 1.0))                 # slice 2: t = -0.0003 (inside the labels margin too)
    tri((-4, 12, 0.5), (6, 15, 2.5), (1, 11, 1.4))                   # crosses the left border: an end rounds to x < 0
    tri((36, 28, 0.6), (44, 30, 2.6), (38, 33.5, 1.7))               # crosses the right and the bottom border
    tri((1.5, 25.5, 1), (-1.5, 27.5, 1), (0.5, 29.5, 2))             # x.5 / y.5 ends on slice 1, negative ones: round half to even
    tri((20.1, 10.1, 1.6), (20.3, 10.2, 2.4), (20.2, 10.4, 2.6))     # both points in one pixel: a segment of one step
    tri((25, 15, 4), (29, 15, 4), (27, 19, 5.5), (0, 0, 1), (0, 0, -1), (1, 0, 0))      # opposite normals: zero at t = 0.5 of 9 steps
    out.append((np.asarray(V, np.float32), np.asarray(T, np.int64), np.asarray(N, np.float32), np.ones(len(T), np.uint16), 40, 32, 0, 8))

    va, ta = sheet(rng, 12, 6, 4.0, 90.0, 30.0, 0.3, 9.7, 6.0, tilt=2.0)
    vb, tb = sheet(rng, 12, 6, 6.0, 92.0, 42.0, 0.2, 9.6, 5.0, tilt=-2.5)
    v = np.vstack([va, vb])
    t = np.vstack([ta, tb + len(va)])
    lab = np.concatenate([np.full(len(ta), 1, np.uint16), np.full(len(tb), 2, np.uint16)])
    out.append((v, t, unit(rng, len(v)), lab, 96, 80, 0, 12))
    return out


def count_hits(M, case, img, lab_img):
    """how often each condition occurs in one case (M: tasks/normals/mesh_targets.py)"""
    v, t, n, lab, w, h, z0, nz = case
    hits = dict.fromkeys(MINIMUM, 0)
    f32 = np.float32
    for k in range(nz):
        z = z0 + k
        zf = f32(z)
        owners, own_count = {}, {}
        for ti, tr in enumerate(t):
            zs = v[tr, 2]
            if not (zs.min() <= zf <= zs.max()):
                continue
            on = int((zs == zf).sum())
            hits["on_plane_vertex"] += on
            hits["in_plane_triangle"] += on == 3
            cand = 0
            for a, b in ((0, 1), (1, 2), (2, 0)):
                s, e = v[tr[a]], v[tr[b]]
                p, _ = M._edge_point_normals(s, e, n[tr[a]], n[tr[b]], zf)
                cand += p is not None
                if s[2] != zf and e[2] != zf:
                    if abs(e[2] - s[2]) <= f32(1e-8):
                        hits["flat_edge_off_plane"] += 1
                    else:
                        tt = (zf - s[2]) / (e[2] - s[2])
                        hits["margin_t_normals"] += bool((f32(-0.01) <= tt < 0) or (1 < tt <= f32(1.01)))
                        td = (np.float64(z) - np.float64(s[2])) / np.float64(e[2] - s[2])
                        hits["margin_t_labels"] += bool((-1e-3 <= td < 0) or (1 < td <= 1 + 1e-3))
                for c in (s[0], s[1]):
                    if s[2] == zf and float(c) % 1 == 0.5:
                        hits["half_coordinate"] += 1
                        hits["negative_half_coordinate"] += c < 0
            segs = M._tri_segments_normals(v, n, tr, zf, w, h)
            pts = M._tri_points_labels(v, tr, np.int64(z))
            npairs = {0: 0, 1: 0, 2: 1, 3: 3}
            hits["duplicate_point"] += cand - len(pts) if cand > len(pts) else 0
            hits["segment_dropped_normals"] += npairs[len(pts)] - len(segs) if npairs[len(pts)] > len(segs) else 0
            hits["one_step_segment"] += sum(M._segment_steps(*s[1:5]) == 1 for s in segs)
            for i in range(len(pts)):
                for j in range(i + 1, len(pts)):
                    hits["label_pixel_clipped"] += sum(not (0 <= x < w and 0 <= y < h) for x, y in M._label_line(pts[i], pts[j]))
        for ti, pair, step, e, x, y, rgb in M._normals_events(v, t, n, z, w, h, EXP_FACTOR):
            owners.setdefault((x, y), set()).add(ti)
            own_count[(x, y, ti)] = own_count.get((x, y, ti), 0) + 1
        hits["pixels_two_triangles"] += sum(len(s) >= 2 for s in owners.values())
        hits["pixels_one_triangle_twice"] += len({(x, y) for (x, y, ti), c in own_count.items() if c >= 2})
        hits["zero_norm_pixel"] += int((img[k] == 32767).all(axis=2).sum())
        hits["empty_slice"] += not img[k].any() and not lab_img[k].any()
        hits["two_label_values"] += len(np.unique(lab_img[k][lab_img[k] > 0])) >= 2
    return hits


def main():
    ref_root = os.environ.get("RX_REFERENCE_ROOT")
    if not ref_root:
        sys.exit("set RX_REFERENCE_ROOT to the reference checkout")
    sys.path.insert(0, ROOT)
    import mt3d_amd  # noqa: F401
    from mt3d_amd.tasks.normals import mesh_targets as M
    ref_n = _load(ref_root, os.path.join("tasks", "normals", "write_face_normals_final.py"), "ref_face_normals")
    ref_l = _load(ref_root, os.path.join("tasks", "normals", "write_mesh_labels.py"), "ref_mesh_labels")
    arrays, total = {}, dict.fromkeys(MINIMUM, 0)
    all_cases = cases()
    for i, case in enumerate(all_cases):
        v, t, n, lab, w, h, z0, nz = case
        assert w <= 96 and h <= 80 and len(t) <= 400 and nz <= 12
        zs = np.arange(z0, z0 + nz)                                    # np.int64, as in the reference's main()
        img = np.zeros((nz, h, w, 3), np.uint16)
        viz = np.zeros((nz, h, w, 3), np.uint8)
        lab_img = np.zeros((nz, h, w), np.uint16)
        for k, z in enumerate(zs):
            img[k], viz[k] = ref_n.process_slice_points(v, t, n, z, w, h, EXP_FACTOR)
            lab_img[k] = ref_l.process_slice_points_label(v, t.astype(np.int32), lab, z, w, h)
        hits = count_hits(M, case, img, lab_img)
        print(f"case {i}: {len(t)} triangles, {w} x {h} x {nz}; painted normals pixels per slice",
              [int(s.any(axis=2).sum()) for s in img], "labels", [int((s > 0).sum()) for s in lab_img])
        for k in total:
            total[k] += int(hits[k])
        arrays.update({f"vertices_{i}": v, f"triangles_{i}": t, f"normals_{i}": n, f"tri_labels_{i}": lab,
                       f"geom_{i}": np.array([w, h, z0, nz], np.int64), f"img_{i}": img, f"viz_{i}": viz, f"lab_{i}": lab_img})
    for k, need in MINIMUM.items():
        print(f"  {k:28s} {total[k]:6d}  (at least {need})")
        assert total[k] >= need, (k, total[k], need)
    names = sorted(MINIMUM)
    arrays["hit_names"] = np.array(names, dtype="U32")
    arrays["hits"] = np.array([total[k] for k in names], np.int64)
    arrays["hit_minimum"] = np.array([MINIMUM[k] for k in names], np.int64)
    arrays["n_cases"] = np.array(len(all_cases), np.int64)
    arrays["exp_factor"] = np.array(EXP_FACTOR, np.float64)
    arrays["numpy_version"] = np.array(np.__version__, dtype="U16")
    np.savez_compressed(OUT, **arrays)
    size = os.path.getsize(OUT)
    print(OUT, size, "bytes")
    assert size < 256 * 1024


if __name__ == "__main__":
    main()
