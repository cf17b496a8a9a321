"""The meshes and cells of the mesh-decimation tests, shared by the CPU tests (the statement's properties), the GPU tests
(ops.mesh_decimate against the statement) and, restated in C++, csrc/tools/meshdecimate_host_check.cpp.  Each is chosen for a way the
kernels can go wrong:

  grid at integer coordinates, cell 1 and 2     vertices sit exactly on cell faces: floor(p / cell) must put them in the upper cell
  the same grid at negative coordinates         floor and truncation differ there
  cell 0.75, 3.5, and one that holds everything a cell that is no divisor of the spacing; one cluster, so an empty result
  a cell below the vertex spacing               every cluster is one vertex: the identity on referenced vertices
  fan(3000) inside one cell, and in 64 cells    one member list of 3001 entries (sorted in place in global memory); lists of about 50
  soup and awkward                              repeated ids within a triangle, repeated triangles, unreferenced vertices
  a two-sided slab thinner than the cell        the two faces merge: opposite-winding duplicates, the lowest index wins
  the surface-nets ball, and a shuffle of it    a closed manifold; the triangle order must not change the vertices
  a 300 x 300 grid                              90000 vertices, no multiple of 256: scans and table cross many workgroups"""
import numpy as np

import mesh_refine_cases as R

F32 = np.float32
BIG = (300, 300)
REPRESENTATIVES = ("mean", "nearest")


def shifted(mesh, by):
    v, t = mesh
    return (v + np.asarray(by, F32)).astype(F32), t


def fan_in_one_cell(degree=3000):
    """`fan(degree)` scaled into (0.1, 0.9)^3: one cluster at cell 1.0"""
    v, t = R.fan(degree)
    return (v * F32(0.004) + F32(0.5)).astype(F32), t


def slab(ny=5, nx=7, gap=0.25):
    """two copies of the grid patch `gap` apart, the upper one with the opposite winding: a sheet with two faces"""
    v, t = R.grid_patch(ny, nx, 3.0)
    w, _ = R.grid_patch(ny, nx, 3.0 + gap)
    return np.concatenate([v, w]).astype(F32), np.concatenate([t, t[:, ::-1] + len(v)]).astype(np.int64)


_CASES = None


def cases():
    """[(id, vertices float32 (V, 3), triangles int64 (T, 3), cell)].  Built once."""
    global _CASES
    if _CASES is None:
        grid, neg = R.grid_patch(), shifted(R.grid_patch(), (-6.0, -4.0, -4.0))      # x -6 .. 0, y -4 .. 0, z -1
        ball = R.ball_mesh()
        out = [("grid-c1", grid, 1.0), ("grid-c2", grid, 2.0), ("grid-neg-c1", neg, 1.0), ("grid-neg-c2", neg, 2.0),
               ("grid-c0.75", grid, 0.75), ("grid-neg-c3.5", neg, 3.5), ("grid-one-cluster", grid, 64.0), ("grid-fine", grid, 0.25),
               ("fan3000-one-cell", fan_in_one_cell(), 1.0), ("fan3000-c50", R.fan(3000), 50.0),
               ("soup257-c3.5", R.soup(257), 3.5), ("soup257-c60", R.soup(257), 60.0), ("soup2100-c40", R.soup(2100), 40.0),
               ("awkward-c50", R.awkward(), 50.0), ("awkward-fine", R.awkward(), 0.01),
               ("slab-c1", slab(), 1.0), ("slab-c2", slab(), 2.0),
               ("ball-c0.75", ball, 0.75), ("ball-c2", ball, 2.0), ("ball-c3.5", ball, 3.5),
               ("ball-shuffled-c2", R.shuffled(*ball), 2.0),
               ("no-triangles", (R._positions(5, 9), np.zeros((0, 3), np.int64)), 30.0),
               ("big-grid-c2", R.grid_patch(*BIG), 2.0), ("big-grid-fine", R.grid_patch(*BIG), 0.5)]
        _CASES = [(name, v, t, cell) for name, (v, t), cell in out]
    return _CASES


def case(name):
    return next(c for c in cases() if c[0] == name)


def unordered(triangles):
    """the rows sorted within, as a sorted list of tuples"""
    return sorted(map(tuple, np.sort(np.asarray(triangles), axis=1).tolist()))


def decimate_plain(vertices, triangles, cell, representative):
    """a plain Python restatement with dicts and loops (float32 scalars, one operation at a time)"""
    c = F32(cell)
    keys, clusters, cluster_of = {}, [], []
    for i, p in enumerate(vertices):
        k = tuple(int(np.floor(x / c)) for x in p)
        if k not in keys:
            keys[k] = len(clusters)
            clusters.append((k, []))
        clusters[keys[k]][1].append(i)
        cluster_of.append(keys[k])
    reps = []
    for k, members in clusters:
        if representative == "mean":
            s = [F32(0), F32(0), F32(0)]
            for m in members:
                s = [s[j] + vertices[m][j] for j in range(3)]
            reps.append([s[j] / F32(len(members)) for j in range(3)])
        else:
            best = None
            for m in members:
                dx = [vertices[m][j] - (F32(k[j]) + F32(0.5)) * c for j in range(3)]
                d = dx[0] * dx[0] + dx[1] * dx[1] + dx[2] * dx[2]
                if best is None or d < best[0]:
                    best = (d, m)
            reps.append(list(vertices[best[1]]))
    seen, kept = set(), []
    for tri in triangles.tolist():
        ct = [cluster_of[i] for i in tri]
        if len(set(ct)) == 3 and tuple(sorted(ct)) not in seen:
            seen.add(tuple(sorted(ct)))
            kept.append(ct)
    used = sorted({c for tri in kept for c in tri})
    row = {c: i for i, c in enumerate(used)}
    return (np.array([reps[c] for c in used], F32).reshape(-1, 3), np.array([[row[c] for c in tri] for tri in kept], np.int64).reshape(-1, 3),
            np.array(cluster_of, np.int64))
