"""The small meshes of the mesh-refinement tests, shared by the CPU tests (the statements' invariants), the GPU tests (ops.mesh_* against
the statements) and, restated in C++, csrc/tools/meshrefine_host_check.cpp.  Each is chosen for a way the kernels can go wrong.

The kernels run a thread per vertex or per triangle in workgroups of 256 and scan 1024 values per workgroup, so the vertex counts
cross a wave (63, 64, 65), a workgroup (257) and two scan groups (2100); a vertex's lists live in global memory and are heap-sorted
in place, so the fans go far past anything a thread could keep in registers or LDS."""
import numpy as np

import isosurface_cases as I
from mesh_cases import BALL, GRID, ball_mesh, fan, grid_patch, shuffled, soup      # noqa: F401 -- the generic builders, reached as R.NAME
from mesh_cases import positions as _positions

F32 = np.float32
SCAN_GROUP = 1024      # csrc/rx_meshrefine.hip: RX_MR_SCAN_GROUP
COUNTS = (1, 63, 64, 65, 257, 2 * SCAN_GROUP + 52)
FANS = (3, 8, 9, 300, 3000)


def grid_interior(ny=GRID[0], nx=GRID[1]):
    j, i = np.indices((ny, nx))
    return ((j > 0) & (j < ny - 1) & (i > 0) & (i < nx - 1)).ravel()


def awkward():
    """vertex 3 isolated; vertex 4 only in a degenerate triangle; (5, 5, 6) repeats an id; (0, 1, 2) appears twice and two more
    triangles use its edge (0, 1), which so has multiplicity 4; three triangles on the edge (7, 8); the last id, V - 1 = 12, in use"""
    t = np.array([[0, 1, 2], [0, 1, 2], [4, 4, 4], [5, 5, 6], [7, 8, 9], [7, 8, 10], [8, 7, 11], [12, 0, 9], [1, 0, 6], [0, 1, 9]], np.int64)
    return _positions(13, 5), t


def closed_meshes():
    """the surface-nets meshes of a few volumes of tests/isosurface_cases.py: closed, not always manifold, degrees from 3 to 12 and more"""
    import mt3d_amd.postprocess as pp
    out = [("ball", ball_mesh())]
    for shape, kind in (((9, 10, 12), "random50"), ((9, 10, 12), "checkerboard"), ((33, 17, 70), "slab"), ((5, 1, 3), "full")):
        out.append((f"{'x'.join(map(str, shape))}-{kind}", pp.surface_nets_numpy(dict(I.volumes(shape, 127))[kind], 127)))
    return out


_CASES = None


def cases():
    """[(id, vertices float32 (V, 3), triangles int64 (T, 3))]: every case, then every case once more shuffled.  Built once."""
    global _CASES
    if _CASES is None:
        base = closed_meshes() + [("grid", grid_patch()), ("awkward", awkward())]
        base += [(f"soup{n}", soup(n)) for n in COUNTS] + [(f"fan{d}", fan(d)) for d in FANS]
        base.append(("no-triangles", (_positions(5, 9), np.zeros((0, 3), np.int64))))
        _CASES = [(name, v, t) for name, (v, t) in base] + [(name + "-shuffled",) + shuffled(v, t) for name, (v, t) in base]
    return _CASES


def adjacency_sets(n_vertices, triangles):
    """a plain Python restatement: (list of neighbour sets, boundary flags)"""
    nbr, uses = [set() for _ in range(n_vertices)], {}
    for tri in triangles.tolist():
        for k in range(3):
            a, b = tri[k], tri[(k + 1) % 3]
            if a != b:
                nbr[a].add(b)
                nbr[b].add(a)
                uses[(min(a, b), max(a, b))] = uses.get((min(a, b), max(a, b)), 0) + 1
    boundary = np.zeros(n_vertices, np.uint8)
    for (a, b), n in uses.items():
        if n == 1:
            boundary[a] = boundary[b] = 1
    return nbr, boundary


def enclosed_volume(vertices, triangles):
    p = vertices[triangles].astype(np.float64)
    return float(np.einsum("ij,ij->i", p[:, 0], np.cross(p[:, 1], p[:, 2])).sum() / 6)
