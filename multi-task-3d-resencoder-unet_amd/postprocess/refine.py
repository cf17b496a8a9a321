"""Refinement of an extracted triangle mesh: the numpy statements of csrc/rx_meshrefine.hip (a canonical vertex adjacency, Taubin
smoothing, area-weighted vertex normals), the config block and the `MeshRefiner` driver (files: mesh_io.py; the driver's skeleton:
stage.py).

Surface nets place one vertex per cell from 8-bit crossings, so a sheet comes out terraced, and the mesh file carries no normals.
Taubin smoothing (a pass with a positive factor, then one with a slightly larger negative factor) removes the terraces without the
shrinkage of a plain Laplacian; the normals are those of the smoothed mesh.

Everything is a property of the mesh alone.  The neighbours of a vertex are taken in ascending id and the triangles at a vertex in
ascending index, every float32 operation is one rounding in the order written here, and the kernels reproduce that: results compare
with array_equal, floats by their bits.  The statements use numpy only."""
import numpy as np

from .mesh_io import F32, _check_mesh, _check_triangles, gather_sum
from .stage import MeshStage, parse_stage_block

F32_MAX = float(np.finfo(np.float32).max)      # a factor or a clamp must be finite as a float32
KEY = "inference_config.postprocess.refine"
# device memory of a resident run, MeshRefiner.scratch_bytes: per vertex the input, two ping-pong buffers and the normals (4 x 12),
# corner counts, fill cursors and degrees (3 x 4), two offset columns (2 x 8) and the boundary flag (1); per triangle its ids (24),
# its three corner slots (3 x 4 triangle index + 3 x 8 edge partners), the compact neighbours (at most 6 x 4) and its face vector (12)
BYTES_PER_VERTEX = 77
BYTES_PER_TRIANGLE = 96
BYTES_FIXED = 24      # the last word of either offset column, the two flags


def scratch_bytes(n_vertices, n_triangles):
    """device bytes of a resident refinement of a mesh of `n_vertices` vertices and `n_triangles` triangles, inputs and outputs included"""
    return BYTES_PER_VERTEX * int(n_vertices) + BYTES_PER_TRIANGLE * int(n_triangles) + BYTES_FIXED


# ---- the statements ---------------------------------------------------------------------------------------------------------------------------
def adjacency_numpy(n_vertices, triangles):
    """-> (offsets int64[V + 1], neighbours int64[E], boundary uint8[V]): the neighbours of v are neighbours[offsets[v]:offsets[v + 1]],
    the distinct vertices that share a triangle edge with v, ascending.  A triangle (a, b, c) has the edge slots (a, b), (b, c),
    (c, a); a slot whose two ids are equal contributes nothing, so a triangle with a repeated id uses its one remaining edge twice.
    boundary[v] = 1 when some edge at v is used by exactly one slot over all triangles (three or more uses are not boundary).  The
    result depends neither on the order of the triangles nor on the order of the ids within one."""
    t = _check_triangles("adjacency_numpy", n_vertices, triangles)
    V = int(n_vertices)
    a, b = t[:, [0, 1, 2]].ravel(), t[:, [1, 2, 0]].ravel()
    keep = a != b
    u, w = np.concatenate([a[keep], b[keep]]), np.concatenate([b[keep], a[keep]])      # every slot seen from either end
    pairs, uses = np.unique(u * max(V, 1) + w, return_counts=True)      # ascending (u, w); below 2^62
    pu, pw = pairs // max(V, 1), pairs % max(V, 1)
    offsets = np.concatenate([[0], np.cumsum(np.bincount(pu, minlength=V))]).astype(np.int64)
    boundary = np.zeros(V, np.uint8)
    boundary[pu[uses == 1]] = 1
    return offsets, pw.astype(np.int64), boundary


def corner_faces_numpy(n_vertices, triangles):
    """-> (face_offsets int64[V + 1], faces int64[3T]): the triangles of the corners at v, ascending (a triangle with a repeated id
    appears once per corner)"""
    t = _check_triangles("corner_faces_numpy", n_vertices, triangles)
    corner = t.ravel()
    order = np.argsort(corner, kind="stable")      # the corners lie in triangle order already
    offsets = np.concatenate([[0], np.cumsum(np.bincount(corner, minlength=int(n_vertices)))]).astype(np.int64)
    return offsets, (order // 3).astype(np.int64)


def _options(fn, iterations, lam, mu, clamp, key=None):
    name = (lambda k: f"{key}.{k}") if key else (lambda k: f"{fn}: {k}")
    if isinstance(iterations, bool) or not isinstance(iterations, (int, np.integer)) or int(iterations) < 0:
        raise ValueError(f"{name('iterations')} {iterations!r} (an integer >= 0)")
    for k, x, optional in (("lambda" if key else "lam", lam, False), ("mu", mu, True)):
        if x is None and optional:
            continue
        if isinstance(x, bool) or not isinstance(x, (int, float, np.integer, np.floating)) or not abs(float(x)) <= F32_MAX:
            raise ValueError(f"{name(k)} {x!r} (a finite number)")
    if clamp is not None and (isinstance(clamp, bool) or not isinstance(clamp, (int, float, np.integer, np.floating))
                              or not 0 <= float(clamp) <= F32_MAX):
        raise ValueError(f"{name('clamp')} {clamp!r} (a finite number >= 0, or None)")
    factors = [F32(lam)] if mu is None else [F32(lam), F32(mu)]
    return int(iterations), factors, None if clamp is None else F32(clamp)


def smooth_numpy(vertices, triangles, iterations, lam=0.5, mu=-0.53, clamp=None, pin_boundary=True, adjacency=None):
    """Taubin smoothing -> float32 (V, 3).  Every iteration is one pass with factor `lam`, then one with `mu` (`mu=None`: `lam`
    passes only, the plain Laplacian).  A pass reads the positions before it and writes new ones; for a vertex of degree d > 0 that is
    not pinned, per component and in float32 with one rounding per operation: s = the sequential sum of the neighbours' positions in
    ascending id (from 0), m = s / float32(d), q = p + f * (m - p) as three operations, and with `clamp` = c then q = lo where
    q < lo, hi where q > hi, with lo = p0 - c and hi = p0 + c of the input position p0.  Vertices of degree 0 and, with
    `pin_boundary`, boundary vertices do not move."""
    p0, t = _check_mesh("smooth_numpy", vertices, triangles)
    iterations, factors, c = _options("smooth_numpy", iterations, lam, mu, clamp)
    offsets, nbr, boundary = adjacency_numpy(len(p0), t) if adjacency is None else adjacency
    deg = np.diff(offsets)
    moving = np.nonzero((deg > 0) & ~(boundary.astype(bool) & bool(pin_boundary)))[0]
    d = deg[moving].astype(F32)[:, None]
    if c is not None:
        lo, hi = p0[moving] - c, p0[moving] + c
    p = p0.copy()
    for _ in range(iterations):
        for f in factors:
            s = gather_sum(p, offsets, nbr, moving)
            here = p[moving]
            m = s / d
            q = here + f * (m - here)
            if c is not None:
                q = np.where(q < lo, lo, q)
                q = np.where(q > hi, hi, q)
            p = p.copy()
            p[moving] = q
    return p


def vertex_normals_numpy(vertices, triangles):
    """area-weighted vertex normals -> float32 (V, 3).  The face vector of (a, b, c) is cross(pb - pa, pc - pa), each component two
    products and one difference; a vertex's vector is the sequential sum (from 0) of the face vectors of its triangle corners in
    ascending triangle index; len = sqrt(x*x + y*y + z*z), summed left to right; the normal is the vector / len, (0, 0, 0) where
    len == 0."""
    p, t = _check_mesh("vertex_normals_numpy", vertices, triangles)
    u, w = p[t[:, 1]] - p[t[:, 0]], p[t[:, 2]] - p[t[:, 0]]
    face = np.stack([u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1], u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2], u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]], 1)
    offsets, faces = corner_faces_numpy(len(p), t)
    acc = gather_sum(face.reshape(-1, 3), offsets, faces, np.arange(len(p)))
    length = np.sqrt(acc[:, 0] * acc[:, 0] + acc[:, 1] * acc[:, 1] + acc[:, 2] * acc[:, 2])
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where((length == 0)[:, None], F32(0), acc / length[:, None]).astype(F32)


def refine_numpy(vertices, triangles, iterations=10, lam=0.5, mu=-0.53, clamp=1.0, pin_boundary=True):
    """smooth, then the normals of the smoothed mesh -> (vertices, normals)"""
    v = smooth_numpy(vertices, triangles, iterations, lam, mu, clamp, pin_boundary)
    return v, vertex_normals_numpy(v, triangles)


# ---- the config block -------------------------------------------------------------------------------------------------------------------------
_DEFAULTS = {"iterations": 10, "lambda": 0.5, "mu": -0.53, "clamp": 1.0, "pin_boundary": True, "normals": True}


def parse_refine_config(m, mesh_tasks):
    """`inference_config.postprocess.refine` -> {tasks, iterations, lam, mu, clamp, pin_boundary, normals, max_device_gb}.  Unknown keys
    and bad values raise ValueError naming the key; `mesh_tasks`: the tasks the `mesh` block of the same config writes a mesh of
    (None: no such block) -- every task refined must be one of them.  `mu: null` is the plain Laplacian, `clamp: null` no clamp."""
    o = parse_stage_block(KEY, m, mesh_tasks, _DEFAULTS)
    iterations, _, _ = _options("parse_refine_config", o["iterations"], o["lambda"], o["mu"], o["clamp"], key=KEY)
    for k in ("pin_boundary", "normals"):
        if not isinstance(o[k], bool):
            raise ValueError(f"{KEY}.{k}: {o[k]!r} (true or false)")
    return dict(tasks=o["tasks"], iterations=iterations, lam=float(o["lambda"]), mu=None if o["mu"] is None else float(o["mu"]),
                clamp=None if o["clamp"] is None else float(o["clamp"]), pin_boundary=o["pin_boundary"], normals=o["normals"],
                max_device_gb=o["max_device_gb"])


# ---- the driver -------------------------------------------------------------------------------------------------------------------------------
class MeshRefiner(MeshStage):
    """The stage (stage.py: MeshStage) that smooths a mesh (`smooth_numpy` is the statement), takes the normals of the smoothed mesh
    (`vertex_normals_numpy`) and writes `<stem>_refined.<ext>`, with `vn` lines and `a//a` corners in an OBJ and `nx ny nz` in a
    PLY.  `normals=False` writes positions only.

    The whole mesh is resident on the device: `scratch_bytes(V, T)` = 77 V + 96 T + 24 bytes (BYTES_PER_VERTEX, BYTES_PER_TRIANGLE,
    inputs and outputs included), and a mesh that needs more than `max_device_bytes` (default: half of the free device memory) raises
    MemoryError.  There is no out-of-core path.  `refiner`: None runs the HIP kernels; a callable
    (vertices, triangles, iterations=, lam=, mu=, clamp=, pin_boundary=) -> (vertices, normals), such as `refine_numpy`, replaces
    them, which is how the driver runs on the host."""
    suffix = "refined"

    def __init__(self, iterations=10, lam=0.5, mu=-0.53, clamp=1.0, pin_boundary=True, normals=True, fmt=None, max_device_bytes=None,
                 refiner=None):
        self.iterations, _, _ = _options("MeshRefiner", iterations, lam, mu, clamp)
        super().__init__(fmt, max_device_bytes)
        self.lam, self.mu, self.clamp = float(lam), None if mu is None else float(mu), None if clamp is None else float(clamp)
        self.pin_boundary, self.normals, self.refiner = bool(pin_boundary), bool(normals), refiner

    scratch_bytes = staticmethod(scratch_bytes)

    def options(self):
        return dict(iterations=self.iterations, lam=self.lam, mu=self.mu, clamp=self.clamp, pin_boundary=self.pin_boundary)

    def refine(self, vertices, triangles):
        """host arrays -> (vertices, normals or None, number of boundary vertices)"""
        if self.refiner is not None:
            v, n = self.refiner(vertices, triangles, **self.options())
            return v, n if self.normals else None, int(adjacency_numpy(len(vertices), triangles)[2].sum())
        import torch
        from ..engine import ops
        self._budget(scratch_bytes(len(vertices), len(triangles)), f"a mesh of {len(vertices)} vertices and {len(triangles)} triangles")
        if not len(vertices):
            return vertices, vertices.copy() if self.normals else None, 0
        dv, dt = torch.from_numpy(vertices).cuda(), torch.from_numpy(triangles).cuda()
        adj = ops.mesh_adjacency(len(vertices), dt)
        v = ops.mesh_smooth(dv, dt, adjacency=adj, **self.options())
        n = ops.mesh_vertex_normals(v, dt, adjacency=adj) if self.normals else None
        return v.cpu().numpy(), None if n is None else n.cpu().numpy(), int(adj.boundary.sum().item())

    def _work(self, vertices, triangles):
        v, n, boundary = self.refine(vertices, triangles)
        moved = float(np.abs(v - vertices).max()) if len(v) else 0.0      # the largest float32 |q - p0| over vertices and components
        return v, triangles, n, dict(vertices=len(v), triangles=len(triangles), boundary_vertices=boundary, iterations=self.iterations,
                                     max_displacement=moved)
