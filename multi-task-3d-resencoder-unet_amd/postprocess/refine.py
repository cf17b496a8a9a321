"""Refinement of an extracted triangle mesh: the numpy statements of csrc/rx_meshrefine.hip (a canonical vertex adjacency, Taubin
smoothing, area-weighted vertex normals), the readers and writers of meshes with normals, the config block and the `MeshRefiner` driver.

Surface nets place one vertex per cell from 8-bit crossings, so a sheet comes out terraced, and the mesh file carries no normals.
Taubin smoothing (a pass with a positive factor, then one with a slightly larger negative factor) removes the terraces without the
shrinkage of a plain Laplacian; the normals are those of the smoothed mesh.

Everything is a property of the mesh alone.  The neighbours of a vertex are taken in ascending id and the triangles at a vertex in
ascending index, every float32 operation is one rounding in the order written here, and the kernels reproduce that: results compare
with array_equal, floats by their bits.  The statements use numpy only."""
import os

import numpy as np

from .isosurface import FORMATS, INT32_MAX, _MeshFile

F32 = np.float32
F32_MAX = float(np.finfo(np.float32).max)      # a factor or a clamp must be finite as a float32
KEY = "inference_config.postprocess.refine"
MAX_VERTICES = 2**31 - 2
MAX_TRIANGLES = (2**31 - 2) // 3      # a vertex's triangle corners are counted in int32
# device memory of a resident run, MeshRefiner.scratch_bytes: per vertex the input, two ping-pong buffers and the normals (4 x 12),
# corner counts, fill cursors and degrees (3 x 4), two offset columns (2 x 8) and the boundary flag (1); per triangle its ids (24),
# its three corner slots (3 x 4 triangle index + 3 x 8 edge partners), the compact neighbours (at most 6 x 4) and its face vector (12)
BYTES_PER_VERTEX = 77
BYTES_PER_TRIANGLE = 96
BYTES_FIXED = 24      # the last word of either offset column, the two flags


def scratch_bytes(n_vertices, n_triangles):
    """device bytes of a resident refinement of a mesh of `n_vertices` vertices and `n_triangles` triangles, inputs and outputs included"""
    return BYTES_PER_VERTEX * int(n_vertices) + BYTES_PER_TRIANGLE * int(n_triangles) + BYTES_FIXED


def _check_mesh(fn, vertices, triangles):
    v = np.ascontiguousarray(vertices, F32)
    t = np.ascontiguousarray(triangles, np.int64)
    if v.ndim != 2 or v.shape[1] != 3:
        raise ValueError(f"{fn}: vertices {v.shape} (expected (V, 3))")
    if not np.isfinite(v).all():
        raise ValueError(f"{fn}: vertices hold a NaN or an infinity")
    return v, _check_triangles(fn, len(v), t)


def _check_triangles(fn, n_vertices, triangles):
    t = np.ascontiguousarray(triangles, np.int64)
    if isinstance(n_vertices, bool) or not isinstance(n_vertices, (int, np.integer)) or not 0 <= int(n_vertices) <= MAX_VERTICES:
        raise ValueError(f"{fn}: n_vertices {n_vertices!r} (0 .. 2^31 - 2)")
    if t.ndim != 2 or t.shape[1] != 3:
        raise ValueError(f"{fn}: triangles {t.shape} (expected (T, 3))")
    if len(t) > MAX_TRIANGLES:
        raise ValueError(f"{fn}: {len(t)} triangles (at most (2^31 - 2) / 3)")
    if len(t) and (t.min() < 0 or t.max() >= n_vertices):
        raise ValueError(f"{fn}: triangles name vertex {int(t.min() if t.min() < 0 else t.max())} outside 0 .. {int(n_vertices) - 1}")
    return t


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


def _gather_sum(values, offsets, entries, rows):
    """per row r of `rows`: the sequential float32 sum of values[entries[offsets[r] + k]] over k = 0, 1, ... -- vectorised over the
    rows, sequential over the rank k, which is the order a kernel thread adds in"""
    deg = offsets[rows + 1] - offsets[rows]
    order = np.argsort(-deg, kind="stable")      # longest lists first: the rows still adding at rank k are a prefix
    rows, deg = rows[order], deg[order]
    s = np.zeros((len(rows), 3), F32)
    for k in range(int(deg.max()) if len(deg) else 0):
        n = int(np.searchsorted(-deg, -k, side="left"))      # rows with deg > k
        s[:n] = s[:n] + values[entries[offsets[rows[:n]] + k]]
    out = np.zeros_like(s)
    out[order] = s
    return out


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
            s = _gather_sum(p, offsets, nbr, moving)
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
    acc = _gather_sum(face.reshape(-1, 3), offsets, faces, np.arange(len(p)))
    length = np.sqrt(acc[:, 0] * acc[:, 0] + acc[:, 1] * acc[:, 1] + acc[:, 2] * acc[:, 2])
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where((length == 0)[:, None], F32(0), acc / length[:, None]).astype(F32)


def refine_numpy(vertices, triangles, iterations=10, lam=0.5, mu=-0.53, clamp=1.0, pin_boundary=True):
    """smooth, then the normals of the smoothed mesh -> (vertices, normals)"""
    v = smooth_numpy(vertices, triangles, iterations, lam, mu, clamp, pin_boundary)
    return v, vertex_normals_numpy(v, triangles)


# ---- files ------------------------------------------------------------------------------------------------------------------------------------
_PLY_PLAIN = ["property float x", "property float y", "property float z"]
_PLY_NORMALS = _PLY_PLAIN + ["property float nx", "property float ny", "property float nz"]


def read_ply(path):
    """a PLY as `write_ply` and `write_refined` write it -> (vertices, triangles, normals or None): binary little-endian, float
    x y z [nx ny nz] vertices, `uchar int` triangle lists.  Anything else is refused."""
    with open(path, "rb") as f:
        raw = f.read()
    head, sep, body = raw.partition(b"end_header\n")
    lines = head.decode("ascii", "replace").split("\n")
    if not sep or lines[:2] != ["ply", "format binary_little_endian 1.0"]:
        raise ValueError(f"{path}: not a binary little-endian PLY")
    lines = [ln for ln in lines[2:] if ln and not ln.startswith("comment")]
    try:
        nv, nt = int(lines[0].split("element vertex ")[1]), None
        at = next(i for i, ln in enumerate(lines) if ln.startswith("element face "))
        nt = int(lines[at].split("element face ")[1])
    except (IndexError, ValueError, StopIteration):
        raise ValueError(f"{path}: expected `element vertex N` and `element face M`") from None
    props = lines[1:at]
    if props not in (_PLY_PLAIN, _PLY_NORMALS) or lines[at + 1:] != ["property list uchar int vertex_indices"]:
        raise ValueError(f"{path}: expected float x y z [nx ny nz] vertices and `uchar int` face lists, got {props + lines[at + 1:]}")
    width = 4 * len(props)
    if len(body) != width * nv + 13 * nt:
        raise ValueError(f"{path}: {len(body)} bytes after the header, {width * nv + 13 * nt} expected (triangles only)")
    rows = np.frombuffer(body[:width * nv], "<f4").reshape(nv, len(props)).astype(F32)
    faces = np.frombuffer(body[width * nv:], dtype=[("n", "u1"), ("i", "<i4", (3,))])
    if nt and (faces["n"] != 3).any():
        raise ValueError(f"{path}: a face that is not a triangle")
    return (np.ascontiguousarray(rows[:, :3]), faces["i"].astype(np.int64).reshape(-1, 3),
            np.ascontiguousarray(rows[:, 3:]) if len(props) == 6 else None)


def read_obj(path):
    """an OBJ as `write_obj` and `write_refined` write it -> (vertices, triangles, normals or None): `v`, `vn` and triangular `f`
    lines with 1-based `a` or `a//a` corners"""
    v, n, t = [], [], []
    with open(path) as f:
        for lineno, line in enumerate(f, 1):
            parts = line.split()
            if not parts:
                continue
            if parts[0] in ("v", "vn"):
                if len(parts) != 4:
                    raise ValueError(f"{path}:{lineno}: three numbers expected")
                (v if parts[0] == "v" else n).append([float(x) for x in parts[1:]])
            elif parts[0] == "f":
                if len(parts) != 4:
                    raise ValueError(f"{path}:{lineno}: a triangle expected")
                t.append([int(c.split("/")[0]) - 1 for c in parts[1:]])
    if n and len(n) != len(v):
        raise ValueError(f"{path}: {len(n)} normals for {len(v)} vertices")
    return (np.asarray(v, F32).reshape(-1, 3), np.asarray(t, np.int64).reshape(-1, 3), np.asarray(n, F32).reshape(-1, 3) if n else None)


def read_mesh(path):
    """`read_obj` or `read_ply` by the file's extension"""
    ext = os.path.splitext(str(path))[1].lower()
    if ext not in (".obj", ".ply"):
        raise ValueError(f"{path}: expected an .obj or a .ply file")
    return (read_obj if ext == ".obj" else read_ply)(str(path))


def write_refined(path, fmt, vertices, triangles, normals=None):
    """OBJ: `v` lines, `vn` lines and `f a//a b//b c//c`, numbers with %.9g (nine significant digits read back to the same float32);
    PLY: binary little-endian float `x y z nx ny nz`, `uchar int` face lists.  Without `normals`: what `write_obj` / `write_ply`
    write.  Written to `<path>.partial` and renamed; an existing `path` is refused."""
    f = _MeshFile(str(path), fmt)
    try:
        if normals is None:
            f.add(vertices, triangles)
        else:
            v, t, n = np.ascontiguousarray(vertices, F32), np.asarray(triangles, np.int64), np.ascontiguousarray(normals, F32)
            if v.shape != n.shape:
                raise ValueError(f"write_refined: normals {n.shape} for vertices {v.shape}")
            f.nv, f.nt = len(v), len(t)
            if fmt == "obj":
                f.v.write("".join("v %.9g %.9g %.9g\n" % tuple(r) for r in v.tolist()).encode())
                f.v.write("".join("vn %.9g %.9g %.9g\n" % tuple(r) for r in n.tolist()).encode())
                f.f.write("".join("f %d//%d %d//%d %d//%d\n" % (a, a, b, b, c, c) for a, b, c in (t + 1).tolist()).encode())
            else:
                if len(t) and t.max() > INT32_MAX:
                    raise ValueError(f"write_refined: vertex id {int(t.max())} does not fit the int faces of a PLY file")
                f.v.write(np.concatenate([v, n], 1).astype("<f4").tobytes())
                rec = np.empty(len(t), dtype=[("n", "u1"), ("i", "<i4", (3,))])
                rec["n"], rec["i"] = 3, t
                f.f.write(rec.tobytes())
        _close(f, normals is not None)
    except BaseException:
        f.abort()
        raise


def _close(f, with_normals):
    """`_MeshFile.close` with the six-property header where the vertex rows hold normals"""
    if f.fmt != "ply" or not with_normals:
        return f.close()
    f.v.close()
    f.f.close()
    with open(f.parts[0] + ".head", "wb") as out:
        props = "".join(p + "\n" for p in _PLY_NORMALS)
        out.write((f"ply\nformat binary_little_endian 1.0\nelement vertex {f.nv}\n{props}element face {f.nt}\n"
                   f"property list uchar int vertex_indices\nend_header\n").encode())
        for p in f.parts:
            with open(p, "rb") as src:
                out.write(src.read())
    os.remove(f.parts[1])
    os.replace(f.parts[0] + ".head", f.parts[0])
    os.rename(f.parts[0], f.path)


# ---- the config block -------------------------------------------------------------------------------------------------------------------------
_DEFAULTS = {"iterations": 10, "lambda": 0.5, "mu": -0.53, "clamp": 1.0, "pin_boundary": True, "normals": True, "max_device_gb": None}


def parse_refine_config(m, mesh_tasks):
    """`inference_config.postprocess.refine` -> {tasks, iterations, lam, mu, clamp, pin_boundary, normals, max_device_gb}.  Unknown keys
    and bad values raise ValueError naming the key; `mesh_tasks`: the tasks the `mesh` block of the same config writes a mesh of
    (None: no such block) -- every task refined must be one of them.  `mu: null` is the plain Laplacian, `clamp: null` no clamp."""
    if not isinstance(m, dict):
        raise ValueError(f"{KEY}: expected a mapping, got {m!r}")
    known = ("tasks",) + tuple(_DEFAULTS)
    for k in m:
        if k not in known:
            raise ValueError(f"{KEY}.{k}: unknown key ({', '.join(known)})")
    tasks = m.get("tasks")
    if isinstance(tasks, str):
        tasks = [tasks]
    if not isinstance(tasks, (list, tuple)) or not tasks:
        raise ValueError(f"{KEY}.tasks: {tasks!r} (a list of task names)")
    for t in tasks:
        if mesh_tasks is None or t not in mesh_tasks:
            raise ValueError(f"{KEY}.tasks: task {t!r} is not listed under inference_config.postprocess.mesh, so no mesh of it is written")
    o = {k: m.get(k, d) for k, d in _DEFAULTS.items()}
    iterations, _, _ = _options("parse_refine_config", o["iterations"], o["lambda"], o["mu"], o["clamp"], key=KEY)
    for k in ("pin_boundary", "normals"):
        if not isinstance(o[k], bool):
            raise ValueError(f"{KEY}.{k}: {o[k]!r} (true or false)")
    gb = o["max_device_gb"]
    if gb is not None and (isinstance(gb, bool) or not isinstance(gb, (int, float)) or not gb > 0):
        raise ValueError(f"{KEY}.max_device_gb: {gb!r} (a positive number)")
    return dict(tasks=tuple(tasks), iterations=iterations, lam=float(o["lambda"]), mu=None if o["mu"] is None else float(o["mu"]),
                clamp=None if o["clamp"] is None else float(o["clamp"]), pin_boundary=o["pin_boundary"], normals=o["normals"],
                max_device_gb=None if gb is None else float(gb))


# ---- the driver -------------------------------------------------------------------------------------------------------------------------------
class MeshRefiner:
    """Reads an OBJ or a PLY mesh as `write_obj` / `write_ply` write them, smooths it (`smooth_numpy` is the statement), takes the
    normals of the smoothed mesh (`vertex_normals_numpy`) and writes `<stem>_refined.<ext>` next to it (or `out`), with `vn` lines and
    `a//a` corners in an OBJ and `nx ny nz` in a PLY.  The file is written under `<name>.partial` and renamed; an existing file is
    refused.  `fmt`: "obj" or "ply"; None keeps the input's.  `normals=False` writes positions only.

    The whole mesh is resident on the device: `scratch_bytes(V, T)` = 77 V + 96 T + 24 bytes (BYTES_PER_VERTEX, BYTES_PER_TRIANGLE,
    inputs and outputs included), and a mesh that needs more than `max_device_bytes` (default: half of the free device memory) raises
    MemoryError.  There is no out-of-core path.  `refiner`: None runs the HIP kernels; a callable
    (vertices, triangles, iterations=, lam=, mu=, clamp=, pin_boundary=) -> (vertices, normals), such as `refine_numpy`, replaces
    them, which is how the driver runs on the host."""

    def __init__(self, iterations=10, lam=0.5, mu=-0.53, clamp=1.0, pin_boundary=True, normals=True, fmt=None, max_device_bytes=None,
                 refiner=None):
        self.iterations, _, _ = _options("MeshRefiner", iterations, lam, mu, clamp)
        if fmt is not None and fmt not in FORMATS:
            raise ValueError(f"MeshRefiner: fmt {fmt!r} (one of {', '.join(FORMATS)}, or None for the input's)")
        if max_device_bytes is not None and int(max_device_bytes) < 1:
            raise ValueError(f"MeshRefiner: max_device_bytes {max_device_bytes}")
        self.lam, self.mu, self.clamp = float(lam), None if mu is None else float(mu), None if clamp is None else float(clamp)
        self.pin_boundary, self.normals, self.fmt = bool(pin_boundary), bool(normals), fmt
        self.max_device_bytes = None if max_device_bytes is None else int(max_device_bytes)
        self.refiner = refiner

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
        need, budget = scratch_bytes(len(vertices), len(triangles)), self.max_device_bytes
        if budget is None:
            budget = torch.cuda.mem_get_info()[0] // 2
        if need > budget:
            raise MemoryError(f"MeshRefiner: a mesh of {len(vertices)} vertices and {len(triangles)} triangles needs {need} bytes on the device, "
                              f"the budget is {budget} (the whole mesh is resident; there is no out-of-core path)")
        if not len(vertices):
            return vertices, vertices.copy() if self.normals else None, 0
        dv, dt = torch.from_numpy(vertices).cuda(), torch.from_numpy(triangles).cuda()
        adj = ops.mesh_adjacency(len(vertices), dt)
        v = ops.mesh_smooth(dv, dt, adjacency=adj, **self.options())
        n = ops.mesh_vertex_normals(v, dt, adjacency=adj) if self.normals else None
        return v.cpu().numpy(), None if n is None else n.cpu().numpy(), int(adj.boundary.sum().item())

    def run(self, path, out=None):
        path = str(path)
        vertices, triangles, _ = read_mesh(path)
        stem, ext = os.path.splitext(path)
        fmt = self.fmt or ext[1:].lower()
        out = f"{stem}_refined.{fmt}" if out is None else str(out)
        if os.path.exists(out):
            raise FileExistsError(f"{out} already exists")
        vertices, triangles = _check_mesh("MeshRefiner", vertices, triangles)
        v, n, boundary = self.refine(vertices, triangles)
        write_refined(out, fmt, v, triangles, n)
        moved = float(np.abs(v - vertices).max()) if len(v) else 0.0      # the largest float32 |q - p0| over vertices and components
        return dict(vertices=len(v), triangles=len(triangles), boundary_vertices=boundary, iterations=self.iterations, max_displacement=moved)
