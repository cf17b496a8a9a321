"""The mesh as a file and as arrays, shared by every mesh stage: the array checks, the OBJ / PLY writers (with or without per-vertex
normals) and readers, and the one piece of numerics more than one stage states its kernels with (`gather_sum`).

A mesh is float32 (V, 3) vertices as (x, y, z) in voxel coordinates and int64 (T, 3) triangles.  OBJ: `v` lines, with normals `vn`
lines after them, and 1-based `f a b c` or `f a//a b//b c//c` lines, numbers with %.9g (nine significant digits read back to the
same float32).  PLY: binary little-endian, float `x y z` or `x y z nx ny nz` vertices, `uchar int` face lists.  numpy only."""
import os

import numpy as np

F32 = np.float32
INT32_MAX = 2**31 - 1
FORMATS = ("obj", "ply")
MAX_VERTICES = 2**31 - 2
MAX_TRIANGLES = (2**31 - 2) // 3      # a vertex's triangle corners are counted in int32
_PLY_PLAIN = ["property float x", "property float y", "property float z"]
_PLY_NORMALS = _PLY_PLAIN + ["property float nx", "property float ny", "property float nz"]


# ---- arrays -----------------------------------------------------------------------------------------------------------------------------------
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


def gather_sum(values, offsets, entries, rows):
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


# ---- writers ----------------------------------------------------------------------------------------------------------------------------------
class _MeshFile:
    """an OBJ or PLY file written piecewise: `add(vertices, triangles, normals=None)` any number of times (triangle ids are global;
    either every piece has normals or none), `close()`.  Everything goes to `<path>.partial`; `close` assembles the file and renames
    it, `abort` removes what was written."""

    def __init__(self, path, fmt):
        if fmt not in FORMATS:
            raise ValueError(f"inference_config.postprocess.mesh.format: {fmt!r} (one of {', '.join(FORMATS)})")
        if os.path.exists(path):
            raise FileExistsError(f"{path} already exists")
        self.path, self.fmt, self.nv, self.nt, self.normals = path, fmt, 0, 0, None
        self.parts = [path + ".partial", path + ".partial.normals", path + ".partial.faces"]      # an OBJ's `vn` lines follow its `v` lines
        self.v, self.n, self.f = (open(p, "wb") for p in self.parts)

    def add(self, vertices, triangles, normals=None):
        v, t = np.ascontiguousarray(vertices, F32).reshape(-1, 3), np.asarray(triangles, np.int64).reshape(-1, 3)
        who = "write_ply" if normals is None else "write_refined"
        if self.normals is None:
            self.normals = normals is not None
        if self.normals != (normals is not None):
            raise ValueError("_MeshFile.add: normals with some pieces only")
        if self.normals:
            n = np.ascontiguousarray(normals, F32)
            if n.shape != v.shape:
                raise ValueError(f"{who}: normals {n.shape} for vertices {v.shape}")
        self.nv += len(v)
        self.nt += len(t)
        if self.fmt == "obj":
            self.v.write("".join("v %.9g %.9g %.9g\n" % (x, y, z) for x, y, z in v.tolist()).encode())
            if self.normals:
                self.n.write("".join("vn %.9g %.9g %.9g\n" % (x, y, z) for x, y, z in n.tolist()).encode())
                self.f.write("".join("f %d//%d %d//%d %d//%d\n" % (a, a, b, b, c, c) for a, b, c in (t + 1).tolist()).encode())
            else:
                self.f.write("".join("f %d %d %d\n" % (a, b, c) for a, b, c in (t + 1).tolist()).encode())
        else:
            if len(t) and t.max() > INT32_MAX:
                raise ValueError(f"{who}: vertex id {int(t.max())} does not fit the int faces of a PLY file")
            self.v.write((np.concatenate([v, n], 1) if self.normals else v).astype("<f4").tobytes())
            rec = np.empty(len(t), dtype=[("n", "u1"), ("i", "<i4", (3,))])
            rec["n"], rec["i"] = 3, t
            self.f.write(rec.tobytes())

    def close(self):
        for f in (self.v, self.n, self.f):
            f.close()
        with open(self.parts[0] + ".head", "wb") as out:
            if self.fmt == "ply":
                props = "".join(p + "\n" for p in (_PLY_NORMALS if self.normals else _PLY_PLAIN))
                out.write((f"ply\nformat binary_little_endian 1.0\nelement vertex {self.nv}\n{props}element face {self.nt}\n"
                           f"property list uchar int vertex_indices\nend_header\n").encode())
            for p in self.parts:
                with open(p, "rb") as src:
                    while True:
                        block = src.read(1 << 24)
                        if not block:
                            break
                        out.write(block)
        for p in self.parts[1:]:
            os.remove(p)
        os.replace(self.parts[0] + ".head", self.parts[0])
        os.rename(self.parts[0], self.path)

    def abort(self):
        for f in (self.v, self.n, self.f):
            f.close()
        for p in self.parts + [self.parts[0] + ".head"]:
            if os.path.exists(p):
                os.remove(p)


def write_refined(path, fmt, vertices, triangles, normals=None):
    """a whole mesh, with `normals` (float32 (V, 3)) or without, as the module docstring lays the two formats out.  Written to
    `<path>.partial` and renamed; an existing `path` is refused."""
    f = _MeshFile(str(path), fmt)
    try:
        f.add(vertices, triangles, normals)
        f.close()
    except BaseException:
        f.abort()
        raise


def write_obj(path, vertices, triangles):
    """`v x y z` and 1-based `f a b c` lines; tasks.normals.mesh_targets.read_obj reads the same arrays back.  Written to
    `<path>.partial` and renamed; an existing `path` is refused."""
    write_refined(path, "obj", vertices, triangles)


def write_ply(path, vertices, triangles):
    """binary little-endian PLY: float x, y, z vertices, `uchar int` face lists.  Written to `<path>.partial` and renamed; an existing
    `path` is refused."""
    write_refined(path, "ply", vertices, triangles)


# ---- readers ----------------------------------------------------------------------------------------------------------------------------------
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
