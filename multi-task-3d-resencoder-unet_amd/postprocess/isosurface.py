"""Triangle mesh of a prediction volume by surface nets: the numpy statement of csrc/rx_isosurface.hip, the config block and the
out-of-core `SurfaceMesher` driver (the OBJ / PLY writers: mesh_io.py).

Surface nets (dual contouring without gradients) need no case table.  The volume is padded with one voxel of 0 on every side; a voxel
is inside when `value > level`; every cell of the (Z+1, Y+1, X+1) grid whose eight corners are not all inside or all outside holds one
vertex, and every lattice edge with one end inside gives one quad between the four cells around it.  Vertices are numbered in ascending
linear cell index and triangles are ordered by (owning cell, axis, first / second), so the mesh is a property of the volume alone:
the statement, the kernels and a run in slabs produce the same arrays and everything compares with array_equal (vertices by their bits).

Vertices are (x, y, z) in voxel coordinates of the unpadded volume -- column 2 is what tasks/normals/mesh_targets.py compares with the
slice index z and columns 0, 1 are what it rounds to the pixel (w, h) of that slice -- so `read_obj` of a written mesh and
`MeshTargetBuilder` paint the surface back where the volume has it.  The statements use numpy only."""
import os

import numpy as np

from .mesh_io import F32, FORMATS, _MeshFile

MAX_EXTENT = 2**24 - 3      # an extent of 2^24 - 2 or more is refused: a position is an exact float32 integer plus a fraction
MAX_CELLS = 2**31 - 2
MAX_BANDS = 2**24 - 1      # the kernels give a band of 4 cell planes x 8 cell rows to a workgroup of 256 threads
KEY = "inference_config.postprocess.mesh"
# device memory of a slab beyond its outputs: the voxel bytes, the active bits (one 64-bit word per 64 cells of a cell row) and,
# per cell row, its two counts (2 x int32) and its two scanned offsets (2 x int64: 3 quads per cell are more than int32 holds)
BYTES_PER_VOXEL = 1
BYTES_PER_CELL_ROW = 24


def scratch_bytes(planes, Y, X):
    """bits + counts + offsets of `planes` voxel planes of a Y x X volume: (planes+1) * (Y+1) cell rows of X+1 cells"""
    rows = (planes + 1) * (Y + 1)
    return rows * (8 * ((X + 1 + 63) // 64) + BYTES_PER_CELL_ROW)


def _check_volume(fn, values, level):
    values = np.asarray(values)
    if values.ndim != 3 or values.dtype != np.uint8:
        raise ValueError(f"{fn}: expected a (Z, Y, X) uint8 volume, got {values.dtype} {values.shape}")
    if isinstance(level, bool) or not isinstance(level, (int, np.integer)) or not 0 <= int(level) <= 254:
        raise ValueError(f"{fn}: level {level!r} (an integer 0 .. 254: inside is value > level)")
    if values.size and max(values.shape) > MAX_EXTENT:
        raise ValueError(f"{fn}: an extent of {max(values.shape)} (at most 2^24 - 3: positions are exact float32)")
    if values.size and np.prod([s + 1 for s in values.shape], dtype=object) > MAX_CELLS:
        raise ValueError(f"{fn}: more than 2^31 - 2 cells in a volume of {values.shape}")
    return values, int(level)


def _inside(values, level):
    """the padded inside mask (Z+2, Y+2, X+2) and the cell grid's extents"""
    ins = np.pad(values > level, 1)
    return ins, tuple(s - 1 for s in ins.shape)


def _active(ins, dims):
    CZ, CY, CX = dims
    n = np.zeros(dims, np.int8)
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                n += ins[dz:dz + CZ, dy:dy + CY, dx:dx + CX]
    return (n > 0) & (n < 8)


def _crossing(ins, dims, axis):
    """per cell: does the lattice edge from its corner 0 along `axis` (0 z, 1 y, 2 x) cross the surface"""
    lo = ins[:dims[0], :dims[1], :dims[2]]
    hi = [slice(0, d) for d in dims]
    hi[axis] = slice(1, dims[axis] + 1)
    return lo != ins[tuple(hi)], lo


def counts_numpy(values, level):
    """(number of vertices, number of triangles) of `surface_nets_numpy(values, level)`"""
    values, level = _check_volume("counts_numpy", values, level)
    if not values.size:
        return 0, 0
    ins, dims = _inside(values, level)
    return int(_active(ins, dims).sum()), 2 * sum(int(_crossing(ins, dims, a)[0].sum()) for a in range(3))


def surface_nets_numpy(values, level, z_base=0):
    """(Z, Y, X) uint8 `values`, integer `level` 0 .. 254 -> (vertices float32 (n, 3) as (x, y, z), triangles int64 (m, 3)).
    `z_base`: the volume's first plane in a larger volume; it is added to the corner-0 z coordinate before that becomes a float32.

    Cell (k, j, i) of the (Z+1, Y+1, X+1) grid has corner 0 at voxel (k-1, j-1, i-1) and the others at +0/1 per axis; voxels outside
    the volume are 0.  Active cells (corners not all inside, not all outside) are numbered in ascending (k*(Y+1) + j)*(X+1) + i.
    Position, float32, one rounding per operation: over the 12 cell edges -- axis z, y, x; within an axis the offsets of the other two
    axes (in z, y, x order) through (0,0), (0,1), (1,0), (1,1) -- an edge a -> b = a + e_axis with exactly one end inside adds
    t = (iso - v_a) / (v_b - v_a), iso = float32(level + 0.5), to the sum of its own axis, a's offset (0.0 or 1.0) to the other two
    sums and 1.0 to the count; position = float32(corner-0 voxel coordinate) + sum / count.
    Triangles: a crossing lattice edge p -> p + e_d (C the cell whose corner 0 is p; (u, v) the other two axes in cyclic order:
    (y, z) for an x edge, (z, x) for y, (x, y) for z) joins A = C - e_u - e_v, B = C - e_v, C, D = C - e_u: (A, B, C), (A, C, D) when p
    is inside, (A, D, C), (A, C, B) when outside, so normals point from inside to outside in right-handed (x, y, z).  They are ordered
    by (linear index of C, axis slot z = 0 / y = 1 / x = 2, first / second)."""
    values, level = _check_volume("surface_nets_numpy", values, level)
    if not values.size:
        return np.zeros((0, 3), F32), np.zeros((0, 3), np.int64)
    ins, dims = _inside(values, level)
    CZ, CY, CX = dims
    V = np.pad(values, 1).astype(F32)
    iso = F32(level + 0.5)
    active = _active(ins, dims)
    vid = np.full(dims, -1, np.int64)
    vid[active] = np.arange(int(active.sum()))
    cell = np.nonzero(active)      # (k, j, i) of every vertex, in id order
    n = cell[0].size
    s = np.zeros((3, n), F32)
    cnt = np.zeros(n, F32)
    for d in range(3):
        others = [a for a in range(3) if a != d]
        for o0 in (0, 1):
            for o1 in (0, 1):
                a = [0, 0, 0]
                a[others[0]], a[others[1]] = o0, o1
                b = list(a)
                b[d] = 1
                ia = tuple(c + o for c, o in zip(cell, a))
                ib = tuple(c + o for c, o in zip(cell, b))
                va, vb = V[ia], V[ib]
                cross = ins[ia] != ins[ib]
                with np.errstate(divide="ignore", invalid="ignore"):
                    t = (iso - va) / (vb - va)
                for ax in range(3):
                    add = t if ax == d else np.full(n, F32(a[ax]), F32)
                    s[ax] = np.where(cross, s[ax] + add, s[ax])
                cnt = np.where(cross, cnt + F32(1), cnt)
    if isinstance(z_base, bool) or not isinstance(z_base, (int, np.integer)) or not 0 <= int(z_base) <= MAX_EXTENT - values.shape[0]:
        raise ValueError(f"surface_nets_numpy: z_base {z_base!r}: plane z_base + {values.shape[0]} must stay below 2^24 - 2")
    corner0 = np.stack(cell) - 1
    corner0[0] += int(z_base)
    pos = corner0.astype(F32) + s / cnt      # (z, y, x) rows
    vertices = np.ascontiguousarray(pos[::-1].T)

    tris, keys = [], []
    cyc = {2: (1, 0), 1: (0, 2), 0: (2, 1)}      # axis (0 z, 1 y, 2 x) -> (u, v): x -> (y, z), y -> (z, x), z -> (x, y)
    for slot, d in enumerate((0, 1, 2)):
        u, v = cyc[d]
        cross, lo = _crossing(ins, dims, d)
        p = np.stack(np.nonzero(cross))      # the cell C == the padded coordinate of the edge's lower voxel
        assert (p[u] >= 1).all() and (p[v] >= 1).all(), "a crossing edge on the padding"

        def at(du, dv):
            q = p.copy()
            q[u] += du
            q[v] += dv
            r = vid[q[0], q[1], q[2]]
            assert (r >= 0).all(), "a cell around a crossing edge is not active"
            return r
        A, B, C, D = at(-1, -1), at(0, -1), at(0, 0), at(-1, 0)
        inside = lo[cross][:, None]
        first = np.where(inside, np.stack([A, B, C], 1), np.stack([A, D, C], 1))
        second = np.where(inside, np.stack([A, C, D], 1), np.stack([A, C, B], 1))
        key = ((p[0] * CY + p[1]) * CX + p[2]) * 3 + slot
        tris.append(np.stack([first, second], 1).reshape(-1, 3))
        keys.append(np.repeat(key * 2, 2) + np.tile([0, 1], key.size))
    tris, keys = np.concatenate(tris), np.concatenate(keys)
    return vertices, np.ascontiguousarray(tris[np.argsort(keys, kind="stable")].astype(np.int64))


# ---- the config block ----------------------------------------------------------------------------------------------------------------------
_DEFAULTS = dict(source="filtered", level=127, format="obj", max_device_gb=None)
SOURCES = ("filtered", "final")


def parse_mesh_config(m, targets, patch_size=None, component_tasks=None):
    """`inference_config.postprocess.mesh` -> {tasks, source, level, format, max_device_gb}.  Unknown keys and bad values raise
    ValueError naming the key; `component_tasks`: the tasks the `components` block of the same config filters (None: no such block)."""
    if not isinstance(m, dict):
        raise ValueError(f"{KEY}: expected a mapping, got {m!r}")
    known = ("tasks",) + tuple(_DEFAULTS)
    for k in m:
        if k not in known:
            raise ValueError(f"{KEY}.{k}: unknown key ({', '.join(known)})")
    if patch_size is not None and len(tuple(patch_size)) != 3:
        raise ValueError(f"{KEY}: a {len(tuple(patch_size))}-D patch_size {tuple(patch_size)}: a mesh is extracted from (Z, Y, X) volumes only")
    tasks = m.get("tasks")
    if isinstance(tasks, str):
        tasks = [tasks]
    if not isinstance(tasks, (list, tuple)) or not tasks:
        raise ValueError(f"{KEY}.tasks: {tasks!r} (a list of task names)")
    for t in tasks:
        if t not in targets:
            raise ValueError(f"{KEY}.tasks: unknown task {t!r} (one of {', '.join(targets)})")
        if int(targets[t].get("channels", 1)) != 1:
            raise ValueError(f"{KEY}.tasks: task {t!r} has {targets[t].get('channels')} channels (single-channel tasks only)")
    source = m.get("source", _DEFAULTS["source"])
    if source not in SOURCES:
        raise ValueError(f"{KEY}.source: {source!r} (one of {', '.join(SOURCES)})")
    if source == "filtered":
        for t in tasks:
            if component_tasks is None or t not in component_tasks:
                raise ValueError(f"{KEY}.source: filtered, but inference_config.postprocess.components does not list task {t!r}, so "
                                 f"{t}_filtered is never written")
    level = m.get("level", _DEFAULTS["level"])
    if isinstance(level, bool) or not isinstance(level, (int, np.integer)) or not 0 <= int(level) <= 254:
        raise ValueError(f"{KEY}.level: {level!r} (an integer 0 .. 254)")
    fmt = m.get("format", _DEFAULTS["format"])
    if fmt not in FORMATS:
        raise ValueError(f"{KEY}.format: {fmt!r} (one of {', '.join(FORMATS)})")
    gb = m.get("max_device_gb")
    if gb is not None and (isinstance(gb, bool) or not isinstance(gb, (int, float)) or not gb > 0):
        raise ValueError(f"{KEY}.max_device_gb: {gb!r} (a positive number)")
    return dict(tasks=tuple(tasks), source=source, level=int(level), format=fmt, max_device_gb=None if gb is None else float(gb))


# ---- the driver ----------------------------------------------------------------------------------------------------------------------------
def _host_slab(mesher, values, level, a, k_emit, k_hi, vertex_base):
    """cell planes [k_emit, k_hi) (local to the voxel planes `values`, which begin at global plane `a`) through a whole-volume
    `mesher`: the slab is meshed as a volume of its own, which closes it at both ends, and what belongs to other planes -- the caps
    and, with them, every vertex whose cell is not in [k_emit, k_hi) -- is cut away.  Cells of those planes see exactly the voxels
    they see in the whole volume, and ids are linear in the cell index, so what is left is the whole volume's, shifted."""
    v, t = mesher(values, level, z_base=a)
    Z, Y, X = values.shape
    ins, dims = _inside(values, level)
    per_plane = _active(ins, dims).reshape(Z + 1, -1).sum(axis=1)
    first = np.concatenate([[0], np.cumsum(per_plane)])      # first[k]: the id of plane k's first vertex
    quads = sum(_crossing(ins, dims, d)[0].reshape(Z + 1, -1).sum(axis=1) for d in range(3))
    tfirst = 2 * np.concatenate([[0], np.cumsum(quads)])
    v = v[first[k_emit]:first[k_hi]]
    t = t[tfirst[k_emit]:tfirst[k_hi]] + (vertex_base - first[max(k_emit - 1, 0)])
    return v, t, int(per_plane[k_hi - 1]) if k_hi > k_emit else 0


class SurfaceMesher:
    """Extracts the surface `value > level` of `<store>/<task>_<source>` (a single-channel (Z, Y, X) uint8 array) as a triangle mesh
    and writes `<store>/<task>_<source>.obj` (or `.ply`, or `path`): `surface_nets_numpy` is the statement.  The file is written
    under `<name>.partial` and renamed when the run has succeeded; a failed run leaves nothing behind; an existing file is refused.

    A volume within the budget runs resident.  A larger one runs in slabs of `slab` cell planes: vertices and triangles of cell plane
    k reference planes k - 1 and k only, so a slab that emits planes [k0, k1) loads voxel planes k0 - 2 .. k1 - 1 (the two before k0
    give the active bits of plane k0 - 1, whose first vertex id is carried over from the slab before) and the writers append.
    The order is linear in the cell index, so a slab run's file is the resident run's file.  Device memory beyond the outputs of a
    slab is BYTES_PER_VOXEL per loaded voxel plus `scratch_bytes` (1/8 byte per cell and BYTES_PER_CELL_ROW per cell row); the
    vertices (12 bytes) and triangles (2 x 24 bytes per quad) of a slab are allocated once their number is known and are not part of
    the budget.  `max_device_bytes` defaults to half of the free device memory.  `mesher`: None runs the HIP kernels; a callable
    (values uint8, level, z_base=0) -> (vertices, triangles) replaces them -- it is called as `mesher(values, level, z_base=a)` with
    `a` the slab's first voxel plane, which it adds to the corner-0 z coordinate before the float32 rounding, as
    `surface_nets_numpy` does -- which is how the slab path runs on the host.  `last_slab` is the number of cell planes per slab the last run used."""

    def __init__(self, level=127, fmt="obj", max_device_bytes=None, slab=None, mesher=None):
        if isinstance(level, bool) or not isinstance(level, (int, np.integer)) or not 0 <= int(level) <= 254:
            raise ValueError(f"{KEY}.level: {level!r} (an integer 0 .. 254)")
        if fmt not in FORMATS:
            raise ValueError(f"{KEY}.format: {fmt!r} (one of {', '.join(FORMATS)})")
        if max_device_bytes is not None and int(max_device_bytes) < 1:
            raise ValueError(f"{KEY}.max_device_gb: {max_device_bytes} bytes")
        if slab is not None and (isinstance(slab, bool) or int(slab) < 1):
            raise ValueError(f"SurfaceMesher: slab {slab!r} (a positive number of cell planes)")
        self.level, self.fmt = int(level), fmt
        self.max_device_bytes = None if max_device_bytes is None else int(max_device_bytes)
        self.slab = None if slab is None else int(slab)
        self.mesher = mesher
        self.last_slab = None

    @staticmethod
    def slab_bytes(planes, Y, X):
        """device bytes, beyond the outputs, of a slab that loads `planes` voxel planes"""
        return BYTES_PER_VOXEL * planes * Y * X + scratch_bytes(planes, Y, X)

    @staticmethod
    def most_planes(Y, X):
        """the most voxel planes of a Y x X volume one pass takes: 2^31 - 2 cells, and 2^24 - 1 bands of 4 cell planes x 8 cell rows
        (one workgroup each; a launch holds fewer than 2^32 threads)"""
        return min(MAX_CELLS // ((Y + 1) * (X + 1)) - 1, (MAX_BANDS // ((Y + 1 + 7) // 8)) * 4 - 1)

    def slab_depth(self, shape):
        """cell planes per slab: Z + 1 (resident) when the whole volume fits, else as many as the budget holds, at least 2"""
        Z, Y, X = shape
        most = self.most_planes(Y, X)
        if most < min(4, Z):
            raise ValueError(f"SurfaceMesher: four planes of a {Y} x {X} volume are more than one pass takes (2^31 - 2 cells, 2^24 - 1 bands "
                             f"of 4 x 8 cell rows)")
        if self.slab is not None:
            if min(self.slab + 2, Z) > most:
                raise ValueError(f"SurfaceMesher: slab {self.slab}: {min(self.slab + 2, Z)} planes of a {Y} x {X} volume are more than one "
                                 f"pass takes (at most {most} planes: 2^31 - 2 cells, 2^24 - 1 bands of 4 x 8 cell rows)")
            return min(self.slab, Z + 1)
        budget = self.max_device_bytes
        if budget is None:
            if self.mesher is not None:
                return Z + 1 if Z <= most else most - 2
            import torch
            budget = torch.cuda.mem_get_info()[0] // 2
        if Z <= most and self.slab_bytes(Z, Y, X) <= budget:
            return Z + 1
        # slab_bytes(p) = p * (Y * X + r) + r with r the scratch of one plane of cell rows; a slab of n cell planes loads n + 2 planes
        r = scratch_bytes(0, Y, X)
        n = min((budget - r) // (BYTES_PER_VOXEL * Y * X + r), most) - 2
        if n < 2:
            raise MemoryError(f"SurfaceMesher: two cell planes of a {Y} x {X} volume load four voxel planes and need "
                              f"{self.slab_bytes(4, Y, X)} bytes on the device, the budget is {budget}")
        return int(n)

    def run(self, store, task, source="filtered", path=None):
        from ..dataloading import zarr_lite
        if source not in SOURCES:
            raise ValueError(f"{KEY}.source: {source!r} (one of {', '.join(SOURCES)})")
        src_path = os.path.join(str(store), f"{task}_{source}")
        try:
            src = zarr_lite.open(src_path)
        except zarr_lite.ZarrLiteError as e:
            raise ValueError(f"SurfaceMesher: task {task!r}: {e}") from None
        if src.ndim != 3 or src.dtype != np.uint8:
            raise ValueError(f"SurfaceMesher: task {task!r}: {src_path} is {src.dtype} {src.shape}; a single-channel (Z, Y, X) uint8 "
                             f"array is required")
        if min(src.shape) < 1 or max(src.shape) > MAX_EXTENT:
            raise ValueError(f"SurfaceMesher: task {task!r}: extents {tuple(src.shape)} (1 .. 2^24 - 3: positions are exact float32)")
        depth = self.slab_depth(src.shape)
        self.last_slab = depth
        out = _MeshFile(str(path) if path is not None else f"{src_path}.{self.fmt}", self.fmt)
        try:
            slabs = self._run(src, depth, out)
            out.close()
        except BaseException:
            out.abort()
            raise
        return dict(level=self.level, vertices=out.nv, triangles=out.nt, slabs=slabs)

    def _run(self, src, depth, out):
        Z, Y, X = src.shape
        emitted = below = slabs = 0      # vertices written so far; how many of them belong to the last plane written
        for k0 in range(0, Z + 1, depth):
            k1 = min(k0 + depth, Z + 1)
            a = max(k0 - 2, 0)
            b = min(k1, Z)      # > a: k1 > k0 and k0 <= Z
            values = np.ascontiguousarray(src[a:b])
            base = emitted - below      # the id of the first vertex of plane k0 - 1
            if self.mesher is not None:
                v, t, below = _host_slab(self.mesher, values, self.level, a, k0 - a, k1 - a, base)
            else:
                v, t, below = self._device_slab(values, a, k0 - a, k1 - a, base)
            out.add(v, t)
            emitted += len(v)
            slabs += 1
        return slabs

    def _device_slab(self, values, a, k_emit, k_hi, base):
        import torch
        from ..engine import ops
        dev = torch.from_numpy(values).cuda()
        # ids count from the first vertex of plane k_lo, and `base` is the id of the first vertex of plane k_emit - 1: that plane
        # is k_lo, also where the slab still begins at the volume's first plane (a == 0 with k_emit == 2 leaves plane 0 out)
        v, t, below = ops.iso_mesh(dev, self.level, vertex_base=base, window=(max(k_emit - 1, 0), k_emit, k_hi), z_base=a,
                                   return_last_plane=True)
        return v.cpu().numpy(), t.cpu().numpy(), below
