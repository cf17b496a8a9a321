"""Orientation of an extracted mesh against the predicted normal field: the numpy statements of csrc/rx_meshsample.hip (trilinear
sampling of a volume at the mesh vertices, the cosine between a triangle's face vector and the sampled vectors of its corners, the
front / back / rim classification and the selection of one face), the config block and the `MeshOrienter` driver.

Surface nets on a sheet mask give a closed shell around a sheet a few voxels thick: a front face, a back face and a rim.  The
mesher orients every quad from inside to outside; the network's `normals` head, written by streaming inference as
`normals_final` ((3, Z, Y, X) uint16, `(v + 1) / 2 * 65535`), points to one consistent side of the sheet.  A triangle whose face
vector agrees with the sampled field is on the front face, one that opposes it on the back face, and the rest is the rim.  One
face, with the sampled vectors as its normals, is an open single-sided sheet again: what `MeshTargetBuilder` takes.

Every float32 operation below is one rounding in the order written, nothing is fused, and the kernels reproduce that: results
compare with array_equal, floats by their bits.  The statements use numpy only."""
import os

import numpy as np

from .mesh_io import F32, _check_mesh
from .refine import vertex_normals_numpy
from .stage import MeshStage, parse_stage_block

KEY = "inference_config.postprocess.orient"
RULES = {"copy": np.float32, "u8": np.uint8, "u16": np.uint16, "normal_u16": np.uint16}      # rule -> the dtype it decodes
SIDES = ("both", "front", "back")
NORMALS = ("predicted", "mesh")
MAX_CHANNELS = 8
MAX_EXTENT = 2**24 - 2      # an index must be an exact float32
# device memory of a run, MeshOrienter.scratch_bytes.  Per vertex: its position (12), the C sampled values, made unit in place
# (4 C), the used flag and its scan (4 + 8), the identity map the emit pass reads (8), the output position and normal (12 + 12);
# per triangle: its ids (24), cos (4), side (1), the keep flag and its scan (4 + 8), the output ids (24); per voxel on the device
# C stored values of `itemsize` bytes.
BYTES_PER_VERTEX = 56
BYTES_PER_VERTEX_CHANNEL = 4
BYTES_PER_TRIANGLE = 65
BYTES_FIXED = 24      # the last word of either scan, the flag, padded


def scratch_bytes(n_vertices, n_triangles, channels, planes, Y, X, itemsize=2):
    """device bytes of an orientation run over a mesh of `n_vertices` vertices and `n_triangles` triangles with `planes` planes of a
    `channels`-channel Y x X volume of `itemsize`-byte values on the device at one time (all Z of a resident run; both buffers of a
    run in slabs), inputs and outputs included"""
    return ((BYTES_PER_VERTEX + BYTES_PER_VERTEX_CHANNEL * int(channels)) * int(n_vertices) + BYTES_PER_TRIANGLE * int(n_triangles) + BYTES_FIXED
            + int(channels) * int(planes) * int(Y) * int(X) * int(itemsize))


# ---- the statements ---------------------------------------------------------------------------------------------------------------------------
def decode_numpy(values, rule):
    """stored values -> float32 under `rule`: first float32(v), then `copy`: unchanged (-0.0 and denormals stay); `u8`: v / 255;
    `u16`: v / 65535; `normal_u16`: (v / 65535) * 2 - 1, a division, a product and a difference"""
    if rule not in RULES:
        raise ValueError(f"decode_numpy: rule {rule!r} (one of {', '.join(RULES)})")
    values = np.asarray(values)
    if values.dtype != RULES[rule]:
        raise ValueError(f"decode_numpy: rule {rule!r} decodes {np.dtype(RULES[rule]).name} values, got {values.dtype}")
    f = values.astype(F32)
    if rule == "copy":
        return f
    if rule == "u8":
        return f / F32(255)
    f = f / F32(65535)
    return f if rule == "u16" else f * F32(2) - F32(1)


def _axis(p, n):
    """one axis of every point: (i0, i1 int64 clamped to [0, n - 1], f float32).  i = floor(p) squashed into [-2, n] as a float
    (a NaN becomes n), then i0 = clamp(i), i1 = clamp(i + 1); f = p - floor(p)."""
    fl = np.floor(p)
    i = np.fmax(np.fmin(fl, F32(n)), F32(-2)).astype(np.int64)
    return np.clip(i, 0, n - 1), np.clip(i + 1, 0, n - 1), (p - fl).astype(F32)


def slab_ranges(z_total, depth):
    """the slabs of an out-of-core run with `depth` owned planes each -> [(z_base, planes)]: slab k starts at k * depth and holds
    one plane past its owned range, [k * depth, min((k + 1) * depth + 1, z_total)); a last slab that would own plane
    z_total - 1 alone is left out, since the slab before it holds that plane already.  Every point has both of its clamped z
    indices inside exactly one of these."""
    z_total, depth = int(z_total), int(depth)
    if z_total < 1 or depth < 1:
        raise ValueError(f"slab_ranges: z_total {z_total}, depth {depth} (both at least 1)")
    starts = [a for a in range(0, z_total, depth) if a < z_total - 1] or [0]
    return [(a, min(a + depth + 1, z_total) - a) for a in starts]


def sample_points_numpy(volume, points, rule, z_base=0, z_total=None):
    """`volume` (C, Zs, Y, X), C in 1 .. 8, sampled at float32 `points` (V, 3) given as (x, y, z) in voxel coordinates ->
    (values float32 (V, C), owned bool (V,)).

    Trilinear with clamped borders, the index and lerp order of dataloading.spatial_device.sample_numpy with border="clamp": per
    axis i = floor(p), f = p - i, the corners are i and i + 1 clamped to [0, n - 1]; each of the eight corners is decoded first
    (`decode_numpy`); then lerp(u, w, f) = u + f * (w - u) along x (four), then y (two), then z (one).  All channels share one set
    of indices.

    `volume` holds planes [z_base, z_base + Zs) of a volume of `z_total` planes (default: z_base + Zs).  Clamping and fractions
    use the global z and z_total; only the fetch subtracts z_base.  A point whose two clamped z indices are not both inside the
    slab is not computed: owned is False and its values are 0."""
    vol = np.asarray(volume)
    if vol.ndim != 4 or not 1 <= vol.shape[0] <= MAX_CHANNELS or min(vol.shape) < 1:
        raise ValueError(f"sample_points_numpy: volume {vol.shape} (expected (C, Z, Y, X) with C in 1 .. {MAX_CHANNELS})")
    if rule not in RULES or vol.dtype != RULES[rule]:
        raise ValueError(f"sample_points_numpy: rule {rule!r} for a {vol.dtype} volume (copy: float32, u8: uint8, u16 and normal_u16: uint16)")
    p = np.ascontiguousarray(points, F32)
    if p.ndim != 2 or p.shape[1] != 3:
        raise ValueError(f"sample_points_numpy: points {p.shape} (expected (V, 3))")
    C, Zs, Y, X = vol.shape
    z_base = int(z_base)
    z_total = z_base + Zs if z_total is None else int(z_total)
    if z_base < 0 or z_base + Zs > z_total or max(z_total, Y, X) > MAX_EXTENT:
        raise ValueError(f"sample_points_numpy: planes {z_base} .. {z_base + Zs} of {z_total} (a slab inside the volume, extents below 2^24 - 2)")
    with np.errstate(invalid="ignore", over="ignore"):
        x0, x1, fx = _axis(p[:, 0], X)
        y0, y1, fy = _axis(p[:, 1], Y)
        z0, z1, fz = _axis(p[:, 2], z_total)
        owned = (z0 >= z_base) & (z1 < z_base + Zs)      # z0 <= z1
        z0, z1 = np.clip(z0 - z_base, 0, Zs - 1), np.clip(z1 - z_base, 0, Zs - 1)      # what is not owned is fetched somewhere and dropped
        flat = vol.reshape(C, -1)

        def fetch(z, y, x):
            return decode_numpy(flat[:, (z * Y + y) * X + x], rule)      # (C, V)

        def lerp(u, w, f):
            return u + f * (w - u)
        zs = []
        for z in (z0, z1):
            ys = [lerp(fetch(z, y, x0), fetch(z, y, x1), fx) for y in (y0, y1)]
            zs.append(lerp(ys[0], ys[1], fy))
        s = lerp(zs[0], zs[1], fz)
    out = np.ascontiguousarray(s.T, F32)
    out[~owned] = 0
    return out, owned


def unit_numpy(vectors):
    """float32 (V, 3) -> v / l with l = sqrt(x*x + y*y + z*z), the products summed left to right, where l > 0; else exactly (0, 0, 0)"""
    v = np.ascontiguousarray(vectors, F32)
    if v.ndim != 2 or v.shape[1] != 3:
        raise ValueError(f"unit_numpy: vectors {v.shape} (expected (V, 3))")
    with np.errstate(invalid="ignore", over="ignore", divide="ignore", under="ignore"):
        length = np.sqrt(v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1] + v[:, 2] * v[:, 2])
        return np.where((length > 0)[:, None], v / length[:, None], F32(0)).astype(F32)


def face_cos_numpy(vertices, triangles, vectors):
    """-> float32 (T,): the cosine between a triangle's face vector and the vectors at its corners.  g = cross(pb - pa, pc - pa),
    each component two products and one difference (`vertex_normals_numpy`); m = (n_a + n_b) + n_c; d = g.m, gg = g.g, mm = m.m,
    each three products summed left to right; cos = d / sqrt(gg * mm).  Where a factor is zero that is 0 / 0 = NaN: the rim."""
    p, t = _check_mesh("face_cos_numpy", vertices, triangles)
    n = np.ascontiguousarray(vectors, F32)
    if n.shape != p.shape:
        raise ValueError(f"face_cos_numpy: vectors {n.shape} for vertices {p.shape}")
    with np.errstate(invalid="ignore", over="ignore", divide="ignore", under="ignore"):
        u, w = p[t[:, 1]] - p[t[:, 0]], p[t[:, 2]] - p[t[:, 0]]
        g = [u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1], u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2], u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]]
        m = (n[t[:, 0]] + n[t[:, 1]]) + n[t[:, 2]]
        m = [m[:, 0], m[:, 1], m[:, 2]]

        def dot(a, b):
            return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]
        return (dot(g, m) / np.sqrt(dot(g, g) * dot(m, m))).astype(F32)


def side_numpy(cos, min_cos):
    """-> int8 (T,): +1 (front) where cos > min_cos, -1 (back) where cos < -min_cos, 0 (rim) otherwise, a NaN included"""
    c, k = np.asarray(cos, F32), F32(min_cos)
    with np.errstate(invalid="ignore"):
        return (c > k).astype(np.int8) - (c < -k).astype(np.int8)


def select_numpy(vertices, triangles, keep_mask, *attrs):
    """the triangles where `keep_mask` holds, in input order, over the vertices some kept triangle names, in ascending id, the
    triangles renumbered to match -> (vertices, triangles, attrs, row_of): `attrs` are per-vertex arrays carried along, `row_of`
    int64 (V,) is the output row of every input vertex, -1 for a dropped one"""
    p, t = _check_mesh("select_numpy", vertices, triangles)
    keep = np.asarray(keep_mask).astype(bool)
    if keep.shape != (len(t),):
        raise ValueError(f"select_numpy: keep_mask {keep.shape} for {len(t)} triangles")
    for a in attrs:
        if len(a) != len(p):
            raise ValueError(f"select_numpy: an attribute of {len(a)} rows for {len(p)} vertices")
    kept = t[keep]
    used = np.unique(kept)
    row_of = np.full(len(p), -1, np.int64)
    row_of[used] = np.arange(len(used))
    return (np.ascontiguousarray(p[used]).reshape(-1, 3), row_of[kept].reshape(-1, 3), tuple(np.ascontiguousarray(np.asarray(a)[used]) for a in attrs),
            row_of)


# ---- the config block -------------------------------------------------------------------------------------------------------------------------
_DEFAULTS = {"normals_task": "normals", "side": "front", "min_cos": 0.2, "normals": "predicted"}


def _side(name, side):
    if side not in SIDES:
        raise ValueError(f"{name} {side!r} (one of {', '.join(SIDES)})")
    return side


def _min_cos(name, min_cos):
    if isinstance(min_cos, bool) or not isinstance(min_cos, (int, float, np.integer, np.floating)) or not 0 <= float(min_cos) < 1:
        raise ValueError(f"{name} {min_cos!r} (a number in [0, 1))")
    return float(min_cos)


def _normals(name, normals):
    if normals not in NORMALS:
        raise ValueError(f"{name} {normals!r} (one of {', '.join(NORMALS)})")
    return normals


def parse_orient_config(m, mesh_tasks, targets):
    """`inference_config.postprocess.orient` -> {tasks, normals_task, side, min_cos, normals, max_device_gb}.  Unknown keys and bad
    values raise ValueError naming the key; `mesh_tasks`: the tasks the `mesh` block of the same config writes a mesh of (None: no
    such block) -- every task oriented must be one of them; `targets`: {task: {"channels": c, ...}} -- `normals_task` must be one
    whose output rule is the 3-channel unit field stored as uint16."""
    from ..inference_schedule import task_output_rule
    o = parse_stage_block(KEY, m, mesh_tasks, _DEFAULTS)
    nt = o["normals_task"]
    if not isinstance(nt, str) or nt not in targets:
        raise ValueError(f"{KEY}.normals_task: {nt!r} is not an inference target (one of {', '.join(targets)})")
    rule = task_output_rule(nt, int(targets[nt].get("channels", 1)))
    if rule[0] != "unit" or rule[1] != "u16":
        raise ValueError(f"{KEY}.normals_task: target {nt!r} with {targets[nt].get('channels', 1)} channels is not written as a 3-channel unit "
                         f"field in uint16 (a target named `normals` with 3 channels is)")
    _side(f"{KEY}.side:", o["side"])
    _normals(f"{KEY}.normals:", o["normals"])
    return dict(o, min_cos=_min_cos(f"{KEY}.min_cos:", o["min_cos"]))


# ---- the driver -------------------------------------------------------------------------------------------------------------------------------
_WANT = {"both": 0, "front": 1, "back": -1}


class MeshOrienter(MeshStage):
    """The stage (stage.py: MeshStage) that reads, beside the mesh, the (3, Z, Y, X) uint16 array `<store>/<normals_name>`
    (zarr_lite), samples the array at the vertices under the rule `normal_u16` (`sample_points_numpy`), makes the samples unit
    (`unit_numpy`), classifies the triangles (`face_cos_numpy`, `side_numpy` with `min_cos`) and writes `<stem>_<side>.<ext>`: the
    triangles of that side and the vertices they name (`select_numpy`).  `side="both"` keeps every triangle, the rim included, and
    is named `_oriented`.  `normals="predicted"` writes the unit samples, the sheet normal, with the same sense on both faces;
    `normals="mesh"` writes `vertex_normals_numpy` of the output mesh.

    Device memory is `scratch_bytes(V, T, 3, planes, Y, X)`.  If the whole array fits `max_device_bytes` (default: half of the
    free device memory; on the host: no limit) beside the mesh it is resident.  Otherwise it goes in z-slabs of full planes
    (`slab_ranges`), each holding one plane past its owned range, through two device buffers, so that the next slab is read from
    the store while the launch on the current one runs (one buffer where only two or three planes fit); every slab launch fills
    its own vertices of one (V, 3) buffer, and the output file is the resident run's, byte for byte.  A mesh that does not fit
    beside two planes raises MemoryError.  `where="host"` runs the statements, over the same slabs.  `last_slabs` is the number of
    slabs the last run used."""

    def __init__(self, side="front", min_cos=0.2, normals="predicted", fmt=None, max_device_bytes=None, where="device"):
        self.side = _side("MeshOrienter: side", side)
        self.min_cos = _min_cos("MeshOrienter: min_cos", min_cos)
        self.normals = _normals("MeshOrienter: normals", normals)
        super().__init__(fmt, max_device_bytes)
        if where not in ("device", "host"):
            raise ValueError(f"MeshOrienter: where {where!r} (device or host)")
        self.where, self.last_slabs = where, None

    scratch_bytes = staticmethod(scratch_bytes)

    @property
    def suffix(self):
        return "oriented" if self.side == "both" else self.side

    def plan(self, V, T, shape, itemsize=2):
        """-> (slabs [(z_base, planes)], number of device buffers) for a (C, Z, Y, X) array beside a mesh of V vertices and T triangles"""
        C, Z, Y, X = shape
        budget = self.max_device_bytes
        if budget is None and self.where == "device":
            import torch
            budget = torch.cuda.mem_get_info()[0] // 2
        if budget is None or scratch_bytes(V, T, C, Z, Y, X, itemsize) <= budget:
            return [(0, Z)], 1
        planes = (budget - scratch_bytes(V, T, C, 0, Y, X, itemsize)) // (C * Y * X * itemsize)
        if planes < 2:
            raise MemoryError(f"MeshOrienter: a mesh of {V} vertices and {T} triangles beside two planes of a {C} x {Y} x {X} array needs "
                              f"{scratch_bytes(V, T, C, 2, Y, X, itemsize)} bytes on the device, the budget is {budget}")
        buffers = 2 if planes >= 4 else 1
        return slab_ranges(Z, planes // buffers - 1), buffers

    def _sample(self, src, vertices, slabs, buffers):
        """-> the unit samples, float32 (V, 3) on the host (where="host") or on the device"""
        Z = src.shape[1]
        if self.where == "host":
            out = np.zeros((len(vertices), 3), F32)
            for z_base, planes in slabs:
                part, owned = sample_points_numpy(src[:, z_base:z_base + planes], vertices, "normal_u16", z_base, Z)
                out[owned] = part[owned]
            return unit_numpy(out)
        import torch
        from ..engine import ops
        points = torch.from_numpy(vertices).cuda()
        out = torch.zeros((len(vertices), 3), dtype=torch.float32, device="cuda")
        deepest = max(p for _, p in slabs)
        bufs = [torch.empty((3, deepest) + tuple(src.shape[2:]), dtype=torch.int16, device="cuda") for _ in range(buffers)]      # uint16 bits
        for k, (z_base, planes) in enumerate(slabs):
            host = np.ascontiguousarray(src[:, z_base:z_base + planes])      # read while the launch on the slab before runs
            if buffers == 1 and k:
                torch.cuda.synchronize()      # the one buffer is still being read
            dev = bufs[k % buffers].view(-1)[:host.size].view(host.shape)
            dev.copy_(torch.from_numpy(host.view(np.int16)))
            ops.mesh_sample(dev, points, "normal_u16", z_base=z_base, z_total=Z, unit=True, out=out)
        return out

    def run(self, mesh_path, store, normals_name="normals_final", out=None):
        return super().run(mesh_path, out, store=store, normals_name=normals_name)

    def _work(self, vertices, triangles, store, normals_name):
        from ..dataloading import zarr_lite
        src_path = os.path.join(str(store), normals_name)
        try:
            src = zarr_lite.open(src_path)
        except zarr_lite.ZarrLiteError as e:
            raise ValueError(f"MeshOrienter: {e}") from None
        if src.ndim != 4 or src.shape[0] != 3 or src.dtype != np.uint16:
            raise ValueError(f"MeshOrienter: {src_path} is {src.dtype} {src.shape}; a (3, Z, Y, X) uint16 array is required (channels-last "
                             f"volumes are not read)")
        V, T = len(vertices), len(triangles)
        slabs, buffers = self.plan(V, T, src.shape)
        self.last_slabs = len(slabs)
        want = _WANT[self.side]
        if self.where == "host":
            unit = self._sample(src, vertices, slabs, buffers)
            cos = face_cos_numpy(vertices, triangles, unit)
            side = side_numpy(cos, self.min_cos)
            v, t, (n,), _ = select_numpy(vertices, triangles, np.ones(T, bool) if want == 0 else side == want, unit)
            if self.normals == "mesh":
                n = vertex_normals_numpy(v, t)
        elif V == 0:
            unit, cos, side = np.zeros((0, 3), F32), np.zeros(0, F32), np.zeros(0, np.int8)
            v, t, n = vertices, triangles, np.zeros((0, 3), F32)
        else:
            import torch
            from ..engine import ops
            dunit = self._sample(src, vertices, slabs, buffers)
            dv, dt = torch.from_numpy(vertices).cuda(), torch.from_numpy(triangles).cuda()
            dcos, dside, dused = ops.mesh_face_cos(dv, dt, dunit, self.min_cos, self.side)
            keep = torch.ones(T, dtype=torch.bool, device="cuda") if want == 0 else dside == want
            ov, ot, (on,), _ = ops.mesh_select(dv, dt, keep, (dunit,), used=dused)
            if self.normals == "mesh":
                on = ops.mesh_vertex_normals(ov, ot)
            unit, cos, side = dunit.cpu().numpy(), dcos.cpu().numpy(), dside.cpu().numpy()
            v, t, n = ov.cpu().numpy(), ot.cpu().numpy(), on.cpu().numpy()
        ok = ~np.isnan(cos)
        return v, t, n, dict(vertices=len(v), triangles=len(t), input_vertices=V, input_triangles=T, front=int((side == 1).sum()),
                             back=int((side == -1).sum()), rim=int((side == 0).sum()), zero_normals=int((unit == 0).all(1).sum()),
                             mean_abs_cos=float(np.abs(cos[ok]).astype(np.float64).mean()) if ok.any() else 0.0)
