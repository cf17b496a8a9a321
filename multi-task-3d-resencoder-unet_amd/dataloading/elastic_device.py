"""Smooth non-rigid deformation that moves the image and every target of a sample together and carries a surface-normals target
with it: the one spatial augmentation `spatial_device.py` (rotation, scale) leaves out.  (The reference imports
`volumentations.ElasticTransform` and never calls it; that library has no vector rule.  The statement below is this project's own.)

A deformation is a displacement field D on the OUTPUT grid, out(o) = in(o + D(o)), given by a coarse lattice of control points
and uniform cubic B-splines between them.  `ElasticField` is that record: `nodes` (3, Gz, Gy, Gx) float32, displacements in voxels
along (z, y, x) with the amplitude folded in, and `spacing` (sz, sy, sx), the lattice pitch in voxels.  Because the output grid is
regular, the whole per-axis dependence is three small tables (`bspline_tables`): the first of the four nodes a voxel index uses,
its four weights, and their derivatives.  `displacement_numpy` states D and its Jacobian E, `elastic_numpy` the resampling, one
float32 operation at a time; they are the oracle of the GPU tests and they ARE the host path (`where: host`).  From the
coordinate p = o + D on, sampling is `spatial_device.sample_numpy`, the code `affine_numpy` runs.

A normal is a covector: under the pull-back it is multiplied by the transpose of I + E and keeps its sampled length, a zero
normal stays exactly zero.  For a field that equals a linear map this is `spatial_device`'s rule: the pull-back matrix is the
`point` matrix and its transpose the `vector` matrix.

`DeviceElastic` draws one field per sample of a batch and applies it to the image (trilinear) and to every target (nearest) on
the current stream (csrc/rx_elastic.hip: rx_elastic_apply)."""
import numpy as np

from . import stages
from .spatial_device import BORDER, INTERP, sample_numpy      # noqa: F401

MIN_SPACING = 8          # the kernel's LDS lines are sized for it: 64 voxels touch at most 12 node columns


def _spacing(owner, value):
    v = (value,) * 3 if isinstance(value, (int, np.integer)) and not isinstance(value, bool) else value
    try:
        v = tuple(v)
    except TypeError:
        v = ()
    if len(v) != 3 or any(isinstance(s, bool) or not isinstance(s, (int, np.integer)) or int(s) < MIN_SPACING for s in v):
        raise ValueError(f"{owner}.spacing: {value!r} (an int or [sz, sy, sx], each an int >= {MIN_SPACING})")
    return tuple(int(s) for s in v)


def grid_shape(shape, spacing):
    """G_d = (n_d - 1) // s_d + 4: the nodes a patch of extents `shape` = (Z, Y, X) needs"""
    return tuple((int(n) - 1) // int(s) + 4 for n, s in zip(shape, spacing))


class ElasticField:
    """`nodes`: float32 (3, Gz, Gy, Gx), read-only -- component c of node (gz, gy, gx) is a displacement in voxels along axis c of
    (z, y, x).  `spacing`: (sz, sy, sx), ints >= 8.  It serves every patch shape with `grid_shape(shape, spacing) == nodes.shape[1:]`."""

    def __init__(self, nodes, spacing):
        self.spacing = _spacing("ElasticField", spacing)
        n = np.array(nodes, dtype=np.float32)
        if n.ndim != 4 or n.shape[0] != 3 or min(n.shape[1:]) < 4:
            raise ValueError(f"ElasticField.nodes: expected (3, Gz, Gy, Gx) with every G >= 4, got shape {n.shape}")
        n = np.ascontiguousarray(n)
        n.setflags(write=False)
        self.nodes = n

    @staticmethod
    def zero(shape, spacing):
        spacing = _spacing("ElasticField", spacing)
        return ElasticField(np.zeros((3,) + grid_shape(shape, spacing), dtype=np.float32), spacing)

    def is_identity(self):
        return bool((self.nodes == 0).all())

    def fits(self, shape):
        return len(shape) == 3 and grid_shape(shape, self.spacing) == self.nodes.shape[1:]

    def __eq__(self, other):
        return (isinstance(other, ElasticField) and self.spacing == other.spacing and self.nodes.shape == other.nodes.shape
                and self.nodes.tobytes() == other.nodes.tobytes())

    def __hash__(self):
        return hash((self.spacing, self.nodes.tobytes()))

    def __repr__(self):
        return f"ElasticField(nodes {self.nodes.shape}, max |node| {float(np.abs(self.nodes).max())!r}, spacing={self.spacing})"


def bspline_tables(n, s):
    """one axis of extent `n` at spacing `s` -> (idx int32 [n], w float32 [n, 4], dw float32 [n, 4]).  For o in range(n), in
    float64: u = o / s, i = floor(u), f = u - i; idx[o] = i (voxel o uses nodes i .. i + 3, the largest is G - 1);
        w  = (1-f)^3/6,   (3f^3 - 6f^2 + 4)/6,   (-3f^3 + 3f^2 + 3f + 1)/6,   f^3/6            the uniform cubic B-spline
        dw = -(1-f)^2/2,  (3f^2 - 4f)/2,         (-3f^2 + 2f + 1)/2,          f^2/2,  each / s   d w / d o
    each rounded to float32 once."""
    n, s = int(n), int(s)
    if n < 1 or s < 1:
        raise ValueError(f"bspline_tables: extent {n}, spacing {s}")
    u = np.arange(n, dtype=np.float64) / float(s)
    i = np.floor(u)
    f = u - i
    g = 1.0 - f
    w = np.stack([g * g * g / 6.0, (3.0 * f ** 3 - 6.0 * f ** 2 + 4.0) / 6.0, (-3.0 * f ** 3 + 3.0 * f ** 2 + 3.0 * f + 1.0) / 6.0,
                  f ** 3 / 6.0], axis=1)
    dw = np.stack([-(g * g) / 2.0, (3.0 * f ** 2 - 4.0 * f) / 2.0, (-3.0 * f ** 2 + 2.0 * f + 1.0) / 2.0, f ** 2 / 2.0], axis=1) / float(s)
    return i.astype(np.int32), np.ascontiguousarray(w.astype(np.float32)), np.ascontiguousarray(dw.astype(np.float32))


def _sum4(w, v, axis_of_v, idx):
    """sum over a of w[:, a] * v[.. idx + a ..] along `axis_of_v`, float32: the first product, then + the others left to right.
    `w` [n, 4], `idx` [n]: the result has extent n where `v` had its nodes."""
    shape = [1] * v.ndim
    shape[axis_of_v] = -1
    acc = None
    for a in range(4):
        term = w[:, a].reshape(shape) * np.take(v, idx + a, axis=axis_of_v)
        acc = term if acc is None else acc + term
    return acc


def displacement_numpy(field, shape):
    """(D, E) of `field` on the voxels of a (Z, Y, X) patch: D float32 (3, Z, Y, X), D[c] the displacement along axis c of (z, y, x);
    E float32 (3, 3, Z, Y, X), E[d][e] = dD_d / do_e.  Everything float32, one rounding per operation, nothing contracted into an
    fma; every sum starts from its first product and adds left to right over the four terms.  With (idx, w, dw) the tables of an
    axis and iz, iy, ix = idx_z[oz], idx_y[oy], idx_x[ox]:
        L1[c][b][k] = sum_a wz[oz][a] * nodes[c][iz+a][iy+b][ix+k]
        L2[c][k]    = sum_b wy[oy][b] * L1[c][b][k]
        D_c         = sum_k wx[ox][k] * L2[c][k]
    z, then y, then x: for a fixed (oz, oy) the L2 line serves the whole x row.  E[d][e] is the same three sums with dw on axis e
    and w on the other two."""
    shape = tuple(int(v) for v in shape)
    if not field.fits(shape):
        raise ValueError(f"displacement_numpy: nodes {field.nodes.shape[1:]} at spacing {field.spacing} do not fit a patch of {shape} "
                         f"(they would be {grid_shape(shape, field.spacing) if len(shape) == 3 else '3-D'})")
    (iz, wz, dwz), (iy, wy, dwy), (ix, wx, dwx) = (bspline_tables(n, s) for n, s in zip(shape, field.spacing))
    iz, iy, ix = iz.astype(np.int64), iy.astype(np.int64), ix.astype(np.int64)
    nodes = field.nodes
    with np.errstate(over="ignore", invalid="ignore"):
        l1, l1d = _sum4(wz, nodes, 1, iz), _sum4(dwz, nodes, 1, iz)                                  # (3, Z, Gy, Gx)
        l2, l2z, l2y = _sum4(wy, l1, 2, iy), _sum4(wy, l1d, 2, iy), _sum4(dwy, l1, 2, iy)              # (3, Z, Y, Gx)
        D = _sum4(wx, l2, 3, ix)
        E = np.stack([_sum4(wx, l2z, 3, ix), _sum4(wx, l2y, 3, ix), _sum4(dwx, l2, 3, ix)], axis=1)    # [d][e]
    return np.ascontiguousarray(D, dtype=np.float32), np.ascontiguousarray(E, dtype=np.float32)


def vector_rule_numpy(s, E):
    """the vector rule on sampled components: `s` float32 (3, ...) in channel order (Nx, Ny, Nz), `E` float32 (3, 3, ...) in (z, y, x)
    order -> the output channels (see `elastic_numpy`)"""
    f32 = np.float32
    n = (s[2], s[1], s[0])                                                      # (n_z, n_y, n_x)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        t = [n[e] + ((E[0][e] * n[0] + E[1][e] * n[1]) + E[2][e] * n[2]) for e in range(3)]
        q = (s[0] * s[0] + s[1] * s[1]) + s[2] * s[2]
        r = (t[2] * t[2] + t[1] * t[1]) + t[0] * t[0]
        k = np.where(r > 0, np.sqrt(q / np.where(r > 0, r, f32(1.0))), f32(0.0)).astype(f32)
        return np.stack([t[2] * k, t[1] * k, t[0] * k])


def elastic_numpy(field, arr, interp, border, fill=0.0, is_normal=False):
    """What rx_elastic_apply computes, in numpy: (Z, Y, X) or (C, Z, Y, X) float32 in, a new contiguous float32 array out.  Every
    arithmetic step is ONE float32 operation (round to nearest even, denormals kept), in the order written.

    Coordinates: with (D, E) = displacement_numpy(field, (Z, Y, X)),   p_d = float32(o_d) + D_d.
    From p_d on the rules are `affine_numpy`'s (spatial_device.sample_numpy is the code): interp "linear" / "nearest", border
    "constant" (`fill` outside) / "clamp", the index squashing, the lerp order x, y, z.  All channels share one set of coordinates.

    is_normal (needs C = 3, channels (Nx, Ny, Nz)): with s the three sampled components and (n_z, n_y, n_x) = (s_2, s_1, s_0), a
    normal is a covector; under the pull-back out(o) = in(o + D(o)) it becomes, per axis e,
        t_e = n_e + ((E[z][e] * n_z + E[y][e] * n_y) + E[x][e] * n_x)
    and keeps the sampled length:
        q = (s_0*s_0 + s_1*s_1) + s_2*s_2        r = (t_x*t_x + t_y*t_y) + t_z*t_z        k = sqrt(q / r) if r > 0 else 0
    (sqrt and / correctly rounded).  Output channel j is t_(x, y, z)[j] * k; a zero normal stays == 0.

    Nodes of any finite size are served: a coordinate beyond the int range counts as outside; a NaN coordinate yields an unspecified
    value and never an access outside the array."""
    arr, a = stages.check_resample_args("elastic_numpy", arr, interp, border, is_normal)
    n = a.shape[1:]
    f32 = np.float32
    D, E = displacement_numpy(field, n)
    shp = [(-1, 1, 1), (1, -1, 1), (1, 1, -1)]
    with np.errstate(over="ignore", invalid="ignore"):
        p = [np.arange(n[d], dtype=f32).reshape(shp[d]) + D[d] for d in range(3)]
        s = sample_numpy(a, p, interp, border, fill)
        if is_normal:
            s = vector_rule_numpy(s, E)
    return stages.finish_resample(s, arr)


def apply_item_numpy(field, item, normal_keys=("normals",), image_border="constant", image_fill=0.0):
    """the host path: `field` on every array of a dataset item, under the rules of `stages.apply_item`"""
    return stages.apply_item(item, normal_keys, image_border, image_fill, lambda *a: elastic_numpy(field, *a))


def draw_elastic(rng, shape, spacing, magnitude=(0.0, 4.0), p=0.3):
    """`rng`: a `random.Random` (or the `random` module).  The calls, in this order: one `rng.random()`; if it is not < p, the zero
    field.  Otherwise one a = `rng.uniform(lo, hi)`, then 3 * Gz * Gy * Gx calls `rng.uniform(-1.0, 1.0)` in C order of
    (c, z, y, x), each multiplied by a in float64 and rounded to float32 once."""
    spacing = _spacing("draw_elastic", spacing)
    g = grid_shape(shape, spacing)
    if not rng.random() < p:
        return ElasticField.zero(shape, spacing)
    lo, hi = magnitude
    a = float(rng.uniform(lo, hi))
    count = 3 * g[0] * g[1] * g[2]
    nodes = np.array([rng.uniform(-1.0, 1.0) * a for _ in range(count)], dtype=np.float64).astype(np.float32)
    return ElasticField(nodes.reshape((3,) + g), spacing)


class DeviceElastic:
    """`elastic(batch_dict) -> batch_dict`: every tensor of the dict is a float32 device batch, (B, C, Z, Y, X) or (B, Z, Y, X); one
    field per SAMPLE (`draw_elastic`) moves the image and every target of that sample together.  `image` is sampled linear with
    `image_border` / `image_fill`; every other tensor nearest, constant, fill 0, the tensors named in `normal_keys` with the vector
    rule.  Runs on the CURRENT stream; outputs come from torch's caching allocator there, the nodes go up with one non-blocking
    copy from pinned memory.  The generator is seeded from `torch.initial_seed()` and the rank, as `DeviceSpatial`'s is: ranks
    differ, a seeded run repeats.  `last_fields` keeps the draws of the last call; a batch whose fields are all zero is handed back
    untouched."""

    def __init__(self, spacing=32, magnitude=(0.0, 4.0), p=0.3, normal_keys=("normals",), image_border="constant", image_fill=0.0,
                 seed=None, rank=0):
        self.spacing = _spacing("DeviceElastic", spacing)
        self.magnitude = check_magnitude("DeviceElastic", magnitude, self.spacing)
        self.p = stages.probability("DeviceElastic", "p", p)
        if image_border not in BORDER:
            raise ValueError(f"DeviceElastic.image_border: {image_border!r} (constant or clamp)")
        self.normal_keys = set(normal_keys)
        self.image_border, self.image_fill = image_border, float(image_fill)
        self.rng = stages.stage_rng(seed, rank)
        self.last_fields = None

    def draw(self, shape):
        return draw_elastic(self.rng, shape, self.spacing, self.magnitude, self.p)

    def __call__(self, batch, fields=None):
        from ..engine import ops as E
        from ..engine.lib import RxError
        B, shape = stages.check_batch("DeviceElastic", batch, self.normal_keys, "the host path is elastic_device.elastic_numpy")
        for k, t in batch.items():
            if tuple(int(v) for v in t.shape[-3:]) != shape:
                raise RxError(f"DeviceElastic: {k!r} {tuple(t.shape)}: every tensor of a batch has the extents {shape}")
        self.last_fields = fields = stages.batch_draws("DeviceElastic", "fields", fields, B, lambda: self.draw(shape))
        if all(f.is_identity() for f in fields):
            return batch
        spacing = fields[0].spacing
        nodes = E.elastic_nodes(fields)
        tables = E.elastic_tables(shape, spacing, next(iter(batch.values())).device)
        return stages.resample_batch(batch, self.normal_keys, self.image_border, self.image_fill,
                                     lambda five, *mode, **kw: E.elastic_apply(five, nodes, tables, spacing, *mode, **kw))


# ---- dataset_config.elastic ---------------------------------------------------------------------------------------------------------
def check_magnitude(owner, value, spacing):
    """[lo, hi], the largest node displacement in voxels: 0 <= lo <= hi < min(spacing) / 6.  The upper limit is derived, not tuned:
    the weights are convex, so |D_d| <= a and |E[d][e]| <= 2a / s_e; then I + E is strictly diagonally dominant -- the map cannot
    fold -- whenever 6 hi / min(spacing) < 1."""
    try:
        lo, hi = (float(v) for v in value)
    except (TypeError, ValueError):
        raise ValueError(f"{owner}.magnitude: {value!r} (two numbers, 0 <= lo <= hi < min(spacing) / 6)") from None
    limit = min(spacing) / 6.0
    if not 0.0 <= lo <= hi:
        raise ValueError(f"{owner}.magnitude: {list(value)} (0 <= lo <= hi < min(spacing) / 6 = {limit:g})")
    if not hi < limit:
        raise ValueError(f"{owner}.magnitude: hi = {hi:g} is not below min(spacing) / 6 = {limit:g}: beyond it I + E is no longer "
                         "diagonally dominant and the deformation may fold")
    return lo, hi


def parse_elastic(dataset_config, patch_size, tasks):
    """`dataset_config.elastic` -> None (absent / false) or {"spacing": (sz, sy, sx), "magnitude": (lo, hi), "p": float,
    "normal_keys": tuple, "image_border": "constant" | "clamp", "where": "device" | "host"}.  Everything that would otherwise fail
    at some later step fails here, with the key named."""
    g = stages.block(dataset_config, "elastic", ("spacing", "magnitude", "p", "normal_keys", "image_border", "where"), "device", None)
    if g is None:
        return None
    stages.patch3d("dataset_config.elastic", patch_size)
    spacing = _spacing("dataset_config.elastic", g.get("spacing", 32))
    return {"spacing": spacing, "magnitude": check_magnitude("dataset_config.elastic", g.get("magnitude", (0.0, 4.0)), spacing),
            "p": stages.probability("dataset_config.elastic", "p", g.get("p", 0.3)),
            "image_border": stages.image_border("dataset_config.elastic", g), "where": g["where"],
            "normal_keys": stages.normal_keys("dataset_config.elastic", g, tasks)}
