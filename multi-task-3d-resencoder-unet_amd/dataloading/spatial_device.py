"""Small-angle rotation and mild isotropic scaling that move the image and every target of a sample together and turn a
surface-normals target with them: the continuous counterpart of `geometry_device.py`'s 48 signed axis permutations.  (The reference
imports an `ElasticTransform` it never calls; its `RandomRotate90WithNormals` shows the intent: rotation with the vector rule.)

Any chain of rotations and scalings about the patch centre is, per array, ONE resampling pass

    out[c][o] = sum_k vector[c][k] * sample(in[k], p(o)),      p(o) = point @ (o - centre) + centre

`AffineOp` is that record: `point` (3 x 3, (z, y, x) axis order) maps OUTPUT voxel offsets to INPUT voxel offsets -- sampling goes
through the inverse of what the content does -- and `vector` (3 x 3, component order (Nx, Ny, Nz) = 0, 1, 2 as in
`geometry_device`) is the forward rotation of a vector field, applied to the arrays named in `normal_keys` only (the identity for
every other array).  Chains compose on the host in float64 (`compose`) and are rounded to float32 once, so the device needs one
pass per tensor whatever was drawn (csrc/rx_affine.hip: rx_affine_apply).  `affine_numpy` states what the kernel computes, one
float32 operation at a time; it is the oracle of the GPU tests and it IS the host path (`where: host`).

`DeviceSpatial` draws one op per sample of a batch (rotation, then scale) and applies it to the image (trilinear) and to every
target (nearest: a dilated label stays binary, a normals target stays exactly zero off the sheet) on the current stream."""
import math
from dataclasses import dataclass

import numpy as np

from ..engine.ops.core import BORDER, INTERP      # noqa: F401 -- the library's codes, kept beside its binding
from . import stages
from .geometry_device import AXIS_OF
from .stages import MAX_EXTENT      # noqa: F401


def _matrix(owner, name, value):
    m64 = np.eye(3) if value is None else np.array(value, dtype=np.float64)
    if m64.shape != (3, 3):
        raise ValueError(f"{owner}.{name}: expected a 3 x 3 matrix, got shape {m64.shape}")
    with np.errstate(over="ignore"):
        m32 = m64.astype(np.float32)
    if not np.isfinite(m64).all() or not np.isfinite(m32).all():
        raise ValueError(f"{owner}.{name}: every entry must be finite in float32, got {m64.tolist()}")
    m64.setflags(write=False)
    m32.setflags(write=False)
    return m64, m32


@dataclass(frozen=True, eq=False)
class AffineOp:
    """`point`, `vector`: 3 x 3 float32 (read-only).  The float64 matrices they were rounded from are kept (`point64`, `vector64`):
    `compose` multiplies those, so a chain is rounded to float32 once, however long it is."""
    point: np.ndarray = None
    vector: np.ndarray = None

    def __post_init__(self):
        for name in ("point", "vector"):
            m64, m32 = _matrix("AffineOp", name, getattr(self, name))
            object.__setattr__(self, name + "64", m64)
            object.__setattr__(self, name, m32)

    @staticmethod
    def identity():
        return AffineOp()

    def is_identity(self):
        eye = np.eye(3, dtype=np.float32)
        return bool((self.point == eye).all() and (self.vector == eye).all())

    def row(self):
        """the 18 float32 of `rx_affine_sample` (include/rxunet.h): point row-major, then vector row-major"""
        return np.concatenate([self.point.ravel(), self.vector.ravel()])

    def __eq__(self, other):
        return isinstance(other, AffineOp) and self.row().tobytes() == other.row().tobytes()

    def __hash__(self):
        return hash(self.row().tobytes())

    def __repr__(self):
        return f"AffineOp(point={self.point.tolist()}, vector={self.vector.tolist()})"


def compose(a, b):
    """`a`, then `b`: the field is turned by `a.vector` first, and an output voxel is traced back through `b`'s map first"""
    return AffineOp(a.point64 @ b.point64, b.vector64 @ a.vector64)


def rotation_op(axis, degrees):
    """the content turns by `degrees` about `axis` ("z" / "y" / "x" or 0 / 1 / 2) through the patch centre, in the sense of
    `geometry_device.rot90_op(axis, 1)` at 90 degrees (np.rot90 in the plane of the other two axes, with the reference's component
    rule).  `vector` is that rotation of the components; `point` is its inverse, written in (z, y, x) order."""
    ax = AXIS_OF[axis.lower()] if isinstance(axis, str) else int(axis)
    if ax not in (0, 1, 2):
        raise ValueError(f"rotation_op: axis {axis!r} (z, y, x or 0, 1, 2)")
    th = math.radians(float(degrees))
    c, s = math.cos(th), math.sin(th)
    if ax == 0:          # about z: (Nx, Ny) <- (Ny, -Nx) at 90 degrees
        v = [[c, s, 0.0], [-s, c, 0.0], [0.0, 0.0, 1.0]]
    elif ax == 1:        # about y: (Nx, Nz) <- (Nz, -Nx)
        v = [[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]]
    else:                # about x: (Ny, Nz) <- (Nz, -Ny)
        v = [[1.0, 0.0, 0.0], [0.0, c, s], [0.0, -s, c]]
    v = np.array(v, dtype=np.float64)
    return AffineOp(v.T[::-1, ::-1], v)      # inverse = transpose; (x, y, z) -> (z, y, x) reverses rows and columns


def scale_op(s):
    """isotropic: the sampling grid is stretched by `s` about the centre (`point` = s * identity), so the content appears at
    1 / s of its size: s > 1 zooms out (sources leave the patch and take the border rule), s < 1 zooms in.  `vector` is the
    identity: an isotropic scaling keeps every direction."""
    s = float(s)
    if not math.isfinite(s) or s <= 0.0:
        raise ValueError(f"scale_op: {s!r} is not a positive scale")
    return AffineOp(np.eye(3) * s, None)


def from_geom(op):
    """the exact 0 / +-1 matrices of a signed permutation (`geometry_device.GeomOp`); for a shape the op preserves,
    `affine_numpy(from_geom(op), ...)` is `apply_op_numpy(op, ...)`"""
    p, v = np.zeros((3, 3)), np.zeros((3, 3))
    for d in range(3):
        p[op.src_axis[d], d] = -1.0 if op.flip[d] else 1.0
        v[d, op.ch_src[d]] = -1.0 if op.ch_neg[d] else 1.0
    return AffineOp(p, v)


def draw_affine(rng, rotation=None, scale=None):
    """`rng`: a `random.Random` (or the `random` module).  The calls, in this order:
      rotation = {axes, max_degrees, p} (None: off): one `rng.random()`; if it is < p, one `rng.uniform(-max_degrees, max_degrees)`
                 per listed axis, in listed order, the rotations composed in that order
      scale    = {range: [lo, hi], p} (None: off):   one `rng.random()`; if it is < p, one `rng.uniform(lo, hi)`
    The result is rotation, then scale."""
    op = AffineOp()
    if rotation is not None:
        if rng.random() < rotation.get("p", 0.5):
            m = float(rotation.get("max_degrees", 30.0))
            for ax in rotation.get("axes", ("z", "y", "x")):
                op = compose(op, rotation_op(ax, rng.uniform(-m, m)))
    if scale is not None:
        if rng.random() < scale.get("p", 0.5):
            lo, hi = scale.get("range", (0.8, 1.25))
            op = compose(op, scale_op(rng.uniform(lo, hi)))
    return op


def _axis_index(v, n, lo):
    """a float32 array of whole numbers -> int64 indices; anything below `lo` becomes `lo`, anything above n (a NaN too) becomes n"""
    return np.fmax(np.fmin(v, np.float32(n)), np.float32(lo)).astype(np.int64)


def sample_numpy(a, p, interp, border, fill=0.0):
    """the sampling half of `affine_numpy`, from the coordinates on: `a` float32 (C, Z, Y, X), `p` = (p_z, p_y, p_x) float32 arrays
    that broadcast to (Z, Y, X) -> the sampled (C, Z, Y, X) values under the interp / border rules stated there (the index
    squashing and the lerp order included).  `elastic_device.elastic_numpy` samples through it with coordinates of its own."""
    f32 = np.float32
    n = a.shape[1:]
    with np.errstate(over="ignore", invalid="ignore"):
        fillv = f32(fill)
        flat = a.reshape(a.shape[0], -1)
        stride = (n[1] * n[2], n[2], 1)

        def fetch(idx):
            """idx: per axis (int64 index array, whole-number float array it came from) -> (C, Z, Y, X) values under the border rule"""
            off, ok = 0, True
            for d in range(3):
                ii, fi = idx[d]
                if border == "constant":
                    ok = ok & (fi >= 0) & (fi <= f32(n[d] - 1))
                off = off + np.clip(ii, 0, n[d] - 1) * stride[d]
            v = flat[:, off]
            return np.where(ok, v, fillv) if border == "constant" else v

        if interp == "nearest":
            r = [np.floor(p[d] + f32(0.5)) for d in range(3)]
            s = fetch([(_axis_index(r[d], n[d], -1), r[d]) for d in range(3)])
        else:
            i0 = [np.floor(p[d]) for d in range(3)]
            f = [p[d] - i0[d] for d in range(3)]
            lo = [_axis_index(i0[d], n[d], -2) for d in range(3)]
            # (index, the float it stands for): i + 1 of a clamped index is outside whenever i + 1 of the true one is
            ax = [((lo[d], lo[d].astype(f32)), (lo[d] + 1, (lo[d] + 1).astype(f32))) for d in range(3)]

            def lerp(u, w, fr):
                return u + fr * (w - u)
            zs = []
            for kz in (0, 1):
                ys = []
                for ky in (0, 1):
                    u = fetch([ax[0][kz], ax[1][ky], ax[2][0]])
                    w = fetch([ax[0][kz], ax[1][ky], ax[2][1]])
                    ys.append(lerp(u, w, f[2]))
                zs.append(lerp(ys[0], ys[1], f[1]))
            s = lerp(zs[0], zs[1], f[0])
    return s


def affine_numpy(op, arr, interp, border, fill=0.0, is_normal=False):
    """What rx_affine_apply computes, in numpy: (Z, Y, X) or (C, Z, Y, X) float32 in, a new contiguous float32 array out.  EVERY
    arithmetic step below is ONE float32 operation (round to nearest even, denormals kept), in the order written, so a kernel that
    does not contract a multiply and an add into an fma reproduces it bit for bit.

    Coordinates, for output voxel o and axis d in (z, y, x), with m = op.point and n = (Z, Y, X):
        c_d = float32(n_d - 1) * 0.5            t_d = float32(o_d) - c_d
        p_d = ((m[d][0] * t_z + m[d][1] * t_y) + m[d][2] * t_x) + c_d
    interp = "linear":   i_d = floor(p_d), f_d = p_d - i_d; the eight corners are i and i + 1 per axis;
                         lerp(a, b, f) = a + f * (b - a), along x first (four), then y (two), then z (one)
    interp = "nearest":  the source index is floor(p_d + 0.5) per axis
    border = "constant": a corner / source voxel with any index outside [0, n_d - 1] has the value float32(fill)
    border = "clamp":    every index is clamped to [0, n_d - 1]
    is_normal (needs C = 3): with s the three sampled components and v = op.vector,
        out_c = (v[c][0] * s_0 + v[c][1] * s_1) + v[c][2] * s_2
    and nothing is renormalised (a rotation keeps length).  All channels of a sample share one set of coordinates.

    A coordinate beyond the int range (a huge matrix entry) counts as outside; one that overflowed to NaN yields an unspecified
    value and never an access outside the array."""
    arr, a = stages.check_resample_args("affine_numpy", arr, interp, border, is_normal)
    n = a.shape[1:]
    f32 = np.float32
    m = op.point
    c = [f32(n[d] - 1) * f32(0.5) for d in range(3)]
    shp = [(-1, 1, 1), (1, -1, 1), (1, 1, -1)]
    t = [(np.arange(n[d], dtype=f32) - c[d]).reshape(shp[d]) for d in range(3)]
    with np.errstate(over="ignore", invalid="ignore"):
        p = [((m[d, 0] * t[0] + m[d, 1] * t[1]) + m[d, 2] * t[2]) + c[d] for d in range(3)]
        s = sample_numpy(a, p, interp, border, fill)
        if is_normal:
            v = op.vector
            s = np.stack([(v[k, 0] * s[0] + v[k, 1] * s[1]) + v[k, 2] * s[2] for k in range(3)])
    return stages.finish_resample(s, arr)


def apply_item_numpy(op, item, normal_keys=("normals",), image_border="constant", image_fill=0.0):
    """the host path: `op` on every array of a dataset item, under the rules of `stages.apply_item`"""
    return stages.apply_item(item, normal_keys, image_border, image_fill, lambda *a: affine_numpy(op, *a))


class DeviceSpatial:
    """`spatial(batch_dict) -> batch_dict`: every tensor of the dict is a float32 device batch, (B, C, Z, Y, X) or (B, Z, Y, X);
    one op per SAMPLE (rotation, then scale: `draw_affine`) moves the image and every target of that sample together.  `image` is
    sampled linear with `image_border` / `image_fill`; every other tensor nearest, constant, fill 0, the tensors named in
    `normal_keys` with the vector rule.  `rotation` / `scale`: the blocks of `draw_affine` (None: off).  Runs on the CURRENT stream;
    outputs come from torch's caching allocator there.  The generator is seeded from `torch.initial_seed()` and the rank, as
    `DeviceGeometry`'s is: ranks differ, a seeded run repeats.  `last_ops` keeps the draws of the last call; a batch whose ops are
    all the identity is handed back untouched."""

    def __init__(self, rotation=None, scale=None, normal_keys=("normals",), image_border="constant", image_fill=0.0, seed=None, rank=0):
        self.rotation = check_rotation("DeviceSpatial", rotation)
        self.scale = check_scale("DeviceSpatial", scale)
        if image_border not in BORDER:
            raise ValueError(f"DeviceSpatial.image_border: {image_border!r} (constant or clamp)")
        self.normal_keys = set(normal_keys)
        self.image_border, self.image_fill = image_border, float(image_fill)
        self.rng = stages.stage_rng(seed, rank)
        self.last_ops = None

    def draw(self):
        return draw_affine(self.rng, self.rotation, self.scale)

    def __call__(self, batch, ops=None):
        from ..engine import ops as E
        B, _ = stages.check_batch("DeviceSpatial", batch, self.normal_keys, "the host path is spatial_device.affine_numpy")
        self.last_ops = ops = stages.batch_draws("DeviceSpatial", "ops", ops, B, self.draw)
        if all(op.is_identity() for op in ops):
            return batch
        table = E.affine_table(ops)
        return stages.resample_batch(batch, self.normal_keys, self.image_border, self.image_fill,
                                     lambda five, *mode, **kw: E.affine_apply(five, table, *mode, **kw))


# ---- dataset_config.spatial ---------------------------------------------------------------------------------------------------------
def check_rotation(owner, kw):
    """the `rotation` block as a config block or a constructor argument: None / False -> None (off), True -> the defaults"""
    if kw is None or kw is False:
        return None
    kw = {} if kw is True else kw
    known = {"axes", "max_degrees", "p"}
    if not isinstance(kw, dict) or set(kw) - known:
        bad = sorted(set(kw) - known) if isinstance(kw, dict) else kw
        raise ValueError(f"{owner}.rotation: unknown key(s) {bad} (known: {sorted(known)})")
    v = kw.get("axes", ("z", "y", "x"))
    axes = tuple(str(a).lower() for a in ((v,) if isinstance(v, str) else v))
    if not axes or any(a not in AXIS_OF for a in axes):
        raise ValueError(f"{owner}.rotation.axes: {list(axes)} (a non-empty list of z, y, x)")
    deg = float(kw.get("max_degrees", 30.0))
    if not 0.0 < deg <= 180.0:
        raise ValueError(f"{owner}.rotation.max_degrees: {kw.get('max_degrees')!r} is outside (0, 180]")
    return {"axes": axes, "max_degrees": deg, "p": stages.probability(f"{owner}.rotation", "p", kw.get("p", 0.5))}


def check_scale(owner, kw):
    """the `scale` block: None / False -> None (off), True -> the defaults"""
    if kw is None or kw is False:
        return None
    kw = {} if kw is True else kw
    known = {"range", "p"}
    if not isinstance(kw, dict) or set(kw) - known:
        bad = sorted(set(kw) - known) if isinstance(kw, dict) else kw
        raise ValueError(f"{owner}.scale: unknown key(s) {bad} (known: {sorted(known)})")
    r = kw.get("range", (0.8, 1.25))
    try:
        lo, hi = (float(v) for v in r)
    except (TypeError, ValueError):
        raise ValueError(f"{owner}.scale.range: {r!r} (two numbers, 0.5 <= lo <= hi <= 2)") from None
    if not 0.5 <= lo <= hi <= 2.0:
        raise ValueError(f"{owner}.scale.range: {list(r)} (0.5 <= lo <= hi <= 2)")
    return {"range": (lo, hi), "p": stages.probability(f"{owner}.scale", "p", kw.get("p", 0.5))}


def parse_spatial(dataset_config, patch_size, tasks):
    """`dataset_config.spatial` -> None (absent / false) or {"rotation": block | None, "scale": block | None, "normal_keys": tuple,
    "image_border": "constant" | "clamp", "where": "device" | "host"}.  Everything that would otherwise fail at some later step
    fails here, with the key named."""
    g = stages.block(dataset_config, "spatial", ("rotation", "scale", "normal_keys", "image_border", "where"), "device", None)
    if g is None:
        return None
    stages.patch3d("dataset_config.spatial", patch_size)
    return {"rotation": check_rotation("dataset_config.spatial", g.get("rotation", None)),
            "scale": check_scale("dataset_config.spatial", g.get("scale", None)),
            "image_border": stages.image_border("dataset_config.spatial", g), "where": g["where"],
            "normal_keys": stages.normal_keys("dataset_config.spatial", g, tasks)}
