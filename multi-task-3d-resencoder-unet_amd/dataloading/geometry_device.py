"""Axis flips and 90-degree rotations that keep a surface-normals target consistent -- the behaviour of the reference's
training/transforms/geometric/geometry.py (RandomFlipWithNormals, RandomRotate90WithNormals) -- as ONE op per sample.

Any chain of those transforms is, per array, a pure gather

    out[c][o] = (-1)^ch_neg[c] * in[ch_src[c]][i],      i[src_axis[d]] = n_d - 1 - o_d if flip[d] else o_d      (d = 0, 1, 2 = z, y, x)

with `src_axis` / `flip` a signed permutation of the axes and `ch_src` / `ch_neg` a signed permutation of the three components
(applied to the arrays named in `normal_keys` only).  `GeomOp` is that record; chains compose on the host (`compose`), so the
device needs one pass per tensor whatever was drawn (csrc/rx_geometry.hip: rx_geom_apply).  `draw_flip` / `draw_rot90` make
the same `random` calls in the same order as the reference classes; `apply_op_numpy` states what the kernel computes and is the
oracle of the GPU tests; the host classes (training/transforms/geometric/geometry.py) are `draw` + `apply_op_numpy`.
Negation is IEEE negation: an exact zero becomes -0.0, as the reference's `*= -1` and unary minus give.

`DeviceGeometry` draws one composed op per sample of a batch (flip, then rot90) and applies it to the image and to every target
on the current stream."""
from dataclasses import dataclass

import numpy as np

from . import stages

AXIS_OF = {"z": 0, "y": 1, "x": 2}
# rotation about an axis turns the plane of the other two: np.rot90(arr, k, axes=PLANE[axis]) on a (Z, Y, X) volume
PLANE = {"z": (1, 2), "y": (0, 2), "x": (0, 1)}
# the component rule of a rotated normals array (Nx, Ny, Nz = components 0, 1, 2), as the reference applies it:
# (axis, k) -> (ch_src, ch_neg)
ROT_COMPONENTS = {
    ("z", 1): ((1, 0, 2), (0, 1, 0)), ("z", 2): ((0, 1, 2), (1, 1, 0)), ("z", 3): ((1, 0, 2), (1, 0, 0)),
    ("y", 1): ((2, 1, 0), (0, 0, 1)), ("y", 2): ((0, 1, 2), (1, 0, 1)), ("y", 3): ((2, 1, 0), (1, 0, 0)),
    ("x", 1): ((0, 2, 1), (0, 0, 1)), ("x", 2): ((0, 1, 2), (0, 1, 1)), ("x", 3): ((0, 2, 1), (0, 1, 0)),
}


@dataclass(frozen=True)
class GeomOp:
    src_axis: tuple = (0, 1, 2)
    flip: tuple = (0, 0, 0)
    ch_src: tuple = (0, 1, 2)
    ch_neg: tuple = (0, 0, 0)

    def __post_init__(self):
        for name in ("src_axis", "flip", "ch_src", "ch_neg"):
            object.__setattr__(self, name, tuple(int(v) for v in getattr(self, name)))
        if sorted(self.src_axis) != [0, 1, 2] or sorted(self.ch_src) != [0, 1, 2]:
            raise ValueError(f"GeomOp: src_axis {self.src_axis} and ch_src {self.ch_src} must be permutations of (0, 1, 2)")
        object.__setattr__(self, "flip", tuple(int(bool(v)) for v in self.flip))
        object.__setattr__(self, "ch_neg", tuple(int(bool(v)) for v in self.ch_neg))

    @staticmethod
    def identity():
        return GeomOp()

    def is_identity(self):
        return self == GeomOp()

    def inverse(self):
        """the op that undoes this one: compose(op, op.inverse()) is the identity"""
        src = tuple(self.src_axis.index(d) for d in range(3))
        ch = tuple(self.ch_src.index(c) for c in range(3))
        return GeomOp(src, tuple(self.flip[src[d]] for d in range(3)), ch, tuple(self.ch_neg[ch[c]] for c in range(3)))

    def preserves(self, shape):
        """True when the op maps a volume of (the last three extents of) `shape` onto one of the same shape"""
        ext = tuple(int(v) for v in tuple(shape)[-3:])
        return all(ext[self.src_axis[d]] == ext[d] for d in range(3))

    def row(self):
        """the 12 integers of `rx_geom_sample` (include/rxunet.h)"""
        return self.src_axis + self.flip + self.ch_src + self.ch_neg

    @staticmethod
    def from_row(row):
        r = [int(v) for v in row]
        return GeomOp(r[0:3], r[3:6], r[6:9], r[9:12])


def compose(a, b):
    """`a`, then `b`"""
    return GeomOp(tuple(a.src_axis[b.src_axis[d]] for d in range(3)),
                  tuple(b.flip[d] ^ a.flip[b.src_axis[d]] for d in range(3)),
                  tuple(a.ch_src[b.ch_src[c]] for c in range(3)),
                  tuple(b.ch_neg[c] ^ a.ch_neg[b.ch_src[c]] for c in range(3)))


def flip_op(axis):
    """a flip along z / y / x (0 / 1 / 2); the normal component along that axis (2 / 1 / 0: components are x, y, z) changes sign"""
    f, n = [0, 0, 0], [0, 0, 0]
    f[axis], n[2 - axis] = 1, 1
    return GeomOp(flip=f, ch_neg=n)


def rot90_op(axis, k):
    """np.rot90(arr, k, axes=PLANE[axis]) of a (Z, Y, X) volume, k in 1..3, with the reference's component rule"""
    a1, a2 = PLANE[axis]
    src, f = [0, 1, 2], [0, 0, 0]
    if k == 2:
        f[a1] = f[a2] = 1
    else:          # k = 1: out[.., i, j] = in[.., j, n - 1 - i];  k = 3: out[.., i, j] = in[.., n - 1 - j, i]
        src[a1], src[a2] = a2, a1
        f[a1 if k == 1 else a2] = 1
    ch, neg = ROT_COMPONENTS[(axis, k)]
    return GeomOp(src, f, ch, neg)


def draw_flip(rng, p=0.5, p_transform=1.0):
    """the draws of RandomFlipWithNormals.__call__: one for `p_transform`, then one per axis Z, Y, X"""
    op = GeomOp()
    if rng.random() >= p_transform:
        return op
    for axis in (0, 1, 2):
        if rng.random() < p:
            op = compose(op, flip_op(axis))
    return op


def draw_rot90(rng, axes=("x", "y", "z"), p=0.5, p_transform=1.0):
    """the draws of RandomRotate90WithNormals.__call__: `p_transform`, `p`, choice(axes), choice([1, 2, 3])"""
    if rng.random() >= p_transform:
        return GeomOp()
    if rng.random() >= p:
        return GeomOp()
    axis = rng.choice(axes)
    k = rng.choice([1, 2, 3])
    return rot90_op(axis, k)


def apply_op_numpy(op, arr, is_normal=False):
    """what rx_geom_apply computes, in numpy: (Z, Y, X) or (C, Z, Y, X) in, a new contiguous array out"""
    arr = np.asarray(arr)
    a = arr[None] if arr.ndim == 3 else arr
    if a.ndim != 4:
        raise ValueError(f"apply_op_numpy: expected (Z, Y, X) or (C, Z, Y, X), got {arr.shape}")
    t = a.transpose(0, 1 + op.src_axis[0], 1 + op.src_axis[1], 1 + op.src_axis[2])
    for d in range(3):
        if op.flip[d]:
            t = np.flip(t, axis=1 + d)
    if is_normal:
        if a.shape[0] != 3:
            raise ValueError(f"apply_op_numpy: a normals array has 3 components, got {a.shape[0]}")
        t = np.stack([np.negative(t[op.ch_src[c]]) if op.ch_neg[c] else t[op.ch_src[c]] for c in range(3)])
    out = np.ascontiguousarray(t)
    if out is a or np.shares_memory(out, arr):
        out = out.copy()
    return out[0] if arr.ndim == 3 else out


def allowed_rot90_axes(patch_shape):
    """the rotation axes whose plane has equal extents (a 90-degree turn of any other plane changes the patch's shape)"""
    ext = tuple(int(v) for v in patch_shape)
    return tuple(ax for ax in ("x", "y", "z") if ext[PLANE[ax][0]] == ext[PLANE[ax][1]])


class DeviceGeometry:
    """`geometry(batch_dict) -> batch_dict`: every tensor of the dict is a float32 device batch, (B, C, Z, Y, X) or (B, Z, Y, X);
    one composed op per SAMPLE (flip, then rot90) moves the image and every target of that sample together, the tensors named in
    `normal_keys` with the component rule.  `flip` / `rot90`: the keyword arguments of `draw_flip` / `draw_rot90` (None: that
    transform is off).  Runs on the CURRENT stream; outputs come from torch's caching allocator there (`DeviceFeeder` calls
    `record_stream` on what it hands over).  The generator is seeded from `torch.initial_seed()` and the rank, as
    `DeviceAugmenter`'s is: ranks differ, a seeded run repeats.  `last_ops` keeps the draws of the last call."""

    def __init__(self, flip=None, rot90=None, normal_keys=("normals",), seed=None, rank=0):
        self.flip = check_transform_kwargs("DeviceGeometry", "flip", flip)
        self.rot90 = check_transform_kwargs("DeviceGeometry", "rot90", rot90)
        self.normal_keys = set(normal_keys)
        self.rng = stages.stage_rng(seed, rank)
        self.last_ops = None

    def draw(self):
        op = GeomOp()
        if self.flip is not None:
            op = compose(op, draw_flip(self.rng, **self.flip))
        if self.rot90 is not None:
            op = compose(op, draw_rot90(self.rng, **self.rot90))
        return op

    def __call__(self, batch, ops=None):
        from ..engine import ops as E
        B, _ = stages.check_batch("DeviceGeometry", batch, self.normal_keys, "the host classes are training/transforms/geometric")
        ops = stages.batch_draws("DeviceGeometry", "ops", ops, B, self.draw)
        for k, t in batch.items():
            for i, op in enumerate(ops):
                if not op.preserves(t.shape):
                    raise ValueError(f"DeviceGeometry: sample {i}: {op} would change the shape of {k!r} {tuple(t.shape)}; "
                                     f"rotation axes this shape allows: {allowed_rot90_axes(t.shape[-3:])}")
        self.last_ops = ops
        if all(op.is_identity() for op in ops):
            return batch
        table = E.geom_table(ops)
        return stages.per_tensor(batch, lambda k, five: E.geom_apply(five, table, k in self.normal_keys))


# ---- dataset_config.geometric -------------------------------------------------------------------------------------------------------
_KNOWN = {"flip": {"p", "p_transform"}, "rot90": {"axes", "p", "p_transform"}}


def check_transform_kwargs(owner, name, kw):
    """the keyword arguments of `draw_flip` / `draw_rot90` as a config block or a constructor argument: None / False -> None (off),
    True -> {} (defaults); unknown names, probabilities outside [0, 1] and bad axis names raise with `owner.name` named"""
    if kw is None or kw is False:
        return None
    kw = {} if kw is True else kw
    if not isinstance(kw, dict) or set(kw) - _KNOWN[name]:
        bad = sorted(set(kw) - _KNOWN[name]) if isinstance(kw, dict) else kw
        raise ValueError(f"{owner}.{name}: unknown key(s) {bad} (known: {sorted(_KNOWN[name])})")
    out = {}
    for k, v in kw.items():
        if k == "axes":
            axes = tuple(str(a).lower() for a in ((v,) if isinstance(v, str) else v))
            if not axes or any(a not in PLANE for a in axes):
                raise ValueError(f"{owner}.{name}.axes: {list(axes)} (a non-empty choice of x, y, z)")
            out[k] = axes
        else:
            out[k] = stages.probability(f"{owner}.{name}", k, v)
    return out


def parse_geometric(dataset_config, patch_size, tasks):
    """`dataset_config.geometric` -> None (absent / false) or {"flip": kwargs | None, "rot90": kwargs | None, "normal_keys": tuple,
    "where": "device" | "host"}.  Everything that would otherwise fail at some later step fails here, with the key named."""
    g = stages.block(dataset_config, "geometric", ("flip", "rot90", "normal_keys", "where"), "device", None)
    if g is None:
        return None
    patch = stages.patch3d("dataset_config.geometric", patch_size)
    out = {name: check_transform_kwargs("dataset_config.geometric", name, g.get(name, None)) for name in ("flip", "rot90")}
    out["where"] = g["where"]
    if out["rot90"] is not None:
        allowed = allowed_rot90_axes(patch)
        axes = out["rot90"].get("axes", ("x", "y", "z"))
        wrong = [a for a in axes if a not in allowed]
        if wrong:
            raise ValueError(f"dataset_config.geometric.rot90.axes: a rotation about {wrong} turns a plane of unequal extents of "
                             f"the patch {list(patch)} and would change its shape; axes this patch allows: {list(allowed)}")
        out["rot90"]["axes"] = axes
    out["normal_keys"] = stages.normal_keys("dataset_config.geometric", g, tasks)
    return out


def host_transforms(cfg, rng=None):
    """the host classes of a parsed config, in application order (flip, then rot90)"""
    from ..training.transforms.geometric.geometry import RandomFlipWithNormals, RandomRotate90WithNormals
    ts = []
    if cfg["flip"] is not None:
        ts.append(RandomFlipWithNormals(normal_keys=cfg["normal_keys"], rng=rng, **cfg["flip"]))
    if cfg["rot90"] is not None:
        ts.append(RandomRotate90WithNormals(normal_keys=cfg["normal_keys"], rng=rng, **cfg["rot90"]))
    return ts
