"""Label dilation -- the reference's `tr_setup.dilate_label` (dataloading/dataset.py: every target that is not `normals` becomes
dilation(t > 0, skimage.morphology.ball(5))) -- stated once in numpy and run on the device (csrc/rx_morph.hip: rx_label_dilate).

The digital ball of radius r is a union of x-runs: for every (dz, dy) with dz^2 + dy^2 <= r^2 it holds the voxels |dx| <= h,
h = isqrt(r^2 - dz^2 - dy^2).  `ball_runs` lists them, `ball` is the structuring element itself, `dilate_numpy` states what the
kernel computes with shifted-slice ORs only (no scipy: it is the oracle of the GPU tests) and returns float32 0/1:

    out[v] = 1 if some voxel u with in[u] > 0 (NaN, -0.0 and negatives are off) lies within |u - v|^2 <= r^2, else 0;

nothing outside the volume is ever on -- the border rule of skimage's `dilation` and of scipy's `binary_dilation`.  The ball is
invariant under every signed permutation of the axes, so dilation commutes with the flips and rotations of `geometry_device`.

`parse_dilate` reads `dataset_config.dilate` ({where: host | device, radius: 1..8}; absent: {where: host, radius: 5}, what the
reference does) under the reference's switch `tr_setup.dilate_label`; `DeviceDilate` is the stage the trainer puts behind the
feeder's copies for `where: device`."""
from math import isqrt

import numpy as np

from . import stages

MAX_RADIUS = 8


def _check_radius(owner, radius):
    if isinstance(radius, bool) or not isinstance(radius, (int, np.integer)) or not 1 <= int(radius) <= MAX_RADIUS:
        raise ValueError(f"{owner}: {radius!r} (an integer in 1..{MAX_RADIUS})")
    return int(radius)


def ball_runs(radius):
    """the ball as x-runs: [(dz, dy, h)] in (dz, dy) lexicographic order -- the run |dx| <= h at every (dz, dy) inside the disc"""
    r = _check_radius("ball_runs: radius", radius)
    return [(dz, dy, isqrt(r * r - dz * dz - dy * dy))
            for dz in range(-r, r + 1) for dy in range(-r, r + 1) if dz * dz + dy * dy <= r * r]


def ball(radius):
    """skimage.morphology.ball(radius) as a boolean (2r+1)^3 array, built from the runs"""
    r = _check_radius("ball: radius", radius)
    out = np.zeros((2 * r + 1,) * 3, dtype=bool)
    for dz, dy, h in ball_runs(r):
        out[r + dz, r + dy, r - h:r + h + 1] = True
    return out


def _or_shifted(dst, src, shift):
    """dst[v] |= src[v - shift] on the last len(shift) axes, with nothing coming in from outside the volume"""
    d, s = [slice(None)] * dst.ndim, [slice(None)] * dst.ndim
    for ax, k in zip(range(dst.ndim - len(shift), dst.ndim), shift):
        n = dst.shape[ax]
        if abs(k) >= n:
            return
        d[ax], s[ax] = slice(max(k, 0), n + min(k, 0)), slice(max(-k, 0), n - max(k, 0))
    dst[tuple(d)] |= src[tuple(s)]


def dilate_numpy(arr, radius=5):
    """what rx_label_dilate computes, in numpy: (Z, Y, X) or (C, Z, Y, X) in (every channel on its own), float32 0/1 of the same
    shape out"""
    r = _check_radius("dilate_numpy: radius", radius)
    arr = np.asarray(arr)
    if arr.ndim not in (3, 4):
        raise ValueError(f"dilate_numpy: expected (Z, Y, X) or (C, Z, Y, X), got {arr.shape}")
    with np.errstate(invalid="ignore"):
        on = arr > 0
    runs = ball_runs(r)
    out = np.zeros(on.shape, dtype=bool)
    for h in sorted({h for _, _, h in runs}):
        xd = on.copy()                                   # the x-run of half-width h, once for all the runs that have it
        for dx in range(1, h + 1):
            _or_shifted(xd, on, (dx,))
            _or_shifted(xd, on, (-dx,))
        for dz, dy, hh in runs:
            if hh == h:
                _or_shifted(out, xd, (dz, dy, 0))
    return out.astype(np.float32)


def dilate_keys(tasks):
    """the targets the reference dilates: every task whose lower-cased name is not `normals`"""
    return [str(k) for k in (tasks or {}) if str(k).lower() != "normals"]


def parse_dilate(dataset_config, dilate_label, tasks):
    """`tr_setup.dilate_label` and `dataset_config.dilate` -> None (the switch is off, whatever the block says) or
    {"radius": r, "where": "host" | "device", "keys": [...]}.  An absent block is {where: host, radius: 5}.  Unknown keys, a `where`
    that is neither host nor device and a radius that is not an integer in 1..8 raise with the key named."""
    if not dilate_label:
        return None
    d = stages.block(dataset_config, "dilate", ("where", "radius"), "host", {})
    radius = _check_radius("dataset_config.dilate.radius", d.get("radius", 5))
    return {"radius": radius, "where": d["where"], "keys": dilate_keys(tasks)}


class DeviceDilate:
    """`dilate(batch_dict) -> batch_dict` on the CURRENT stream: the tensors named in `keys` -- float32 device batches,
    (B, C, Z, Y, X) or (B, Z, Y, X) -- are dilated in place with the ball of `radius`; `image` and every other entry stay the
    tensor objects they were.  The bit scratch comes from torch's caching allocator on that stream."""

    def __init__(self, keys, radius=5):
        self.keys = [str(k) for k in keys]
        self.radius = _check_radius("DeviceDilate: radius", radius)

    def __call__(self, batch):
        from ..engine import ops as E
        from ..engine.lib import RxError
        for k in self.keys:
            if k not in batch:
                raise RxError(f"DeviceDilate: the batch has no {k!r} (it has {sorted(batch)})")
            t = batch[k]
            stages.check_tensor("DeviceDilate", k, t, "dataset_config.dilate.where: host dilates in the dataset")
            E.label_dilate(t if t.dim() == 5 else t.unsqueeze(1), self.radius)
        return batch
