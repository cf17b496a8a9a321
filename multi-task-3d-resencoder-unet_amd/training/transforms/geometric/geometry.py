"""Host-side flips and 90-degree rotations of a patch dictionary that keep surface normals consistent: the reference's
training/transforms/geometric/geometry.py, class for class and argument for argument.  Each class draws an op
(dataloading/geometry_device.py: the same `random` calls in the same order as upstream) and applies it with `apply_op_numpy`,
the statement the device kernel is held against -- so host and device agree by construction.

`data_dict`: {key: (Z, Y, X) or (C, Z, Y, X) array}; every array moves alike, the arrays named in `normal_keys` (components
Nx, Ny, Nz = channels 0, 1, 2) also have their components permuted and negated.  `rng`: a `random.Random`; default: the `random`
module itself, as upstream."""
import random

from ....dataloading.geometry_device import apply_op_numpy, draw_flip, draw_rot90


class _GeometricTransform:
    def _draw(self):
        raise NotImplementedError

    def __call__(self, data_dict):
        op = self._draw()
        self.last_op = op
        if op.is_identity():
            return data_dict
        for k in list(data_dict):
            data_dict[k] = apply_op_numpy(op, data_dict[k], k in self.normal_keys)
        return data_dict


class RandomFlipWithNormals(_GeometricTransform):
    """flip along Z, Y, X independently with probability `p` each; the whole transform happens with probability `p_transform`"""

    def __init__(self, p=0.5, p_transform=1.0, normal_keys=("normals",), rng=None):
        self.p = p
        self.p_transform = p_transform
        self.normal_keys = set(normal_keys)
        self.rng = random if rng is None else rng
        self.last_op = None

    def _draw(self):
        return draw_flip(self.rng, self.p, self.p_transform)


class RandomRotate90WithNormals(_GeometricTransform):
    """with probability `p_transform` * `p`: a rotation by 90, 180 or 270 degrees about one of `axes` ('x', 'y', 'z')"""

    def __init__(self, axes=("x", "y", "z"), p=0.5, p_transform=1.0, normal_keys=("normals",), rng=None):
        self.axes = axes
        self.p = p
        self.p_transform = p_transform
        self.normal_keys = set(normal_keys)
        self.rng = random if rng is None else rng
        self.last_op = None

    def _draw(self):
        return draw_rot90(self.rng, self.axes, self.p, self.p_transform)
