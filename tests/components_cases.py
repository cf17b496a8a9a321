"""The case list of the connected-component tests, shared by the CPU tests (label_numpy against scipy), the GPU tests (ops.cc_label
against label_numpy) and, restated in C++ with its own random generator, csrc/tools/components_host_check.cpp.

The kernel's tile is 8 x 8 x 64 (z, y, x: RX_CC_TZ, RX_CC_TY, RX_CC_TX of csrc/rx_components_core.h), so no tile extent exceeds 40
along z or y and the issue's shapes already cross several tiles on every axis: (40, 40, 130) is 5 x 5 x 3 tiles, (33, 17, 70)
5 x 3 x 2, (130, 3, 5) 17 tiles along z, (3, 130, 5) 17 along y, (2, 3, 257) 5 along x.  No further shape is needed."""
import numpy as np

TILE = (8, 8, 64)
SHAPES = [(1, 1, 1), (1, 1, 70), (1, 70, 1), (5, 1, 3), (9, 10, 12), (33, 17, 70), (3, 130, 5), (130, 3, 5), (2, 3, 257), (40, 40, 130)]
CONNECTIVITIES = (6, 18, 26)


def serpentine(shape):
    """full-x rows on every second y, joined alternately at x = X - 1 and x = 0, on every z: one component whose graph diameter is
    about Y * X / 2 (where the shape has room for it)"""
    Z, Y, X = shape
    m = np.zeros(shape, bool)
    m[:, ::2, :] = True
    for y in range(1, Y, 2):
        m[:, y, X - 1 if (y // 2) % 2 == 0 else 0] = True
    return m


def _corner(shape):
    """the first tile boundary of every axis that has one, else the middle of the axis"""
    return tuple(t if n > t else (n + 1) // 2 for n, t in zip(shape, TILE))


def _box(m, lo, hi):
    m[tuple(slice(max(a, 0), max(b, 0)) for a, b in zip(lo, hi))] = True


def corner_pair(shape):
    """two thick blocks that touch only in one voxel pair, diagonally across a tile corner: joined at 26, separate at 18 and 6"""
    cz, cy, cx = _corner(shape)
    m = np.zeros(shape, bool)
    _box(m, (cz - 3, cy - 3, cx - 3), (cz, cy, cx))
    _box(m, (cz, cy, cx), (cz + 3, cy + 3, cx + 3))
    return m


def edge_pair(shape):
    """two thick slabs, full along x, that touch only across a tile edge: joined at 26 and 18, separate at 6"""
    cz, cy, _ = _corner(shape)
    m = np.zeros(shape, bool)
    _box(m, (cz - 3, cy - 3, 0), (cz, cy, shape[2]))
    _box(m, (cz, cy, 0), (cz + 3, cy + 3, shape[2]))
    return m


def backward_root(shape):
    """one path: along x from voxel (0, 0, 1) to (0, 0, X - 1), along y to (0, Y - 1, X - 1), along z to the volume's last voxel.  The
    component's smallest index, (0, 0, 1), lies in the first tile and its far end in the last one, so every other tile's local root
    has to be linked back to it, through every seam on the way"""
    Z, Y, X = shape
    m = np.zeros(shape, bool)
    m[:, Y - 1, X - 1] = True
    m[0, :, X - 1] = True
    m[0, 0, :] = True
    m[0, 0, 0] = Z * Y * X == 1
    return m


def masks(shape, seed=0):
    """[(name, bool mask)] of one shape"""
    rng = np.random.default_rng(seed + 1000 * shape[0] + 10 * shape[1] + shape[2])
    zz, yy, xx = np.indices(shape)
    corners = np.zeros(shape, bool)
    corners[0, 0, 0] = corners[-1, -1, -1] = True
    out = [("empty", np.zeros(shape, bool)), ("full", np.ones(shape, bool)), ("corners", corners)]
    out += [(f"random{int(p * 100)}", rng.random(shape) < p) for p in (0.1, 0.3, 0.6)]
    out += [("checkerboard", (zz + yy + xx) % 2 == 0), ("serpentine", serpentine(shape)), ("corner_pair", corner_pair(shape)),
            ("edge_pair", edge_pair(shape)), ("backward_root", backward_root(shape))]
    return out


def cases():
    """[(id, bool mask)] over every shape"""
    return [(f"{'x'.join(map(str, s))}-{name}", m) for s in SHAPES for name, m in masks(s)]


def sheet_values(shape, seed=5, p=0.3):
    """uint8 values whose mask `> 127` is random at `p`, plus one plate that spans every z and one blob in rows 12 and 13, which lie in
    one slab at slab depths 2, 3, 7 and 20"""
    rng = np.random.default_rng(seed)
    v = np.where(rng.random(shape) < p, rng.integers(128, 256, shape), rng.integers(0, 128, shape)).astype(np.uint8)
    v[:, 2:4, 3:9] = 200                                    # spans every slab
    v[11:15, 14:21, 20:30] = 0
    v[12:14, 15:20, 21:29] = 255                            # isolated by a shell of zeros
    return v
