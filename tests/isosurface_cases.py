"""The case list of the surface-nets tests, shared by the CPU tests (the statement's invariants), the GPU tests (ops.iso_mesh against the
statement) and, restated in C++ with its own random generator, csrc/tools/isosurface_host_check.cpp.

A cell row is walked 64 cells at a time and a workgroup owns a band of 4 cell planes x 8 cell rows, so the shapes cover single planes
and rows, rows past one 64-lane wave ((1,1,70), (5,5,70) ...) and past 256 ((2,3,257)), and row counts past one band on either axis
((3,130,5), (130,3,5), (40,40,130))."""
import numpy as np

SHAPES = [(1, 1, 1), (1, 1, 70), (1, 70, 1), (5, 1, 3), (9, 10, 12), (33, 17, 70), (3, 130, 5), (130, 3, 5), (2, 3, 257), (40, 40, 130)]
LEVELS = (0, 127, 254)
BALL = dict(shape=(24, 24, 24), R=9.3, centre=(11.2, 12.1, 11.7))      # centre in (z, y, x)


def ball(shape, R=None, centre=None):
    """the graded ball clip(rint(127.5 + 32 * (R - r))): inside at level 127 where r < R, with a ramp that gives t many values"""
    shape = tuple(shape)
    centre = [(n - 1) / 2 + 0.2 for n in shape] if centre is None else centre
    R = 0.4 * min(shape) if R is None else R
    g = np.stack(np.meshgrid(*[np.arange(n) for n in shape], indexing="ij"), -1)
    r = np.linalg.norm(g - np.asarray(centre), axis=-1)
    return np.clip(np.rint(127.5 + 32 * (R - r)), 0, 255).astype(np.uint8)


def volumes(shape, level, seed=0):
    """[(name, uint8 volume)] of one shape at one level"""
    rng = np.random.default_rng(seed + 1000 * shape[0] + 10 * shape[1] + shape[2] + 7 * level)
    zz, yy, xx = np.indices(shape)
    out = [("zero", np.zeros(shape, np.uint8)), ("full", np.full(shape, 255, np.uint8)),
           ("checkerboard", (((zz + yy + xx) % 2 == 0) * 255).astype(np.uint8))]
    for p in (0.1, 0.5, 0.9):      # foreground in level+1 .. 255, background in 0 .. level: level and level + 1 lie side by side
        fg = rng.integers(level + 1, 256, shape)
        bg = rng.integers(0, level + 1, shape)
        out.append((f"random{int(p * 100)}", np.where(rng.random(shape) < p, fg, bg).astype(np.uint8)))
    out.append(("ball", ball(shape)))
    slab = np.zeros(shape, np.uint8)      # touches every face of the volume
    slab[:, shape[1] // 2:shape[1] // 2 + 2, :] = 200
    slab[shape[0] // 2, :, :] = 255
    slab[:, :, shape[2] // 2] = 129
    out.append(("slab", slab))
    return out


def cases():
    """[(id, level, uint8 volume)] over every shape and level"""
    return [(f"{'x'.join(map(str, s))}-{name}-{level}", level, v) for s in SHAPES for level in LEVELS for name, v in volumes(s, level)]


def edge_uses(triangles):
    """(undirected edge use counts, whether every directed edge is used as often as its reverse)"""
    t = np.asarray(triangles, np.int64)
    e = np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])
    if not len(e):
        return np.zeros(0, np.int64), True
    n = int(e.max()) + 1
    _, und = np.unique(np.sort(e, 1) @ np.array([n, 1]), return_counts=True)
    fk, fc = np.unique(e @ np.array([n, 1]), return_counts=True)
    rk, rc = np.unique(e[:, ::-1] @ np.array([n, 1]), return_counts=True)
    return und, bool(np.array_equal(fk, rk) and np.array_equal(fc, rc))
