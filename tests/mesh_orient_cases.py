"""The volumes, points and meshes of the mesh-orientation tests, shared by the CPU tests (the statements' properties) and the GPU
tests (ops.mesh_sample / mesh_face_cos / mesh_select against the statements); csrc/tools/meshsample_host_check.cpp restates the
same kinds in C++.  Each is chosen for a way the kernels can go wrong:

  points at lattice coordinates                 f = 0 on every axis: the sample is the decoded voxel
  points outside on each of the six sides       both corners clamp to the border plane
  points on the last plane / row / column       i + 1 clamps while i does not
  V = 0, 1, 255, 256, 257                       nothing to do; one thread; a block boundary and a tail (workgroups of 256)
  C = 1, 3 and 8, all four rules                every instantiation, the channel loop at its ends
  odd extents (5, 6, 7), (3, 9, 4), (1, 1, 1)   no multiple of anything; a volume of one voxel, where every index clamps to 0
  -0.0 and denormals under `copy`               the decode must not touch them
  the slab sheet and the graded ball            a shell with two faces and a rim under a constant field
  a degenerate triangle, a zero vector          cos is 0 / 0 = NaN: the rim"""
import numpy as np

import isosurface_cases as I
from mesh_cases import ball_mesh      # noqa: F401 -- also reached as O.ball_mesh

F32 = np.float32
RULES = {"copy": np.float32, "u8": np.uint8, "u16": np.uint16, "normal_u16": np.uint16}
COUNTS = (0, 1, 255, 256, 257)
CHANNELS = (1, 3, 8)
SHEET = dict(shape=(10, 12, 14), z=(4, 7))      # the mask is 255 on planes 4, 5, 6; the mid-plane of the sheet is z = 5
UP = (32768, 32768, 65535)      # the uint16 codes of the constant field (Nx, Ny, Nz) = (0, 0, 1) (32768 decodes to 1.5e-5)


def volume(rule, shape, seed=0):
    """a random (C, Z, Y, X) volume of the dtype `rule` decodes; `copy`: values in (-4, 4)"""
    rng = np.random.default_rng(seed + 31 * shape[0] + sum(shape[1:]))
    if rule == "copy":
        return rng.uniform(-4, 4, shape).astype(F32)
    return rng.integers(0, 256 if rule == "u8" else 65536, shape).astype(RULES[rule])


def lattice(shape_zyx):
    """every voxel centre as an (x, y, z) point"""
    z, y, x = np.indices(shape_zyx)
    return np.stack([x.ravel(), y.ravel(), z.ravel()], 1).astype(F32)


def outside(shape_zyx):
    """for each of the six sides a few points beyond it -> [(points (n, 3), clamped lattice points (n, 3))]"""
    Z, Y, X = shape_zyx
    base = lattice(shape_zyx)[:: max(1, Z * Y * X // 7)]
    out = []
    for axis, n in ((0, X), (1, Y), (2, Z)):
        for value, clamped in ((-0.75, 0), (-3.0, 0), (-1e30, 0), (n - 1 + 0.25, n - 1), (n + 2.5, n - 1), (1e30, n - 1)):
            p, q = base.copy(), base.copy()
            p[:, axis], q[:, axis] = value, clamped
            out.append((p, q))
    return out


def points(shape_zyx, n, seed=0):
    """n points: the corners of the volume, points on and beyond every border, lattice points, and random ones inside"""
    Z, Y, X = shape_zyx
    rng = np.random.default_rng(seed + n)
    hi = np.array([X - 1, Y - 1, Z - 1], F32)
    fixed = [np.array([[0, 0, 0], hi, [X - 1, 0, 0], [0, Y - 1, 0], [0, 0, Z - 1], hi - F32(0.5), hi + F32(0.5), [-0.5, -0.5, -0.5],
                       [X, Y, Z], [-2, Y + 3, 0.25]], F32)]
    fixed.append(np.stack([rng.uniform(-1.5, X + 0.5, 12), rng.uniform(-1.5, Y + 0.5, 12), np.arange(12) % Z], 1).astype(F32))      # whole z
    fixed = np.concatenate(fixed)
    rest = rng.uniform(-1.0, 1.0, (max(n - len(fixed), 0), 3)).astype(F32) * F32(0.6) * (hi + F32(1)) + hi * F32(0.5)
    return np.ascontiguousarray(np.concatenate([fixed, rest])[:n], F32)


_SAMPLE = None


def sample_cases():
    """[(id, volume (C, Z, Y, X), points float32 (V, 3), rule)].  Built once."""
    global _SAMPLE
    if _SAMPLE is None:
        out = []
        for rule in RULES:
            for C in CHANNELS:
                shape = (C, 5, 6, 7)
                out.append((f"{rule}-c{C}-v257", volume(rule, shape, C), points(shape[1:], 257, C), rule))
            for V in COUNTS:
                out.append((f"{rule}-small-v{V}", volume(rule, (3, 3, 9, 4), V), points((3, 9, 4), V, V), rule))
            out.append((f"{rule}-lattice", volume(rule, (2, 5, 6, 7), 9), lattice((5, 6, 7)), rule))
            out.append((f"{rule}-one-voxel", volume(rule, (3, 1, 1, 1), 4), points((1, 1, 1), 40, 4), rule))
        out.append(("copy-signed-zero-denormal", special_copy_volume(), lattice((3, 3, 3)), "copy"))
        _SAMPLE = out
    return _SAMPLE


def sample_case(name):
    return next(c for c in sample_cases() if c[0] == name)


def special_copy_volume():
    """(1, 3, 3, 3) float32, negative everywhere, with -0.0 at (z, y, x) = (1, 1, 1) and the denormals 1e-45 and -3e-42 at (0, 1, 1)
    and (1, 0, 1).  At a lattice point f = 0, so a lerp is u + 0 * (w - u): a -0.0 survives it where w - u is negative, which is
    the case here and not in general (-0.0 + +0.0 is +0.0 in IEEE arithmetic)."""
    v = -(np.arange(27, dtype=F32).reshape(1, 3, 3, 3) + F32(1))
    v[0, 1, 1, 1] = F32(-0.0)
    v[0, 0, 1, 1] = np.array([1], np.int32).view(F32)[0]
    v[0, 1, 0, 1] = -np.array([2142], np.int32).view(F32)[0]
    return v


def constant_field(shape_zyx, codes=UP):
    """a (3, Z, Y, X) uint16 volume holding one code per channel"""
    return np.broadcast_to(np.asarray(codes, np.uint16)[:, None, None, None], (3,) + tuple(shape_zyx)).copy()


def sheet_volume():
    v = np.zeros(SHEET["shape"], np.uint8)
    v[SHEET["z"][0]:SHEET["z"][1]] = 255
    return v


_MESHES = {}


def sheet_mesh():
    """the surface-nets shell of the slab sheet"""
    import mt3d_amd.postprocess as pp
    if "sheet" not in _MESHES:
        _MESHES["sheet"] = pp.surface_nets_numpy(sheet_volume(), 127)
    return _MESHES["sheet"]


def rim_mesh():
    """-> (vertices, triangles, vectors): triangle 0 is degenerate (two equal corners), triangle 1 has zero vectors at its three
    corners, triangles 2 and 3 face up and down under the vectors (0, 0, 1): rim, rim, front, back"""
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [5, 5, 1], [6, 5, 1], [5, 6, 1], [2, 2, 2], [3, 2, 2], [2, 3, 2]], F32)
    t = np.array([[0, 1, 1], [3, 4, 5], [6, 7, 8], [6, 8, 7]], np.int64)
    n = np.tile(np.array([0, 0, 1], F32), (9, 1))
    n[3:6] = 0
    return v, t, n


def mesh_cases():
    """[(id, vertices, triangles, vectors float32 (V, 3), min_cos)]: the vectors are the unit samples of the constant field, or stated"""
    import mt3d_amd.postprocess as pp
    out = []
    for name, (v, t), shape in (("sheet", sheet_mesh(), SHEET["shape"]), ("ball", ball_mesh(), I.BALL["shape"])):
        n = pp.unit_numpy(pp.sample_points_numpy(constant_field(shape), v, "normal_u16")[0])
        out.append((name, v, t, n, 0.2))
    v, t, n = rim_mesh()
    out.append(("rim", v, t, n, 0.2))
    rng = np.random.default_rng(5)
    v, t = ball_mesh()
    out.append(("ball-random-vectors", v, t, rng.normal(size=v.shape).astype(F32), 0.0))
    return out
