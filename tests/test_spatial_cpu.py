"""CPU: dataloading/spatial_device.py -- `affine_numpy` (the statement of rx_affine_apply and the host path) against the signed
permutations of geometry_device (bit for bit) and against torch's grid_sample in float64 (an independent formulation, within a
derived bound); the draw order, compose and the vector rule, the config parser, the host path of the datasets, and the kernel's
own per-voxel functions run on the CPU under AddressSanitizer."""
import math
import os
import random
import struct
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import mt3d_amd  # noqa: F401
from mt3d_amd.dataloading import geometry_device as G
from mt3d_amd.dataloading import spatial_device as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24          # unit roundoff of float32


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and bool((a.view(np.int32) == b.view(np.int32)).all())


def signed_permutations():
    """the 48 ops flips and 90-degree rotations generate, each with the component rule the reference gives it"""
    gens = [G.flip_op(d) for d in range(3)] + [G.rot90_op(ax, 1) for ax in "xyz"]
    seen, todo = {G.GeomOp()}, [G.GeomOp()]
    while todo:
        op = todo.pop()
        for g in gens:
            n = G.compose(op, g)
            if n not in seen:
                seen.add(n)
                todo.append(n)
    ops = sorted(seen, key=lambda o: o.row())
    assert len({(o.src_axis, o.flip) for o in ops}) == 48
    return ops


def positive_field(shape, seed):
    """no -0.0 and no exact 0.0: a lerp with weight 0 computes a + 0 * (b - a), which turns a = -0.0 into +0.0"""
    return (np.random.default_rng(seed).random(shape, dtype=np.float32) + np.float32(0.25)).astype(np.float32)


# ---- signed permutations --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(10, 10, 10), (6, 12, 12)])
def test_signed_permutations_are_apply_op_numpy(shape):
    ops = [op for op in signed_permutations() if op.preserves(shape)]
    assert len({(o.src_axis, o.flip) for o in ops}) == (48 if shape[0] == shape[1] == shape[2] else 16)
    x1, x3 = positive_field((1, *shape), 1), positive_field((3, *shape), 2)
    for op in ops:
        a = S.from_geom(op)
        assert set(np.unique(a.point)) <= {-1.0, 0.0, 1.0} and set(np.unique(a.vector)) <= {-1.0, 0.0, 1.0}
        for x in (x1, x3, x1[0]):
            want = G.apply_op_numpy(op, x)
            assert same_bits(S.affine_numpy(a, x, "linear", "constant"), want), op
            assert same_bits(S.affine_numpy(a, x, "linear", "clamp"), want), op
            assert same_bits(S.affine_numpy(a, x, "nearest", "constant"), want), op
        # The vector rule is a 3-term sum with two exact zeros, (v0 * s0 + v1 * s1) + v2 * s2: the value is +-s_k exactly, but a
        # product 0 * s carries the sign of s and a sum of zeros of both signs is +0.0, so where the selected component is itself
        # zero (none here) or the other two products are -0.0 the SIGN OF A ZERO can differ from apply_op_numpy's sign-bit flip.
        # Compare values, not bits.
        got = S.affine_numpy(a, x3, "nearest", "constant", is_normal=True)
        assert (got == G.apply_op_numpy(op, x3, True)).all(), op
    assert S.from_geom(G.GeomOp()).is_identity() and S.AffineOp().is_identity() and not S.from_geom(ops[1]).is_identity()


def test_from_geom_composes_like_geom_ops_and_rotation_op_meets_rot90_at_right_angles():
    ops = signed_permutations()
    for i in range(0, 48, 5):
        for j in range(1, 48, 7):
            assert S.compose(S.from_geom(ops[i]), S.from_geom(ops[j])) == S.from_geom(G.compose(ops[i], ops[j]))
    for ax in "zyx":
        for k in (1, 2, 3):
            r, g = S.rotation_op(ax, 90.0 * k), S.from_geom(G.rot90_op(ax, k))
            assert np.abs(r.point - g.point).max() < 1e-6 and np.abs(r.vector - g.vector).max() < 1e-6, (ax, k)
    # float64 on the host, float32 once: a chain of 36 ten-degree turns is the identity to float32 rounding of ONE matrix
    op = S.AffineOp()
    for _ in range(36):
        op = S.compose(op, S.rotation_op("y", 10.0))
    assert np.abs(op.point - np.eye(3)).max() < 2 * U and np.abs(op.vector - np.eye(3)).max() < 2 * U
    assert S.scale_op(1.25).point.tolist() == (np.eye(3, dtype=np.float32) * np.float32(1.25)).tolist()
    assert (S.scale_op(0.8).vector == np.eye(3)).all()
    with pytest.raises(ValueError):
        S.AffineOp(np.full((3, 3), np.nan), None)
    with pytest.raises(ValueError):
        S.AffineOp(np.eye(3) * 1e300, None)


# ---- anchor: torch grid_sample in float64 ---------------------------------------------------------------------------------------
SHAPE = (14, 18, 22)


def smooth_field(shape):
    z, y, x = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij")
    return (np.sin(0.31 * z + 0.2) * np.cos(0.23 * y - 0.4) + 0.5 * np.sin(0.17 * x + 0.11 * y)).astype(np.float32)


def grid_sample64(op, x, mode, padding):
    """torch's own affine_grid + grid_sample in float64, align_corners=True: normalised coordinate 2 o / (n - 1) - 1 per axis,
    theta in (x, y, z) order = point reversed, rescaled by the half extents"""
    n = np.array(x.shape[-3:], dtype=np.float64)
    half = (n[::-1] - 1.0) / 2.0                                        # (x, y, z)
    m = op.point.astype(np.float64)[::-1, ::-1]                         # (x, y, z) order
    theta = np.zeros((1, 3, 4))
    theta[0, :, :3] = m * half[None, :] / half[:, None]
    t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64))[None, None]
    grid = torch.nn.functional.affine_grid(torch.from_numpy(theta), list(t.shape), align_corners=True)
    return torch.nn.functional.grid_sample(t, grid, mode=mode, padding_mode=padding, align_corners=True)[0, 0].numpy()


def source_coords64(op, shape):
    c = [(n - 1) / 2.0 for n in shape]
    t = np.meshgrid(*[np.arange(n, dtype=np.float64) - c[d] for d, n in enumerate(shape)], indexing="ij")
    m = op.point.astype(np.float64)
    return [m[d, 0] * t[0] + m[d, 1] * t[1] + m[d, 2] * t[2] + c[d] for d in range(3)]


ANCHOR = [(ax, deg, s) for ax in "zyx" for deg in (7.0, 30.0, 45.0) for s in (0.8, 1.25)]


@pytest.mark.parametrize("border,padding", [("constant", "zeros"), ("clamp", "border")])
def test_linear_against_grid_sample_in_float64(border, padding):
    """Tolerance, derived and not tuned.  affine_numpy differs from exact arithmetic on the same float32 matrix by the rounding of
    the source coordinate: p_d is 3 products and 3 sums, f_d = p_d - floor(p_d) one more operation, 7 roundings, each at most
    U = 2^-24 times the largest intermediate magnitude L = max_d (sum_k |m_dk| |t_k| + c_d) over the patch -- the coordinate
    rounding bound at the patch's largest coordinate, dp = 7 U L.  A trilinear interpolant changes by at most the largest
    difference D between neighbouring voxels per unit of coordinate and axis (for `constant` the volume continues with zeros, so
    D includes the step from the outermost voxels to 0), and it is continuous across cell boundaries, so rounding p to the other
    side of an integer costs no more.  Three axes: tol = 3 * D * dp."""
    x = smooth_field(SHAPE)
    xp = np.pad(x.astype(np.float64), 1) if border == "constant" else x.astype(np.float64)
    D = max(np.abs(np.diff(xp, axis=d)).max() for d in range(3))
    worst = 0.0
    for ax, deg, s in ANCHOR:
        op = S.compose(S.rotation_op(ax, deg), S.scale_op(s))
        c = np.array([(n - 1) / 2.0 for n in SHAPE])
        L = (np.abs(op.point.astype(np.float64)) @ c + c).max()
        tol = 3.0 * D * 7.0 * U * L
        got = S.affine_numpy(op, x, "linear", border)
        want = grid_sample64(op, x, "bilinear", padding)
        err = np.abs(got.astype(np.float64) - want).max()
        worst = max(worst, err / tol)
        print(f"{border} {ax} {deg} {s}: max error {err:.3e}, bound {tol:.3e}")
        assert err <= tol, (ax, deg, s, err, tol)
        assert np.abs(want).max() > 0.3          # (the comparison is not of an empty patch)
    print(f"{border}: worst error / bound = {worst:.3f}")


def test_nearest_against_grid_sample_in_float64():
    """grid_sample rounds half to even, the statement rounds half up, and a float32 coordinate within rounding of a half-integer
    may land on the other side: voxels whose float64 source coordinate lies within 1e-3 of a half-integer on any axis are left
    out -- at most 1 % per case -- and the rest must match exactly.  With a rotation about ONE axis the coordinate along that axis
    is s * t + c, which sits exactly on half-integers for whole planes (0.8 * 2.5, 1.25 * 2), so every case here tilts the
    patch by a further 19 degrees about the next axis (chosen so that the left-out share stays below 1 %, asserted below); the
    angles and scales of the linear test stay."""
    x = smooth_field(SHAPE)
    nxt = {"z": "y", "y": "x", "x": "z"}
    for ax, deg, s in ANCHOR:
        op = S.compose(S.compose(S.rotation_op(ax, deg), S.rotation_op(nxt[ax], 19.0)), S.scale_op(s))
        p = source_coords64(op, SHAPE)
        near = np.zeros(SHAPE, dtype=bool)
        for d in range(3):
            near |= np.abs((p[d] - np.floor(p[d])) - 0.5) < 1e-3
        share = near.mean()
        assert share <= 0.01, (ax, deg, s, share)
        got = S.affine_numpy(op, x, "nearest", "constant")
        want = grid_sample64(op, x, "nearest", "zeros")
        assert (got[~near].astype(np.float64) == want[~near]).all(), (ax, deg, s)
        assert (want[~near] != 0).mean() > 0.2


def test_border_rules_channels_and_shapes():
    x = positive_field((2, 5, 6, 7), 3)
    far = S.scale_op(2.0)
    got = S.affine_numpy(far, x, "linear", "constant", fill=0.5)
    assert got.shape == x.shape and got.dtype == np.float32 and (got[:, 0] == 0.5).all() and (got != 0.5).any()
    near = S.affine_numpy(far, x, "nearest", "clamp")
    assert set(np.unique(near)) <= set(np.unique(x))
    assert same_bits(S.affine_numpy(far, x[1], "linear", "clamp"), S.affine_numpy(far, x, "linear", "clamp")[1])      # channels share coordinates
    huge = S.AffineOp(np.eye(3) * 1e30, None)          # coordinates beyond any index: all outside, no overflow in the index
    assert (S.affine_numpy(huge, x, "nearest", "constant", fill=2.0)[:, 0, 0, 0] == 2.0).all()
    with pytest.raises(ValueError):
        S.affine_numpy(far, x, "cubic", "constant")
    with pytest.raises(ValueError):
        S.affine_numpy(far, x, "linear", "reflect")
    with pytest.raises(ValueError):
        S.affine_numpy(far, x, "nearest", "constant", is_normal=True)          # 2 channels
    with pytest.raises(ValueError):
        S.affine_numpy(far, x.astype(np.float64), "linear", "constant")


# ---- draw order -----------------------------------------------------------------------------------------------------------------
def test_draw_order():
    rot = {"axes": ("y", "z"), "max_degrees": 25.0, "p": 0.6}
    sc = {"range": (0.8, 1.25), "p": 0.4}
    hits = set()
    for seed in range(40):
        got = S.draw_affine(random.Random(seed), rot, sc)
        r = random.Random(seed)
        want = S.AffineOp()
        took_r = r.random() < 0.6
        if took_r:
            for ax in ("y", "z"):
                want = S.compose(want, S.rotation_op(ax, r.uniform(-25.0, 25.0)))
        took_s = r.random() < 0.4
        if took_s:
            want = S.compose(want, S.scale_op(r.uniform(0.8, 1.25)))
        assert got == want, seed
        hits.add((took_r, took_s))
    assert len(hits) == 4
    for seed in range(5):          # the edges: p = 0 never, p = 1 always, and each block still takes its one random()
        r0 = random.Random(seed)
        assert S.draw_affine(r0, dict(rot, p=0.0), dict(sc, p=0.0)).is_identity()
        ref = random.Random(seed)
        ref.random(), ref.random()
        assert r0.random() == ref.random()
        r1, ref = random.Random(seed), random.Random(seed)
        op = S.draw_affine(r1, dict(rot, p=1.0), dict(sc, p=1.0))
        ref.random()
        a, b = ref.uniform(-25.0, 25.0), ref.uniform(-25.0, 25.0)
        ref.random()
        s = ref.uniform(0.8, 1.25)
        assert op == S.compose(S.compose(S.rotation_op("y", a), S.rotation_op("z", b)), S.scale_op(s))
    assert S.draw_affine(random.Random(0)).is_identity()
    r = random.Random(0)
    r.random()
    assert S.draw_affine(random.Random(0), None, dict(sc, p=1.0)) == S.scale_op(r.uniform(0.8, 1.25))          # rotation off: no call for it


# ---- compose and the vector rule ------------------------------------------------------------------------------------------------
def test_rotated_normals_stay_perpendicular_to_the_rotated_plane():
    """A plane n . (r - centre) = 0 with unit normal n (components x, y, z), as a mask of the voxels within 0.8 of it and a normals
    target n on the mask, 0 elsewhere.  After `op` both are sampled nearest, so every output voxel holds vector @ n or 0.  The
    rotated plane's in-plane directions are vector @ u for u perpendicular to n; a sampled normal must be perpendicular to them.
    Bound: the dot product is a 3-term float32 sum of products of numbers of magnitude <= 1, evaluated on vectors that carry the
    rounding of the float32 matrix (U per entry, 3 entries per component) and of the 3-term vector rule (3 roundings): every one of
    the three components is off by at most 6 U, so |dot| <= 3 * 6 U plus 3 U for the dot product itself taken in float64 from
    float32 inputs: 21 U.  Where the mask is 0 the normals stay EXACTLY 0."""
    shape = (20, 20, 20)
    n = np.array([0.36, 0.48, 0.8])
    z, y, x = np.meshgrid(*[np.arange(k, dtype=np.float64) - (k - 1) / 2.0 for k in shape], indexing="ij")
    mask = (np.abs(n[0] * x + n[1] * y + n[2] * z) < 0.8).astype(np.float32)
    normals = (n.astype(np.float32)[:, None, None, None] * mask[None]).astype(np.float32)
    op = S.compose(S.compose(S.rotation_op("z", 25.0), S.rotation_op("x", -17.0)), S.scale_op(0.9))
    m2 = S.affine_numpy(op, mask, "nearest", "constant")
    n2 = S.affine_numpy(op, normals, "nearest", "constant", is_normal=True)
    on = m2 > 0
    assert 0.05 < on.mean() < 0.5 and set(np.unique(m2)) <= {0.0, 1.0}
    assert (n2[:, ~on] == 0).all() and same_bits(np.abs(n2[:, ~on]), np.zeros_like(n2[:, ~on]))
    V = op.vector64
    u1 = np.cross(n, [1.0, 0.0, 0.0])
    u1 /= np.linalg.norm(u1)
    u2 = np.cross(n, u1)
    got = n2[:, on].astype(np.float64)          # (3, K)
    n32 = n.astype(np.float32).astype(np.float64)
    for u in (V @ u1, V @ u2):
        # the float32 rounding of n itself moves it off the plane's normal by |n32 - n| <= U / 2 per component: 3 * U / 2 more
        assert np.abs(u @ got).max() <= 21 * U + 1.5 * U
    assert np.abs(np.linalg.norm(got, axis=0) - np.linalg.norm(n32)).max() <= 21 * U          # a rotation keeps length
    # the sampled mask IS the rotated plane: its voxels lie within the slab of the plane with normal V n (scaled by 1 / 0.9),
    # up to the half-voxel diagonal of nearest sampling
    vn = V @ n
    dist = np.abs(vn[0] * x + vn[1] * y + vn[2] * z)[on] * 0.9
    assert dist.max() < 0.8 + math.sqrt(3.0) / 2.0
    # compose(a, b) is a, then b: at right angles it is geometry_device's compose (which test_geometry_cpu pins to the reference's
    # classes applied one after the other), and the other order is a different op
    a, b = S.rotation_op("y", 90.0), S.rotation_op("z", 90.0)
    ga, gb = G.rot90_op("y", 1), G.rot90_op("z", 1)
    ab, ba = S.compose(a, b), S.compose(b, a)
    for got, want in ((ab, S.from_geom(G.compose(ga, gb))), (ba, S.from_geom(G.compose(gb, ga)))):
        assert np.abs(got.point - want.point).max() < 1e-6 and np.abs(got.vector - want.vector).max() < 1e-6
    assert np.abs(ab.point - ba.point).max() > 0.9
    assert np.allclose(S.compose(a, b).vector64, b.vector64 @ a.vector64)


# ---- dataset_config.spatial -----------------------------------------------------------------------------------------------------
TASKS = {"sheet": {"channels": 1}, "normals": {"channels": 3}}
BLOCK = {"rotation": {"axes": ["z", "y", "x"], "max_degrees": 30, "p": 0.5}, "scale": {"range": [0.8, 1.25], "p": 0.3},
         "normal_keys": ["normals"], "image_border": "constant", "where": "device"}


def test_parse_spatial():
    assert S.parse_spatial({}, (8, 8, 8), TASKS) is None and S.parse_spatial(None, (8, 8, 8), TASKS) is None
    assert S.parse_spatial({"spatial": False}, (8, 8, 8), TASKS) is None
    got = S.parse_spatial({"spatial": BLOCK}, (8, 16, 16), TASKS)
    assert got == {"rotation": {"axes": ("z", "y", "x"), "max_degrees": 30.0, "p": 0.5}, "scale": {"range": (0.8, 1.25), "p": 0.3},
                   "normal_keys": ("normals",), "image_border": "constant", "where": "device"}
    assert S.parse_spatial({"spatial": {"scale": {"range": [0.5, 2], "p": 1}, "where": "HOST", "image_border": "clamp"}}, (8, 8, 8), TASKS) == {
        "rotation": None, "scale": {"range": (0.5, 2.0), "p": 1.0}, "normal_keys": ("normals",), "image_border": "clamp", "where": "host"}
    refused = {
        "spatial: unknown": dict(BLOCK, elastic=True),
        "spatial.rotation: unknown": dict(BLOCK, rotation={"degrees": 3}),
        "spatial.scale: unknown": dict(BLOCK, scale={"factor": 3}),
        "spatial.rotation.p": dict(BLOCK, rotation={"p": 1.5}),
        "spatial.scale.p": dict(BLOCK, scale={"p": -0.1}),
        "spatial.rotation.max_degrees": dict(BLOCK, rotation={"max_degrees": 0}),
        "spatial.rotation.max_degrees:": dict(BLOCK, rotation={"max_degrees": 181}),
        "spatial.scale.range": dict(BLOCK, scale={"range": [0.4, 1.0]}),
        "spatial.scale.range:": dict(BLOCK, scale={"range": [1.0, 2.5]}),
        "spatial.scale.range: ": dict(BLOCK, scale={"range": [1.2, 1.1]}),
        "spatial.rotation.axes": dict(BLOCK, rotation={"axes": ["z", "w"]}),
        "spatial.where": dict(BLOCK, where="gpu"),
        "spatial.image_border": dict(BLOCK, image_border="reflect"),
    }
    for key, block in refused.items():
        with pytest.raises(ValueError, match=key.rstrip(": ").replace(".", r"\.")):
            S.parse_spatial({"spatial": block}, (8, 8, 8), TASKS)
    with pytest.raises(ValueError, match=r"dataset_config\.spatial.*3-D patch"):
        S.parse_spatial({"spatial": BLOCK}, (64, 64), TASKS)
    with pytest.raises(ValueError, match=r"dataset_config\.spatial\.normal_keys.*sheet"):
        S.parse_spatial({"spatial": dict(BLOCK, normal_keys=["sheet"])}, (8, 8, 8), TASKS)
    assert S.parse_spatial({"spatial": dict(BLOCK, rotation={"max_degrees": 180})}, (8, 8, 8), TASKS)["rotation"]["max_degrees"] == 180.0
    # the geometric block and its parser are untouched by the new one
    assert G.parse_geometric({"spatial": BLOCK}, (8, 8, 8), TASKS) is None


def test_zarr_dataset_refuses_host_spatial_behind_device_stages(tmp_path):
    from mt3d_amd.dataloading.dataset import ZarrSegmentationDataset3D

    def mgr(dilate_label=False, **dataset_config):
        return SimpleNamespace(model_name="m", tasks=TASKS, train_patch_size=(16, 16, 16), min_labeled_ratio=0.1, min_bbox_percent=0.9,
                               dilate_label=dilate_label, use_cache=False, cache_folder=str(tmp_path), volume_paths=[],
                               dataset_config=dict(augment=False, **dataset_config))
    host = dict(BLOCK, where="host")
    with pytest.raises(ValueError, match=r"dataset_config\.spatial\.where.*ingest"):
        ZarrSegmentationDataset3D(mgr(spatial=host, ingest={"where": "device"}))
    with pytest.raises(ValueError, match=r"dataset_config\.spatial\.where.*dilate"):
        ZarrSegmentationDataset3D(mgr(dilate_label=True, spatial=host, dilate={"where": "device"}))
    # the same block on the device, or on the host behind host stages, is accepted
    assert ZarrSegmentationDataset3D(mgr(spatial=BLOCK, ingest={"where": "device"})).device_spatial["where"] == "device"
    ds = ZarrSegmentationDataset3D(mgr(dilate_label=True, spatial=host, dilate={"where": "host"}))
    assert ds.device_spatial is None and ds.spatial["where"] == "host"
    assert ZarrSegmentationDataset3D(mgr()).spatial is None


# ---- host path ------------------------------------------------------------------------------------------------------------------
def _synthetic(**dataset_config):
    from mt3d_amd.dataloading.dataset import SyntheticPatchDataset
    tasks = {"sheet": {"channels": 1}, "normals": {"channels": 3, "loss_fn": "MaskedCosineLoss"}}
    return SyntheticPatchDataset(SimpleNamespace(train_patch_size=(12, 12, 12), in_channels=1, tasks=tasks,
                                                 dataset_config=dict(synthetic_length=8, synthetic_pool=4, **dataset_config)))


def test_host_path_of_the_synthetic_dataset():
    plain, dev = _synthetic(), _synthetic(spatial=BLOCK)
    assert plain.spatial is None and plain.device_spatial is None
    assert dev.device_spatial == dev.spatial and dev.spatial["where"] == "device"
    for k, v in dev[1].items():          # where: device leaves the items alone
        assert torch.equal(v, plain[1][k])
    block = dict(BLOCK, where="host", rotation=dict(BLOCK["rotation"], p=1.0), scale=dict(BLOCK["scale"], p=1.0))
    host = _synthetic(spatial=block)
    assert host.device_spatial is None
    host.spatial_rng = random.Random(7)
    want_rng = random.Random(7)
    for idx in (1, 2, 1):
        item, raw = host[idx], plain[idx]
        op = S.draw_affine(want_rng, host.spatial["rotation"], host.spatial["scale"])
        assert host.last_spatial_op == op and not op.is_identity()
        assert same_bits(item["image"].numpy(), S.affine_numpy(op, raw["image"].numpy(), "linear", "constant", 0.0))
        assert same_bits(item["sheet"].numpy(), S.affine_numpy(op, raw["sheet"].numpy(), "nearest", "constant", 0.0))
        assert same_bits(item["normals"].numpy(), S.affine_numpy(op, raw["normals"].numpy(), "nearest", "constant", 0.0, True))
        assert set(np.unique(item["sheet"].numpy())) <= {0.0, 1.0}
        assert item["image"].dtype == torch.float32 and item["normals"].shape == raw["normals"].shape
    for k, v in plain[1].items():          # the pool's cached items were not written to
        assert torch.equal(v, _synthetic()[1][k])


# ---- the kernel's per-voxel functions on the CPU, under AddressSanitizer ---------------------------------------------------------
def test_kernel_arithmetic_on_the_cpu_matches_the_statement(tmp_path):
    """csrc/rx_affine_core.h is what the kernel calls per voxel.  A stand-alone C++ program runs it over the GPU tests' shapes and
    modes against a dump of affine_numpy, compiled with -fsanitize=address,undefined (and without fp contraction): every voxel
    must have affine_numpy's bits and no tap may leave the sample's heap buffer, whatever the matrix."""
    csrc = os.path.join(ROOT, "multi-task-3d-resencoder-unet_amd", "csrc")
    exe = str(tmp_path / "affine_host_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-Wno-unknown-pragmas", os.path.join(csrc, "tools", "affine_host_check.cpp"), "-o", exe])
    rng = random.Random(3)
    ops = [S.AffineOp(), S.from_geom(G.rot90_op("x", 1)), S.rotation_op("z", 7.0), S.rotation_op("y", 30.0), S.rotation_op("x", 45.0),
           S.compose(S.rotation_op("z", 90.0), S.rotation_op("y", 30.0)), S.scale_op(0.5), S.scale_op(2.0),
           S.draw_affine(rng, {"p": 1.0}, {"p": 1.0}), S.AffineOp(np.eye(3) * 1e30, None),
           S.AffineOp([[3e38, -3e38, 0], [0, 1, 0], [0, 0, 1]], None)]          # the last: inf - inf, a NaN coordinate
    cases = []
    for shape in [(10, 10, 10), (6, 12, 20), (9, 5, 33)]:
        for ci, (channels, interp, border, fill, vector) in enumerate([(1, "linear", "constant", 0.0, False), (2, "linear", "constant", 0.5, False),
                                                                       (3, "linear", "clamp", 0.0, True), (3, "nearest", "constant", 0.0, True),
                                                                       (3, "nearest", "clamp", 0.0, False)]):
            x = positive_field((channels, *shape), ci)
            for op in ops:
                want = S.affine_numpy(op, x, interp, border, fill, vector)
                if np.isnan(want).any():          # (a NaN coordinate: the value is unspecified; the run must still stay in bounds)
                    want = None
                cases.append((x, op, S.INTERP[interp], S.BORDER[border], fill, vector, want))
    nan_cases = [i for i, c in enumerate(cases) if c[6] is None]
    assert nan_cases and len(cases) - len(nan_cases) > 100
    dump = tmp_path / "cases.bin"
    with open(dump, "wb") as f:
        f.write(struct.pack("<i", len(cases)))
        for x, op, interp, border, fill, vector, want in cases:
            f.write(struct.pack("<7i", *x.shape, interp, border, int(vector)))
            f.write(struct.pack("<f", fill))
            f.write(op.row().astype("<f4").tobytes())
            f.write(x.astype("<f4").tobytes())
            f.write((x if want is None else want).astype("<f4").tobytes())
    r = subprocess.run([exe, str(dump)], capture_output=True, text=True, timeout=300)
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    bad = [int(l.split()[1]) for l in r.stdout.splitlines() if l.startswith("case ")]
    assert set(bad) <= set(nan_cases), r.stdout[-3000:]
    assert r.returncode in (0, 1) and f"{len(cases)} cases" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
