"""CPU: the statements of mesh orientation (postprocess/orient.py) over the shared case list -- sampling at lattice points, beyond the
six borders and in slabs, the unit rule, the front / back / rim partition of the slab sheet and the graded ball, the selection of
one face and its way back into `MeshTargetBuilder` -- the config block, the `MeshOrienter` driver on the host, resident and in
slabs, and the kernels' own per-vertex and per-triangle work (csrc/rx_meshsample_core.h) run serially under the address and
undefined-behaviour sanitizers.  Everything compares with array_equal, floats by their bits."""
import os
import subprocess

import numpy as np
import pytest

import isosurface_cases as I
import mesh_orient_cases as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


def _pp():
    import mt3d_amd  # noqa: F401
    import mt3d_amd.postprocess as pp
    return pp


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.int32)


def _at(vol, q, rule, pp):
    """the decoded voxels at the lattice points q (x, y, z) -> (V, C)"""
    i = q.astype(np.int64)
    return pp.decode_numpy(vol[:, i[:, 2], i[:, 1], i[:, 0]], rule).T


# ---- sampling ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule", list(O.RULES))
def test_lattice_points_return_the_decoded_voxel(rule):
    pp = _pp()
    _, vol, pts, _ = O.sample_case(f"{rule}-lattice")
    got, owned = pp.sample_points_numpy(vol, pts, rule)
    assert got.dtype == F32 and got.shape == (len(pts), vol.shape[0]) and owned.all()
    assert np.array_equal(_bits(got), _bits(_at(vol, pts, rule, pp)))
    assert np.array_equal(_bits(got), _bits(pp.decode_numpy(vol, rule).reshape(vol.shape[0], -1).T))      # lattice order is voxel order


@pytest.mark.parametrize("rule", list(O.RULES))
def test_points_outside_equal_the_clamped_border(rule):
    pp = _pp()
    vol = O.volume(rule, (3, 5, 6, 7), 2)
    sides = O.outside((5, 6, 7))
    assert len(sides) == 18      # six sides, three distances each
    for p, q in sides:
        got, owned = pp.sample_points_numpy(vol, p, rule)
        assert owned.all() and np.array_equal(_bits(got), _bits(_at(vol, q, rule, pp)))


def test_copy_keeps_signed_zero_and_denormals():
    pp = _pp()
    _, vol, pts, rule = O.sample_case("copy-signed-zero-denormal")
    got, _ = pp.sample_points_numpy(vol, pts, rule)
    assert np.array_equal(_bits(got[:, 0]), _bits(vol.ravel()))
    flat = _bits(got[:, 0])
    assert flat[13] == np.int32(-2**31) and flat[4] == 1 and flat[10] == np.int32(-2**31) + 2142      # -0.0, 1e-45, -3e-42
    # halfway between two denormals the lerp is exact: still a denormal
    v = np.zeros((1, 1, 1, 2), F32)
    v[0, 0, 0] = np.array([2, 6], np.int32).view(F32)
    got, _ = pp.sample_points_numpy(v, np.array([[0.5, 0, 0]], F32), "copy")
    assert _bits(got)[0, 0] == 4


def test_rule_must_match_the_dtype_and_the_channels_are_limited():
    pp = _pp()
    p = np.zeros((1, 3), F32)
    for rule, dtype in (("copy", np.uint8), ("u8", np.uint16), ("u16", np.uint8), ("normal_u16", np.float32), ("other", np.uint8)):
        with pytest.raises(ValueError, match="rule"):
            pp.sample_points_numpy(np.zeros((1, 2, 2, 2), dtype), p, rule)
    for shape in ((9, 2, 2, 2), (2, 2, 2), (0, 2, 2, 2)):
        with pytest.raises(ValueError, match="volume"):
            pp.sample_points_numpy(np.zeros(shape, np.uint8), p, "u8")
    for z_base, z_total in ((-1, 4), (3, 4), (0, 1)):
        with pytest.raises(ValueError, match="slab"):
            pp.sample_points_numpy(np.zeros((1, 2, 2, 2), np.uint8), p, "u8", z_base, z_total)


def test_every_split_into_slabs_gives_the_resident_bits_and_owns_each_point_once():
    pp = _pp()
    vol = O.volume("u16", (3, 5, 6, 7), 1)
    pts = O.points((5, 6, 7), 40, 3)
    assert (pts[:, 2] < 0).any() and (pts[:, 2] > 4).any() and (pts[:, 2] == 4).any() and (pts[:, 2] == 0).any()
    for rule in ("u16", "normal_u16"):
        want, all_owned = pp.sample_points_numpy(vol, pts, rule)
        assert all_owned.all()
        for depth in (1, 2, 3, 4, 5):
            slabs = pp.slab_ranges(5, depth)
            assert slabs[0][0] == 0 and slabs[-1][0] + slabs[-1][1] == 5 and all(p <= depth + 1 for _, p in slabs)
            union, times = np.full_like(want, np.nan), np.zeros(len(pts), np.int64)
            for z_base, planes in slabs:
                got, owned = pp.sample_points_numpy(vol[:, z_base:z_base + planes], pts, rule, z_base, 5)
                assert (got[~owned] == 0).all()
                union[owned] = got[owned]
                times += owned
            assert (times == 1).all(), depth
            assert np.array_equal(_bits(union), _bits(want)), depth
    assert pp.slab_ranges(1, 3) == [(0, 1)] and pp.slab_ranges(5, 1) == [(0, 2), (1, 2), (2, 2), (3, 2)] and pp.slab_ranges(5, 2) == [(0, 3), (2, 3)]


def test_unit_numpy():
    pp = _pp()
    v = np.array([[0, 0, 0], [-0.0, 0, 0], [3, 0, 4], [1e-30, 0, 0], [0, -2, 0], [1e-45, 0, 0]], F32)
    u = pp.unit_numpy(v)
    assert np.array_equal(_bits(u[0]), np.zeros(3, np.int32)) and np.array_equal(_bits(u[1]), np.zeros(3, np.int32))      # exactly +0
    assert np.array_equal(u[2], np.array([3, 0, 4], F32) / F32(5)) and np.array_equal(u[4], [0, -1, 0])
    assert np.array_equal(_bits(u[3]), np.zeros(3, np.int32)) and np.array_equal(_bits(u[5]), np.zeros(3, np.int32))      # x*x underflows: l is 0


# ---- classification and selection -------------------------------------------------------------------------------------------------------------
def _classified(pp, name):
    _, v, t, n, min_cos = next(c for c in O.mesh_cases() if c[0] == name)
    cos = pp.face_cos_numpy(v, t, n)
    return v, t, n, cos, pp.side_numpy(cos, min_cos)


def _face_z(v, t):
    p = v[t].astype(np.float64)
    return np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])[:, 2]


def test_slab_sheet_front_back_and_rim():
    pp = _pp()
    v, t, n, cos, side = _classified(pp, "sheet")
    assert cos.dtype == F32 and side.dtype == np.int8 and set(np.unique(side)) == {-1, 0, 1}
    front, back, rim = side == 1, side == -1, side == 0
    assert front.sum() + back.sum() + rim.sum() == len(t) and front.sum() == back.sum() > 0 and rim.sum() > 0
    assert (_face_z(v, t)[front] > 0).all() and (_face_z(v, t)[back] < 0).all()
    fv, ft, (fn,), row_of = pp.select_numpy(v, t, front, n)
    mid = (O.SHEET["z"][0] + O.SHEET["z"][1] - 1) / 2
    assert len(fv) and (fv[:, 2] > mid).all() and fn.shape == fv.shape
    edges = np.sort(np.concatenate([ft[:, [0, 1]], ft[:, [1, 2]], ft[:, [2, 0]]]), 1)
    _, uses = np.unique(edges, axis=0, return_counts=True)
    assert (uses == 1).any() and uses.max() == 2      # open: it has a boundary
    # row_of is consistent with the outputs
    used = np.unique(t[front])
    assert row_of.dtype == np.int64 and row_of.shape == (len(v),) and np.array_equal(np.nonzero(row_of >= 0)[0], used)
    assert np.array_equal(row_of[used], np.arange(len(fv))) and np.array_equal(_bits(fv), _bits(v[used])) and np.array_equal(_bits(fn), _bits(n[used]))
    assert np.array_equal(ft, row_of[t[front]]) and np.array_equal(_bits(fv[ft]), _bits(v[t[front]]))      # input order, same corners
    bv, _, _, _ = pp.select_numpy(v, t, back)
    assert (bv[:, 2] < mid).all()
    ev, et, _, erow = pp.select_numpy(v, t, np.zeros(len(t), bool))
    assert ev.shape == (0, 3) and et.shape == (0, 3) and (erow == -1).all()


def test_ball_front_is_above_the_centre_and_back_below():
    pp = _pp()
    v, t, n, cos, side = _classified(pp, "ball")
    centroid_z = v[t][:, :, 2].astype(np.float64).mean(1)
    cz = I.BALL["centre"][0]
    assert (side == 1).sum() > 100 and (side == -1).sum() > 100 and (side == 0).sum() > 0
    assert (centroid_z[side == 1] > cz).all() and (centroid_z[side == -1] < cz).all()


def test_degenerate_triangle_and_zero_vector_are_rim():
    pp = _pp()
    v, t, n, cos, side = _classified(pp, "rim")
    assert np.isnan(cos[0]) and np.isnan(cos[1]) and cos[2] == 1 and cos[3] == -1
    assert side.tolist() == [0, 0, 1, -1]
    assert pp.side_numpy(np.array([0.2, -0.2, 0.21, -0.21, np.nan, np.inf, -np.inf], F32), 0.2).tolist() == [0, 0, 1, -1, 0, 1, -1]


def test_front_face_goes_back_into_the_mesh_target_builder(tmp_path):
    """loop closure: the front face of the slab sheet with its predicted normals is a mesh `MeshTargetBuilder` accepts, and what it
    paints points up"""
    pp = _pp()
    from mt3d_amd.dataloading import zarr_lite
    from mt3d_amd.tasks.normals.mesh_targets import MeshTargetBuilder
    v, t, n, cos, side = _classified(pp, "sheet")
    fv, ft, (fn,), _ = pp.select_numpy(v, t, side == 1, n)
    Z, Y, X = O.SHEET["shape"]
    MeshTargetBuilder([(fv, ft, fn)], (Z, Y, X), where="host").normals_volume(str(tmp_path / "normals.zarr"))
    vol = zarr_lite.open(str(tmp_path / "normals.zarr" / "volume"))[...]
    painted = (vol != 0).any(-1)
    assert vol.dtype == np.uint16 and painted.sum() > 0
    assert (vol[painted][:, 2].astype(np.float64) / 32767.5 - 1 > 0.9).all()


# ---- the config block -------------------------------------------------------------------------------------------------------------------------
TARGETS = {"sheet": {"channels": 1}, "normals": {"channels": 3}, "ink": {"channels": 1}}


def test_parse_orient_config():
    pp = _pp()
    mesh = {"tasks": ["sheet"], "source": "final"}
    got = pp.parse_config({"mesh": mesh, "orient": {"tasks": ["sheet"]}}, TARGETS, (16, 16, 16))
    assert got["orient"] == dict(tasks=("sheet",), normals_task="normals", side="front", min_cos=0.2, normals="predicted", max_device_gb=None)
    full = {"tasks": "sheet", "normals_task": "normals", "side": "back", "min_cos": 0, "normals": "mesh", "max_device_gb": 8}
    assert pp.parse_config({"mesh": mesh, "orient": full}, TARGETS)["orient"] == dict(tasks=("sheet",), normals_task="normals", side="back",
                                                                                     min_cos=0.0, normals="mesh", max_device_gb=8.0)
    without = pp.parse_config({"mesh": mesh}, TARGETS)
    assert "orient" not in without and pp.parse_config(None, TARGETS) is None


@pytest.mark.parametrize("key,block", [
    ("orient.cell", {"tasks": ["sheet"], "cell": 2}),
    ("orient.tasks", {}),
    ("orient.tasks", {"tasks": ["ink"]}),
    ("orient.tasks", {"tasks": []}),
    ("orient.normals_task", {"tasks": ["sheet"], "normals_task": "nothing"}),
    ("orient.normals_task", {"tasks": ["sheet"], "normals_task": "sheet"}),
    ("orient.normals_task", {"tasks": ["sheet"], "normals_task": 3}),
    ("orient.side", {"tasks": ["sheet"], "side": "top"}),
    ("orient.side", {"tasks": ["sheet"], "side": None}),
    ("orient.min_cos", {"tasks": ["sheet"], "min_cos": 1}),
    ("orient.min_cos", {"tasks": ["sheet"], "min_cos": -0.1}),
    ("orient.min_cos", {"tasks": ["sheet"], "min_cos": "0.2"}),
    ("orient.min_cos", {"tasks": ["sheet"], "min_cos": True}),
    ("orient.min_cos", {"tasks": ["sheet"], "min_cos": float("nan")}),
    ("orient.normals", {"tasks": ["sheet"], "normals": True}),
    ("orient.normals", {"tasks": ["sheet"], "normals": "sampled"}),
    ("orient.max_device_gb", {"tasks": ["sheet"], "max_device_gb": 0}),
    ("orient.max_device_gb", {"tasks": ["sheet"], "max_device_gb": -1}),
    ("orient.max_device_gb", {"tasks": ["sheet"], "max_device_gb": True}),
])
def test_every_refusal_of_the_parser_names_its_key(key, block):
    pp = _pp()
    with pytest.raises(ValueError, match=f"inference_config.postprocess.{key}".replace(".", r"\.")):
        pp.parse_config({"mesh": {"tasks": ["sheet"], "source": "final"}, "orient": block}, TARGETS)


def test_parser_refusals_that_depend_on_the_siblings():
    pp = _pp()
    with pytest.raises(ValueError, match=r"postprocess\.orient\.tasks"):      # no mesh block
        pp.parse_config({"orient": {"tasks": ["sheet"]}}, TARGETS)
    with pytest.raises(ValueError, match=r"postprocess\.orient\.normals_task"):      # a `normals` target with another channel count
        pp.parse_config({"mesh": {"tasks": ["sheet"], "source": "final"}, "orient": {"tasks": ["sheet"]}},
                        {"sheet": {"channels": 1}, "normals": {"channels": 2}})
    with pytest.raises(ValueError, match=r"postprocess\.orient: expected a mapping"):
        pp.parse_config({"mesh": {"tasks": ["sheet"], "source": "final"}, "orient": ["sheet"]}, TARGETS)
    with pytest.raises(ValueError, match=r"postprocess\.orients: unknown key"):
        pp.parse_config({"orients": {}}, TARGETS)


def test_config_manager_reads_the_block(tmp_path):
    import yaml
    import mt3d_amd  # noqa: F401
    from mt3d_amd.configuration.config_manager import ConfigManager
    p = tmp_path / "c.yaml"
    p.write_text(yaml.safe_dump({"tr_setup": {}, "tr_config": {"patch_size": [16, 16, 16]}, "model_config": {},
                                 "dataset_config": {"targets": {"sheet": {"channels": 1, "activation": "sigmoid"},
                                                                "normals": {"channels": 3, "activation": "none"}}},
                                 "inference_config": {"postprocess": {"mesh": {"tasks": ["sheet"], "source": "final"},
                                                                      "orient": {"tasks": ["sheet"], "side": "both"}}}}))
    m = ConfigManager(str(p), verbose=False)
    assert m.infer_postprocess["orient"] == dict(tasks=("sheet",), normals_task="normals", side="both", min_cos=0.2, normals="predicted",
                                                 max_device_gb=None)


# ---- the driver on the host -------------------------------------------------------------------------------------------------------------------
def _store(tmp_path, pp, fmt="obj", name="sheet"):
    from mt3d_amd.dataloading import zarr_lite
    v, t = O.sheet_mesh()
    store = tmp_path / "store"
    rng = np.random.default_rng(8)
    field = O.constant_field(O.SHEET["shape"]).astype(np.int64) + rng.integers(-3000, 3000, (3,) + O.SHEET["shape"])      # a field that varies
    zarr_lite.write_array(str(store / "normals_final"), np.clip(field, 0, 65535).astype(np.uint16), (3, 4, 8, 8), compressor="zlib")
    (pp.write_obj if fmt == "obj" else pp.write_ply)(str(store / f"{name}.{fmt}"), v, t)
    return store, v, t


@pytest.mark.parametrize("fmt", ["obj", "ply"])
def test_host_driver_resident_and_in_slabs_writes_the_same_bytes(tmp_path, fmt):
    pp = _pp()
    from mt3d_amd.dataloading import zarr_lite
    store, v, t = _store(tmp_path, pp, fmt)
    field = zarr_lite.open(str(store / "normals_final"))[...]
    unit = pp.unit_numpy(pp.sample_points_numpy(field, v, "normal_u16")[0])
    cos = pp.face_cos_numpy(v, t, unit)
    side = pp.side_numpy(cos, 0.2)
    files, Z, Y, X = {}, *O.SHEET["shape"]
    for how, budget in (("resident", None), ("slabs", pp.MeshOrienter.scratch_bytes(len(v), len(t), 3, 6, Y, X))):      # six planes: two buffers of three
        o = pp.MeshOrienter(max_device_bytes=budget, where="host")
        out = tmp_path / f"{how}.{fmt}"
        summary = o.run(str(store / f"sheet.{fmt}"), str(store), out=str(out))
        files[how] = (summary, out.read_bytes())
        assert o.last_slabs == (1 if how == "resident" else 5) and not os.path.exists(str(out) + ".partial")
    assert files["resident"] == files["slabs"] and len(files["resident"][1]) > 1000
    s = files["resident"][0]
    fv, ft, (fn,), _ = pp.select_numpy(v, t, side == 1, unit)
    assert s == dict(vertices=len(fv), triangles=len(ft), input_vertices=len(v), input_triangles=len(t), front=int((side == 1).sum()),
                     back=int((side == -1).sum()), rim=int((side == 0).sum()), zero_normals=0,
                     mean_abs_cos=float(np.abs(cos[~np.isnan(cos)]).astype(np.float64).mean()))
    gv, gt, gn = pp.read_mesh(str(tmp_path / f"resident.{fmt}"))
    assert np.array_equal(_bits(gv), _bits(fv)) and np.array_equal(gt, ft) and np.array_equal(_bits(gn), _bits(fn))


def test_host_driver_names_sides_and_normals(tmp_path):
    pp = _pp()
    store, v, t = _store(tmp_path, pp)
    mesh = str(store / "sheet.obj")
    for side, name in (("front", "sheet_front.obj"), ("back", "sheet_back.obj"), ("both", "sheet_oriented.obj")):
        s = pp.MeshOrienter(side=side, where="host").run(mesh, str(store))
        assert (store / name).exists() and s["triangles"] == {"front": s["front"], "back": s["back"], "both": len(t)}[side]
    with pytest.raises(FileExistsError, match="sheet_front.obj already exists"):      # an existing output file is refused
        pp.MeshOrienter(where="host").run(mesh, str(store))
    s = pp.MeshOrienter(normals="mesh", where="host").run(mesh, str(store), out=str(tmp_path / "m.obj"))
    gv, gt, gn = pp.read_mesh(str(tmp_path / "m.obj"))
    assert np.array_equal(_bits(gn), _bits(pp.vertex_normals_numpy(gv, gt))) and s["vertices"] == len(gv)
    both = pp.read_mesh(str(store / "sheet_oriented.obj"))
    assert np.array_equal(_bits(both[0]), _bits(v)) and np.array_equal(both[1], t)


def test_host_driver_refusals(tmp_path):
    pp = _pp()
    from mt3d_amd.dataloading import zarr_lite
    store, v, t = _store(tmp_path, pp)
    mesh = str(store / "sheet.obj")
    Z, Y, X = O.SHEET["shape"]
    need = pp.MeshOrienter.scratch_bytes(len(v), len(t), 3, 2, Y, X)
    with pytest.raises(MemoryError, match=f"needs {need} bytes"):
        pp.MeshOrienter(max_device_bytes=need - 1, where="host").run(mesh, str(store))
    o = pp.MeshOrienter(max_device_bytes=need, where="host")      # two planes fit: one buffer, slabs of one owned plane
    o.run(mesh, str(store), out=str(tmp_path / "two.obj"))
    assert o.last_slabs == Z - 1
    assert (tmp_path / "two.obj").read_bytes() == _run_bytes(pp, mesh, store, tmp_path / "all.obj")
    zarr_lite.write_array(str(store / "last_final"), np.zeros((Z, Y, X, 3), np.uint16), (4, 8, 8, 3))
    zarr_lite.write_array(str(store / "bytes_final"), np.zeros((3, Z, Y, X), np.uint8), (3, 4, 8, 8))
    for name in ("last_final", "bytes_final", "missing_final"):
        with pytest.raises(ValueError, match="MeshOrienter"):
            pp.MeshOrienter(where="host").run(mesh, str(store), name, out=str(tmp_path / "never.obj"))
    assert not (tmp_path / "never.obj").exists()
    for kw in (dict(side="top"), dict(min_cos=1.0), dict(normals="none"), dict(fmt="stl"), dict(max_device_bytes=0), dict(where="gpu")):
        with pytest.raises(ValueError, match="MeshOrienter"):
            pp.MeshOrienter(**kw)


def _run_bytes(pp, mesh, store, out):
    pp.MeshOrienter(where="host").run(mesh, str(store), out=str(out))
    return out.read_bytes()


def test_command_line_on_the_host(tmp_path):
    pp = _pp()
    store, v, t = _store(tmp_path, pp)
    import sys
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "orient_mesh.py"), "--mesh", str(store / "sheet.obj"), "--store", str(store),
                        "--side", "back", "--min-cos", "0.3", "--where", "host", "--out", str(tmp_path / "cli.obj")],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    pp.MeshOrienter("back", 0.3, where="host").run(str(store / "sheet.obj"), str(store), out=str(tmp_path / "want.obj"))
    assert (tmp_path / "cli.obj").read_bytes() == (tmp_path / "want.obj").read_bytes() and '"back":' in r.stdout


# ---- the kernels' own work on the CPU, under the sanitizers -----------------------------------------------------------------------------------
def test_host_check_program(tmp_path):
    """csrc/rx_meshsample_core.h is what the kernels call.  A stand-alone C++ program runs the sampling of every rule and channel
    count, resident and in slabs of every depth, the unit rule, the cosine and the side serially over this file's kinds of volume,
    point and mesh against a direct restatement, compiled with -fsanitize=address,undefined."""
    csrc = os.path.join(ROOT, "multi-task-3d-resencoder-unet_amd", "csrc")
    exe = str(tmp_path / "meshsample_host_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-Wall", "-Wno-unknown-pragmas", os.path.join(csrc, "tools", "meshsample_host_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0 and "0 differ from the direct restatement" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
