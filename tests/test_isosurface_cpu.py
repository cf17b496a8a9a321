"""CPU: the invariants of the surface-nets statement over the shared case list, the graded ball, the OBJ / PLY writers, the whole
`SurfaceMesher` slab path with the statement in place of the kernels, the config block, and the kernels' own per-cell arithmetic
(csrc/rx_isosurface_core.h) run serially under the address and undefined-behaviour sanitizers."""
import os
import subprocess

import numpy as np
import pytest

import isosurface_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _pp():
    import mt3d_amd  # noqa: F401
    import mt3d_amd.postprocess as pp
    return pp


@pytest.mark.parametrize("level", C.LEVELS)
def test_statement_invariants(level):
    pp = _pp()
    for name, lv, values in C.cases():
        if lv != level:
            continue
        v, t = pp.surface_nets_numpy(values, level)
        assert v.dtype == np.float32 and v.shape == (len(v), 3) and t.dtype == np.int64 and t.shape == (len(t), 3), name
        assert pp.counts_numpy(values, level) == (len(v), len(t)), name
        uses, oriented = C.edge_uses(t)
        assert (uses % 2 == 0).all() and oriented, name      # closed (possibly non-manifold) and consistently oriented
        if len(t):
            assert t.min() >= 0 and t.max() < len(v), name
        assert np.isfinite(v).all(), name
        if len(v):
            assert (v.min(0) >= -1).all() and (v.max(0) <= np.array(values.shape[::-1], np.float32)).all(), name
        if name.split("-")[1] == "zero" or (values <= level).all():
            assert len(v) == 0 and len(t) == 0, name
        if name.split("-")[1] == "full":      # the closed box: every cell on the border of the cell grid, 2 triangles per face voxel
            Z, Y, X = values.shape
            assert len(v) == (Z + 1) * (Y + 1) * (X + 1) - max(Z - 1, 0) * max(Y - 1, 0) * max(X - 1, 0), name
            assert len(t) == 4 * (Z * Y + Y * X + Z * X), name
        if name.split("-")[1] == "checkerboard" and min(values.shape) > 1:
            # every cell is active but the corner cells of the grid whose one voxel is outside
            outside = int((values[np.ix_((0, -1), (0, -1), (0, -1))] <= level).sum())
            assert len(v) == np.prod([s + 1 for s in values.shape]) - outside, name


def test_empty_volume_and_bad_arguments():
    pp = _pp()
    v, t = pp.surface_nets_numpy(np.zeros((0, 4, 4), np.uint8), 127)
    assert v.shape == (0, 3) and v.dtype == np.float32 and t.shape == (0, 3) and t.dtype == np.int64
    assert pp.counts_numpy(np.zeros((0, 4, 4), np.uint8), 127) == (0, 0)
    for bad, level in ((np.zeros((4, 4), np.uint8), 127), (np.zeros((2, 2, 2), np.float32), 127), (np.zeros((2, 2, 2), np.uint8), 255),
                       (np.zeros((2, 2, 2), np.uint8), -1), (np.zeros((2, 2, 2), np.uint8), True)):
        with pytest.raises(ValueError, match="surface_nets_numpy"):
            pp.surface_nets_numpy(bad, level)


def test_one_voxel_positions_and_orientation():
    """a single voxel of 255 at level 127: t = 127.5 / 255 = 0.5 on every crossing edge.  Each of the eight cells has three crossing
    edges, which meet in the voxel; along an axis their mean offset is 2.5 / 3 seen from the cell's low side and 0.5 / 3 from its high
    side, so the vertices are the corners of a small cube around the voxel centre, oriented outwards"""
    pp = _pp()
    f = np.float32
    values = np.zeros((1, 1, 1), np.uint8) + 255
    v, t = pp.surface_nets_numpy(values, 127)
    lo, hi = f(-1) + f(2.5) / f(3), f(0) + f(0.5) / f(3)
    assert len(v) == 8 and len(t) == 12 and np.array_equal(np.unique(v), [lo, hi])
    assert np.array_equal(v[0], [lo, lo, lo]) and np.array_equal(v[1], [hi, lo, lo]) and np.array_equal(v[4], [lo, lo, hi])      # (x, y, z)
    p = v[t].astype(np.float64)
    assert np.isclose(np.einsum("ij,ij->i", p[:, 0], np.cross(p[:, 1], p[:, 2])).sum() / 6, (float(hi) - float(lo))**3)


def test_graded_ball():
    pp = _pp()
    R, centre = C.BALL["R"], np.array(C.BALL["centre"])
    values = C.ball(C.BALL["shape"], R, C.BALL["centre"])
    v, t = pp.surface_nets_numpy(values, 127)
    uses, oriented = C.edge_uses(t)
    assert (uses == 2).all() and oriented      # a closed 2-manifold
    p = v[t].astype(np.float64)
    volume = np.einsum("ij,ij->i", p[:, 0], np.cross(p[:, 1], p[:, 2])).sum() / 6
    sphere = 4 / 3 * np.pi * R**3
    dist = np.abs(np.linalg.norm(v.astype(np.float64) - centre[::-1], axis=1) - R)
    print("volume", volume, "sphere", sphere, "max distance", dist.max())
    assert volume > 0 and abs(volume - sphere) <= 0.03 * sphere
    assert dist.max() <= np.sqrt(3) + 0.1      # a vertex lies in a cell with a sign change; the diagonal is sqrt(3); 0.1 for the uint8 rounding


# ---- writers ---------------------------------------------------------------------------------------------------------------------------
def test_obj_round_trip_and_ply(tmp_path):
    pp = _pp()
    from mt3d_amd.tasks.normals.mesh_targets import read_obj
    values = dict(C.volumes((9, 10, 12), 127))["random50"]
    v, t = pp.surface_nets_numpy(values, 127)
    obj = tmp_path / "m.obj"
    pp.write_obj(str(obj), v, t)
    rv, rt = read_obj(str(obj))
    assert rv.dtype == np.float32 and np.array_equal(rv.view(np.int32), v.view(np.int32)) and np.array_equal(rt, t)
    assert sorted(os.listdir(tmp_path)) == ["m.obj"]
    with pytest.raises(FileExistsError, match="m.obj"):
        pp.write_obj(str(obj), v, t)
    ply = tmp_path / "m.ply"
    pp.write_ply(str(ply), v, t)
    raw = open(ply, "rb").read()
    head, body = raw.split(b"end_header\n", 1)
    assert head.startswith(b"ply\nformat binary_little_endian 1.0\n") and f"element vertex {len(v)}\n".encode() in head
    assert f"element face {len(t)}\n".encode() in head and b"property list uchar int vertex_indices" in head
    assert len(body) == 12 * len(v) + 13 * len(t)
    assert np.array_equal(np.frombuffer(body[:12 * len(v)], "<f4").reshape(-1, 3).view(np.int32), v.view(np.int32))
    faces = np.frombuffer(body[12 * len(v):], dtype=[("n", "u1"), ("i", "<i4", (3,))])
    assert (faces["n"] == 3).all() and np.array_equal(faces["i"], t)
    with pytest.raises(FileExistsError):
        pp.write_ply(str(ply), v, t)
    with pytest.raises(ValueError, match="int faces"):
        pp.write_ply(str(tmp_path / "big.ply"), v, t + 2**31)
    assert sorted(os.listdir(tmp_path)) == ["m.obj", "m.ply"]      # the refused file left nothing


# ---- the driver on the host --------------------------------------------------------------------------------------------------------------
def _store(tmp_path, name, values, array="sheet_filtered"):
    from mt3d_amd.dataloading import zarr_lite
    store = tmp_path / name
    os.makedirs(store)
    zarr_lite.write_array(str(store / array), values, (8, 16, 16), compressor="zlib")
    return str(store)


@pytest.mark.parametrize("fmt", ["obj", "ply"])
def test_surface_mesher_is_the_same_at_every_slab_depth(tmp_path, fmt):
    pp = _pp()
    values = C.ball((20, 24, 40))
    values[3:9, 2:5, 30:39] = np.random.default_rng(2).integers(0, 256, (6, 3, 9))      # noise that crosses slab borders
    want = pp.surface_nets_numpy(values, 127)
    files = []
    for slab, slabs in ((2, 11), (3, 7), (7, 3), (None, 1)):
        store = _store(tmp_path, f"{fmt}{slab}", values)
        m = pp.SurfaceMesher(127, fmt, slab=slab, mesher=pp.surface_nets_numpy)
        assert m.run(store, "sheet") == dict(level=127, vertices=len(want[0]), triangles=len(want[1]), slabs=slabs), slab
        assert m.last_slab == (slab or 21) and sorted(os.listdir(store)) == ["sheet_filtered", f"sheet_filtered.{fmt}"]
        files.append(open(os.path.join(store, f"sheet_filtered.{fmt}"), "rb").read())
    assert all(f == files[0] for f in files)
    if fmt == "obj":
        from mt3d_amd.tasks.normals.mesh_targets import read_obj
        v, t = read_obj(os.path.join(store, "sheet_filtered.obj"))
        assert np.array_equal(v.view(np.int32), want[0].view(np.int32)) and np.array_equal(t, want[1])
    else:
        reference = tmp_path / "whole.ply"
        pp.write_ply(str(reference), *want)
        assert open(reference, "rb").read() == files[0]


def test_source_path_budget_and_refusals(tmp_path):
    pp = _pp()
    from mt3d_amd.postprocess import isosurface as M
    values = C.ball((6, 8, 8))
    host = dict(mesher=pp.surface_nets_numpy)
    store = _store(tmp_path, "a", values, "sheet_final")
    with pytest.raises(ValueError, match="sheet_filtered"):      # the default source is `filtered`
        pp.SurfaceMesher(**host).run(store, "sheet")
    out = tmp_path / "elsewhere.obj"
    got = pp.SurfaceMesher(**host).run(store, "sheet", source="final", path=str(out))
    assert out.exists() and got["vertices"] == pp.counts_numpy(values, 127)[0] and sorted(os.listdir(store)) == ["sheet_final"]
    pp.SurfaceMesher(**host).run(store, "sheet", "final")
    with pytest.raises(FileExistsError, match="sheet_final.obj"):
        pp.SurfaceMesher(**host).run(store, "sheet", "final")
    with pytest.raises(ValueError, match="source"):
        pp.SurfaceMesher(**host).run(store, "sheet", "raw")
    from mt3d_amd.dataloading import zarr_lite
    zarr_lite.write_array(os.path.join(store, "normals_final"), np.zeros((3, 4, 8, 8), np.uint8), (3, 4, 8, 8))
    zarr_lite.write_array(os.path.join(store, "wide_final"), np.zeros((4, 8, 8), np.uint16), (4, 8, 8))
    for task in ("normals", "wide", "ink"):
        with pytest.raises(ValueError, match=task):
            pp.SurfaceMesher(**host).run(store, task, "final")
    # the budget: 1 byte per loaded voxel + 8 bytes per 64 cells of a cell row + 24 bytes per cell row
    assert M.BYTES_PER_VOXEL == 1 and M.BYTES_PER_CELL_ROW == 24
    assert M.scratch_bytes(6, 8, 8) == 7 * 9 * (8 + 24) and M.scratch_bytes(2, 3, 257) == 3 * 4 * (8 * 5 + 24)
    whole, four = 6 * 64 + 7 * 9 * 32, 4 * 64 + 5 * 9 * 32
    assert pp.SurfaceMesher.slab_bytes(6, 8, 8) == whole and pp.SurfaceMesher.slab_bytes(4, 8, 8) == four
    assert pp.SurfaceMesher(max_device_bytes=whole, **host).slab_depth((6, 8, 8)) == 7          # resident
    assert pp.SurfaceMesher(max_device_bytes=whole - 1, **host).slab_depth((6, 8, 8)) == 3      # 5 voxel planes: 5 * 64 + 6 * 9 * 32 fit
    assert pp.SurfaceMesher(max_device_bytes=four, **host).slab_depth((6, 8, 8)) == 2
    with pytest.raises(MemoryError, match=rf"two cell planes of a 8 x 8 volume load four voxel planes and need {four} bytes"):
        pp.SurfaceMesher(max_device_bytes=four - 1, **host).slab_depth((6, 8, 8))
    m = pp.SurfaceMesher(max_device_bytes=four, **host)
    s = _store(tmp_path, "b", values)
    assert m.run(s, "sheet")["slabs"] == 4 and m.last_slab == 2
    for kw, key in ((dict(level=255), "level"), (dict(level=-1), "level"), (dict(fmt="stl"), "format"), (dict(max_device_bytes=0), "max_device_gb"),
                    (dict(slab=0), "slab")):
        with pytest.raises(ValueError, match=key):
            pp.SurfaceMesher(**kw)


def test_a_slab_never_exceeds_what_one_pass_takes():
    pp = _pp()
    host = dict(mesher=pp.surface_nets_numpy)
    M = pp.SurfaceMesher
    # 2^31 - 2 cells: a (2^14 - 1)^2 plane has 2^28 cells per cell plane, so 7 cell planes, 6 voxel planes
    plane = ((1 << 14) - 1, (1 << 14) - 1)
    assert M.most_planes(*plane) == 6
    assert M(**host).slab_depth((10,) + plane) == 4 and M(max_device_bytes=1 << 50).slab_depth((10,) + plane) == 4
    assert M(slab=4, **host).slab_depth((10,) + plane) == 4
    with pytest.raises(ValueError, match="slab 5: 7 planes.*at most 6 planes"):
        M(slab=5, **host).slab_depth((10,) + plane)
    # 2^24 - 1 bands: y = 30000, x = 1 has 3751 bands per 4 cell planes, so 4472 * 4 cell planes
    assert M.most_planes(30000, 1) == 4472 * 4 - 1
    assert M(**host).slab_depth((30000, 30000, 1)) == 4472 * 4 - 3 and M(**host).slab_depth((4472 * 4 - 1, 30000, 1)) == 4472 * 4
    with pytest.raises(ValueError, match="four planes of a 65535 x 65535 volume"):
        M(**host).slab_depth((8, 65535, 65535))


def test_a_mesher_gets_z_base(tmp_path):
    """the documented contract of `mesher`: called as mesher(values, level, z_base=first voxel plane of the slab)"""
    pp = _pp()
    store = _store(tmp_path, "z", C.ball((12, 8, 8)))
    seen = []

    def mesher(values, level, z_base=0):
        seen.append((values.shape[0], level, z_base))
        return pp.surface_nets_numpy(values, level, z_base=z_base)
    pp.SurfaceMesher(slab=5, mesher=mesher).run(store, "sheet")
    assert seen == [(5, 127, 0), (7, 127, 3), (4, 127, 8)]      # cell planes [0, 5), [5, 10), [10, 13): two voxel planes before each


def test_a_failed_run_leaves_no_partial_file(tmp_path):
    pp = _pp()
    values = C.ball((20, 24, 40))
    store = _store(tmp_path, "s", values)
    calls = []

    def failing(v, level, z_base=0):
        calls.append(1)
        if len(calls) == 3:
            raise RuntimeError("mesher gave up")
        return pp.surface_nets_numpy(v, level, z_base=z_base)
    with pytest.raises(RuntimeError, match="gave up"):
        pp.SurfaceMesher(slab=5, mesher=failing).run(store, "sheet")
    assert sorted(os.listdir(store)) == ["sheet_filtered"]
    pp.SurfaceMesher(slab=5, mesher=pp.surface_nets_numpy).run(store, "sheet")      # the rerun is not blocked
    assert sorted(os.listdir(store)) == ["sheet_filtered", "sheet_filtered.obj"]


# ---- config ----------------------------------------------------------------------------------------------------------------------------------
TARGETS = {"sheet": {"channels": 1, "activation": "sigmoid"}, "normals": {"channels": 3}}
COMPONENTS = {"tasks": ["sheet"], "min_voxels": 20000}


def test_parse_config():
    pp = _pp()
    only_components = pp.parse_config({"components": COMPONENTS}, TARGETS)
    assert set(only_components) == {"components"}
    both = pp.parse_config({"components": COMPONENTS, "mesh": {"tasks": ["sheet"]}}, TARGETS, (16, 16, 16))
    assert both["components"] == only_components["components"]      # exactly as it was
    assert both["mesh"] == dict(tasks=("sheet",), source="filtered", level=127, format="obj", max_device_gb=None)
    full = {"tasks": "sheet", "source": "final", "level": 100, "format": "ply", "max_device_gb": 8}
    only_mesh = pp.parse_config({"mesh": full}, TARGETS)      # no longer None
    assert only_mesh == {"mesh": dict(tasks=("sheet",), source="final", level=100, format="ply", max_device_gb=8.0)}
    ok = {"tasks": ["sheet"], "source": "final"}
    bad = [({"mesh": {**ok, "colour": 1}}, "mesh.colour"), ({"mesh": {**ok, "tasks": ["ink"]}}, "mesh.tasks.*ink"),
           ({"mesh": {**ok, "tasks": ["normals"]}}, "mesh.tasks.*normals"), ({"mesh": {"tasks": ["sheet"]}}, "mesh.source"),
           ({"mesh": {"tasks": ["sheet"], "source": "filtered"}, "components": {**COMPONENTS, "tasks": ["sheet"]}, "holes": {}}, "holes"),
           ({"mesh": {**ok, "level": 255}}, "mesh.level"), ({"mesh": {**ok, "level": -1}}, "mesh.level"), ({"mesh": {**ok, "level": 1.5}}, "mesh.level"),
           ({"mesh": {**ok, "format": "stl"}}, "mesh.format"), ({"mesh": {**ok, "max_device_gb": 0}}, "mesh.max_device_gb"),
           ({"mesh": {**ok, "max_device_gb": -2}}, "mesh.max_device_gb"), ({"mesh": {**ok, "source": "raw"}}, "mesh.source"),
           ({"mesh": {"source": "final"}}, "mesh.tasks"), ({"mesh": ["sheet"]}, "mesh: expected a mapping")]
    for block, key in bad:
        with pytest.raises(ValueError, match=f"inference_config.postprocess.*{key}"):
            pp.parse_config(block, TARGETS)
    two = {**TARGETS, "ink": {"channels": 1}}
    with pytest.raises(ValueError, match="mesh.source.*'ink'"):      # filtered, but the components block filters another task
        pp.parse_config({"components": COMPONENTS, "mesh": {"tasks": ["ink"]}}, two)
    with pytest.raises(ValueError, match="mesh.*patch_size"):
        pp.parse_config({"mesh": ok}, TARGETS, (64, 64))


def test_config_manager_key(tmp_path):
    import yaml
    import mt3d_amd  # noqa: F401
    from mt3d_amd.configuration.config_manager import ConfigManager

    def cfg(ic):
        p = tmp_path / "cfg.yaml"
        p.write_text(yaml.safe_dump({"tr_setup": {}, "tr_config": {"patch_size": [16, 16, 16]}, "model_config": {},
                                     "dataset_config": {"targets": {"sheet": {"channels": 1, "activation": "sigmoid"}}},
                                     "inference_config": ic}))
        return str(p)
    m = ConfigManager(cfg({"postprocess": {"components": {"tasks": ["sheet"], "min_voxels": 7},
                                           "mesh": {"tasks": ["sheet"], "source": "filtered", "level": 127, "format": "obj", "max_device_gb": 8}}}),
                      verbose=False)
    assert m.infer_postprocess["mesh"] == dict(tasks=("sheet",), source="filtered", level=127, format="obj", max_device_gb=8.0)
    assert m.infer_postprocess["components"]["min_voxels"] == 7
    assert ConfigManager(cfg({"postprocess": {"mesh": {"tasks": ["sheet"], "source": "final"}}}), verbose=False).infer_postprocess["mesh"]["source"] == "final"
    with pytest.raises(ValueError, match="inference_config.postprocess.mesh.format"):
        ConfigManager(cfg({"postprocess": {"mesh": {"tasks": ["sheet"], "source": "final", "format": "stl"}}}), verbose=False)


def test_command_line(tmp_path, capsys):
    import json
    import runpy
    pp = _pp()
    from mt3d_amd.tasks.normals.mesh_targets import read_obj
    values = C.ball((20, 24, 40))
    store = _store(tmp_path, "cli", values, "sheet_final")
    tool = runpy.run_path(os.path.join(ROOT, "scripts", "volume_to_mesh.py"))
    got = tool["main"](["--store", store, "--task", "sheet", "--source", "final", "--slab", "7", "--where", "host"])
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1]) == got and got["slabs"] == 3
    v, t = read_obj(os.path.join(store, "sheet_final.obj"))
    want = pp.surface_nets_numpy(values, 127)
    assert np.array_equal(v.view(np.int32), want[0].view(np.int32)) and np.array_equal(t, want[1])


# ---- the kernels' own arithmetic on the CPU, under the sanitizers -----------------------------------------------------------------------------
def test_host_check_program(tmp_path):
    """csrc/rx_isosurface_core.h is what the kernels call.  A stand-alone C++ program runs classify, scan and emit serially over this
    file's shapes, levels and kinds of volume, in three row orders, against a direct restatement of its own, compiled with
    -fsanitize=address,undefined."""
    csrc = os.path.join(ROOT, "multi-task-3d-resencoder-unet_amd", "csrc")
    exe = str(tmp_path / "isosurface_host_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-Wno-unknown-pragmas", os.path.join(csrc, "tools", "isosurface_host_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    n = len(C.SHAPES) * len(C.LEVELS) * len(C.volumes((2, 2, 2), 127)) * 3
    assert r.returncode == 0 and f"{n} cases, 0 differ from the direct restatement" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
