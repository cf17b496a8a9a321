"""CPU: the statement of mesh decimation by vertex clustering (postprocess/decimate.py) over the shared case list -- against a plain
Python restatement, the identity under a fine cell, exact counts and normals on the integer grid, idempotence, independence of the
triangle order, a clean result, the displacement bound -- the config block, the `MeshDecimator` driver and the command line on the
host, and the kernels' own per-vertex and per-triangle work (csrc/rx_meshdecimate_core.h) run serially under the address and
undefined-behaviour sanitizers."""
import os
import subprocess

import numpy as np
import pytest

import mesh_decimate_cases as D
import mesh_refine_cases as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = float(np.finfo(np.float32).eps)      # 2^-23


def _pp():
    import mt3d_amd  # noqa: F401
    import mt3d_amd.postprocess as pp
    return pp


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _same(a, b):
    return (a[0].shape == b[0].shape and np.array_equal(_bits(a[0]), _bits(b[0])) and a[1].shape == b[1].shape and np.array_equal(a[1], b[1])
            and np.array_equal(a[2], b[2]))


def test_statement_equals_a_plain_restatement():
    pp = _pp()
    for name, v, t, cell in D.cases():
        if len(v) > 4000:
            continue
        for representative in D.REPRESENTATIVES:
            got = pp.decimate_numpy(v, t, cell, representative)
            assert got[0].dtype == np.float32 and got[1].dtype == np.int64 and got[2].dtype == np.int64 and got[2].shape == (len(v),), name
            assert _same(got, D.decimate_plain(v, t, cell, representative)), (name, representative)


def test_fine_cell_returns_the_input():
    """a cell below the smallest vertex spacing: every cluster is one vertex, so the grid comes back bit for bit with its triangles;
    on the awkward mesh the unreferenced vertices, the degenerate triangles and the repeated triangle go"""
    pp = _pp()
    for name in ("grid-fine", "big-grid-fine"):
        _, v, t, cell = D.case(name)
        for representative in D.REPRESENTATIVES:
            gv, gt, gc = pp.decimate_numpy(v, t, cell, representative)
            assert np.array_equal(_bits(gv), _bits(v)) and np.array_equal(gt, t) and np.array_equal(gc, np.arange(len(v))), (name, representative)
    _, v, t, cell = D.case("awkward-fine")
    gv, gt, gc = pp.decimate_numpy(v, t, cell)
    live = [0, 4, 5, 6, 7, 8, 9]      # (0, 1, 2) once; (4, 4, 4) and (5, 5, 6) are degenerate
    referenced = np.unique(t[live])
    assert np.array_equal(_bits(gv), _bits(v[referenced])) and np.array_equal(referenced[gt], t[live]) and np.array_equal(gc, np.arange(13))
    assert pp.cluster_rows(gc, t).tolist() == [0, 1, 2, -1, -1, -1, 3, 4, 5, 6, 7, 8, 9]


def test_integer_grid_counts_and_normals():
    pp = _pp()
    for name in ("grid-c2", "grid-neg-c2", "big-grid-c2"):
        _, v, t, cell = D.case(name)
        ny, nx = D.BIG if name.startswith("big") else R.GRID
        cy, cx = -(-ny // 2), -(-nx // 2)
        for representative in D.REPRESENTATIVES:
            gv, gt, gc = pp.decimate_numpy(v, t, cell, representative)
            assert int(gc.max()) + 1 == cy * cx and len(gv) == cy * cx and len(gt) == 2 * (cy - 1) * (cx - 1), (name, representative)
            n = pp.vertex_normals_numpy(gv, gt)
            up = np.tile(np.float32([0, 0, 1]), (len(gv), 1))
            assert np.array_equal(_bits(n), _bits(up)) or np.array_equal(_bits(n), _bits(-up)), (name, representative)
    # vertices exactly on a cell face belong to the upper cell, at negative coordinates too: floor, not truncation
    _, v, t, cell = D.case("grid-neg-c2")
    k, _ = __import__("mt3d_amd.postprocess.decimate", fromlist=["cell_keys_numpy"]).cell_keys_numpy(v, cell)
    assert np.array_equal(k, np.floor(v.astype(np.float64) / 2).astype(np.int64)) and k.min() == -3 and (k[:, 2] == -1).all()


def test_nearest_is_idempotent():
    pp = _pp()
    for name, v, t, cell in D.cases():
        once = pp.decimate_numpy(v, t, cell, "nearest")
        again = pp.decimate_numpy(once[0], once[1], cell, "nearest")
        assert np.array_equal(_bits(again[0]), _bits(once[0])) and np.array_equal(again[1], once[1]), name
        assert np.array_equal(again[2], np.arange(len(once[0]))), name


def test_mean_is_idempotent_where_every_mean_stays_in_its_cell():
    """a mean can leave its cell only by rounding (the cell is convex), and where none does, every output vertex is alone in its cell,
    so a second run is the identity.  The cases are selected by that condition, checked here on the statement's own keys."""
    pp = _pp()
    from mt3d_amd.postprocess.decimate import cell_keys_numpy
    qualify = 0
    for name, v, t, cell in D.cases():
        once = pp.decimate_numpy(v, t, cell, "mean")
        rows = pp.cluster_rows(once[2], t)[once[2]]
        inside = np.array_equal(cell_keys_numpy(once[0][rows[rows >= 0]], cell)[1], cell_keys_numpy(v[rows >= 0], cell)[1])
        if not inside:
            continue
        qualify += 1
        again = pp.decimate_numpy(once[0], once[1], cell, "mean")
        assert np.array_equal(_bits(again[0]), _bits(once[0])) and np.array_equal(again[1], once[1]), name
    print("cases whose means stay inside their cells:", qualify, "of", len(D.cases()))
    assert 2 * qualify >= len(D.cases())


def test_triangle_order_does_not_change_the_vertices():
    pp = _pp()
    for name, v, t, cell in D.cases():
        if len(v) > 4000 or not len(t):
            continue
        for representative in D.REPRESENTATIVES:
            a = pp.decimate_numpy(v, t, cell, representative)
            b = pp.decimate_numpy(*R.shuffled(v, t, seed=5), cell, representative)
            assert np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(a[2], b[2]) and D.unordered(a[1]) == D.unordered(b[1]), (name, representative)
    a, b = pp.decimate_numpy(*D.case("ball-c2")[1:]), pp.decimate_numpy(*D.case("ball-shuffled-c2")[1:])
    assert np.array_equal(_bits(a[0]), _bits(b[0])) and D.unordered(a[1]) == D.unordered(b[1]) and not np.array_equal(a[1], b[1])


def test_result_is_clean_and_keeps_the_lowest_triangle():
    pp = _pp()
    for name, v, t, cell in D.cases():
        for representative in D.REPRESENTATIVES:
            gv, gt, gc = pp.decimate_numpy(v, t, cell, representative)
            assert not ((gt[:, 0] == gt[:, 1]) | (gt[:, 1] == gt[:, 2]) | (gt[:, 0] == gt[:, 2])).any(), name      # no degenerate triangle
            assert len(np.unique(np.sort(gt, axis=1), axis=0)) == len(gt), name      # no unordered triple twice
            assert np.array_equal(np.unique(gt), np.arange(len(gv))), name      # every output vertex is referenced
            rows = pp.cluster_rows(gc, t)
            assert (rows >= 0).sum() == len(gv) and np.array_equal(rows[rows >= 0], np.arange(len(gv))), name
    # the two faces of the slab merge; the lower face comes first in the input, so its triangles and its winding stay, and the
    # normals are the lower face's (0, 0, 1) although "nearest" picks the upper face's vertices (3.25 is nearer 3.5 than 3.0 is)
    _, v, t, cell = D.case("slab-c1")
    gv, gt, _ = pp.decimate_numpy(v, t, cell, "nearest")
    assert np.array_equal(gt, t[:len(t) // 2]) and np.array_equal(_bits(gv), _bits(v[len(v) // 2:]))
    assert np.array_equal(_bits(pp.vertex_normals_numpy(gv, gt)), _bits(np.tile(np.float32([0, 0, 1]), (len(gv), 1))))
    one = pp.decimate_numpy(*D.case("grid-one-cluster")[1:])
    assert one[0].shape == (0, 3) and one[1].shape == (0, 3) and not one[2].any()
    fan = pp.decimate_numpy(*D.case("fan3000-one-cell")[1:])
    assert fan[0].shape == (0, 3) and fan[1].shape == (0, 3) and not fan[2].any()


def test_displacement_bound(tmp_path):
    """|representative - p| per component, for a cluster of n members with |p| <= M.  With u = eps / 2 = 2^-24: the members share
    floor(fl(p / cell)), so each lies within u M of the cell and two of them are at most cell + 2 u M = cell + eps M apart; the exact
    mean lies between them.  The sequential float32 sum of n terms is off by at most (n - 1) u / (1 - (n - 1) u) times the sum of the
    |p|, which is at most n M; the division by n adds a relative u; so the computed mean is off by at most about n u M = (n / 2)
    eps M, and the float32 subtraction that takes the displacement adds a relative u.  For n u < 1/2 all of it is covered by
        cell (1 + eps) + (n + 2) eps M.
    `nearest` moves a vertex onto a member of its cell: n = 1 in the same bound."""
    pp = _pp()
    for name, v, t, cell in D.cases():
        if len(v) > 4000 or not len(t):
            continue
        for representative in D.REPRESENTATIVES:
            src = tmp_path / f"{name}_{representative}.ply"
            pp.write_ply(str(src), v, t)
            summary = pp.MeshDecimator(cell, representative, decimator=pp.decimate_numpy).run(str(src))
            n = int(np.bincount(pp.decimate_numpy(v, t, cell, representative)[2]).max()) if representative == "mean" else 1
            bound = cell * (1 + EPS) + (n + 2) * EPS * float(np.abs(v).max())
            print(name, representative, "max_displacement", summary["max_displacement"], "bound", bound, "n", n)
            assert 0 <= summary["max_displacement"] <= bound, (name, representative)


def test_statement_refusals():
    pp = _pp()
    v, t = R.grid_patch()
    nan = v.copy()
    nan[3, 1] = np.nan
    for call, word in ((lambda: pp.decimate_numpy(nan, t, 1.0), "NaN"), (lambda: pp.decimate_numpy(v, t + 100, 1.0), "triangles"),
                       (lambda: pp.decimate_numpy(v[:, :2], t, 1.0), "vertices"), (lambda: pp.decimate_numpy(v, t, 0), "cell"),
                       (lambda: pp.decimate_numpy(v, t, -1.0), "cell"), (lambda: pp.decimate_numpy(v, t, float("nan")), "cell"),
                       (lambda: pp.decimate_numpy(v, t, float("inf")), "cell"), (lambda: pp.decimate_numpy(v, t, 1e39), "cell"),
                       (lambda: pp.decimate_numpy(v, t, 1e-50), "cell"), (lambda: pp.decimate_numpy(v, t, True), "cell"),
                       (lambda: pp.decimate_numpy(v, t, 2.0**-18), "cell"),      # 6 / 2^-18 = 1.5 * 2^20: a key out of range
                       (lambda: pp.decimate_numpy(v, t, 1e-44), "cell"),         # 6 / a denormal: an infinity
                       (lambda: pp.decimate_numpy(v, t, 1.0, "median"), "representative")):
        with pytest.raises(ValueError, match=word):
            call()
    assert len(pp.decimate_numpy(v, t, 2.0**-17)[0]) == len(v)      # 6 * 2^17 < 2^20: the largest key in range
    e = pp.decimate_numpy(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int64), 1.0)
    assert e[0].shape == (0, 3) and e[1].shape == (0, 3) and e[2].shape == (0,)


# ---- the driver and the command line on the host --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["obj", "ply"])
def test_mesh_decimator_on_the_host(tmp_path, fmt):
    pp = _pp()
    _, v, t, cell = D.case("ball-c2")
    src = tmp_path / f"sheet_filtered_refined.{fmt}"
    pp.write_refined(str(src), fmt, v, t, pp.vertex_normals_numpy(v, t))      # what the refiner writes: the normals in it are not used
    d = pp.MeshDecimator(cell, decimator=pp.decimate_numpy)
    summary = d.run(str(src))
    want_v, want_t, cluster_of = pp.decimate_numpy(v, t, cell)
    rows = pp.cluster_rows(cluster_of, t)[cluster_of]
    assert summary == dict(vertices=len(want_v), triangles=len(want_t), input_vertices=len(v), input_triangles=len(t), clusters=int(cluster_of.max()) + 1,
                           cell=2.0, max_displacement=float(np.abs(want_v[rows[rows >= 0]] - v[rows >= 0]).max()))
    assert 0 < summary["vertices"] < len(v) and 0 < summary["max_displacement"] < 2.0
    rv, rt, rn = pp.read_mesh(str(tmp_path / f"sheet_filtered_refined_decimated.{fmt}"))
    assert np.array_equal(_bits(rv), _bits(want_v)) and np.array_equal(rt, want_t) and np.array_equal(_bits(rn), _bits(pp.vertex_normals_numpy(want_v, want_t)))
    with pytest.raises(FileExistsError, match="_decimated"):
        d.run(str(src))
    other = "ply" if fmt == "obj" else "obj"
    out = tmp_path / f"elsewhere.{other}"
    pp.MeshDecimator(cell, "nearest", normals=False, fmt=other, decimator=pp.decimate_numpy).run(str(src), out=str(out))
    ov, ot, on = pp.read_mesh(str(out))
    near = pp.decimate_numpy(v, t, cell, "nearest")
    assert np.array_equal(_bits(ov), _bits(near[0])) and np.array_equal(ot, near[1]) and on is None
    assert sorted(os.listdir(tmp_path)) == sorted([src.name, f"sheet_filtered_refined_decimated.{fmt}", out.name])
    empty = tmp_path / f"one.{fmt}"
    gv, gt, gcell = D.case("grid-one-cluster")[1:]
    (pp.write_obj if fmt == "obj" else pp.write_ply)(str(empty), gv, gt)
    assert pp.MeshDecimator(gcell, decimator=pp.decimate_numpy).run(str(empty)) == dict(
        vertices=0, triangles=0, input_vertices=len(gv), input_triangles=len(gt), clusters=1, cell=64.0, max_displacement=0.0)
    # the documented device bytes, and the refusal that names them (no device is touched: the budget is checked first)
    from mt3d_amd.postprocess import decimate as M
    assert M.BYTES_PER_VERTEX == 156 and M.BYTES_PER_TRIANGLE == 72 and pp.MeshDecimator.scratch_bytes(10, 20) == 1560 + 1440 + 96
    need = pp.MeshDecimator.scratch_bytes(len(v), len(t))
    with pytest.raises(MemoryError, match=f"needs {need} bytes"):
        pp.MeshDecimator(cell, max_device_bytes=need - 1).run(str(src), out=str(tmp_path / "never.obj"))
    assert not (tmp_path / "never.obj").exists()
    for kw, word in ((dict(cell=0), "cell"), (dict(cell=float("nan")), "cell"), (dict(cell=1.0, representative="mode"), "representative"),
                     (dict(cell=1.0, fmt="stl"), "fmt"), (dict(cell=1.0, max_device_bytes=0), "max_device_bytes")):
        with pytest.raises(ValueError, match=word):
            pp.MeshDecimator(**kw)


def test_command_line_on_the_host(tmp_path, capsys):
    import json
    import runpy
    pp = _pp()
    _, v, t, cell = D.case("ball-c3.5")
    src = tmp_path / "m.ply"
    pp.write_ply(str(src), v, t)
    tool = runpy.run_path(os.path.join(ROOT, "scripts", "decimate_mesh.py"))
    got = tool["main"](["--mesh", str(src), "--cell", "3.5", "--representative", "nearest", "--where", "host"])
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1]) == got and got["cell"] == 3.5
    want = pp.decimate_numpy(v, t, 3.5, "nearest")
    rv, rt, rn = pp.read_mesh(str(tmp_path / "m_decimated.ply"))
    assert np.array_equal(_bits(rv), _bits(want[0])) and np.array_equal(rt, want[1]) and rn is not None
    tool["main"](["--mesh", str(src), "--cell", "3.5", "--no-normals", "--out", str(tmp_path / "o.obj"), "--where", "host"])
    ov, ot, on = pp.read_mesh(str(tmp_path / "o.obj"))
    assert on is None and np.array_equal(_bits(ov), _bits(pp.decimate_numpy(v, t, 3.5)[0]))


# ---- config -------------------------------------------------------------------------------------------------------------------------------------
TARGETS = {"sheet": {"channels": 1, "activation": "sigmoid"}, "ink": {"channels": 1}, "normals": {"channels": 3}}
COMPONENTS = {"tasks": ["sheet"], "min_voxels": 20000}
MESH = {"tasks": ["sheet"], "source": "filtered"}
REFINE = {"tasks": ["sheet"], "iterations": 3}


def test_parse_config():
    pp = _pp()
    before = pp.parse_config({"components": COMPONENTS, "mesh": MESH, "refine": REFINE}, TARGETS, (16, 16, 16))
    full = {"tasks": ["sheet"], "cell": 4, "representative": "nearest", "normals": False, "max_device_gb": 8}
    got = pp.parse_config({"components": COMPONENTS, "mesh": MESH, "refine": REFINE, "decimate": full}, TARGETS, (16, 16, 16))
    assert {k: got[k] for k in before} == before and set(before) == {"components", "mesh", "refine"}      # the siblings stay exactly as they were
    assert got["decimate"] == dict(tasks=("sheet",), cell=4.0, representative="nearest", normals=False, max_device_gb=8.0)
    short = pp.parse_config({"mesh": {"tasks": "sheet", "source": "final"}, "decimate": {"tasks": "sheet", "cell": 2.5}}, TARGETS)      # no refine block
    assert short["decimate"] == dict(tasks=("sheet",), cell=2.5, representative="mean", normals=True, max_device_gb=None) and "refine" not in short
    ok = {"tasks": ["sheet"], "cell": 2.0}
    final = {"tasks": ["sheet"], "source": "final"}
    bad = [({**ok, "colour": 1}, "decimate.colour"), ({"tasks": ["sheet"]}, "decimate.cell"), ({**ok, "cell": 0}, "decimate.cell"),
           ({**ok, "cell": -2}, "decimate.cell"), ({**ok, "cell": float("inf")}, "decimate.cell"), ({**ok, "cell": float("nan")}, "decimate.cell"),
           ({**ok, "cell": "2"}, "decimate.cell"), ({**ok, "cell": None}, "decimate.cell"), ({**ok, "cell": True}, "decimate.cell"),
           ({**ok, "representative": "median"}, "decimate.representative"), ({**ok, "representative": None}, "decimate.representative"),
           ({**ok, "normals": "yes"}, "decimate.normals"), ({**ok, "normals": 1}, "decimate.normals"), ({**ok, "max_device_gb": 0}, "decimate.max_device_gb"),
           ({"cell": 2.0}, "decimate.tasks"), ({"tasks": ["ink"], "cell": 2.0}, "decimate.tasks.*'ink'"), (["sheet"], "decimate: expected a mapping")]
    for block, key in bad:
        with pytest.raises(ValueError, match=f"inference_config.postprocess.{key}"):
            pp.parse_config({"mesh": final, "decimate": block}, TARGETS)
    with pytest.raises(ValueError, match="decimate.tasks.*postprocess.mesh"):      # no mesh block at all
        pp.parse_config({"decimate": ok}, TARGETS)
    with pytest.raises(ValueError, match=r"postprocess.simplify: unknown key \(components, mesh, refine, decimate\)"):
        pp.parse_config({"mesh": final, "simplify": ok}, TARGETS)


def test_config_manager_key(tmp_path):
    import yaml
    import mt3d_amd  # noqa: F401
    from mt3d_amd.configuration.config_manager import ConfigManager
    p = tmp_path / "cfg.yaml"
    p.write_text(yaml.safe_dump({"tr_setup": {}, "tr_config": {"patch_size": [16, 16, 16]}, "model_config": {},
                                 "dataset_config": {"targets": {"sheet": {"channels": 1, "activation": "sigmoid"}}},
                                 "inference_config": {"postprocess": {"mesh": {"tasks": ["sheet"], "source": "final"},
                                                                      "decimate": {"tasks": ["sheet"], "cell": 3}}}}))
    m = ConfigManager(str(p), verbose=False)
    assert m.infer_postprocess["decimate"] == dict(tasks=("sheet",), cell=3.0, representative="mean", normals=True, max_device_gb=None)


# ---- the kernels' own work on the CPU, under the sanitizers -----------------------------------------------------------------------------------
def test_host_check_program(tmp_path):
    """csrc/rx_meshdecimate_core.h is what the kernels call.  A stand-alone C++ program runs keys, the hash table at its smallest and at
    the default capacity, numbering, member lists, both representatives, the triangle lists and the compaction serially over this
    file's kinds of mesh, with vertices and triangles taking their turns in three orders, against a restatement with std::map and
    std::set, compiled with -fsanitize=address,undefined."""
    csrc = os.path.join(ROOT, "multi-task-3d-resencoder-unet_amd", "csrc")
    exe = str(tmp_path / "meshdecimate_host_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-Wno-unknown-pragmas", os.path.join(csrc, "tools", "meshdecimate_host_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    n = 20 * 2 * 3 * 2      # twenty meshes, both representatives, three orders, two table capacities
    assert r.returncode == 0 and f"{n} runs, 0 differ from the direct restatement" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
