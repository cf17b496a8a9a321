"""CPU: the statements of the mesh refinement (postprocess/refine.py) over the shared case list -- the adjacency against plain Python
sets and under shuffles, exact results on the flat grid patch, the clamp, outward normals and Taubin's volume property on a
surface-nets ball -- the files with normals, the `MeshRefiner` driver on the host, the config block, and the kernels' own per-vertex
work (csrc/rx_meshrefine_core.h) run serially under the address and undefined-behaviour sanitizers."""
import os
import subprocess

import numpy as np
import pytest

import mesh_refine_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _pp():
    import mt3d_amd  # noqa: F401
    import mt3d_amd.postprocess as pp
    return pp


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def test_adjacency_equals_a_set_construction_and_ignores_the_triangle_order():
    pp = _pp()
    plain = {}
    for name, v, t in C.cases():
        off, nbr, bnd = pp.adjacency_numpy(len(v), t)
        assert off.dtype == np.int64 and nbr.dtype == np.int64 and bnd.dtype == np.uint8 and off.shape == (len(v) + 1,) and bnd.shape == (len(v),), name
        sets, boundary = C.adjacency_sets(len(v), t)
        for i in range(len(v)):
            assert nbr[off[i]:off[i + 1]].tolist() == sorted(sets[i]), (name, i)
        assert np.array_equal(bnd, boundary), name
        base = name.replace("-shuffled", "")
        if base in plain:      # the shuffled twin
            assert all(np.array_equal(a, b) for a, b in zip(plain[base], (off, nbr, bnd))), name
        plain[base] = (off, nbr, bnd)
    off, nbr, bnd = pp.adjacency_numpy(13, C.awkward()[1])
    assert off[4] - off[3] == 0 and off[5] - off[4] == 0 and not bnd[3] and not bnd[4]      # isolated; only in a degenerate triangle
    assert nbr[off[5]:off[6]].tolist() == [6] and not bnd[5]      # (5, 5, 6) uses its edge twice
    assert bnd[7] and bnd[8] and nbr[off[7]:off[8]].tolist() == [8, 9, 10, 11]      # three on (7, 8): not boundary there, but (7, 9) is
    assert nbr[off[12]:off[13]].tolist() == [0, 9] and bnd[12]
    for bad in (np.array([[0, 1, 13]]), np.array([[0, -1, 2]])):
        with pytest.raises(ValueError, match="triangles"):
            pp.adjacency_numpy(13, bad)


def test_grid_patch_is_exact():
    """interior vertices of the flat patch sit at the mean of their six neighbours, and every sum and mean there is exact: with the
    border pinned they keep their bits after any number of passes; the normals are exactly (0, 0, 1), or (0, 0, -1) turned over"""
    pp = _pp()
    v, t = C.grid_patch()
    inner = C.grid_interior()
    _, _, bnd = pp.adjacency_numpy(len(v), t)
    assert np.array_equal(bnd.astype(bool), ~inner)
    for iterations in (1, 2, 7):
        for mu in (-0.53, None):
            q = pp.smooth_numpy(v, t, iterations, mu=mu)
            assert np.array_equal(_bits(q), _bits(v)), (iterations, mu)
    free = pp.smooth_numpy(v, t, 3, pin_boundary=False)
    assert not np.array_equal(free[~inner], v[~inner]) and np.array_equal(_bits(free[:, 2]), _bits(v[:, 2]))      # the border moves, in the plane
    n = pp.vertex_normals_numpy(v, t)
    assert np.array_equal(_bits(n), _bits(np.tile(np.float32([0, 0, 1]), (len(v), 1))))
    assert np.array_equal(_bits(pp.vertex_normals_numpy(v, t[:, ::-1])), _bits(np.tile(np.float32([0, 0, -1]), (len(v), 1))))


def test_clamp_holds_exactly_and_zero_iterations_return_the_input():
    """max |q - p0| <= clamp for every vertex and component, with no tolerance.  The statement rounds the two bounds p0 - c and p0 + c
    once, so on arbitrary positions the property that can hold exactly is lo <= q <= hi against those float32 bounds (|hi - p0| itself
    may exceed c by half an ulp of hi: 90.09 + 1 is not a float32); where p0 -+ c are float32 numbers -- the grid patch with c = 0.25
    -- it is checked literally, in float64."""
    pp = _pp()
    gv, gt = C.grid_patch()
    gq = pp.smooth_numpy(gv, gt, 6, clamp=0.25, pin_boundary=False)
    moved = np.abs(gq.astype(np.float64) - gv.astype(np.float64))
    assert moved.max() == 0.25 and np.abs(pp.smooth_numpy(gv, gt, 6, pin_boundary=False) - gv).max() > 0.25      # it binds, and holds
    for name, v, t in C.cases():
        if not name.startswith(("ball", "9x10x12-random50", "soup65", "fan300", "awkward")):
            continue
        assert np.array_equal(_bits(pp.smooth_numpy(v, t, 0)), _bits(v)), name
        for clamp in (0.0, 0.25, 1.0):
            q = pp.smooth_numpy(v, t, 4, clamp=clamp, pin_boundary=False)
            lo, hi = v - np.float32(clamp), v + np.float32(clamp)
            assert ((q >= lo) & (q <= hi)).all(), (name, clamp)
            if clamp == 0.0:
                assert np.array_equal(_bits(q), _bits(v)), name
        if name.startswith("soup"):      # positions up to 100 apart: the clamp binds
            free, held = pp.smooth_numpy(v, t, 4, pin_boundary=False), pp.smooth_numpy(v, t, 4, clamp=1.0, pin_boundary=False)
            at_bound = (held == v - np.float32(1)) | (held == v + np.float32(1))
            assert np.abs(free - v).max() > 1 and at_bound.any() and np.abs(held.astype(np.float64) - v).max() <= 1 + 2.0**-18      # half an ulp of 128


def test_ball_normals_point_outwards_and_taubin_keeps_the_volume():
    pp = _pp()
    v, t = C.ball_mesh()
    centre = np.array(C.BALL["centre"])[::-1]      # (x, y, z)
    for q in (v, pp.smooth_numpy(v, t, 10)):
        n = pp.vertex_normals_numpy(q, t)
        assert (np.einsum("ij,ij->i", n.astype(np.float64), q - centre) > 0).all()
        assert np.allclose(np.linalg.norm(n.astype(np.float64), axis=1), 1, atol=1e-6)
    vol = C.enclosed_volume(v, t)
    taubin, laplace = (C.enclosed_volume(pp.smooth_numpy(v, t, 10, mu=mu), t) for mu in (-0.53, None))
    print("volume", vol, "taubin", taubin, "laplacian", laplace)
    assert 0 < laplace < taubin and vol - laplace > vol - taubin      # the plain Laplacian shrinks strictly more
    got_v, got_n = pp.refine_numpy(v, t)
    want_v = pp.smooth_numpy(v, t, 10, clamp=1.0)
    assert np.array_equal(_bits(got_v), _bits(want_v)) and np.array_equal(_bits(got_n), _bits(pp.vertex_normals_numpy(want_v, t)))


def test_statement_refusals():
    pp = _pp()
    v, t = C.grid_patch()
    nan = v.copy()
    nan[3, 1] = np.nan
    for call, word in ((lambda: pp.smooth_numpy(nan, t, 1), "NaN"), (lambda: pp.vertex_normals_numpy(nan, t), "NaN"),
                       (lambda: pp.smooth_numpy(v, t, -1), "iterations"), (lambda: pp.smooth_numpy(v, t, 1.5), "iterations"),
                       (lambda: pp.smooth_numpy(v, t, 1, lam=float("inf")), "lam"), (lambda: pp.smooth_numpy(v, t, 1, mu=float("nan")), "mu"),
                       (lambda: pp.smooth_numpy(v, t, 1, clamp=-0.5), "clamp"), (lambda: pp.smooth_numpy(v, t + 100, 1), "triangles"),
                       (lambda: pp.smooth_numpy(v[:, :2], t, 1), "vertices")):
        with pytest.raises(ValueError, match=word):
            call()


# ---- files and the driver on the host -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["obj", "ply"])
def test_files_round_trip_to_the_same_bits(tmp_path, fmt):
    pp = _pp()
    v, t = C.ball_mesh()
    q, n = pp.refine_numpy(v, t, iterations=3)
    path = tmp_path / f"m.{fmt}"
    pp.write_refined(str(path), fmt, q, t, n)
    rv, rt, rn = pp.read_mesh(str(path))
    assert np.array_equal(_bits(rv), _bits(q)) and np.array_equal(rt, t) and rt.dtype == np.int64 and np.array_equal(_bits(rn), _bits(n))
    with pytest.raises(FileExistsError):
        pp.write_refined(str(path), fmt, q, t, n)
    plain = tmp_path / f"plain.{fmt}"
    (pp.write_obj if fmt == "obj" else pp.write_ply)(str(plain), v, t)      # what the mesher writes
    pv, pt, pn = pp.read_mesh(str(plain))
    assert np.array_equal(_bits(pv), _bits(v)) and np.array_equal(pt, t) and pn is None
    again = tmp_path / f"again.{fmt}"
    pp.write_refined(str(again), fmt, v, t, None)
    assert open(again, "rb").read() == open(plain, "rb").read()
    assert sorted(os.listdir(tmp_path)) == sorted([f"m.{fmt}", f"plain.{fmt}", f"again.{fmt}"])
    if fmt == "obj":
        text = open(path).read().splitlines()
        assert text[0].startswith("v ") and text[len(q)].startswith("vn ") and text[2 * len(q)] == "f %d//%d %d//%d %d//%d" % tuple(np.repeat(t[0] + 1, 2))
    else:
        head = open(path, "rb").read().split(b"end_header\n")[0]
        assert b"property float nz\nelement face" in head and os.path.getsize(path) == len(head) + 11 + 24 * len(q) + 13 * len(t)
    (tmp_path / "bad.ply").write_bytes(b"ply\nformat ascii 1.0\nend_header\n")
    with pytest.raises(ValueError, match="binary little-endian"):
        pp.read_ply(str(tmp_path / "bad.ply"))
    with pytest.raises(ValueError, match="obj or a .ply"):
        pp.read_mesh(str(tmp_path / "m.stl"))


def test_mesh_refiner_on_the_host(tmp_path):
    pp = _pp()
    v, t = C.ball_mesh()
    src = tmp_path / "sheet_filtered.obj"
    pp.write_obj(str(src), v, t)
    r = pp.MeshRefiner(iterations=4, refiner=pp.refine_numpy)
    summary = r.run(str(src))
    want_v, want_n = pp.refine_numpy(v, t, iterations=4)
    assert summary == dict(vertices=len(v), triangles=len(t), boundary_vertices=0, iterations=4,
                           max_displacement=float(np.abs(want_v - v).max()))
    assert 0 < summary["max_displacement"] <= 1.0
    rv, rt, rn = pp.read_mesh(str(tmp_path / "sheet_filtered_refined.obj"))
    assert np.array_equal(_bits(rv), _bits(want_v)) and np.array_equal(rt, t) and np.array_equal(_bits(rn), _bits(want_n))
    with pytest.raises(FileExistsError, match="sheet_filtered_refined.obj"):
        r.run(str(src))
    assert sorted(os.listdir(tmp_path)) == ["sheet_filtered.obj", "sheet_filtered_refined.obj"]
    out = tmp_path / "elsewhere.ply"
    pp.MeshRefiner(iterations=4, fmt="ply", normals=False, refiner=pp.refine_numpy).run(str(src), out=str(out))
    ov, ot, on = pp.read_mesh(str(out))
    assert np.array_equal(_bits(ov), _bits(want_v)) and np.array_equal(ot, t) and on is None
    gv, gt = C.grid_patch()
    grid = tmp_path / "grid.ply"
    pp.write_ply(str(grid), gv, gt)
    assert pp.MeshRefiner(refiner=pp.refine_numpy).run(str(grid))["boundary_vertices"] == int((~C.grid_interior()).sum())
    assert (tmp_path / "grid_refined.ply").exists()
    # the documented device bytes, and the refusal that names them (no device is touched: the budget is checked first)
    from mt3d_amd.postprocess import refine as R
    assert R.BYTES_PER_VERTEX == 77 and R.BYTES_PER_TRIANGLE == 96 and pp.MeshRefiner.scratch_bytes(10, 20) == 770 + 1920 + 24
    need = pp.MeshRefiner.scratch_bytes(len(v), len(t))
    with pytest.raises(MemoryError, match=f"needs {need} bytes"):
        pp.MeshRefiner(max_device_bytes=need - 1).run(str(src), out=str(tmp_path / "never.obj"))
    assert not (tmp_path / "never.obj").exists()
    for kw, word in ((dict(iterations=-1), "iterations"), (dict(lam=float("nan")), "lam"), (dict(clamp=-1), "clamp"), (dict(fmt="stl"), "fmt"),
                     (dict(max_device_bytes=0), "max_device_bytes")):
        with pytest.raises(ValueError, match=word):
            pp.MeshRefiner(**kw)


def test_command_line_on_the_host(tmp_path, capsys):
    import json
    import runpy
    pp = _pp()
    v, t = C.ball_mesh()
    src = tmp_path / "m.ply"
    pp.write_ply(str(src), v, t)
    tool = runpy.run_path(os.path.join(ROOT, "scripts", "refine_mesh.py"))
    got = tool["main"](["--mesh", str(src), "--iterations", "3", "--lambda", "0.4", "--mu", "-0.43", "--clamp", "0.5", "--no-pin-boundary",
                        "--where", "host"])
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1]) == got and got["iterations"] == 3
    want_v, want_n = pp.refine_numpy(v, t, iterations=3, lam=0.4, mu=-0.43, clamp=0.5, pin_boundary=False)
    rv, _, rn = pp.read_mesh(str(tmp_path / "m_refined.ply"))
    assert np.array_equal(_bits(rv), _bits(want_v)) and np.array_equal(_bits(rn), _bits(want_n))
    tool["main"](["--mesh", str(src), "--no-normals", "--out", str(tmp_path / "o.ply"), "--where", "host"])
    assert pp.read_mesh(str(tmp_path / "o.ply"))[2] is None


# ---- config -------------------------------------------------------------------------------------------------------------------------------------
TARGETS = {"sheet": {"channels": 1, "activation": "sigmoid"}, "ink": {"channels": 1}, "normals": {"channels": 3}}
COMPONENTS = {"tasks": ["sheet"], "min_voxels": 20000}
MESH = {"tasks": ["sheet"], "source": "filtered"}


def test_parse_config():
    pp = _pp()
    before = pp.parse_config({"components": COMPONENTS, "mesh": MESH}, TARGETS, (16, 16, 16))
    full = {"tasks": ["sheet"], "iterations": 10, "lambda": 0.5, "mu": -0.53, "clamp": 1.0, "pin_boundary": True, "normals": True, "max_device_gb": 8}
    got = pp.parse_config({"components": COMPONENTS, "mesh": MESH, "refine": full}, TARGETS, (16, 16, 16))
    assert got["components"] == before["components"] and got["mesh"] == before["mesh"] and set(before) == {"components", "mesh"}
    assert got["mesh"] == dict(tasks=("sheet",), source="filtered", level=127, format="obj", max_device_gb=None)      # exactly as it was
    assert got["refine"] == dict(tasks=("sheet",), iterations=10, lam=0.5, mu=-0.53, clamp=1.0, pin_boundary=True, normals=True, max_device_gb=8.0)
    short = pp.parse_config({"mesh": {"tasks": "sheet", "source": "final"}, "refine": {"tasks": "sheet", "mu": None, "clamp": None}}, TARGETS)
    assert short["refine"] == dict(tasks=("sheet",), iterations=10, lam=0.5, mu=None, clamp=None, pin_boundary=True, normals=True, max_device_gb=None)
    assert pp.parse_config({"components": COMPONENTS}, TARGETS) == {"components": before["components"]}
    assert pp.parse_config(None, TARGETS) is None
    ok = {"tasks": ["sheet"]}
    final = {"tasks": ["sheet"], "source": "final"}
    bad = [({**ok, "colour": 1}, "refine.colour"), ({**ok, "iterations": -1}, "refine.iterations"), ({**ok, "iterations": 2.5}, "refine.iterations"),
           ({**ok, "lambda": float("inf")}, "refine.lambda"), ({**ok, "lambda": None}, "refine.lambda"), ({**ok, "mu": "x"}, "refine.mu"),
           ({**ok, "clamp": -1}, "refine.clamp"), ({**ok, "pin_boundary": 1}, "refine.pin_boundary"), ({**ok, "normals": "yes"}, "refine.normals"),
           ({**ok, "max_device_gb": 0}, "refine.max_device_gb"), ({"iterations": 3}, "refine.tasks"), ({"tasks": ["ink"]}, "refine.tasks.*'ink'"),
           (["sheet"], "refine: expected a mapping")]
    for block, key in bad:
        with pytest.raises(ValueError, match=f"inference_config.postprocess.{key}"):
            pp.parse_config({"mesh": final, "refine": block}, TARGETS)
    with pytest.raises(ValueError, match="refine.tasks.*postprocess.mesh"):      # no mesh block at all
        pp.parse_config({"refine": ok}, TARGETS)


def test_config_manager_key(tmp_path):
    import yaml
    import mt3d_amd  # noqa: F401
    from mt3d_amd.configuration.config_manager import ConfigManager
    p = tmp_path / "cfg.yaml"
    p.write_text(yaml.safe_dump({"tr_setup": {}, "tr_config": {"patch_size": [16, 16, 16]}, "model_config": {},
                                 "dataset_config": {"targets": {"sheet": {"channels": 1, "activation": "sigmoid"}}},
                                 "inference_config": {"postprocess": {"mesh": {"tasks": ["sheet"], "source": "final"},
                                                                      "refine": {"tasks": ["sheet"], "iterations": 3}}}}))
    m = ConfigManager(str(p), verbose=False)
    assert m.infer_postprocess["refine"]["iterations"] == 3 and m.infer_postprocess["mesh"]["source"] == "final"


# ---- the kernels' own work on the CPU, under the sanitizers -----------------------------------------------------------------------------------
def test_host_check_program(tmp_path):
    """csrc/rx_meshrefine_core.h is what the kernels call.  A stand-alone C++ program runs count, fill, canonicalise, compact, smooth
    and normals serially over this file's kinds of mesh, with the corners filled in three orders and every mesh once more shuffled,
    against a restatement with std::set and std::map, compiled with -fsanitize=address,undefined."""
    csrc = os.path.join(ROOT, "multi-task-3d-resencoder-unet_amd", "csrc")
    exe = str(tmp_path / "meshrefine_host_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-Wno-unknown-pragmas", os.path.join(csrc, "tools", "meshrefine_host_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    n = (3 + len(C.COUNTS) + len(C.FANS) + 1) * 2 * 3      # grid, octahedron, awkward; the counts; the fans; no triangles
    assert r.returncode == 0 and f"{n} runs, 0 differ from the direct restatement" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
