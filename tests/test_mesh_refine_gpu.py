"""Mesh refinement on the device: ops.mesh_adjacency / ops.mesh_smooth / ops.mesh_vertex_normals (csrc/rx_meshrefine.hip) against the
numpy statements of postprocess/refine.py over the shared case list, `MeshRefiner` on the device against the host run, and the refined
mesh at the end of streaming inference.  Everything compares with array_equal, floats by their bits."""
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import mesh_refine_cases as C

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _mods():
    import mt3d_amd  # noqa: F401
    import mt3d_amd.postprocess as pp
    from mt3d_amd.engine import lib as L
    from mt3d_amd.engine import ops
    L.require_device()
    return L, ops, pp


def _bits(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else a
    return np.ascontiguousarray(a, np.float32).view(np.int32)


_WANT = {}


def _statement(pp):
    """the statements over the case list, computed once: adjacency, corner faces, normals"""
    if not _WANT:
        from mt3d_amd.postprocess.refine import corner_faces_numpy
        for name, v, t in C.cases():
            _WANT[name] = (pp.adjacency_numpy(len(v), t), corner_faces_numpy(len(v), t), pp.vertex_normals_numpy(v, t))
    return _WANT


def test_adjacency_and_normals_every_case_twice():
    _, ops, pp = _mods()
    want = _statement(pp)
    got = []
    for name, v, t in C.cases():
        dv, dt = torch.from_numpy(v).cuda(), torch.from_numpy(t).cuda()
        a, b = ops.mesh_adjacency(len(v), dt), ops.mesh_adjacency(len(v), dt)
        got.append((a, b, ops.mesh_vertex_normals(dv, dt, adjacency=a), ops.mesh_vertex_normals(dv, dt)))
    torch.cuda.synchronize()
    for (name, v, t), (a, b, n, n2) in zip(C.cases(), got):
        (off, nbr, bnd), (foff, faces), normals = want[name]
        assert a.offsets.dtype == torch.int64 and a.neighbours.dtype == torch.int32 and a.boundary.dtype == torch.uint8, name
        for x, w in zip(a, (off, nbr, bnd, foff, faces)):
            assert tuple(x.shape) == w.shape and np.array_equal(x.cpu().numpy(), w), name
        assert all(torch.equal(x, y) for x, y in zip(a, b)), name      # twice: the same bytes
        assert n.dtype == torch.float32 and np.array_equal(_bits(n), _bits(normals)) and torch.equal(n.view(torch.int32), n2.view(torch.int32)), name


@pytest.mark.parametrize("iterations", [1, 5])
def test_smooth_every_case_and_option(iterations):
    _, ops, pp = _mods()
    want = _statement(pp)
    for name, v, t in C.cases():
        dv, dt = torch.from_numpy(v).cuda(), torch.from_numpy(t).cuda()
        adj = ops.mesh_adjacency(len(v), dt)
        for clamp, mu, pin in itertools.product((None, 1.0), (-0.53, None), (True, False)):
            got = ops.mesh_smooth(dv, dt, iterations, 0.5, mu, clamp, pin, adjacency=adj)
            ref = pp.smooth_numpy(v, t, iterations, 0.5, mu, clamp, pin, adjacency=want[name][0])
            assert got.dtype == torch.float32 and got.data_ptr() != dv.data_ptr(), name
            assert np.array_equal(_bits(got), _bits(ref)), (name, clamp, mu, pin)
        again = ops.mesh_smooth(dv, dt, iterations, clamp=1.0)      # builds its own adjacency; the same bytes
        assert np.array_equal(_bits(again), _bits(pp.smooth_numpy(v, t, iterations, clamp=1.0, adjacency=want[name][0]))), name
        assert np.array_equal(_bits(dv), _bits(v)), name      # the input is left alone


def test_empty_meshes_and_zero_iterations():
    _, ops, pp = _mods()
    v, t = C.grid_patch()
    dv, dt = torch.from_numpy(v).cuda(), torch.from_numpy(t).cuda()
    none = torch.zeros((0, 3), dtype=torch.int64, device="cuda")
    a = ops.mesh_adjacency(len(v), none)
    assert a.offsets.tolist() == [0] * (len(v) + 1) and a.neighbours.numel() == 0 and a.boundary.tolist() == [0] * len(v) and a.faces.numel() == 0
    assert np.array_equal(_bits(ops.mesh_smooth(dv, none, 3)), _bits(v)) and not ops.mesh_vertex_normals(dv, none).any()
    got = ops.mesh_smooth(dv, dt, 0)
    assert np.array_equal(_bits(got), _bits(v)) and got.data_ptr() != dv.data_ptr()
    e = torch.zeros((0, 3), device="cuda")
    assert ops.mesh_adjacency(0, none).offsets.tolist() == [0] and ops.mesh_smooth(e, none, 2).shape == (0, 3) and ops.mesh_vertex_normals(e, none).shape == (0, 3)


def test_nothing_is_written_beyond_a_capacity():
    """the C entry points with outputs longer than the stated capacity, filled with a marker: the part beyond it keeps the marker"""
    L, ops, pp = _mods()
    from mt3d_amd.engine.ops.core import _ptr
    so, st = L.load(), L.stream_ptr
    v, t = C.ball_mesh()
    V, T = len(v), len(t)
    dt = torch.from_numpy(t).cuda()
    a = ops.mesh_adjacency(V, dt)
    E, M = a.neighbours.numel(), -77
    i32 = lambda n: torch.full((n,), M, dtype=torch.int32, device="cuda")      # noqa: E731
    counts, flag, foff = i32(V + 8), torch.zeros(1, dtype=torch.int32, device="cuda"), torch.full((V + 9,), M, dtype=torch.int64, device="cuda")
    L.check(so.rx_mesh_count(_ptr(dt), T, V, _ptr(counts), _ptr(flag), st()), "count")
    L.check(so.rx_mesh_scan(_ptr(counts), V, _ptr(foff), st()), "scan")
    assert (counts[V:] == M).all() and (foff[V + 1:] == M).all() and torch.equal(foff[:V + 1], a.face_offsets) and flag.item() == 0
    half = 3 * T // 2      # a capacity below what the mesh needs: the slots from `half` on are never stored
    cursor, faces, raw = i32(V + 8), i32(3 * T), i32(6 * T)
    L.check(so.rx_mesh_fill(_ptr(dt), T, V, _ptr(foff), _ptr(cursor), half, _ptr(faces), _ptr(raw), st()), "fill")
    assert (cursor[V:] == M).all() and (faces[half:] == M).all() and (raw[2 * half:] == M).all() and (faces[:half] != M).all()
    cursor, faces, raw = i32(V + 8), i32(3 * T + 8), i32(6 * T + 8)
    L.check(so.rx_mesh_fill(_ptr(dt), T, V, _ptr(foff), _ptr(cursor), 3 * T, _ptr(faces), _ptr(raw), st()), "fill")
    deg, bnd = i32(V + 8), torch.full((V + 8,), 9, dtype=torch.uint8, device="cuda")
    L.check(so.rx_mesh_canonical(V, _ptr(foff), 3 * T, _ptr(faces), _ptr(raw), _ptr(deg), _ptr(bnd), st()), "canonical")
    assert (faces[3 * T:] == M).all() and (raw[6 * T:] == M).all() and (deg[V:] == M).all() and (bnd[V:] == 9).all()
    assert torch.equal(faces[:3 * T], a.faces) and torch.equal(bnd[:V], a.boundary)
    nbr = i32(E + 8)
    L.check(so.rx_mesh_compact(V, _ptr(foff), _ptr(raw), 3 * T, _ptr(a.offsets), E, _ptr(nbr), st()), "compact")
    assert (nbr[E:] == M).all() and torch.equal(nbr[:E], a.neighbours)
    short = i32(E)
    L.check(so.rx_mesh_compact(V, _ptr(foff), _ptr(raw), 3 * T, _ptr(a.offsets), E // 2, _ptr(short), st()), "compact")
    assert (short[E // 2:] == M).all()      # a vertex whose list would cross the capacity writes nothing
    dv = torch.from_numpy(v).cuda()
    out = torch.full((V + 4, 3), -7.0, device="cuda")
    L.check(so.rx_mesh_smooth_pass(_ptr(dv), None, V, _ptr(a.offsets), _ptr(a.neighbours), E, _ptr(a.boundary), 0.5, 0.0, _ptr(out), st()), "smooth")
    assert (out[V:] == -7).all() and np.array_equal(_bits(out[:V]), _bits(pp.smooth_numpy(v, t, 1, mu=None)))
    fvec, nrm = torch.full((T + 4, 3), -7.0, device="cuda"), torch.full((V + 4, 3), -7.0, device="cuda")
    L.check(so.rx_mesh_face_vectors(_ptr(dv), V, _ptr(dt), T, _ptr(fvec), st()), "faces")
    L.check(so.rx_mesh_vertex_normals(V, _ptr(a.face_offsets), _ptr(a.faces), 3 * T, _ptr(fvec), T, _ptr(nrm), st()), "normals")
    assert (fvec[T:] == -7).all() and (nrm[V:] == -7).all() and np.array_equal(_bits(nrm[:V]), _bits(pp.vertex_normals_numpy(v, t)))


def test_refusals():
    L, ops, _ = _mods()
    v, t = C.grid_patch()
    dv, dt = torch.from_numpy(v).cuda(), torch.from_numpy(t).cuda()
    for bad in (dt + len(v), dt - 1, torch.tensor([[0, 1, len(v)]], device="cuda")):
        with pytest.raises(L.RxError, match="triangles"):
            ops.mesh_adjacency(len(v), bad)
        with pytest.raises(L.RxError, match="triangles"):
            ops.mesh_smooth(dv, bad, 1)
        with pytest.raises(L.RxError, match="triangles"):
            ops.mesh_vertex_normals(dv, bad)
    for bad in (dt.cpu(), dt.int(), dt[:, :2], dt.float()):
        with pytest.raises(L.RxError, match="triangles"):
            ops.mesh_adjacency(len(v), bad)
    for value in (float("nan"), float("inf"), -float("inf")):
        nv = dv.clone()
        nv[17, 1] = value
        with pytest.raises(L.RxError, match="vertices"):
            ops.mesh_smooth(nv, dt, 1)
        with pytest.raises(L.RxError, match="vertices"):
            ops.mesh_vertex_normals(nv, dt)
    for bad in (dv.cpu(), dv.double(), dv[:, :2], dv[0]):
        with pytest.raises(L.RxError, match="vertices"):
            ops.mesh_smooth(bad, dt, 1)
    for kw, word in ((dict(iterations=-1), "iterations"), (dict(iterations=1.5), "iterations"), (dict(iterations=1, lam=float("nan")), "lam"),
                     (dict(iterations=1, lam=float("inf")), "lam"), (dict(iterations=1, mu=float("nan")), "mu"), (dict(iterations=1, mu=1e39), "mu"),
                     (dict(iterations=1, clamp=-0.5), "clamp"), (dict(iterations=1, clamp=float("nan")), "clamp")):
        with pytest.raises(L.RxError, match=word):
            ops.mesh_smooth(dv, dt, **kw)
    with pytest.raises(L.RxError, match="adjacency"):
        ops.mesh_smooth(dv, dt, 1, adjacency=ops.mesh_adjacency(len(v), dt[:-1]))
    # the library's own limits, refused with a status before any launch (the pointers are never read)
    from ctypes import c_void_p
    so, p = L.load(), c_void_p(dv.data_ptr())
    assert so.rx_mesh_count(p, 1, 2**31 - 1, p, p, None) != 0 and b"vertices" in so.rx_last_error()
    assert so.rx_mesh_count(p, (2**31 - 2) // 3 + 1, 4, p, p, None) != 0 and b"triangles" in so.rx_last_error()
    assert so.rx_mesh_count(None, 1, 4, p, p, None) != 0 and b"null" in so.rx_last_error()
    assert so.rx_mesh_scan(p, 0, p, None) != 0 and b"values" in so.rx_last_error()
    assert so.rx_mesh_fill(p, 1, 4, p, p, -1, p, p, None) != 0 and b"capacity" in so.rx_last_error()
    assert so.rx_mesh_smooth_pass(p, None, 4, p, p, 0, None, float("nan"), 0.0, c_void_p(dv.data_ptr() + 4096), None) != 0 and b"factor" in so.rx_last_error()
    assert so.rx_mesh_smooth_pass(p, p, 4, p, p, 0, None, 0.5, -1.0, c_void_p(dv.data_ptr() + 4096), None) != 0 and b"clamp" in so.rx_last_error()
    assert so.rx_mesh_smooth_pass(p, None, 4, p, p, 0, None, 0.5, 0.0, p, None) != 0 and b"another buffer" in so.rx_last_error()


@pytest.mark.parametrize("fmt", ["obj", "ply"])
def test_mesh_refiner_device_file_is_the_host_file(tmp_path, fmt):
    _, _, pp = _mods()
    files = {}
    for name, (v, t) in (("ball", C.ball_mesh()), ("grid", C.grid_patch())):
        for where, refiner in (("host", pp.refine_numpy), ("device", None)):
            src = tmp_path / f"{name}_{where}.{fmt}"
            (pp.write_obj if fmt == "obj" else pp.write_ply)(str(src), v, t)
            summary = pp.MeshRefiner(iterations=4, refiner=refiner).run(str(src))
            files[name, where] = (summary, open(tmp_path / f"{name}_{where}_refined.{fmt}", "rb").read())
        assert files[name, "host"] == files[name, "device"] and len(files[name, "host"][1]) > 1000, name
    assert files["grid", "device"][0]["boundary_vertices"] == int((~C.grid_interior()).sum())
    need = pp.MeshRefiner.scratch_bytes(*map(len, C.ball_mesh()))
    with pytest.raises(MemoryError, match=f"needs {need} bytes"):
        pp.MeshRefiner(max_device_bytes=need - 1).run(str(tmp_path / f"ball_device.{fmt}"), out=str(tmp_path / "never.obj"))


CHILD = r"""
import os, sys
import numpy as np, torch, yaml
sys.path.insert(0, sys.argv[1])
tmp = sys.argv[2]
import mt3d_amd
from mt3d_amd import inference
from mt3d_amd.builders.build_network_from_config import NetworkFromConfig
from mt3d_amd.configuration.config_manager import ConfigManager
from mt3d_amd.dataloading import zarr_lite
def cfg(name, ic):
    c = {"tr_setup": {}, "tr_config": {"patch_size": [16, 16, 16], "batch_size": 2}, "model_config": {},
         "dataset_config": {"targets": {"sheet": {"channels": 1, "activation": "sigmoid"}}}, "inference_config": ic}
    p = os.path.join(tmp, name + ".yaml")
    open(p, "w").write(yaml.safe_dump(c))
    return p
vol = np.random.default_rng(4).integers(0, 256, (32, 32, 32)).astype(np.uint8)
src = zarr_lite.write_array(os.path.join(tmp, "vol.zarr"), vol, (16, 16, 16), compressor="zlib")
base = {"checkpoint_path": os.path.join(tmp, "model.pt"), "input_path": str(src.path), "overlap": 0.5}
torch.manual_seed(3)
torch.save({"model": NetworkFromConfig(ConfigManager(cfg("plain", base), verbose=False)).cuda().state_dict()}, base["checkpoint_path"])
plain = inference.main(["--config_path", cfg("plain", {**base, "output_path": os.path.join(tmp, "a")})])
level = min(int(np.median(zarr_lite.open(os.path.join(plain, "sheet_final"))[...])), 254)
block = {"components": {"tasks": ["sheet"], "level": level, "min_voxels": 4},
         "mesh": {"tasks": ["sheet"], "source": "filtered", "level": level, "format": "obj", "max_device_gb": 8},
         "refine": {"tasks": ["sheet"], "iterations": 3, "lambda": 0.5, "mu": -0.53, "clamp": 1.0, "pin_boundary": True, "normals": True,
                    "max_device_gb": 8}}
store = inference.main(["--config_path", cfg("mesh", {**base, "output_path": os.path.join(tmp, "b"), "postprocess": block})])
print("LEVEL", level)
print("STORE", store)
"""


def test_refined_mesh_at_the_end_of_streaming_inference(tmp_path):
    """`python -m mt3d_amd.inference` with postprocess: {components, mesh, refine} on the tiny store of the isosurface test, in a
    fresh child process: the `_refined` file is the statement applied to the statement's mesh of `sheet_filtered`"""
    _, _, pp = _mods()
    from mt3d_amd.dataloading import zarr_lite
    script = tmp_path / "child.py"
    script.write_text(CHILD)
    r = subprocess.run([sys.executable, str(script), ROOT, str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = dict(ln.split(" ", 1) for ln in r.stdout.splitlines() if ln.startswith(("LEVEL ", "STORE ")))
    store, level = lines["STORE"], int(lines["LEVEL"])
    v, t = pp.surface_nets_numpy(zarr_lite.open(os.path.join(store, "sheet_filtered"))[...], level)
    assert len(v) > 0
    want_v, want_n = pp.refine_numpy(v, t, iterations=3)
    gv, gt, gn = pp.read_mesh(os.path.join(store, "sheet_filtered_refined.obj"))
    assert np.array_equal(_bits(gv), _bits(want_v)) and np.array_equal(gt, t) and np.array_equal(_bits(gn), _bits(want_n))
    assert f"'vertices': {len(v)}" in r.stdout and "'max_displacement'" in r.stdout
