"""Mesh decimation on the device: ops.mesh_decimate (csrc/rx_meshdecimate.hip) against the numpy statement of postprocess/decimate.py
over the shared case list, the C entry points at the smallest and the default table capacity and with outputs longer than their
stated capacity, the refusals, `MeshDecimator` on the device against the host run, and the decimated mesh at the end of streaming
inference.  Everything compares with array_equal, floats by their bits."""
import os
import subprocess
import sys
from ctypes import c_void_p

import numpy as np
import pytest
import torch

import mesh_decimate_cases as D
import mesh_refine_cases as R

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


def _statement(pp, name, representative):
    """the statement of one case, computed once and shared"""
    if (name, representative) not in _WANT:
        _, v, t, cell = D.case(name)
        _WANT[name, representative] = pp.decimate_numpy(v, t, cell, representative)
    return _WANT[name, representative]


@pytest.mark.parametrize("representative", D.REPRESENTATIVES)
def test_every_case_twice_equals_the_statement(representative):
    _, ops, pp = _mods()
    for name, v, t, cell in D.cases():
        dv, dt = torch.from_numpy(v).cuda(), torch.from_numpy(t).cuda()
        a, b = ops.mesh_decimate(dv, dt, cell, representative), ops.mesh_decimate(dv, dt, cell, representative)
        wv, wt, wc = _statement(pp, name, representative)
        assert a[0].dtype == torch.float32 and a[1].dtype == torch.int64 and a[2].dtype == torch.int64, name
        assert tuple(a[0].shape) == wv.shape and tuple(a[1].shape) == wt.shape and tuple(a[2].shape) == wc.shape, name
        assert np.array_equal(_bits(a[0]), _bits(wv)), name
        assert np.array_equal(a[1].cpu().numpy(), wt) and np.array_equal(a[2].cpu().numpy(), wc), name
        assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]), name      # twice: the same bytes
        assert np.array_equal(_bits(dv), _bits(v)) and np.array_equal(dt.cpu().numpy(), t), name      # the inputs are left alone


def _pipeline(L, v, t, cell, representative, capacity, pad=0, marker=-77):
    """the C entry points one by one, with every output `pad` entries longer than its stated capacity and filled with `marker`
    -> (vertices, triangles, cluster_of, [(name, tail)]): the tails must still hold the marker"""
    from mt3d_amd.engine.ops.core import _ptr
    so, st = L.load(), L.stream_ptr
    V, T = len(v), len(t)
    dv, dt = torch.from_numpy(v).cuda(), torch.from_numpy(t).cuda()
    tails = []

    def buf(name, n, dtype=torch.int32, width=1):
        x = torch.full(((n + pad) * width,), marker, dtype=dtype, device="cuda")
        tails.append((name, x[n * width:]))
        return x
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    keys, tk, tm = buf("keys", V, torch.int64), buf("table_keys", capacity, torch.int64), buf("table_min", capacity)
    slot, first, rank, cluster_of = buf("slot_of", V), buf("first", V), buf("rank", V + 1, torch.int64), buf("cluster_of", V, torch.int64)
    L.check(so.rx_mesh_cluster_keys(_ptr(dv), V, cell, _ptr(keys), _ptr(flag), st()), "keys")
    L.check(so.rx_mesh_cluster_assign(_ptr(keys), V, capacity, _ptr(tk), _ptr(tm), _ptr(slot), _ptr(first), _ptr(flag), st()), "assign")
    L.check(so.rx_mesh_scan(_ptr(first), V, _ptr(rank), st()), "scan")
    L.check(so.rx_mesh_cluster_number(V, _ptr(slot), capacity, _ptr(tm), _ptr(rank), _ptr(cluster_of), st()), "number")
    C = int(rank[V].item())
    assert flag.item() == 0
    counts, reps = buf("counts", C), buf("reps", C, torch.float32, 3)
    if representative == "mean":
        moff, members = buf("member_offsets", C + 1, torch.int64), buf("members", V)
        L.check(so.rx_mesh_cluster_count(_ptr(cluster_of), V, C, _ptr(counts), st()), "count")
        L.check(so.rx_mesh_scan(_ptr(counts), C, _ptr(moff), st()), "scan")
        L.check(so.rx_mesh_cluster_fill(_ptr(cluster_of), V, C, _ptr(moff), _ptr(counts), V, _ptr(members), st()), "fill")
        L.check(so.rx_mesh_cluster_mean(_ptr(dv), V, C, _ptr(moff), _ptr(members), V, _ptr(reps), st()), "mean")
    else:
        best = buf("best", C, torch.int64)
        L.check(so.rx_mesh_cluster_nearest(_ptr(dv), _ptr(keys), V, cell, _ptr(cluster_of), C, _ptr(best), _ptr(reps), st()), "nearest")
    used, toff, uoff = buf("used", C), buf("entry_offsets", C + 1, torch.int64), buf("used_offsets", C + 1, torch.int64)
    entries, keep, koff = buf("entries", T, width=3), buf("keep", T), buf("keep_offsets", T + 1, torch.int64)
    L.check(so.rx_mesh_cluster_remap(_ptr(dt), T, V, _ptr(cluster_of), C, _ptr(counts), _ptr(used), _ptr(flag), st()), "remap")
    L.check(so.rx_mesh_scan(_ptr(counts), C, _ptr(toff), st()), "scan")
    L.check(so.rx_mesh_scan(_ptr(used), C, _ptr(uoff), st()), "scan")
    L.check(so.rx_mesh_cluster_unique(_ptr(dt), T, V, _ptr(cluster_of), C, _ptr(toff), _ptr(counts), T, _ptr(entries), _ptr(keep), st()), "unique")
    L.check(so.rx_mesh_scan(_ptr(keep), T, _ptr(koff), st()), "scan")
    nv, nt = int(uoff[C].item()), int(koff[T].item())
    out_v, out_t = buf("out_vertices", nv, torch.float32, 3), buf("out_triangles", nt, torch.int64, 3)
    L.check(so.rx_mesh_cluster_emit(_ptr(dt), T, V, _ptr(cluster_of), C, _ptr(keep), _ptr(koff), _ptr(used), _ptr(uoff), _ptr(reps), nv, _ptr(out_v),
                                    nt, _ptr(out_t), st()), "emit")
    assert flag.item() == 0
    return out_v[:3 * nv].reshape(nv, 3), out_t[:3 * nt].reshape(nt, 3), cluster_of[:V], tails


@pytest.mark.parametrize("representative", D.REPRESENTATIVES)
def test_smallest_table_capacity_gives_the_same_result(representative):
    """the hash table at the smallest capacity the library accepts (the power of two just above V: long probe chains where every
    vertex is its own cluster) and at the default of the ops layer"""
    L, ops, pp = _mods()
    from mt3d_amd.engine.ops.mesh import _table_capacity
    for name in ("big-grid-fine", "big-grid-c2", "ball-c0.75", "soup257-c3.5", "fan3000-c50"):
        _, v, t, cell = D.case(name)
        wv, wt, wc = _statement(pp, name, representative)
        smallest = 1 << len(v).bit_length()      # the smallest power of two above V
        assert len(v) < smallest <= _table_capacity(len(v)) and _table_capacity(len(v)) >= 2 * len(v) + 2 > _table_capacity(len(v)) // 2
        for capacity in (smallest, _table_capacity(len(v))):
            gv, gt, gc, _ = _pipeline(L, v, t, cell, representative, capacity)
            assert np.array_equal(_bits(gv), _bits(wv)) and np.array_equal(gt.cpu().numpy(), wt) and np.array_equal(gc.cpu().numpy(), wc), (name, capacity)


@pytest.mark.parametrize("representative", D.REPRESENTATIVES)
def test_nothing_is_written_beyond_a_capacity(representative):
    """every output eight entries longer than the capacity the call is told, filled with a marker: the part beyond keeps it"""
    L, ops, pp = _mods()
    for name in ("ball-c2", "soup2100-c40", "awkward-c50"):
        _, v, t, cell = D.case(name)
        wv, wt, wc = _statement(pp, name, representative)
        gv, gt, gc, tails = _pipeline(L, v, t, cell, representative, 1 << len(v).bit_length(), pad=8)
        assert np.array_equal(_bits(gv), _bits(wv)) and np.array_equal(gt.cpu().numpy(), wt) and np.array_equal(gc.cpu().numpy(), wc), name
        for what, tail in tails:
            assert tail.numel() >= 8 and (tail == -77).all(), (name, what)
    # outputs shorter than the result: the rows from the capacity on are never stored
    from mt3d_amd.engine.ops.core import _ptr
    _, v, t, cell = D.case("ball-c2")
    wv, wt, wc = _statement(pp, "ball-c2", representative)
    V, T, C = len(v), len(t), int(wc.max()) + 1
    dt, dc = torch.from_numpy(t).cuda(), torch.from_numpy(wc).cuda()
    rows = pp.cluster_rows(wc, t)
    ct = wc[t]
    live = (ct[:, 0] != ct[:, 1]) & (ct[:, 1] != ct[:, 2]) & (ct[:, 0] != ct[:, 2])
    keep = np.zeros(T, np.int32)
    keep[np.nonzero(live)[0][np.unique(np.sort(ct[live], axis=1), axis=0, return_index=True)[1]]] = 1      # the lowest index of each triple
    used = (rows >= 0).astype(np.int32)
    koff = np.concatenate([[0], np.cumsum(keep)]).astype(np.int64)
    uoff = np.concatenate([[0], np.cumsum(used)]).astype(np.int64)
    reps = torch.zeros((C, 3), device="cuda")
    nv, nt = len(wv), len(wt)
    out_v, out_t = torch.full((nv, 3), -7.0, device="cuda"), torch.full((nt, 3), -77, dtype=torch.int64, device="cuda")
    dkeep, dkoff, dused, duoff = (torch.from_numpy(a).cuda() for a in (keep, koff, used, uoff))
    L.check(L.load().rx_mesh_cluster_emit(_ptr(dt), T, V, _ptr(dc), C, _ptr(dkeep), _ptr(dkoff), _ptr(dused), _ptr(duoff), _ptr(reps),
                                          nv // 2, _ptr(out_v), nt // 2, _ptr(out_t), L.stream_ptr()), "emit")
    assert (out_v[nv // 2:] == -7).all() and (out_t[nt // 2:] == -77).all() and (out_v[:nv // 2] == 0).all()
    assert np.array_equal(out_t[:nt // 2].cpu().numpy(), wt[:nt // 2])


def test_empty_inputs_and_one_cluster():
    _, ops, pp = _mods()
    e, none = torch.zeros((0, 3), device="cuda"), torch.zeros((0, 3), dtype=torch.int64, device="cuda")
    for representative in D.REPRESENTATIVES:
        v, t, c = ops.mesh_decimate(e, none, 1.0, representative)
        assert v.shape == (0, 3) and v.dtype == torch.float32 and t.shape == (0, 3) and t.dtype == torch.int64 and c.shape == (0,) and c.dtype == torch.int64
        pv, pt, pcell = D.case("no-triangles")[1:]
        v, t, c = ops.mesh_decimate(torch.from_numpy(pv).cuda(), none, pcell, representative)
        assert v.shape == (0, 3) and t.shape == (0, 3) and np.array_equal(c.cpu().numpy(), pp.decimate_numpy(pv, pt, pcell, representative)[2])
        gv, gt, gcell = D.case("grid-one-cluster")[1:]
        v, t, c = ops.mesh_decimate(torch.from_numpy(gv).cuda(), torch.from_numpy(gt).cuda(), gcell, representative)
        assert v.shape == (0, 3) and v.dtype == torch.float32 and t.shape == (0, 3) and t.dtype == torch.int64 and c.tolist() == [0] * len(gv)


def test_refusals():
    L, ops, _ = _mods()
    v, t = R.grid_patch()
    dv, dt = torch.from_numpy(v).cuda(), torch.from_numpy(t).cuda()
    for bad in (dt + len(v), dt - 1, torch.tensor([[0, 1, len(v)]], device="cuda"), dt.cpu(), dt.int(), dt[:, :2], dt.float()):      # as mesh_smooth
        with pytest.raises(L.RxError, match="triangles"):
            ops.mesh_decimate(dv, bad, 1.0)
    for value in (float("nan"), float("inf"), -float("inf")):
        nv = dv.clone()
        nv[17, 1] = value
        with pytest.raises(L.RxError, match="vertices"):
            ops.mesh_decimate(nv, dt, 1.0)
    for bad in (dv.cpu(), dv.double(), dv[:, :2], dv[0]):
        with pytest.raises(L.RxError, match="vertices"):
            ops.mesh_decimate(bad, dt, 1.0)
    for cell in (0, 0.0, -1.0, float("nan"), float("inf"), 1e39, 1e-50, True, "1", None):
        with pytest.raises(L.RxError, match="cell"):
            ops.mesh_decimate(dv, dt, cell)
    with pytest.raises(L.RxError, match="cell"):      # 6 / 2^-18 = 2^20 * 1.5: a key out of range
        ops.mesh_decimate(dv, dt, 2.0**-18)
    for representative in ("median", None, 1):
        with pytest.raises(L.RxError, match="representative"):
            ops.mesh_decimate(dv, dt, 1.0, representative)
    # the library's own limits, refused with a status and a message before any launch (the pointers are never read)
    so, p, V = L.load(), c_void_p(dv.data_ptr()), len(v)
    for capacity in (V, V - 1, 48, 63, 0, -64, 2**32):      # not above V, or no power of two, or beyond 2^31
        assert so.rx_mesh_cluster_assign(p, V, capacity, p, p, p, p, p, None) != 0 and b"capacity" in so.rx_last_error(), capacity
    assert so.rx_mesh_cluster_assign(None, V, 64, p, p, p, p, p, None) != 0 and b"null" in so.rx_last_error()
    assert so.rx_mesh_cluster_assign(p, V, 64, p, None, p, p, p, None) != 0 and b"null" in so.rx_last_error()
    assert so.rx_mesh_cluster_keys(None, V, 1.0, p, p, None) != 0 and b"null" in so.rx_last_error()
    for cell in (0.0, -1.0, float("nan"), float("inf")):
        assert so.rx_mesh_cluster_keys(p, V, cell, p, p, None) != 0 and b"cell" in so.rx_last_error()
        assert so.rx_mesh_cluster_nearest(p, p, V, cell, p, 1, p, p, None) != 0 and b"cell" in so.rx_last_error()
    assert so.rx_mesh_cluster_keys(p, 2**31 - 1, 1.0, p, p, None) != 0 and b"vertices" in so.rx_last_error()
    assert so.rx_mesh_cluster_count(p, V, V + 1, p, None) != 0 and b"clusters" in so.rx_last_error()
    assert so.rx_mesh_cluster_remap(p, (2**31 - 2) // 3 + 1, V, p, 1, p, p, p, None) != 0 and b"triangles" in so.rx_last_error()
    assert so.rx_mesh_cluster_unique(p, 1, V, p, 1, p, p, -1, p, p, None) != 0 and b"capacity" in so.rx_last_error()
    assert so.rx_mesh_cluster_emit(p, 1, V, p, 1, p, p, p, p, p, -1, p, 0, p, None) != 0 and b"capacity" in so.rx_last_error()
    assert so.rx_mesh_cluster_mean(p, V, 1, p, p, 4, c_void_p(dv.data_ptr() + 2), None) != 0 and b"misaligned" in so.rx_last_error()


@pytest.mark.parametrize("fmt", ["obj", "ply"])
def test_mesh_decimator_device_file_is_the_host_file(tmp_path, fmt):
    _, _, pp = _mods()
    files = {}
    for name, representative in (("ball-c2", "mean"), ("slab-c1", "nearest")):
        _, v, t, cell = D.case(name)
        for where, decimator in (("host", pp.decimate_numpy), ("device", None)):
            src = tmp_path / f"{name}_{where}.{fmt}"
            (pp.write_obj if fmt == "obj" else pp.write_ply)(str(src), v, t)
            summary = pp.MeshDecimator(cell, representative, decimator=decimator).run(str(src))
            files[name, where] = (summary, open(tmp_path / f"{name}_{where}_decimated.{fmt}", "rb").read())
        assert files[name, "host"] == files[name, "device"] and len(files[name, "host"][1]) > 1000, name
    assert files["ball-c2", "device"][0]["vertices"] == len(_statement(pp, "ball-c2", "mean")[0])
    _, v, t, cell = D.case("ball-c2")
    need = pp.MeshDecimator.scratch_bytes(len(v), len(t))
    with pytest.raises(MemoryError, match=f"needs {need} bytes"):
        pp.MeshDecimator(cell, max_device_bytes=need - 1).run(str(tmp_path / f"ball-c2_device.{fmt}"), out=str(tmp_path / "never.obj"))
    assert not (tmp_path / "never.obj").exists()


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
                    "max_device_gb": 8},
         "decimate": {"tasks": ["sheet"], "cell": 2.5, "representative": "mean", "normals": True, "max_device_gb": 8}}
store = inference.main(["--config_path", cfg("mesh", {**base, "output_path": os.path.join(tmp, "b"), "postprocess": block})])
print("LEVEL", level)
print("STORE", store)
"""


def test_decimated_mesh_at_the_end_of_streaming_inference(tmp_path):
    """`python -m mt3d_amd.inference` with postprocess: {components, mesh, refine, decimate} on the 32^3 store of the refine test, in a
    fresh child process: the `_refined_decimated` file is the statement applied to the statement's refined mesh of `sheet_filtered`"""
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
    rv, _ = pp.refine_numpy(v, t, iterations=3)
    want_v, want_t, cluster_of = pp.decimate_numpy(rv, t, 2.5, "mean")
    want_n = pp.vertex_normals_numpy(want_v, want_t)
    gv, gt, gn = pp.read_mesh(os.path.join(store, "sheet_filtered_refined_decimated.obj"))
    assert 0 < len(want_v) < len(v) and 0 < len(want_t) < len(t)
    assert np.array_equal(_bits(gv), _bits(want_v)) and np.array_equal(gt, want_t) and np.array_equal(_bits(gn), _bits(want_n))
    assert f"'input_vertices': {len(v)}" in r.stdout and f"'clusters': {int(cluster_of.max()) + 1}" in r.stdout and "'max_displacement'" in r.stdout
