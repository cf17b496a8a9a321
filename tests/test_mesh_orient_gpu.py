"""Mesh orientation on the device: ops.mesh_sample, mesh_face_cos and mesh_select (csrc/rx_meshsample.hip) against the numpy
statements of postprocess/orient.py over the shared case list, slab launches into one buffer, outputs longer than their stated
capacity, the refusals, `MeshOrienter` on the device against the host run, and the oriented mesh at the end of streaming
inference.  Everything compares with array_equal, floats by their bits."""
import os
import subprocess
import sys
from ctypes import c_void_p

import numpy as np
import pytest
import torch

import mesh_orient_cases as O

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARK = -77.0


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


def _dev(a):
    """a numpy array on the device; uint16 as the int16 tensor that holds its bits"""
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).cuda()


_WANT = {}


def _statement(pp, name):
    """the statement of one sampling case, computed once and shared"""
    if name not in _WANT:
        _, vol, pts, rule = O.sample_case(name)
        _WANT[name] = pp.sample_points_numpy(vol, pts, rule)[0]
    return _WANT[name]


def test_every_sampling_case_twice_equals_the_statement():
    _, ops, pp = _mods()
    seen = set()
    for name, vol, pts, rule in O.sample_cases():
        dvol, dpts = _dev(vol), _dev(pts)
        keep_vol, keep_pts = dvol.clone(), dpts.clone()
        a, b = ops.mesh_sample(dvol, dpts, rule), ops.mesh_sample(dvol, dpts, rule)
        want = _statement(pp, name)
        assert a.dtype == torch.float32 and tuple(a.shape) == want.shape, name
        assert np.array_equal(_bits(a), _bits(want)), name
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), name      # twice: the same bytes
        assert torch.equal(dvol, keep_vol) and torch.equal(dpts.view(torch.int32), keep_pts.view(torch.int32)), name      # the inputs are left alone
        seen.add((rule, vol.shape[0], len(pts)))
    assert {r for r, _, _ in seen} == set(O.RULES) and {c for _, c, _ in seen} >= {1, 3, 8} and {v for _, _, v in seen} >= set(O.COUNTS)


@pytest.mark.parametrize("rule", ["copy", "normal_u16"])
def test_unit_epilogue(rule):
    _, ops, pp = _mods()
    _, vol, pts, _ = O.sample_case(f"{rule}-c3-v257")
    vol = vol.copy()
    if rule == "copy":
        vol[:, 0] = 0      # plane 0 samples to the zero vector, which stays exactly zero
    want = pp.unit_numpy(pp.sample_points_numpy(vol, pts, rule)[0])
    got = ops.mesh_sample(_dev(vol), _dev(pts), rule, unit=True)
    assert np.array_equal(_bits(got), _bits(want))
    if rule == "copy":
        assert (want == 0).all(1).any()


@pytest.mark.parametrize("rule", list(O.RULES))
def test_slab_launches_fill_one_buffer_with_the_resident_bits(rule):
    _, ops, pp = _mods()
    _, vol, pts, _ = O.sample_case(f"{rule}-c3-v257")
    Z = vol.shape[1]
    want, dpts = _statement(pp, f"{rule}-c3-v257"), _dev(pts)
    for depth in (1, 2, Z):
        out = torch.full((len(pts), 3), MARK, device="cuda")
        owned_by_now = np.zeros(len(pts), bool)
        for z_base, planes in pp.slab_ranges(Z, depth):
            part = np.ascontiguousarray(vol[:, z_base:z_base + planes])
            ops.mesh_sample(_dev(part), dpts, rule, z_base=z_base, z_total=Z, out=out)
            owned_by_now |= pp.sample_points_numpy(part, pts, rule, z_base, Z)[1]
            host = out.cpu().numpy()
            assert (host[~owned_by_now] == MARK).all(), (depth, z_base)      # what no slab so far owns keeps the marker
            assert np.array_equal(_bits(host[owned_by_now]), _bits(want[owned_by_now])), (depth, z_base)
        assert owned_by_now.all() and np.array_equal(_bits(out), _bits(want)), depth


def test_nothing_is_written_beyond_a_capacity():
    """the C entry points with every output eight entries longer than the call is told, filled with a marker: the tails keep it"""
    L, ops, pp = _mods()
    from mt3d_amd.engine.ops.core import _ptr
    so, st, pad = L.load(), L.stream_ptr, 8
    _, vol, pts, rule = O.sample_case("u8-c8-v257")
    V, C = len(pts), vol.shape[0]
    out = torch.full(((V + pad) * C,), MARK, device="cuda")
    dvol, dpts = _dev(vol), _dev(pts)      # held: a pointer alone does not keep a tensor alive
    L.check(so.rx_mesh_sample(_ptr(dvol), L.RX_MESH_SAMPLE_U8, C, 0, vol.shape[1], vol.shape[1], vol.shape[2], vol.shape[3], _ptr(dpts), V, 0,
                              _ptr(out), st()), "sample")
    assert (out[V * C:] == MARK).all() and np.array_equal(_bits(out[:V * C].view(V, C)), _bits(_statement(pp, "u8-c8-v257")))
    for name, v, t, n, min_cos in O.mesh_cases():
        V, T = len(v), len(t)
        dv, dt, dn = _dev(v), _dev(t), _dev(n)
        cos, side = torch.full((T + pad,), MARK, device="cuda"), torch.full((T + pad,), 77, dtype=torch.int8, device="cuda")
        keep, used = torch.full((T + pad,), 77, dtype=torch.int32, device="cuda"), torch.full((V + pad,), 77, dtype=torch.int32, device="cuda")
        flag = torch.zeros(1, dtype=torch.int32, device="cuda")
        L.check(so.rx_mesh_face_cos(_ptr(dv), _ptr(dn), V, _ptr(dt), T, min_cos, 1, _ptr(cos), _ptr(side), _ptr(keep), _ptr(used), _ptr(flag), st()), "cos")
        wcos = pp.face_cos_numpy(v, t, n)
        wside = pp.side_numpy(wcos, min_cos)
        assert flag.item() == 0 and (cos[T:] == MARK).all() and (side[T:] == 77).all() and (keep[T:] == 77).all() and (used[V:] == 77).all(), name
        assert np.array_equal(_bits(cos[:T]), _bits(wcos)) and np.array_equal(side[:T].cpu().numpy(), wside), name
        assert np.array_equal(keep[:T].cpu().numpy(), (wside == 1).astype(np.int32)), name
        wused = np.zeros(V, np.int32)
        wused[np.unique(t[wside == 1])] = 1
        assert np.array_equal(used[:V].cpu().numpy(), wused), name
        used2 = torch.full((V + pad,), 77, dtype=torch.int32, device="cuda")
        L.check(so.rx_mesh_select_mark(_ptr(dt), T, V, _ptr(keep), _ptr(used2), _ptr(flag), st()), "mark")
        assert flag.item() == 0 and torch.equal(used2, used), name


@pytest.mark.parametrize("side", ["front", "back", "both"])
def test_face_cos_and_select_twice_equal_the_statements(side):
    _, ops, pp = _mods()
    want_side = {"front": 1, "back": -1, "both": 0}[side]
    for name, v, t, n, min_cos in O.mesh_cases():
        dv, dt, dn = _dev(v), _dev(t), _dev(n)
        wcos = pp.face_cos_numpy(v, t, n)
        wside = pp.side_numpy(wcos, min_cos)
        wkeep = np.ones(len(t), bool) if want_side == 0 else wside == want_side
        runs = []
        for _ in range(2):
            cos, sd, used = ops.mesh_face_cos(dv, dt, dn, min_cos, side)
            keep = torch.from_numpy(wkeep).cuda()
            a = ops.mesh_select(dv, dt, keep, (dn,), used=used)
            b = ops.mesh_select(dv, dt, keep.to(torch.int32), (dn, dv))      # marks the used vertices itself
            runs.append((cos, sd, used, a, b))
        cos, sd, used, a, b = runs[0]
        assert cos.dtype == torch.float32 and sd.dtype == torch.int8 and used.dtype == torch.int32, name
        assert np.array_equal(_bits(cos), _bits(wcos)) and np.array_equal(sd.cpu().numpy(), wside), name
        wv, wt, (wn,), wrow = pp.select_numpy(v, t, wkeep, n)
        for got in (a, b):
            assert got[0].dtype == torch.float32 and got[1].dtype == torch.int64 and got[3].dtype == torch.int64, name
            assert tuple(got[0].shape) == wv.shape and tuple(got[1].shape) == wt.shape, name
            assert np.array_equal(_bits(got[0]), _bits(wv)) and np.array_equal(got[1].cpu().numpy(), wt), name
            assert np.array_equal(_bits(got[2][0]), _bits(wn)) and np.array_equal(got[3].cpu().numpy(), wrow), name
        assert np.array_equal(_bits(b[2][1]), _bits(wv)), name
        for x, y in zip(runs[0][:3], runs[1][:3]):      # twice: the same bytes
            assert torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y), name
        for k in (3, 4):
            assert torch.equal(runs[0][k][0].view(torch.int32), runs[1][k][0].view(torch.int32)) and torch.equal(runs[0][k][1], runs[1][k][1]), name
        assert np.array_equal(_bits(dv), _bits(v)) and np.array_equal(dt.cpu().numpy(), t) and np.array_equal(_bits(dn), _bits(n)), name
    # the rim rule
    v, t, n = O.rim_mesh()
    cos, sd, _ = ops.mesh_face_cos(_dev(v), _dev(t), _dev(n), 0.2, side)
    assert torch.isnan(cos[:2]).all() and sd.tolist() == [0, 0, 1, -1]


def test_empty_inputs():
    _, ops, pp = _mods()
    vol = _dev(O.volume("u8", (3, 2, 2, 2)))
    out = ops.mesh_sample(vol, torch.zeros((0, 3), device="cuda"), "u8")
    assert out.shape == (0, 3) and out.dtype == torch.float32
    v, none = _dev(O.rim_mesh()[0]), torch.zeros((0, 3), dtype=torch.int64, device="cuda")
    cos, sd, used = ops.mesh_face_cos(v, none, v, 0.2, "front")
    assert cos.shape == (0,) and sd.shape == (0,) and sd.dtype == torch.int8 and used.tolist() == [0] * len(v)
    sv, st, sa, row = ops.mesh_select(v, none, torch.zeros(0, dtype=torch.bool, device="cuda"), (v,))
    assert sv.shape == (0, 3) and st.shape == (0, 3) and sa[0].shape == (0, 3) and row.tolist() == [-1] * len(v)
    t = _dev(O.rim_mesh()[1])
    sv, st, sa, row = ops.mesh_select(v, t, torch.zeros(len(t), dtype=torch.bool, device="cuda"))      # nothing kept
    assert sv.shape == (0, 3) and st.shape == (0, 3) and sa == () and row.tolist() == [-1] * len(v)


def test_refusals():
    L, ops, _ = _mods()
    vol, pts = _dev(O.volume("u16", (3, 4, 5, 6))), _dev(O.points((4, 5, 6), 30))
    u8, f32 = _dev(O.volume("u8", (3, 4, 5, 6))), _dev(O.volume("copy", (3, 4, 5, 6)))
    for bad, rule in ((vol.cpu(), "u16"), (u8, "u16"), (f32, "normal_u16"), (vol, "u8"), (vol, "copy"), (u8, "copy"), (vol.int(), "u16"), (vol, "u32"),
                      (vol, None)):
        with pytest.raises(L.RxError, match="volume|rule"):
            ops.mesh_sample(bad, pts, rule)
    for bad in (_dev(O.volume("u8", (9, 2, 2, 2))), u8[0], u8[:, :0], u8[None]):      # C outside 1 .. 8, wrong rank, empty
        with pytest.raises(L.RxError, match="volume"):
            ops.mesh_sample(bad, pts, "u8")
    for bad in (pts.cpu(), pts.double(), pts[:, :2], pts[0]):
        with pytest.raises(L.RxError, match="points"):
            ops.mesh_sample(vol, bad, "u16")
    for value in (float("nan"), float("inf"), -float("inf")):
        p = pts.clone()
        p[7, 2] = value
        with pytest.raises(L.RxError, match="points"):
            ops.mesh_sample(vol, p, "u16")
    for z_base, z_total in ((-1, 4), (1, 4), (0, 3), (2, 5), (0, 4.0), (True, 8), ("0", 4)):      # the slab (four planes) must lie inside z_total
        with pytest.raises(L.RxError, match="slab"):
            ops.mesh_sample(vol, pts, "u16", z_base=z_base, z_total=z_total)
    with pytest.raises(L.RxError, match="unit"):
        ops.mesh_sample(u8[:2], pts, "u8", unit=True)
    with pytest.raises(L.RxError, match="unit"):
        ops.mesh_sample(u8, pts, "u8", unit=1)
    for bad in (torch.zeros((30, 2), device="cuda"), torch.zeros((30, 3), dtype=torch.float64, device="cuda"), torch.zeros((30, 3))):
        with pytest.raises(L.RxError, match="out"):
            ops.mesh_sample(vol, pts, "u16", out=bad)
    v, t, n = (_dev(a) for a in O.rim_mesh())
    for bad in (t + len(v), t - 1, torch.tensor([[0, 1, len(v)]], device="cuda"), t.cpu(), t.int(), t[:, :2]):      # ids outside the mesh
        with pytest.raises(L.RxError, match="triangles"):
            ops.mesh_face_cos(v, bad, n, 0.2, "front")
        keep = torch.ones(len(bad), dtype=torch.bool, device="cuda")
        with pytest.raises(L.RxError, match="triangles"):
            ops.mesh_select(v, bad, keep)
    for bad in (v.cpu(), v.double(), v[:, :2]):
        with pytest.raises(L.RxError, match="vertices"):
            ops.mesh_face_cos(bad, t, n, 0.2, "front")
        with pytest.raises(L.RxError, match="vertices"):
            ops.mesh_select(bad, t, torch.ones(len(t), dtype=torch.bool, device="cuda"))
    nv = v.clone()
    nv[2, 0] = float("nan")
    with pytest.raises(L.RxError, match="vertices"):
        ops.mesh_face_cos(nv, t, n, 0.2, "front")
    for bad in (n.cpu(), n.double(), n[:-1], n[:, :2]):
        with pytest.raises(L.RxError, match="vectors"):
            ops.mesh_face_cos(v, t, bad, 0.2, "front")
    for bad in (1, 1.5, -0.1, float("nan"), True, "0.2", None):
        with pytest.raises(L.RxError, match="min_cos"):
            ops.mesh_face_cos(v, t, n, bad, "front")
    for bad in ("top", 1, None):
        with pytest.raises(L.RxError, match="side"):
            ops.mesh_face_cos(v, t, n, 0.2, bad)
    ok = torch.ones(len(t), dtype=torch.bool, device="cuda")
    for bad in (ok.cpu(), ok[:-1], ok.float(), ok.long(), None):
        with pytest.raises(L.RxError, match="keep"):
            ops.mesh_select(v, t, bad)
    for bad in (n.cpu(), n.double(), n[:-1]):
        with pytest.raises(L.RxError, match="attribute"):
            ops.mesh_select(v, t, ok, (bad,))
    for bad in (torch.ones(len(v), device="cuda"), torch.ones(len(v) + 1, dtype=torch.int32, device="cuda"), torch.ones(len(v), dtype=torch.int32)):
        with pytest.raises(L.RxError, match="used"):
            ops.mesh_select(v, t, ok, used=bad)
    # the library's own limits, refused with a status and a message before any launch (the pointers are never read)
    so, p = L.load(), c_void_p(v.data_ptr())
    assert so.rx_mesh_sample(None, 1, 3, 0, 4, 4, 5, 6, p, 9, 0, p, None) != 0 and b"null" in so.rx_last_error()
    assert so.rx_mesh_sample(p, 1, 3, 0, 4, 4, 5, 6, p, 9, 0, None, None) != 0 and b"null" in so.rx_last_error()
    for rule in (-1, 4):
        assert so.rx_mesh_sample(p, rule, 3, 0, 4, 4, 5, 6, p, 9, 0, p, None) != 0 and b"rule" in so.rx_last_error()
    for channels in (0, 9):
        assert so.rx_mesh_sample(p, 1, channels, 0, 4, 4, 5, 6, p, 9, 0, p, None) != 0 and b"channels" in so.rx_last_error()
    assert so.rx_mesh_sample(p, 1, 2, 0, 4, 4, 5, 6, p, 9, 1, p, None) != 0 and b"unit" in so.rx_last_error()
    for z_base, z_depth, z_total in ((-1, 4, 4), (1, 4, 4), (0, 0, 4), (0, 5, 4), (4, 1, 4), (2**31 - 1, 2, 4)):
        assert so.rx_mesh_sample(p, 1, 3, z_base, z_depth, z_total, 5, 6, p, 9, 0, p, None) != 0 and b"slab" in so.rx_last_error()
    for z, y, x in ((0, 5, 6), (4, 0, 6), (4, 5, 0), (2**24 - 1, 5, 6), (4, 2**24, 6)):
        assert so.rx_mesh_sample(p, 1, 3, 0, 1, z, y, x, p, 9, 0, p, None) != 0 and b"extents" in so.rx_last_error()
    for count in (0, -1, 2**31 - 1):
        assert so.rx_mesh_sample(p, 1, 3, 0, 4, 4, 5, 6, p, count, 0, p, None) != 0 and b"points" in so.rx_last_error()
    assert so.rx_mesh_sample(c_void_p(v.data_ptr() + 1), 2, 3, 0, 4, 4, 5, 6, p, 9, 0, p, None) != 0 and b"misaligned" in so.rx_last_error()
    assert so.rx_mesh_face_cos(p, p, 9, p, 4, 1.0, 1, p, p, p, p, p, None) != 0 and b"min_cos" in so.rx_last_error()
    assert so.rx_mesh_face_cos(p, p, 9, p, 4, float("nan"), 1, p, p, p, p, p, None) != 0 and b"min_cos" in so.rx_last_error()
    assert so.rx_mesh_face_cos(p, p, 9, p, 4, 0.2, 2, p, p, p, p, p, None) != 0 and b"want" in so.rx_last_error()
    assert so.rx_mesh_face_cos(p, p, 0, p, 4, 0.2, 1, p, p, p, p, p, None) != 0 and b"vertices" in so.rx_last_error()
    assert so.rx_mesh_face_cos(p, p, 9, p, (2**31 - 2) // 3 + 1, 0.2, 1, p, p, p, p, p, None) != 0 and b"triangles" in so.rx_last_error()
    assert so.rx_mesh_face_cos(p, None, 9, p, 4, 0.2, 1, p, p, p, p, p, None) != 0 and b"null" in so.rx_last_error()
    assert so.rx_mesh_select_mark(p, 4, 9, p, None, p, None) != 0 and b"null" in so.rx_last_error()
    assert so.rx_mesh_select_mark(p, 0, 9, p, p, p, None) != 0 and b"triangles" in so.rx_last_error()
    assert so.rx_mesh_select_mark(p, 4, 9, c_void_p(v.data_ptr() + 2), p, p, None) != 0 and b"misaligned" in so.rx_last_error()


def _store(tmp_path, pp, fmt):
    from mt3d_amd.dataloading import zarr_lite
    v, t = O.ball_mesh()
    store = tmp_path / "store"
    shape = (24, 24, 24)
    rng = np.random.default_rng(8)
    field = O.constant_field(shape).astype(np.int64) + rng.integers(-9000, 9000, (3,) + shape)
    zarr_lite.write_array(str(store / "normals_final"), np.clip(field, 0, 65535).astype(np.uint16), (3, 8, 16, 16), compressor="zlib")
    for where in ("host", "device"):
        (pp.write_obj if fmt == "obj" else pp.write_ply)(str(store / f"ball_{where}.{fmt}"), v, t)
    return store, v, t


@pytest.mark.parametrize("fmt", ["obj", "ply"])
def test_mesh_orienter_device_file_is_the_host_file(tmp_path, fmt):
    _, _, pp = _mods()
    store, v, t = _store(tmp_path, pp, fmt)
    plane = lambda n: pp.MeshOrienter.scratch_bytes(len(v), len(t), 3, n, 24, 24)      # noqa: E731
    files = {}
    for how, budget, slabs, kw in (("resident", None, 1, {}), ("slabs", plane(8), 8, {}), ("one-buffer", plane(3), 12, dict(side="back", normals="mesh")),
                                   ("both", plane(5), 23, dict(side="both", min_cos=0.5))):
        for where in ("host", "device"):
            o = pp.MeshOrienter(max_device_bytes=budget, where=where, **kw)
            out = tmp_path / f"{how}_{where}.{fmt}"
            summary = o.run(str(store / f"ball_{where}.{fmt}"), str(store), out=str(out))
            assert o.last_slabs == slabs, (how, where)
            files[how, where] = (summary, out.read_bytes())
        assert files[how, "host"] == files[how, "device"] and len(files[how, "host"][1]) > 1000, how
    assert files["resident", "device"] == files["slabs", "device"]
    s = files["resident", "device"][0]
    assert s["front"] > 100 and s["back"] > 100 and s["rim"] > 0 and s["input_vertices"] == len(v) and s["triangles"] == s["front"]
    assert files["both", "device"][0]["triangles"] == len(t)
    with pytest.raises(MemoryError, match=f"needs {plane(2)} bytes"):
        pp.MeshOrienter(max_device_bytes=plane(2) - 1).run(str(store / f"ball_device.{fmt}"), str(store), out=str(tmp_path / "never.obj"))
    with pytest.raises(FileExistsError):
        pp.MeshOrienter().run(str(store / f"ball_device.{fmt}"), str(store), out=str(tmp_path / f"resident_device.{fmt}"))
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
         "dataset_config": {"targets": {"sheet": {"channels": 1, "activation": "sigmoid"}, "normals": {"channels": 3, "activation": "none"}}},
         "inference_config": ic}
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
         "orient": {"tasks": ["sheet"], "normals_task": "normals", "side": "front", "min_cos": 0.2, "normals": "predicted", "max_device_gb": 8}}
store = inference.main(["--config_path", cfg("mesh", {**base, "output_path": os.path.join(tmp, "b"), "postprocess": block})])
print("STORE", store)
"""


def test_front_face_at_the_end_of_streaming_inference(tmp_path):
    """`python -m mt3d_amd.inference` with postprocess: {components, mesh, orient} on the 32^3 store of the mesh tests, in a fresh
    child process: the `_front` file exists, reads back, and is the statement applied to the mesher's file and `normals_final`"""
    _, _, pp = _mods()
    from mt3d_amd.dataloading import zarr_lite
    script = tmp_path / "child.py"
    script.write_text(CHILD)
    r = subprocess.run([sys.executable, str(script), ROOT, str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    store = dict(ln.split(" ", 1) for ln in r.stdout.splitlines() if ln.startswith("STORE "))["STORE"]
    v, t, _ = pp.read_mesh(os.path.join(store, "sheet_filtered.obj"))
    gv, gt, gn = pp.read_mesh(os.path.join(store, "sheet_filtered_front.obj"))
    assert len(v) > 0 and gn is not None and gn.shape == gv.shape and len(gt) <= len(t)
    field = zarr_lite.open(os.path.join(store, "normals_final"))[...]
    unit = pp.unit_numpy(pp.sample_points_numpy(field, v, "normal_u16")[0])
    side = pp.side_numpy(pp.face_cos_numpy(v, t, unit), 0.2)
    wv, wt, (wn,), _ = pp.select_numpy(v, t, side == 1, unit)
    assert np.array_equal(_bits(gv), _bits(wv)) and np.array_equal(gt, wt) and np.array_equal(_bits(gn), _bits(wn))
    assert f"'input_vertices': {len(v)}" in r.stdout and f"'front': {int((side == 1).sum())}" in r.stdout and "'mean_abs_cos'" in r.stdout
