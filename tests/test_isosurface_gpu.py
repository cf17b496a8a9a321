"""Surface nets on the device: ops.iso_counts / ops.iso_mesh (csrc/rx_isosurface.hip) against the numpy statement of
postprocess/isosurface.py over the shared case list, `SurfaceMesher` resident and in slabs, and the mesh at the end of streaming
inference.  Triangles compare with array_equal and vertices by their bits."""
import os

import numpy as np
import pytest
import torch

import isosurface_cases as C

pytestmark = pytest.mark.gpu


def _mods():
    import mt3d_amd  # noqa: F401
    import mt3d_amd.postprocess as pp
    from mt3d_amd.engine import lib as L
    from mt3d_amd.engine import ops
    L.require_device()
    return L, ops, pp


def _same(got, want):
    v, t = got
    return (v.dtype == torch.float32 and t.dtype == torch.int64 and tuple(v.shape) == want[0].shape and tuple(t.shape) == want[1].shape
            and np.array_equal(v.cpu().numpy().view(np.int32), want[0].view(np.int32)) and np.array_equal(t.cpu().numpy(), want[1]))


@pytest.mark.parametrize("level", C.LEVELS)
def test_mesh_and_counts_every_case(level):
    _, ops, pp = _mods()
    cases = [(name, v) for name, lv, v in C.cases() if lv == level]
    got = []
    for name, v in cases:
        d = torch.from_numpy(v).cuda()
        got.append((ops.iso_counts(d, level), ops.iso_mesh(d, level), ops.iso_mesh(d, level)))
    torch.cuda.synchronize()
    for (name, v), (counts, a, b) in zip(cases, got):
        want = pp.surface_nets_numpy(v, level)
        assert counts == pp.counts_numpy(v, level) == (len(want[0]), len(want[1])), name
        assert _same(a, want), name
        assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1], b[1]), name      # twice: the same bytes


def test_vertex_base_out_and_storage():
    _, ops, pp = _mods()
    v = dict(C.volumes((33, 17, 70), 127))["random50"]
    want = pp.surface_nets_numpy(v, 127)
    d = torch.from_numpy(v).cuda()
    base = 2**40 + 5
    got = ops.iso_mesh(d, 127, vertex_base=base)
    assert _same(got, (want[0], want[1] + base))
    out = (torch.full((len(want[0]), 3), -7.0, device="cuda"), torch.full((len(want[1]), 3), -7, dtype=torch.int64, device="cuda"))
    res = ops.iso_mesh(d, 127, out=out)
    assert res[0] is out[0] and res[1] is out[1] and _same(out, want)
    wide = torch.from_numpy(np.ascontiguousarray(np.stack([v, v], -1))).cuda()[..., 0]      # not contiguous: made so by the wrapper
    assert _same(ops.iso_mesh(wide, 127), want)
    assert ops.iso_mesh(d, 127, window=None, z_base=0)[0].shape == want[0].shape
    shifted = pp.surface_nets_numpy(v, 127, z_base=1000)
    assert not np.array_equal(shifted[0], want[0]) and _same(ops.iso_mesh(d, 127, z_base=1000), shifted)


def test_refusals():
    L, ops, _ = _mods()
    v = torch.zeros((4, 5, 6), dtype=torch.uint8, device="cuda")
    for bad in (v.cpu(), v.float(), v[0], v[None], v[:0]):
        with pytest.raises(L.RxError, match="surface_nets_numpy|uint8"):
            ops.iso_mesh(bad)
        with pytest.raises(L.RxError):
            ops.iso_counts(bad)
    for level in (-1, 255, 1.5, True):
        with pytest.raises(L.RxError, match="level"):
            ops.iso_mesh(v, level)
    with pytest.raises(L.RxError, match="vertex_base"):
        ops.iso_mesh(v, 127, vertex_base=-1)
    with pytest.raises(L.RxError, match="out"):
        ops.iso_mesh(v + 255, 127, out=(torch.zeros((1, 3), device="cuda"), torch.zeros((1, 3), dtype=torch.int64, device="cuda")))
    with pytest.raises(L.RxError, match="window"):
        ops.iso_mesh(v, 127, window=(2, 1, 3))
    # the library's own limits, refused with a status before any launch (no device memory is touched: the pointers are never read)
    from ctypes import c_void_p
    so, p = L.load(), c_void_p(v.data_ptr())
    for z, y, x, word in ((2**24 - 2, 1, 1, "2^24 - 2"), (1, 1, 2**24 - 2, "2^24 - 2"), (1 << 11, 1 << 10, 1 << 10, "cells"), (0, 4, 4, "positive"),
                          (30000, 30000, 1, "bands")):      # 7501 x 3751 workgroups of 256 threads: more than 2^32 threads in a launch
        assert so.rx_iso_classify(p, 127, z, y, x, 0, z + 1, p, p, None) != 0 and word.encode() in so.rx_last_error(), (z, y, x)
        assert so.rx_iso_emit(p, 127, z, y, x, 0, p, p, 0, 0, 0, 0, 1, 1, p, p, None) != 0 and word.encode() in so.rx_last_error(), (z, y, x)
    assert so.rx_iso_classify(None, 127, 4, 5, 6, 0, 5, p, p, None) != 0 and b"null" in so.rx_last_error()
    assert so.rx_iso_classify(p, 255, 4, 5, 6, 0, 5, p, p, None) != 0 and b"level" in so.rx_last_error()
    assert so.rx_iso_classify(p, 127, 4, 5, 6, 0, 6, p, p, None) != 0 and b"cell planes" in so.rx_last_error()
    assert so.rx_iso_scan(p, 0, p, p, None) != 0 and b"cell rows" in so.rx_last_error()
    assert so.rx_iso_scan(p, 4, None, p, None) != 0 and b"null" in so.rx_last_error()
    assert so.rx_iso_emit(p, 127, 4, 5, 6, 2**24 - 6, p, p, 0, 0, 0, 0, 1, 1, p, p, None) != 0 and b"z_base" in so.rx_last_error()


def _store(tmp_path, name, values, array="sheet_filtered"):
    from mt3d_amd.dataloading import zarr_lite
    store = tmp_path / name
    os.makedirs(store)
    zarr_lite.write_array(str(store / array), values, (8, 16, 16), compressor="zlib")
    return str(store)


def test_surface_mesher_resident_and_in_slabs(tmp_path):
    _, _, pp = _mods()
    values = C.ball((40, 40, 130))
    want = pp.surface_nets_numpy(values, 127)
    files = {}
    for name, kw in (("host", dict(mesher=pp.surface_nets_numpy)), ("resident", {}), ("slab2", dict(slab=2)), ("slab5", dict(slab=5))):
        store = _store(tmp_path, name, values)
        m = pp.SurfaceMesher(127, "obj", **kw)
        summary = m.run(store, "sheet")
        assert summary == dict(level=127, vertices=len(want[0]), triangles=len(want[1]),
                               slabs={"host": 1, "resident": 1, "slab2": 21, "slab5": 9}[name]), name
        files[name] = open(os.path.join(store, "sheet_filtered.obj"), "rb").read()
        assert sorted(os.listdir(store)) == ["sheet_filtered", "sheet_filtered.obj"], name
    assert files["host"] == files["resident"] == files["slab2"] == files["slab5"] and len(files["host"]) > 1000
    from mt3d_amd.tasks.normals.mesh_targets import read_obj
    v, t = read_obj(os.path.join(store, "sheet_filtered.obj"))
    assert np.array_equal(v.view(np.int32), want[0].view(np.int32)) and np.array_equal(t, want[1])


@pytest.mark.parametrize("kind", ["slab", "full", "random50"])
def test_device_slabs_when_the_first_cell_planes_hold_vertices(tmp_path, kind):
    """the surface touches the z = 0 face, so cell plane 0 holds vertices: the slab that begins at cell plane 2 still loads the
    volume's first voxel plane, and its ids must count from plane 1, not from plane 0.  Depths 1, 2 and 3 put a slab start at cell
    planes 1, 2 and 3; every file is the resident file, byte for byte, which is the statement's."""
    _, _, pp = _mods()
    values = dict(C.volumes((9, 10, 70), 127))[kind]
    want = pp.surface_nets_numpy(values, 127)
    assert (want[0][:, 2] < 0).any()      # vertices in cell plane 0
    reference = tmp_path / "statement.obj"
    pp.write_obj(str(reference), *want)
    for slab in (None, 1, 2, 3):
        store = _store(tmp_path, f"{kind}{slab}", values)
        summary = pp.SurfaceMesher(127, "obj", slab=slab).run(store, "sheet")
        assert summary["vertices"] == len(want[0]) and summary["triangles"] == len(want[1]), slab
        assert open(os.path.join(store, "sheet_filtered.obj"), "rb").read() == open(reference, "rb").read(), slab
    # the smallest depth the budget gives: two cell planes, four voxel planes
    store = _store(tmp_path, f"{kind}budget", values)
    m = pp.SurfaceMesher(127, "obj", max_device_bytes=pp.SurfaceMesher.slab_bytes(4, 10, 70))
    m.run(store, "sheet")
    assert m.last_slab == 2 and open(os.path.join(store, "sheet_filtered.obj"), "rb").read() == open(reference, "rb").read()


def test_mesh_at_the_end_of_streaming_inference(tmp_path, capsys):
    """`python -m mt3d_amd.inference` with postprocess: {components, mesh}: the mesh written is the statement's mesh of `sheet_filtered`"""
    _, _, pp = _mods()
    import yaml
    from mt3d_amd import inference
    from mt3d_amd.builders.build_network_from_config import NetworkFromConfig
    from mt3d_amd.configuration.config_manager import ConfigManager
    from mt3d_amd.dataloading import zarr_lite
    def cfg(name, ic):
        c = {"tr_setup": {}, "tr_config": {"patch_size": [16, 16, 16], "batch_size": 2}, "model_config": {},
             "dataset_config": {"targets": {"sheet": {"channels": 1, "activation": "sigmoid"}}}, "inference_config": ic}
        p = tmp_path / f"{name}.yaml"
        p.write_text(yaml.safe_dump(c))
        return str(p)
    vol = np.random.default_rng(4).integers(0, 256, (32, 32, 32)).astype(np.uint8)
    src = zarr_lite.write_array(str(tmp_path / "vol.zarr"), vol, (16, 16, 16), compressor="zlib")
    base = {"checkpoint_path": str(tmp_path / "model.pt"), "input_path": str(src.path), "overlap": 0.5}
    torch.manual_seed(3)
    torch.save({"model": NetworkFromConfig(ConfigManager(cfg("plain", base), verbose=False)).cuda().state_dict()}, base["checkpoint_path"])
    plain = inference.main(["--config_path", cfg("plain", {**base, "output_path": str(tmp_path / "a")})])
    assert not os.path.exists(os.path.join(plain, "sheet_final.obj"))      # without the key nothing more is written
    level = min(int(np.median(zarr_lite.open(os.path.join(plain, "sheet_final"))[...])), 254)      # leaves voxels on both sides
    block = {"components": {"tasks": ["sheet"], "level": level, "min_voxels": 4},
             "mesh": {"tasks": ["sheet"], "source": "filtered", "level": level, "format": "obj", "max_device_gb": 8}}
    capsys.readouterr()
    store = inference.main(["--config_path", cfg("mesh", {**base, "output_path": str(tmp_path / "b"), "postprocess": block})])
    filtered = zarr_lite.open(os.path.join(store, "sheet_filtered"))[...]
    want = pp.surface_nets_numpy(filtered, level)
    assert len(want[0]) > 0
    from mt3d_amd.tasks.normals.mesh_targets import read_obj
    v, t = read_obj(os.path.join(store, "sheet_filtered.obj"))
    assert np.array_equal(v.view(np.int32), want[0].view(np.int32)) and np.array_equal(t, want[1])
    assert f"'vertices': {len(want[0])}" in capsys.readouterr().out
