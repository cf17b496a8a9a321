"""CPU: the numpy statement of label dilation (dataloading/dilate_device.py) against scipy's binary_dilation, its config block,
the dataset's host / device switch, and the C ABI of rx_label_dilate as far as it goes without a device.  Every comparison of
dilated data is exact: 0.0 / 1.0 float32, no tolerance anywhere."""
import ctypes
import itertools
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import mt3d_amd  # noqa: F401
from mt3d_amd.dataloading import dilate_device as D
from mt3d_amd.dataloading import geometry_device as G
from mt3d_amd.dataloading import zarr_lite
from mt3d_amd.dataloading.dataset import ZarrSegmentationDataset3D, _ball

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VALUES = np.array([0.0, -1.0, -0.0, np.nan, 1.0 / 255.0, 0.5, 1.0], dtype=np.float32)
ON_VALUES = np.array([1.0 / 255.0, 0.5, 1.0], dtype=np.float32)
OFF_VALUES = np.array([0.0, -1.0, -0.0, np.nan], dtype=np.float32)


def label(shape, seed, density=0.01):
    """the data recipe of the dilation tests: about `density` of the voxels on (values 1/255, 0.5, 1), the rest drawn from the
    values that count as off (0, -1, -0.0, NaN), and the 8 corner voxels of every (Z, Y, X) volume forced on"""
    rng = np.random.default_rng(seed)
    on = rng.random(shape) < density
    a = np.where(on, rng.choice(ON_VALUES, size=shape), rng.choice(OFF_VALUES, size=shape)).astype(np.float32)
    for cz, cy, cx in itertools.product((0, -1), repeat=3):
        a[..., cz, cy, cx] = 1.0
    return a


def same_01(a, b):
    """equal values and, for the zeros, equal sign bits"""
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_label_recipe_uses_every_value():
    a = label((20, 23, 70), 0)
    assert np.isnan(a).any() and (a == -1).any() and np.signbit(a[a == 0]).any() and not np.signbit(a[a == 0]).all()
    assert {float(v) for v in ON_VALUES} <= set(np.unique(a[a > 0]).tolist())


def test_ball_runs():
    runs = D.ball_runs(5)
    assert len(runs) == 81 and sum(2 * h + 1 for _, _, h in runs) == 515
    assert runs == sorted(runs) and sorted({h for _, _, h in runs}) == [0, 2, 3, 4, 5]
    assert len(D.ball_runs(8)) == 197
    for bad in (0, 9, 2.0, True, "5"):
        with pytest.raises(ValueError, match="radius"):
            D.ball_runs(bad)


@pytest.mark.parametrize("r", [1, 2, 5, 8])
def test_ball_is_the_dataset_ball(r):
    b = D.ball(r)
    assert b.dtype == bool and b.shape == (2 * r + 1,) * 3 and np.array_equal(b, _ball(r))


@pytest.mark.parametrize("r", [1, 2, 5, 8])
@pytest.mark.parametrize("shape", [(20, 23, 70), (3, 4, 5), (1, 12, 64), (2, 13, 11, 130)])
def test_dilate_numpy_is_scipy_binary_dilation(shape, r):
    ndi = pytest.importorskip("scipy.ndimage")
    a = label(shape, 7 * r + len(shape))
    got = D.dilate_numpy(a, r)
    assert got.dtype == np.float32 and got.shape == a.shape
    with np.errstate(invalid="ignore"):
        on = a > 0
    vols = on if a.ndim == 3 else list(on)
    want = (ndi.binary_dilation(vols, structure=_ball(r)) if a.ndim == 3
            else np.stack([ndi.binary_dilation(v, structure=_ball(r)) for v in vols]))
    assert same_01(got, want.astype(np.float32))


def test_a_single_voxel_becomes_the_ball_and_nothing_stays_nothing():
    a = np.zeros((11, 11, 11), dtype=np.float32)
    assert same_01(D.dilate_numpy(a, 5), a)
    off = np.full((5, 6, 70), -0.0, dtype=np.float32)
    off[1, 2, 3], off[2, 2, 2] = np.nan, -1.0
    assert same_01(D.dilate_numpy(off, 8), np.zeros_like(off))          # +0.0 out, whatever counted as off
    a[5, 5, 5] = 1.0 / 255.0
    assert same_01(D.dilate_numpy(a, 5), D.ball(5).astype(np.float32))
    with pytest.raises(ValueError):
        D.dilate_numpy(np.zeros((4, 4)), 5)


def all_ops():
    ops = [G.GeomOp(src, flip) for src in itertools.permutations(range(3)) for flip in itertools.product((0, 1), repeat=3)]
    assert len(set(ops)) == 48
    return ops


def test_dilation_commutes_with_every_signed_axis_permutation():
    """the ball is invariant under all 48 of them, so the device stages (dilate, then geometry) may run in either order"""
    a = label((12, 12, 12), 3, density=0.004)
    d = D.dilate_numpy(a, 5)
    assert 0 < d.sum() < d.size
    for op in all_ops():
        assert same_01(D.dilate_numpy(G.apply_op_numpy(op, a, False), 5), G.apply_op_numpy(op, d, False)), op


# ---- dataset_config.dilate --------------------------------------------------------------------------------------------------------
TASKS = {"sheet": {"channels": 1}, "Normals": {"channels": 3}, "ink": {"channels": 1}}


def test_parse_dilate():
    assert D.parse_dilate({}, True, TASKS) == {"radius": 5, "where": "host", "keys": ["sheet", "ink"]}
    assert D.parse_dilate(None, True, TASKS) == {"radius": 5, "where": "host", "keys": ["sheet", "ink"]}
    assert D.parse_dilate({"dilate": {"where": "device", "radius": 3}}, True, TASKS) == {"radius": 3, "where": "device", "keys": ["sheet", "ink"]}
    assert D.parse_dilate({"dilate": {"where": "Device"}}, True, {"normals": {}}) == {"radius": 5, "where": "device", "keys": []}
    # the reference's switch rules: off means off, whatever the block says (a malformed one included)
    assert D.parse_dilate({"dilate": {"where": "device", "radius": 5}}, False, TASKS) is None
    assert D.parse_dilate({"dilate": {"where": "nowhere", "bogus": 1}}, False, TASKS) is None
    for block, key in [({"where": "device", "size": 5}, r"dataset_config\.dilate: unknown key\(s\) \['size'\]"),
                       ({"where": "gpu"}, r"dataset_config\.dilate\.where"), ({"where": None}, r"dataset_config\.dilate\.where"),
                       ({"radius": 0}, r"dataset_config\.dilate\.radius"), ({"radius": 9}, r"dataset_config\.dilate\.radius"),
                       ({"radius": 5.0}, r"dataset_config\.dilate\.radius"), ({"radius": "5"}, r"dataset_config\.dilate\.radius"),
                       ({"radius": True}, r"dataset_config\.dilate\.radius"), ("device", r"dataset_config\.dilate: expected a mapping")]:
        with pytest.raises(ValueError, match=key):
            D.parse_dilate({"dilate": block}, True, TASKS)


def _volume(tmp_path):
    """a wavy sheet about 3 voxels thick (uint8 0 / 255) with an image and a normals volume beside it"""
    rng = np.random.default_rng(5)
    n = 40
    z, y, x = np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij")
    sheet = np.abs(((y + 5 * np.sin(x / 6.0) + 3 * np.cos(z / 5.0)) % 14) - 7) < 1.5
    img = rng.integers(0, 255, size=sheet.shape, dtype=np.uint8)
    nrm = rng.integers(0, 65535, size=(n, n, n, 3), dtype=np.uint16)
    paths = {}
    for name, arr, ch in [("img", img, (16, 16, 16)), ("sheet", (sheet * 255).astype(np.uint8), (16, 16, 16)),
                          ("normals", nrm, (16, 16, 16, 3))]:
        paths[name] = str(tmp_path / f"{name}.zarr")
        zarr_lite.write_array(paths[name], arr, ch, compressor="zlib")
    return paths


def _mgr(tmp_path, paths, dilate_label=True, **dataset_config):
    tasks = {"sheet": {"channels": 1}, "normals": {"channels": 3}}
    return SimpleNamespace(model_name="m", tasks=tasks, train_patch_size=(16, 20, 24), min_labeled_ratio=0.05, min_bbox_percent=0.5,
                           dilate_label=dilate_label, use_cache=False, cache_folder=str(tmp_path / "cache"),
                           dataset_config=dict(augment=False, **dataset_config),
                           volume_paths=[{"input": paths["img"], "sheet": paths["sheet"], "normals": paths["normals"], "ref_label": "sheet"}])


def test_dataset_host_and_device_switch(tmp_path):
    pytest.importorskip("scipy")
    paths = _volume(tmp_path)
    absent = ZarrSegmentationDataset3D(_mgr(tmp_path, paths))
    host = ZarrSegmentationDataset3D(_mgr(tmp_path, paths, dilate={"where": "host"}))
    dev = ZarrSegmentationDataset3D(_mgr(tmp_path, paths, dilate={"where": "device", "radius": 5}))
    off = ZarrSegmentationDataset3D(_mgr(tmp_path, paths, dilate_label=False, dilate={"where": "device"}))
    raw = ZarrSegmentationDataset3D(_mgr(tmp_path, paths, dilate_label=False))
    host2 = ZarrSegmentationDataset3D(_mgr(tmp_path, paths, dilate={"radius": 2}))
    assert absent.device_dilate is None and host.device_dilate is None and off.device_dilate is None
    assert absent.dilate == {"radius": 5, "where": "host", "keys": ["sheet"]}
    assert dev.device_dilate == {"radius": 5, "where": "device", "keys": ["sheet"]}
    assert len(absent) == len(dev) > 1
    for i in (0, len(dev) - 1):
        a, h, d, o, r, h2 = absent[i], host[i], dev[i], off[i], raw[i], host2[i]
        for k in ("image", "sheet", "normals"):
            assert same_01(a[k].numpy(), h[k].numpy())                      # no block == where: host, bit for bit
            assert same_01(d[k].numpy(), r[k].numpy()) and same_01(o[k].numpy(), r[k].numpy())      # where: device == raw items
        for k in ("image", "normals"):
            assert same_01(d[k].numpy(), h[k].numpy())                      # only the label targets differ
        z0, y0, x0 = dev.all_valid_patches[i]["start_pos"]
        lab = zarr_lite.open(paths["sheet"])[z0:z0 + 16, y0:y0 + 20, x0:x0 + 24]
        assert d["sheet"].shape == (1, 16, 20, 24) and same_01(d["sheet"][0].numpy(), lab.astype(np.float32) / 255.0)
        assert 0 < float(d["sheet"].sum()) < float(h["sheet"].sum())
        assert same_01(D.dilate_numpy(d["sheet"].numpy(), 5), h["sheet"].numpy())      # the device stage's statement == the host item
        assert same_01(D.dilate_numpy(d["sheet"].numpy(), 2), h2["sheet"].numpy())
    for block, key in [({"where": "both"}, r"dilate\.where"), ({"radius": 12}, r"dilate\.radius"), ({"ball": 5}, r"unknown key")]:
        with pytest.raises(ValueError, match=key):
            ZarrSegmentationDataset3D(_mgr(tmp_path, paths, dilate=block))


def test_device_dilate_refuses_host_tensors():
    from mt3d_amd.engine import ops as E
    from mt3d_amd.engine.lib import RxError
    batch = {"image": torch.zeros(1, 1, 4, 4, 4), "sheet": torch.zeros(1, 1, 4, 4, 4)}
    with pytest.raises(RxError, match="sheet"):
        D.DeviceDilate(["sheet"], 5)(batch)
    with pytest.raises(RxError, match="ink"):
        D.DeviceDilate(["ink"], 5)(batch)
    with pytest.raises(RxError, match="label_dilate"):
        E.label_dilate(batch["sheet"], 5)
    with pytest.raises(ValueError, match="radius"):
        D.DeviceDilate(["sheet"], 9)


# ---- the C ABI, as far as it goes without a device -----------------------------------------------------------------------------------
def test_entry_points_are_declared_exported_and_bound():
    from mt3d_amd.engine import lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rxunet.h")).read(), flags=re.S)
    so = ctypes.CDLL(lib.LIB_PATH)
    for name in ("rx_label_dilate", "rx_dilate_workspace"):
        assert re.search(rf"\b{name}\s*\(", hdr) and hasattr(so, name) and name in lib.exported_symbols()
    L = lib.load()
    assert L.rx_dilate_workspace(2, 1, 3, 4, 70) == 2 * 3 * 4 * 2 * 8
    assert L.rx_dilate_workspace(1, 1, 128, 128, 128) == 128 * 128 * 2 * 8
    assert L.rx_dilate_workspace(1, 1, 1, 1, 64) == 8 and L.rx_dilate_workspace(1, 1, 1, 1, 65) == 16
    for bad in [(0, 1, 3, 4, 70), (2, 1, 3, 4, 0), (2, -1, 3, 4, 70)]:
        assert L.rx_dilate_workspace(*bad) == 0
    # refused on the host, before any device call: the status and the entry's name
    assert L.rx_label_dilate(None, None, None, 0, 1, 1, 4, 4, 4, 5, None) == -1
    assert b"rx_label_dilate" in L.rx_last_error()
