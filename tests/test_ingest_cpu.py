"""CPU: the numpy statement of ingest (dataloading/ingest_device.py) against the unchanged host `__getitem__`, its config block, the
dataset's host / device switch, and the C ABI of rx_ingest as far as it goes without a device.  Every comparison of data is on
the float32 bit patterns: no tolerance anywhere."""
import ctypes
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import mt3d_amd  # noqa: F401
from mt3d_amd.dataloading import ingest_device as I
from mt3d_amd.dataloading import zarr_lite
from mt3d_amd.dataloading.dataset import ZarrSegmentationDataset3D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATCH = (8, 10, 12)


def same_bits(a, b):
    """equal shapes and equal float32 bit patterns"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype == np.float32 and a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def write_volume(tmp, image_dtype=np.uint8, normals_dtype=np.uint16, sheet_dtype=np.uint8, n=24, tag=""):
    """an n^3 volume as zarr_lite stores: a slab label (so every half-stride patch is valid), an image and channels-last normals,
    each holding the extremes of its dtype"""
    rng = np.random.default_rng(11)
    shape = (n, n, n)
    sheet = np.ones(shape, dtype=bool)
    sheet[:, :, ::5] = False

    def draw(dt, sh):
        if np.dtype(dt) == np.float32:
            return rng.random(sh, dtype=np.float32)
        hi = np.iinfo(dt).max
        a = rng.integers(0, hi, size=sh, endpoint=True).astype(dt)
        a.flat[:3] = (0, 1, hi)
        return a
    img, nrm = draw(image_dtype, shape), draw(normals_dtype, shape + (3,))
    lab = (sheet * (1.0 if np.dtype(sheet_dtype) == np.float32 else np.iinfo(sheet_dtype).max)).astype(sheet_dtype)
    os.makedirs(tmp, exist_ok=True)
    paths = {k: os.path.join(tmp, f"{k}{tag}.zarr") for k in ("img", "sheet", "normals")}
    zarr_lite.write_array(paths["img"], img, (16, 16, 16), compressor="zlib")
    zarr_lite.write_array(paths["sheet"], lab, (16, 16, 16), compressor="zlib")
    zarr_lite.write_array(paths["normals"], nrm, (16, 16, 16, 3), compressor="zlib")
    return paths


def mgr(tmp, paths, dilate_label=False, patch=PATCH, **dataset_config):
    tasks = {"sheet": {"channels": 1}, "normals": {"channels": 3}}
    vols = paths if isinstance(paths, list) else [paths]
    return SimpleNamespace(model_name="m", tasks=tasks, train_patch_size=patch, min_labeled_ratio=0.05, min_bbox_percent=0.5,
                           dilate_label=dilate_label, use_cache=False, cache_folder=os.path.join(str(tmp), "cache"),
                           dataset_config=dict({"augment": False}, **dataset_config),
                           volume_paths=[{"input": p["img"], "sheet": p["sheet"], "normals": p["normals"], "ref_label": "sheet"} for p in vols])


def test_rules_and_their_codes():
    assert I.RULES == ("copy", "div255", "div65535", "normal_u16", "normal_mul2")
    from mt3d_amd.engine import lib
    assert [lib.RX_INGEST_COPY, lib.RX_INGEST_DIV255, lib.RX_INGEST_DIV65535, lib.RX_INGEST_NORMAL_U16,
            lib.RX_INGEST_NORMAL_MUL2] == [I.rule_code(r) for r in I.RULES] == [0, 1, 2, 3, 4]
    hdr = open(os.path.join(ROOT, "include", "rxunet.h")).read()
    for i, r in enumerate(I.RULES):
        assert re.search(rf"RX_INGEST_{r.upper()} = {i}\b", hdr)
    assert I.rule_code("DIV255") == 1 and I.rule_code(np.int64(3)) == 3
    for bad in ("div256", 5, -1, True, None, 1.0):
        with pytest.raises(ValueError, match="rule"):
            I.rule_code(bad)
    assert I.ingest_rule("image", np.uint8) == "div255" and I.ingest_rule("image", "<u2") == "div65535"
    assert I.ingest_rule("image", np.float32) == "copy" and I.ingest_rule("sheet", np.uint8) == "div255"
    assert I.ingest_rule("Normals", np.uint16) == "normal_u16"
    assert I.ingest_rule("normals", np.uint8) == "normal_mul2" and I.ingest_rule("normals", np.float32) == "normal_mul2"


def test_ingest_numpy_statement():
    a = np.array([[[0, 1, 255]]], dtype=np.uint8)
    assert same_bits(I.ingest_numpy(a, "div255"), (a.astype(np.float32) / np.float32(255.0))[None])
    assert same_bits(I.ingest_numpy(a, "normal_mul2"), np.array([[[[-1.0, 1.0, 509.0]]]], dtype=np.float32))
    u = np.arange(2 * 3 * 4 * 3, dtype=np.uint16).reshape(2, 3, 4, 3) * 911
    got = I.ingest_numpy(u, "normal_u16")
    assert got.shape == (3, 2, 3, 4) and got.flags.c_contiguous
    for c in range(3):
        assert same_bits(got[c], u[..., c].astype(np.float32) / np.float32(32767.5) - np.float32(1.0))
    f = np.array([[[-0.0, np.nan, np.inf, 1e-45]]], dtype=np.float32)
    f.view(np.uint32)[0, 0, 1] = 0x7fc12345
    assert same_bits(I.ingest_numpy(f, "copy"), f[None])
    with pytest.raises(ValueError):
        I.ingest_numpy(np.zeros((4, 4)), "copy")


@pytest.mark.parametrize("image_dtype,normals_dtype,sheet_dtype", [(np.uint8, np.uint16, np.uint8), (np.uint16, np.float32, np.uint16),
                                                                   (np.float32, np.uint8, np.float32)])
def test_raw_items_through_ingest_numpy_are_the_host_items(tmp_path, image_dtype, normals_dtype, sheet_dtype):
    """uint8 / uint16 / float32 image and label, uint16 / float32 / uint8 channels-last normals: ingest_numpy of the raw slice
    under ingest_rule(key, dtype) has the bits of the unchanged host __getitem__"""
    paths = write_volume(str(tmp_path), image_dtype, normals_dtype, sheet_dtype)
    host = ZarrSegmentationDataset3D(mgr(tmp_path, paths))
    dev = ZarrSegmentationDataset3D(mgr(tmp_path, paths, ingest={"where": "device"}))
    dts = {"image": image_dtype, "sheet": sheet_dtype, "normals": normals_dtype}
    assert host.device_ingest is None and host.ingest == {"where": "host"}
    assert dev.device_ingest == {k: I.ingest_rule(k, dt) for k, dt in dts.items()}
    assert len(host) == len(dev) > 1 and host.all_valid_patches == dev.all_valid_patches
    stores = {"image": zarr_lite.open(paths["img"]), "sheet": zarr_lite.open(paths["sheet"]), "normals": zarr_lite.open(paths["normals"])}
    for i in (0, len(dev) - 1):
        h, d = host[i], dev[i]
        z0, y0, x0 = dev.all_valid_patches[i]["start_pos"]
        assert set(h) == set(d) == set(dts)
        for k, dt in dts.items():
            raw = d[k].numpy()
            assert raw.dtype == np.dtype(dt) and raw.shape == PATCH + ((3,) if k == "normals" else ())      # what the store holds
            assert np.array_equal(raw, stores[k][z0:z0 + PATCH[0], y0:y0 + PATCH[1], x0:x0 + PATCH[2]])
            assert h[k].dtype == torch.float32 and h[k].shape == ((3,) if k == "normals" else (1,)) + PATCH
            assert same_bits(I.ingest_numpy(raw, dev.device_ingest[k]), h[k].numpy()), (k, dt)


def test_parse_ingest():
    assert I.parse_ingest({}) == {"where": "host"} and I.parse_ingest(None) == {"where": "host"}
    assert I.parse_ingest({"ingest": None}) == {"where": "host"} and I.parse_ingest({"ingest": {}}) == {"where": "host"}
    assert I.parse_ingest({"ingest": {"where": "Device"}}) == {"where": "device"}
    for block, key in [({"where": "device", "dtype": "u8"}, r"dataset_config\.ingest: unknown key\(s\) \['dtype'\]"),
                       ({"where": "gpu"}, r"dataset_config\.ingest\.where"), ({"where": None}, r"dataset_config\.ingest\.where"),
                       ({"where": True}, r"dataset_config\.ingest\.where"), ("device", r"dataset_config\.ingest: expected a mapping")]:
        with pytest.raises(ValueError, match=key):
            I.parse_ingest({"ingest": block})


def test_absent_block_and_where_host_are_the_items_of_before(tmp_path):
    """the key absent, `where: host`, and the conversion spelled out here as the parent's __getitem__ has it: the same bits"""
    paths = write_volume(str(tmp_path))
    absent = ZarrSegmentationDataset3D(mgr(tmp_path, paths))
    host = ZarrSegmentationDataset3D(mgr(tmp_path, paths, ingest={"where": "host"}))
    assert absent.device_ingest is None and host.device_ingest is None
    for i in range(len(absent)):
        a, h = absent[i], host[i]
        z0, y0, x0 = absent.all_valid_patches[i]["start_pos"]
        sl = np.s_[z0:z0 + PATCH[0], y0:y0 + PATCH[1], x0:x0 + PATCH[2]]
        img = zarr_lite.open(paths["img"])[sl].astype(np.float32)
        img /= 255.0
        lab = zarr_lite.open(paths["sheet"])[sl].astype(np.float32)
        lab /= 255.0
        nrm = ((zarr_lite.open(paths["normals"])[sl].astype(np.float32) / 32767.5) - 1.0).transpose(3, 0, 1, 2).copy()
        for k, want in (("image", img[None]), ("sheet", lab[None]), ("normals", nrm)):
            assert same_bits(a[k].numpy(), want) and same_bits(h[k].numpy(), want), k


def test_dataset_refuses_host_stages_that_need_scaled_floats(tmp_path):
    paths = write_volume(str(tmp_path))
    ing = {"where": "device"}
    geo_host = {"where": "host", "flip": {"p": 0.5}}
    geo_dev = {"where": "device", "flip": {"p": 0.5}}
    for kw, key in [(dict(augment="restated"), r"dataset_config\.augment"),
                    (dict(geometric=geo_host), r"dataset_config\.geometric"),
                    (dict(dilate_label=True), r"dataset_config\.dilate"),
                    (dict(dilate_label=True, dilate={"where": "host"}), r"dataset_config\.dilate")]:
        with pytest.raises(ValueError, match=key):
            ZarrSegmentationDataset3D(mgr(tmp_path, paths, ingest=ing, **kw))
    for block, key in [({"where": "both"}, r"ingest\.where"), ({"rule": "copy"}, r"unknown key")]:
        with pytest.raises(ValueError, match=key):
            ZarrSegmentationDataset3D(mgr(tmp_path, paths, ingest=block))
    # every accepted combination: the stages off, or on the device
    for kw in (dict(), dict(augment="device"), dict(geometric=geo_dev), dict(dilate_label=True, dilate={"where": "device"}),
               dict(dilate_label=False, dilate={"where": "host"})):
        ds = ZarrSegmentationDataset3D(mgr(tmp_path, paths, ingest=ing, **kw))
        assert ds.device_ingest == {"image": "div255", "sheet": "div255", "normals": "normal_u16"}
        assert ds[0]["image"].dtype == torch.uint8 and ds[0]["normals"].dtype == torch.uint16


def test_dataset_refuses_volumes_that_disagree_and_foreign_dtypes(tmp_path):
    a = write_volume(str(tmp_path / "a"))
    b = write_volume(str(tmp_path / "b"), image_dtype=np.uint16)
    with pytest.raises(ValueError, match=r"'image' is uint8 .* volume 0 and uint16 .* volume 1"):
        ZarrSegmentationDataset3D(mgr(tmp_path, [a, b], ingest={"where": "device"}))
    ZarrSegmentationDataset3D(mgr(tmp_path, [a, b]))                                  # the host path converts each on its own
    c = dict(a)
    c["normals"] = os.path.join(str(tmp_path), "n3.zarr")                             # (Z, Y, X) normals against (Z, Y, X, 3)
    zarr_lite.write_array(c["normals"], np.zeros((24, 24, 24), dtype=np.uint16), (16, 16, 16), compressor="zlib")
    with pytest.raises(ValueError, match=r"'normals' is uint16 with 4 dimensions in volume 0 and uint16 with 3 in volume 1"):
        ZarrSegmentationDataset3D(mgr(tmp_path, [a, c], ingest={"where": "device"}))
    d = dict(a)
    d["img"] = os.path.join(str(tmp_path), "i16.zarr")
    zarr_lite.write_array(d["img"], np.zeros((24, 24, 24), dtype=np.int16), (16, 16, 16), compressor="zlib")
    with pytest.raises(ValueError, match=r"'image' of volume 0 is int16"):
        ZarrSegmentationDataset3D(mgr(tmp_path, d, ingest={"where": "device"}))


def test_raw_items_collate_in_their_own_dtype(tmp_path):
    """default_collate and the pinned ring both keep uint8 / uint16: the batch is as wide as the store"""
    from torch.utils.data import default_collate
    from mt3d_amd.train import PinnedRingCollate
    paths = write_volume(str(tmp_path))
    dev = ZarrSegmentationDataset3D(mgr(tmp_path, paths, ingest={"where": "device"}))
    items = [dev[0], dev[1]]
    for collate in (default_collate, PinnedRingCollate(depth=2)):
        batch = collate(items)
        assert batch["image"].dtype == torch.uint8 and batch["image"].shape == (2,) + PATCH
        assert batch["normals"].dtype == torch.uint16 and batch["normals"].shape == (2,) + PATCH + (3,)
        for j in range(2):
            for k in items[j]:
                assert np.array_equal(batch[k][j].numpy(), items[j][k].numpy())


def test_device_ingest_and_the_wrapper_refuse_host_tensors():
    from mt3d_amd.engine import ops as E
    from mt3d_amd.engine.lib import RxError
    stage = I.DeviceIngest({"image": "div255", "normals": 3})
    assert stage.rules == {"image": "div255", "normals": "normal_u16"}
    batch = {"image": torch.zeros(1, 4, 4, 4, dtype=torch.uint8), "normals": torch.zeros(1, 4, 4, 4, 3, dtype=torch.uint16)}
    with pytest.raises(RxError, match="image"):
        stage(batch)
    with pytest.raises(RxError, match="no rule"):
        I.DeviceIngest({})({"image": batch["image"]})
    with pytest.raises(RxError, match="ingest"):
        E.ingest(batch["image"], "div255")
    with pytest.raises(ValueError, match="rule"):
        I.DeviceIngest({"image": "div256"})


# ---- the C ABI, as far as it goes without a device -----------------------------------------------------------------------------------
def test_entry_point_is_declared_exported_and_bound():
    from mt3d_amd.engine import lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rxunet.h")).read(), flags=re.S)
    so = ctypes.CDLL(lib.LIB_PATH)
    assert re.search(r"\brx_ingest\s*\(", hdr) and hasattr(so, "rx_ingest") and "rx_ingest" in lib.exported_symbols()


def test_bad_arguments_are_refused_on_the_host():
    """refused before any device call: the status and the entry's name (addresses are never dereferenced)"""
    from mt3d_amd.engine import lib
    L = lib.load()
    assert L.rx_ingest(None, 0, None, 1, 4, 4, 4, 1, 0, None) == -1
    assert L.rx_last_error().startswith(b"rx_ingest:")
    i, o = 0x10000, 0x20000
    refused = {
        "null in": (None, 0, o, 1, 4, 4, 4, 1, 0), "null out": (i, 0, None, 1, 4, 4, 4, 1, 0), "in == out": (i, 0, i, 1, 4, 4, 4, 1, 0),
        "dtype 3": (i, 3, o, 1, 4, 4, 4, 1, 0), "dtype -1": (i, -1, o, 1, 4, 4, 4, 1, 0),
        "rule 5": (i, 0, o, 1, 4, 4, 4, 1, 5), "rule -1": (i, 0, o, 1, 4, 4, 4, 1, -1),
        "batch 0": (i, 0, o, 0, 4, 4, 4, 1, 0), "z 0": (i, 0, o, 1, 0, 4, 4, 1, 0), "y -1": (i, 0, o, 1, 4, -1, 4, 1, 0),
        "x 0": (i, 0, o, 1, 4, 4, 0, 1, 0), "c 0": (i, 0, o, 1, 4, 4, 4, 0, 0), "c 9": (i, 0, o, 1, 4, 4, 4, 9, 0),
        "2^31 elements": (i, 0, o, 1, 2048, 1024, 1024, 1, 0), "2^31 elements with c": (i, 0, o, 1, 1024, 1024, 1024, 2, 0),
        "factors that overflow 64 bits": (i, 0, o, 1, 2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1, 8, 0),
        "uint16 at an odd address": (i + 1, 1, o, 1, 4, 4, 4, 1, 0), "float32 at address 2 mod 4": (i + 2, 2, o, 1, 4, 4, 4, 1, 0),
        "out at address 2 mod 4": (i, 0, o + 2, 1, 4, 4, 4, 1, 0),
    }
    for name, args in refused.items():
        assert L.rx_ingest(*args, None) == -1, name
        assert L.rx_last_error().startswith(b"rx_ingest:"), name
