"""CPU: the valid-patch search.  The host functions (`dataset.find_label_bounding_box`, `find_valid_patches`) against a fixture of
the REAL reference's `helpers.py` (tests/golden/patch_search.npz, made by scripts/make_patch_search_fixture.py; live too where
RX_REFERENCE_ROOT points at the reference tree), the numpy statement of the device kernel (`box_stats_numpy`) plus the shared
decision code against the host search, `dataset_config.patch_search` parsing, and the C ABI as far as it goes without a device."""
import ctypes
import importlib.util
import json
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import mt3d_amd  # noqa: F401
from mt3d_amd.dataloading import patch_search_device as P
from mt3d_amd.dataloading import zarr_lite
from mt3d_amd.dataloading.dataset import ZarrSegmentationDataset3D, find_label_bounding_box, find_valid_patches
from patch_search_cases import from_stats, labels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _fixture():
    g = np.load(os.path.join(ROOT, "tests", "golden", "patch_search.npz"))
    for i in range(int(g["n_cases"])):
        yield (i, g[f"label_{int(g[f'label_of_{i}'])}"], tuple(int(v) for v in g[f"patch_{i}"]), float(g[f"thr_{i}"][0]),
               float(g[f"thr_{i}"][1]), tuple(int(v) for v in g[f"bbox_{i}"]), g[f"starts_{i}"].tolist())


def test_host_search_equals_the_reference_fixture():
    n, kept, dtypes, patches, empty = 0, 0, set(), set(), 0
    for i, lab, patch, bt, lt, bbox, starts in _fixture():
        assert find_label_bounding_box(lab) == bbox, i
        found = find_valid_patches(lab, patch, bt, lt)
        assert [p["start_pos"] for p in found] == starts, i
        assert all(p["volume_idx"] == 0 and set(p) == {"volume_idx", "start_pos"} for p in found)
        n, kept, empty = n + 1, kept + len(starts), empty + (len(starts) == 0)
        dtypes.add(lab.dtype.name), patches.add(patch)
    # the fixture covers what it says: both dtypes, an odd and an anisotropic patch, cases without a patch (an all-zero label, a
    # bounding box thinner than the patch)
    assert n >= 20 and kept > 500 and empty >= 2 and dtypes == {"uint8", "uint16"}
    assert (9, 11, 13) in patches and (8, 12, 16) in patches
    assert any(bbox[1] < 0 for _, _, _, _, _, bbox, _ in _fixture())
    assert any(bbox[1] >= 0 and bbox[3] - bbox[2] + 1 < patch[1] for _, _, patch, _, _, bbox, _ in _fixture())
    ref_root = os.environ.get("RX_REFERENCE_ROOT")
    if ref_root and os.path.exists(os.path.join(ref_root, "helpers.py")):      # the live comparison, same cases plus the seeded labels
        spec = importlib.util.spec_from_file_location("make_patch_search_fixture", os.path.join(ROOT, "scripts", "make_patch_search_fixture.py"))
        gen = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(gen)
        ref = gen.load_reference_helpers(ref_root)
        live = [(lab, patch, bt, lt) for _, lab, patch, bt, lt, _, _ in _fixture()][::4]
        live += [c for c in labels().values() if c[0].dtype != np.float32]
        for lab, patch, bt, lt in live:
            bbox, starts = gen.run_reference(ref, lab, patch, bt, lt)
            assert find_label_bounding_box(lab) == tuple(bbox.tolist())
            assert [p["start_pos"] for p in find_valid_patches(lab, patch, bt, lt)] == starts.tolist()


def _host_rules(lab, patch, bt, lt):
    """find_valid_patches with a counter at each of its three `continue`s: (kept, {rule: rejected})"""
    pZ, pY, pX = patch
    minz, maxz, miny, maxy, minx, maxx = find_label_bounding_box(lab)
    kept, rej = [], {"empty": 0, "bbox": 0, "label": 0}
    for z in range(minz, maxz - pZ + 2, max(pZ // 2, 1)):
        for y in range(miny, maxy - pY + 2, max(pY // 2, 1)):
            for x in range(minx, maxx - pX + 2, max(pX // 2, 1)):
                p = lab[z:z + pZ, y:y + pY, x:x + pX]
                with np.errstate(invalid="ignore"):
                    nz = np.argwhere(p > 0)
                if nz.size == 0:
                    rej["empty"] += 1
                    continue
                ext = nz.max(axis=0) - nz.min(axis=0) + 1
                if float(ext[0] * ext[1] * ext[2]) / p.size < bt:
                    rej["bbox"] += 1
                    continue
                if np.count_nonzero(p) / p.size < lt:
                    rej["label"] += 1
                    continue
                kept.append([z, y, x])
    return kept, rej


def test_numpy_statement_reproduces_the_host_search():
    total = {"empty": 0, "bbox": 0, "label": 0}
    for name, (lab, patch, bt, lt) in labels().items():
        want = find_valid_patches(lab, patch, bt, lt)
        # conditions of the test, on the host function alone: something is kept, and the counters are the host function's own
        kept, rej = _host_rules(lab, patch, bt, lt)
        assert len(want) > 0 and [p["start_pos"] for p in want] == kept, name
        got, rej2 = from_stats(P.box_stats_numpy, lab, patch, bt, lt)
        assert got == want and rej2 == rej, name
        count, ext = P.box_stats_numpy(lab, [[0, 0, 0, *lab.shape]])
        assert tuple(int(v) for v in ext[0]) == find_label_bounding_box(lab) and int(count[0]) == np.count_nonzero(lab)
        for k in total:
            total[k] += rej[k]
    assert min(total.values()) >= 1, total          # every rule rejects at least one candidate
    lab, patch, bt, lt = labels()["f32"]
    assert np.isnan(lab).sum() == 1 and (lab < 0).sum() > 0 and np.signbit(lab[lab == 0]).sum() == 1
    kept, rej = _host_rules(lab, patch, bt, lt)
    assert rej["empty"] >= 1                        # candidates inside the negative hole: counted voxels, no positive one


def test_box_stats_numpy_records():
    a = np.zeros((5, 6, 7), np.float32)
    a[1, 2, 3], a[4, 5, 6], a[2, 2, 2], a[3, 3, 3], a[0, 0, 1] = 1.0, 2.0, -1.0, np.nan, -0.0
    count, ext = P.box_stats_numpy(a, [[0, 0, 0, 5, 6, 7], [1, 2, 3, 1, 1, 1], [2, 2, 2, 2, 2, 2], [0, 0, 0, 1, 6, 7], [1, 1, 1, 4, 5, 6]])
    assert count.dtype == np.uint64 and ext.dtype == np.int32 and count.tolist() == [4, 1, 2, 0, 4]
    assert ext.tolist() == [[1, 4, 2, 5, 3, 6], [0, 0, 0, 0, 0, 0], [2, -1, 2, -1, 2, -1], [1, -1, 6, -1, 7, -1], [0, 3, 1, 4, 2, 5]]
    for bad in ([[0, 0, 0, 6, 6, 7]], [[0, 0, 0, 0, 1, 1]], [[-1, 0, 0, 1, 1, 1]], [[0, 0, 0, 1, 1]]):
        with pytest.raises(ValueError, match="box_stats_numpy"):
            P.box_stats_numpy(a, bad)


def test_parse_patch_search():
    assert P.parse_patch_search({}) == {"where": "host", "max_device_bytes": None}
    assert P.parse_patch_search(None) == {"where": "host", "max_device_bytes": None}
    assert P.parse_patch_search({"patch_search": {"where": "Device", "max_device_gb": 8}}) == {"where": "device", "max_device_bytes": 8 << 30}
    assert P.parse_patch_search({"patch_search": {"max_device_gb": 0.5}}) == {"where": "host", "max_device_bytes": 1 << 29}
    for block, key in [({"where": "device", "budget": 1}, r"dataset_config\.patch_search: unknown key\(s\) \['budget'\]"),
                       ({"where": "gpu"}, r"dataset_config\.patch_search\.where"), ({"where": None}, r"dataset_config\.patch_search\.where"),
                       ({"max_device_gb": 0}, r"dataset_config\.patch_search\.max_device_gb"),
                       ({"max_device_gb": -2}, r"dataset_config\.patch_search\.max_device_gb"),
                       ({"max_device_gb": "8"}, r"dataset_config\.patch_search\.max_device_gb"),
                       ({"max_device_gb": True}, r"dataset_config\.patch_search\.max_device_gb"),
                       ({"max_device_gb": float("nan")}, r"dataset_config\.patch_search\.max_device_gb"),
                       ("device", r"dataset_config\.patch_search: expected a mapping")]:
        with pytest.raises(ValueError, match=key):
            P.parse_patch_search({"patch_search": block})


def _mgr(tmp_path, cache, **dataset_config):
    lab = labels()["volume"][0]
    paths = {}
    for name, arr in [("img", (lab // 2 + 3).astype(np.uint8)), ("sheet", lab)]:
        paths[name] = str(tmp_path / f"{name}.zarr")
        if not os.path.exists(paths[name]):
            zarr_lite.write_array(paths[name], arr, (16, 16, 16), compressor="zlib")
    return SimpleNamespace(model_name="m", tasks={"sheet": {"channels": 1}}, train_patch_size=(16, 16, 16), min_labeled_ratio=0.1,
                           min_bbox_percent=0.9, dilate_label=False, use_cache=True, cache_folder=str(tmp_path / cache),
                           dataset_config=dict(augment=False, **dataset_config),
                           volume_paths=[{"input": paths["img"], "sheet": paths["sheet"], "ref_label": "sheet"}])


def test_absent_block_is_the_host_search(tmp_path):
    lab, patch, bt, lt = labels()["volume"]
    want = find_valid_patches(lab, patch, bt, lt)
    absent = ZarrSegmentationDataset3D(_mgr(tmp_path, "a"))
    host = ZarrSegmentationDataset3D(_mgr(tmp_path, "h", patch_search={"where": "host"}))
    assert absent.patch_search == host.patch_search == {"where": "host", "max_device_bytes": None}
    assert absent.all_valid_patches == host.all_valid_patches == want and len(want) > 0
    assert absent.cache_file.name == host.cache_file.name == "m_16_16_16_cache.json"
    assert absent.cache_file.read_bytes() == host.cache_file.read_bytes() == json.dumps(want).encode()
    for block, key in [({"where": "both"}, r"patch_search\.where"), ({"max_device_gb": 0}, r"max_device_gb"), ({"gb": 1}, r"unknown key")]:
        with pytest.raises(ValueError, match=key):
            ZarrSegmentationDataset3D(_mgr(tmp_path, "x", patch_search=block))


def test_entry_points_are_declared_exported_and_validate_on_the_host():
    from mt3d_amd.engine import lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rxunet.h")).read(), flags=re.S)
    so = ctypes.CDLL(lib.LIB_PATH)
    for name in ("rx_box_stats", "rx_box_stats_workspace"):
        assert re.search(rf"\b{name}\s*\(", hdr) and hasattr(so, name) and name in lib.exported_symbols()
    L = lib.load()
    assert L.rx_box_stats_workspace(0) == 0 and L.rx_box_stats_workspace(-3) == 0
    assert L.rx_box_stats_workspace(1) == 32 and L.rx_box_stats_workspace(2) == 48 and L.rx_box_stats_workspace(3000) == 72000
    # refused on the host, before any device call (the pointers below are never dereferenced): the status and the entry's name
    fake = ctypes.c_void_p(0x10000)

    def call(boxes, vol=fake, dtype=lib.RX_SW_U8, shape=(8, 9, 10), n=None, ws=fake, ws_bytes=1 << 20, count=fake, ext=fake):
        t = np.ascontiguousarray(boxes, np.int32)
        return L.rx_box_stats(vol, dtype, *shape, t.ctypes.data if t.size else None, len(t) if n is None else n, ws, ws_bytes, count, ext, None)

    good = [[0, 0, 0, 8, 9, 10]]
    for kw, word in [(dict(vol=None), b"null"), (dict(ws=None), b"null"), (dict(count=None), b"null"), (dict(ext=None), b"null"),
                     (dict(dtype=3), b"dtype"), (dict(dtype=-1), b"dtype"), (dict(shape=(0, 9, 10)), b"positive"),
                     (dict(shape=(8, 9, -1)), b"positive"), (dict(n=0), b"n_boxes"), (dict(n=-1), b"n_boxes"),
                     (dict(ws=ctypes.c_void_p(0x10008)), b"aligned"), (dict(vol=ctypes.c_void_p(0x10001), dtype=lib.RX_SW_U16), b"aligned"),
                     (dict(count=ctypes.c_void_p(0x10004)), b"aligned")]:
        assert call(good, **kw) == -1, kw
        assert L.rx_last_error().startswith(b"rx_box_stats:") and word in L.rx_last_error(), (kw, L.rx_last_error())
    assert L.rx_box_stats(None, 0, 8, 9, 10, None, 1, None, 0, None, None, None) == -1 and b"rx_box_stats" in L.rx_last_error()
    for boxes, word in [([[0, 0, 0, 8, 9, 11]], b"leaves"), ([[1, 0, 0, 8, 9, 10]], b"leaves"), ([[0, -1, 0, 1, 1, 1]], b"leaves"),
                        ([[0, 0, 0, 8, 9, 10], [7, 8, 9, 1, 1, 2]], b"box 1"), ([[0, 0, 0, 0, 9, 10]], b"non-positive"),
                        ([[0, 0, 0, 8, -2, 10]], b"non-positive"), ([[0, 0, 2147483647, 1, 1, 2]], b"leaves")]:
        assert call(boxes) == -1, boxes
        assert L.rx_last_error().startswith(b"rx_box_stats:") and word in L.rx_last_error(), (boxes, L.rx_last_error())
    assert call(good, ws_bytes=16) == -4 and b"rx_box_stats_workspace" in L.rx_last_error()


def test_wrappers_refuse_what_they_cannot_run(tmp_path):
    from mt3d_amd.engine import ops as E
    from mt3d_amd.engine.lib import RxError
    with pytest.raises(RxError, match="box_stats"):
        E.box_stats(torch.zeros(4, 4, 4, dtype=torch.uint8), [[0, 0, 0, 1, 1, 1]])      # a host tensor
    with pytest.raises(RxError, match="box_stats"):
        E.box_stats(np.zeros((4, 4, 4), np.uint8), [[0, 0, 0, 1, 1, 1]])
    for arr, patch in [(np.zeros((4, 4), np.uint8), (2, 2, 2)), (np.zeros((2, 4, 4, 4), np.uint8), (2, 2, 2)),
                       (np.zeros((4, 4, 4), np.int64), (2, 2, 2)), (np.zeros((4, 4, 4), np.uint8), (2, 2)),
                       (np.zeros((4, 4, 4), np.uint8), (2, 0, 2))]:
        with pytest.raises(ValueError, match="find_valid_patches_device"):             # before the device is asked for
            P.find_valid_patches_device(arr, patch)
    lab, patch, bt, lt = labels()["volume"]
    if torch.cuda.is_available():                   # with a device the switch works and agrees (the GPU tests go further)
        dev = ZarrSegmentationDataset3D(_mgr(tmp_path, "d", patch_search={"where": "device"}))
        assert dev.all_valid_patches == find_valid_patches(lab, patch, bt, lt)
        return
    with pytest.raises(RxError, match="no HIP device"):
        P.find_valid_patches_device(lab, patch, bt, lt)
    with pytest.raises(RxError, match="no HIP device"):
        ZarrSegmentationDataset3D(_mgr(tmp_path, "d", patch_search={"where": "device"}))
    assert not os.path.exists(tmp_path / "d" / "m_16_16_16_cache.json")                 # nothing was cached on the way out
