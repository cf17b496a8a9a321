"""GPU: rx_box_stats against its numpy statement (`patch_search_device.box_stats_numpy`), exactly, and the device search against
the host search: same lists, same cache files, resident and streamed."""
import ctypes
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import mt3d_amd  # noqa: F401
from mt3d_amd.dataloading import patch_search_device as P
from mt3d_amd.dataloading import zarr_lite
from mt3d_amd.dataloading.dataset import ZarrSegmentationDataset3D, find_valid_patches
from mt3d_amd.engine import lib as L
from mt3d_amd.engine import ops as E
from patch_search_cases import from_stats, labels

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SHAPES = [(5, 7, 9), (13, 11, 70), (9, 37, 130), (40, 6, 257)]


def _volume(shape, dtype, seed):
    rng = np.random.default_rng(seed)
    on = rng.random(shape) < 0.3
    if dtype == np.float32:
        v = (on * rng.uniform(0.5, 2.0, size=shape)).astype(np.float32)
        kind = rng.integers(0, 12, size=shape)
        v[kind == 0] = -1.5              # counted, never extends a box
        v[kind == 1] = np.nan            # the same
        v[kind == 2] = -0.0              # neither
        v[kind == 3] = np.inf            # both
        return v
    return (on * rng.integers(1, np.iinfo(dtype).max + 1, size=shape)).astype(dtype)


def _to_device(a):
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).to(DEV)


def _boxes(shape, seed):
    """the boxes the kernel's paths need: one voxel, the whole volume (deeper than a z-chunk: the widest box of these calls has
    at most 257 * 4 bytes a row, so a chunk is at most 4096 / 9 = 455 rows of the (5, 7, 9) volume's 35 and, on (40, 6, 257), 16
    rows of its 240), every head / tail alignment, boxes that end on the last column"""
    Z, Y, X = shape
    rng = np.random.default_rng(seed)
    out = [[Z // 2, Y // 2, X // 2, 1, 1, 1], [0, 0, 0, 1, 1, 1], [Z - 1, Y - 1, X - 1, 1, 1, 1], [0, 0, 0, Z, Y, X]]
    for x0 in (0, 1, 15, 17):
        for dx in (1, 16, 33, X - x0):
            if x0 < X and dx >= 1 and x0 + dx <= X:
                z0, y0 = int(rng.integers(0, Z)), int(rng.integers(0, Y))
                out.append([z0, y0, x0, int(rng.integers(1, Z - z0 + 1)), int(rng.integers(1, Y - y0 + 1)), dx])
                out.append([0, 0, x0, Z, Y, dx])
    return np.array(out, np.int32)


def _random_boxes(shape, n, seed):
    rng = np.random.default_rng(seed)
    lo = np.stack([rng.integers(0, s, size=n) for s in shape], axis=1)
    ext = np.stack([rng.integers(1, s - lo[:, d] + 1) for d, s in enumerate(shape)], axis=1)
    b = np.concatenate([lo, ext], axis=1).astype(np.int32)
    b[n // 2:n // 2 + n // 10] = b[:n // 10]              # duplicates
    return b


def _same(got, want):
    return (got[0].dtype == np.uint64 and got[1].dtype == np.int32 and np.array_equal(got[0], want[0])
            and np.array_equal(got[1], want[1]))


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.float32], ids=lambda d: np.dtype(d).name)
def test_box_stats_equals_the_numpy_statement(shape, dtype):
    a = _volume(shape, dtype, sum(shape))
    t = _to_device(a)
    boxes = _boxes(shape, 3)
    got, want = E.box_stats(t, boxes), P.box_stats_numpy(a, boxes)
    assert _same(got, want), np.nonzero((got[1] != want[1]).any(axis=1) | (got[0] != want[0]))
    assert int(want[0][3]) == np.count_nonzero(a) and 0 < int(want[0][3]) < a.size
    many = _random_boxes(shape, 3200, 5)
    assert len(np.unique(many, axis=0)) < len(many)
    assert _same(E.box_stats(t, many), P.box_stats_numpy(a, many))
    assert _same(E.box_stats(t, boxes), want)              # the same call again: the same bits
    if dtype == np.uint16 and hasattr(torch, "uint16"):
        assert _same(E.box_stats(t.view(torch.uint16), boxes), want)


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.float32], ids=lambda d: np.dtype(d).name)
def test_planted_corners_and_outside_neighbours(dtype):
    a = np.zeros((12, 14, 70), dtype)
    box = (3, 4, 17, 5, 6, 35)
    z0, y0, x0, dz, dy, dx = box
    for z in (z0, z0 + dz - 1):
        for y in (y0, y0 + dy - 1):
            for x in (x0, x0 + dx - 1):
                a[z, y, x] = 7
    inner = [[z0 + 1, y0 + 1, x0 + 1, dz - 2, dy - 2, dx - 2]]
    boxes = np.array([list(box)] + inner + [[0, 0, 0, 12, 14, 70]], np.int32)
    got = E.box_stats(_to_device(a), boxes)
    assert got[0].tolist() == [8, 0, 8]
    assert got[1].tolist() == [[0, dz - 1, 0, dy - 1, 0, dx - 1], [dz - 2, -1, dy - 2, -1, dx - 2, -1],
                               [z0, z0 + dz - 1, y0, y0 + dy - 1, x0, x0 + dx - 1]]
    for z, y, x in [(z0 - 1, y0 + 2, x0 + 5), (z0 + dz, y0 + 2, x0 + 5), (z0 + 2, y0 - 1, x0 + 5), (z0 + 2, y0 + dy, x0 + 5),
                    (z0 + 2, y0 + 2, x0 - 1), (z0 + 2, y0 + 2, x0 + dx)]:
        a[z, y, x] = 9                                      # one step outside each face
    got = E.box_stats(_to_device(a), boxes)
    assert got[0].tolist() == [8, 0, 14]                    # the box does not see them, the whole volume does
    assert got[1][:2].tolist() == [[0, dz - 1, 0, dy - 1, 0, dx - 1], [dz - 2, -1, dy - 2, -1, dx - 2, -1]]
    assert got[1][2].tolist() == [z0 - 1, z0 + dz, y0 - 1, y0 + dy, x0 - 1, x0 + dx]
    assert _same(got, P.box_stats_numpy(a, boxes))


def test_empty_boxes_and_float_predicates():
    for dtype in (np.uint8, np.uint16, np.float32):
        a = np.zeros((6, 5, 40), dtype)
        a[5, 4, 39] = 1
        boxes = np.array([[0, 0, 0, 6, 5, 39], [1, 2, 3, 4, 1, 33], [5, 4, 39, 1, 1, 1], [0, 0, 0, 5, 5, 40]], np.int32)
        count, ext = E.box_stats(_to_device(a), boxes)
        assert count.tolist() == [0, 0, 1, 0]
        assert ext.tolist() == [[6, -1, 5, -1, 39, -1], [4, -1, 1, -1, 33, -1], [0, 0, 0, 0, 0, 0], [5, -1, 5, -1, 40, -1]]
    a = np.zeros((4, 5, 37), np.float32)
    a[0, 0, 0], a[1, 1, 1], a[3, 4, 36], a[2, 2, 20] = -2.0, np.nan, -0.0, -np.inf      # nothing > 0 anywhere
    a[0, 3, 5] = np.float32(1e-45)                                                       # the smallest subnormal is > 0
    a[2, 1, 30] = np.inf
    boxes = np.array([[0, 0, 0, 4, 5, 37], [0, 0, 0, 2, 3, 5], [3, 4, 36, 1, 1, 1], [2, 2, 20, 1, 1, 1], [0, 0, 1, 4, 5, 36]], np.int32)
    count, ext = E.box_stats(_to_device(a), boxes)
    assert count.tolist() == [5, 2, 0, 1, 4]                # negatives and the NaN count; -0.0 does not
    assert ext.tolist() == [[0, 2, 1, 3, 5, 30], [2, -1, 3, -1, 5, -1], [1, -1, 1, -1, 1, -1], [1, -1, 1, -1, 1, -1], [0, 2, 1, 3, 4, 29]]
    assert _same((count, ext), P.box_stats_numpy(a, boxes))


def test_offsets_beyond_2_to_31():
    free = torch.cuda.mem_get_info(torch.device(DEV))[0]
    if free < 4 * 10 ** 9:
        pytest.skip(f"{free} bytes free on the device, the 2.2e9-voxel volume needs 4e9 to be safe")
    Z, Y, X = 2, 33000, 33000
    assert Z * Y * X > 2 ** 31
    t = torch.zeros((Z, Y, X), dtype=torch.uint8, device=DEV)
    voxels = [(0, 0, 3), (0, 5, 32999), (0, 32999, 17), (1, 2, 1), (1, 32990, 32985), (1, 32998, 32999), (1, 32999, 32998)]
    for z, y, x in voxels:
        t[z, y, x] = 200
    far = (1, 32980, 32970, 1, 20, 30)
    boxes = np.array([[0, 0, 0, Z, Y, X], list(far), [1, 0, 0, 1, Y, X], [0, 32999, 0, 2, 1, X]], np.int32)
    count, ext = E.box_stats(t, boxes)
    del t
    for i, (z0, y0, x0, dz, dy, dx) in enumerate(boxes.tolist()):
        inside = [(z - z0, y - y0, x - x0) for z, y, x in voxels if z0 <= z < z0 + dz and y0 <= y < y0 + dy and x0 <= x < x0 + dx]
        assert len(inside) > 0 and int(count[i]) == len(inside), i
        want = [f(v[d] for v in inside) for d in range(3) for f in (min, max)]
        assert ext[i].tolist() == want, i
    assert int(count[0]) == len(voxels) and int(count[1]) == 3


@pytest.mark.parametrize("name", list(labels()))
def test_device_search_equals_the_host_search(tmp_path, name):
    lab, patch, bt, lt = labels()[name]
    want = find_valid_patches(lab, patch, bt, lt)
    assert len(want) > 0
    t = _to_device(lab)
    assert from_stats(lambda a, b: E.box_stats(t, b), lab, patch, bt, lt) == from_stats(P.box_stats_numpy, lab, patch, bt, lt)
    store = zarr_lite.write_array(str(tmp_path / "lab.zarr"), lab, (16, 16, 16), compressor="zlib")
    slab = patch[0] * lab.shape[1] * lab.shape[2] * lab.itemsize      # the smallest budget there is: one patch-deep slab
    for arr in (lab, store):
        assert P.find_valid_patches_device(arr, patch, bt, lt, device=DEV) == want
        assert P.last_timing["mode"] == "resident" and P.last_timing["launches"] == 2 and P.last_timing["bytes_read"] == lab.nbytes
        assert P.find_valid_patches_device(arr, patch, bt, lt, max_device_bytes=slab, device=DEV) == want
        tm = dict(P.last_timing)
        assert tm["mode"] == "streamed" and tm["slabs_a"] >= 3 and tm["groups_b"] >= 2, tm
        assert tm["launches"] == tm["slabs_a"] + tm["groups_b"] and tm["candidates"] >= len(want)
        with pytest.raises(ValueError, match="below one patch-deep slab"):
            P.find_valid_patches_device(arr, patch, bt, lt, max_device_bytes=slab - 1, device=DEV)
    assert P.find_valid_patches_device(np.zeros((20, 24, 28), np.uint8), (8, 8, 8), 0.5, 0.05, device=DEV) == []
    assert P.find_valid_patches_device(np.zeros((20, 24, 28), np.uint8), (8, 8, 8), 0.5, 0.05, max_device_bytes=6000, device=DEV) == []
    assert P.last_timing["mode"] == "streamed" and P.last_timing["groups_b"] == 0


def test_bad_arguments_on_a_live_device_leave_the_next_call_working():
    a = _volume((9, 10, 33), np.uint8, 1)
    t = _to_device(a)
    so = L.load()
    good = np.array([[0, 0, 0, 9, 10, 33], [2, 3, 4, 5, 6, 7]], np.int32)
    want = P.box_stats_numpy(a, good)
    ws = torch.empty(64, dtype=torch.uint8, device=DEV)
    count = torch.empty(2, dtype=torch.int64, device=DEV)
    ext = torch.empty((2, 6), dtype=torch.int32, device=DEV)

    def call(boxes, vol=t.data_ptr(), dtype=L.RX_SW_U8, shape=(9, 10, 33), n=2, wsp=ws.data_ptr(), ws_bytes=64, cnt=count.data_ptr(),
             ex=ext.data_ptr()):
        b = np.ascontiguousarray(boxes, np.int32)
        rc = so.rx_box_stats(ctypes.c_void_p(vol), dtype, *shape, b.ctypes.data, n, ctypes.c_void_p(wsp), ws_bytes, ctypes.c_void_p(cnt),
                             ctypes.c_void_p(ex), L.stream_ptr())
        torch.cuda.synchronize()
        return rc

    bad = [(dict(vol=None), -1), (dict(wsp=None), -1), (dict(cnt=None), -1), (dict(ex=None), -1), (dict(dtype=7), -1),
           (dict(shape=(9, 0, 33)), -1), (dict(n=0), -1), (dict(wsp=ws.data_ptr() + 4), -1), (dict(cnt=count.data_ptr() + 4), -1),
           (dict(ws_bytes=32), -4)]
    for kw, status in bad:
        assert call(good, **kw) == status, kw
        assert so.rx_last_error().startswith(b"rx_box_stats:"), so.rx_last_error()
        assert call(good) == 0
        assert _same((count.cpu().numpy().view(np.uint64), ext.cpu().numpy()), want), kw
    for boxes in ([[0, 0, 0, 9, 10, 34], [0, 0, 0, 1, 1, 1]], [[0, 0, 0, 1, 1, 1], [8, 9, 32, 2, 1, 1]], [[0, 0, 0, 1, 0, 1], [0, 0, 0, 1, 1, 1]],
                  [[-1, 0, 0, 2, 2, 2], [0, 0, 0, 1, 1, 1]]):
        assert call(boxes) == -1 and so.rx_last_error().startswith(b"rx_box_stats: box")
        assert _same(E.box_stats(t, good), want)
    for vol, boxes in [(t.cpu(), good), (t.to(torch.int32), good), (t[:, :, 1:], good[1:]), (t, good.astype(np.float32)),
                       (t, good[:, :5]), (t, good[:0])]:
        with pytest.raises(L.RxError, match="box_stats"):
            E.box_stats(vol, boxes)
    with pytest.raises(L.RxError, match="leaves"):
        E.box_stats(t, [[0, 0, 0, 10, 10, 33]])
    assert _same(E.box_stats(t, good), want)


def test_dataset_device_and_host_searches_agree(tmp_path):
    lab = labels()["volume"][0]
    img = np.random.default_rng(4).integers(0, 255, size=lab.shape, dtype=np.uint8)
    paths = {}
    for name, arr in [("img", img), ("sheet", lab)]:
        paths[name] = str(tmp_path / f"{name}.zarr")
        zarr_lite.write_array(paths[name], arr, (16, 16, 16), compressor="zlib")

    def mgr(cache, **dataset_config):
        return SimpleNamespace(model_name="m", tasks={"sheet": {"channels": 1}}, train_patch_size=(16, 16, 16), min_labeled_ratio=0.1,
                               min_bbox_percent=0.9, dilate_label=False, use_cache=True, cache_folder=str(tmp_path / cache),
                               dataset_config=dict(augment=False, **dataset_config),
                               volume_paths=[{"input": paths["img"], "sheet": paths["sheet"], "ref_label": "sheet"}])

    host = ZarrSegmentationDataset3D(mgr("h", patch_search={"where": "host"}))
    dev = ZarrSegmentationDataset3D(mgr("d", patch_search={"where": "device", "max_device_gb": 1}))
    assert P.last_timing["mode"] == "resident" and P.last_timing["candidates"] >= len(dev) > 0
    assert dev.patch_search == {"where": "device", "max_device_bytes": 1 << 30}
    assert dev.all_valid_patches == host.all_valid_patches == find_valid_patches(lab, (16, 16, 16), 0.9, 0.1)
    assert dev.cache_file.name == host.cache_file.name and dev.cache_file.read_bytes() == host.cache_file.read_bytes()
    again = ZarrSegmentationDataset3D(mgr("h", patch_search={"where": "device"}))      # the host's cache serves the device config
    assert again.all_valid_patches == host.all_valid_patches
    a, b = host[len(host) // 2], dev[len(dev) // 2]
    assert set(a) == set(b) == {"image", "sheet"} and all(torch.equal(a[k], b[k]) for k in a)
