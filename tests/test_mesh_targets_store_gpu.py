"""GPU: tasks/normals/mesh_targets.py: MeshTargetBuilder on the device -- two meshes into 32^3 zarr stores in a temp directory, read
back through zarr_lite equal to the numpy statement, and served by ZarrSegmentationDataset3D: unit vectors on the painted voxels,
exactly -1 (code 0) elsewhere, as in the reference's volumes."""
import json
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import mt3d_amd  # noqa: F401
from mt3d_amd.dataloading import zarr_lite
from mt3d_amd.dataloading.dataset import ZarrSegmentationDataset3D
from mt3d_amd.tasks.normals import mesh_targets as M

pytestmark = pytest.mark.gpu
D = 32


def wavy_sheet(seed, y_mid, tilt):
    rng = np.random.default_rng(seed)
    nu, nv = 7, 7
    u, v = np.meshgrid(np.arange(nu), np.arange(nv), indexing="ij")
    x = 1.5 + 29.0 * u / (nu - 1) + rng.uniform(-0.3, 0.3, u.shape)
    y = y_mid + 3.0 * np.sin(0.8 * u + 0.4 * v) + tilt * (u - 3) + rng.uniform(-0.3, 0.3, u.shape)
    z = -0.5 + 32.0 * v / (nv - 1) + rng.uniform(-0.2, 0.2, u.shape)
    verts = np.stack([x, y, z], axis=-1).reshape(-1, 3).astype(np.float32)
    tris = []
    for i in range(nu - 1):
        for j in range(nv - 1):
            a, b, c, d = i * nv + j, (i + 1) * nv + j, (i + 1) * nv + j + 1, i * nv + j + 1
            tris += [[a, b, c], [a, c, d]]
    return verts, np.asarray(tris, np.int64)


def test_builder_device_store_and_dataset(tmp_path):
    meshes = [wavy_sheet(1, 11.0, 0.8), wavy_sheet(2, 21.0, -1.0)]
    b = M.MeshTargetBuilder(meshes, (D, D, D), slab=12)          # slabs of 12, 12 and 8 slices
    n_path, l_path, m_path = b.normals_volume(tmp_path / "normals.zarr"), b.labels_volume(tmp_path / "labels.zarr"), b.sheet_mask(tmp_path / "sheet.zarr")
    want_n = M.normals_volume_numpy(b.vertices, b.triangles, b.normals, D, D, 0, D)
    want_l = M.labels_volume_numpy(b.vertices, b.triangles, b.tri_labels, D, D, 0, D)
    arr = zarr_lite.open(n_path)
    assert arr.shape == (D, D, D, 3) and arr.dtype == np.uint16 and arr.chunks == (128, 128, 128, 3)
    got_n = arr[:]
    assert np.array_equal(got_n, want_n) and want_n.any(axis=3).sum() > 2000
    got_l = zarr_lite.open(l_path)[:]
    assert np.array_equal(got_l, want_l) and set(np.unique(got_l)) == {0, 1, 2}
    mask = zarr_lite.open(m_path)[:]
    assert mask.dtype == np.uint8 and np.array_equal(mask, want_n.any(axis=3).astype(np.uint8) * 255)
    attrs = json.load(open(tmp_path / "normals.zarr" / ".zattrs"))
    assert attrs["n_channels"] == 3 and attrs["min_z"] == 0 and attrs["max_z"] == D - 1 and attrs["chunk_size"] == [128, 128, 128, 3]
    # a window and a shifted z origin through the same path
    win = M.MeshTargetBuilder(meshes, (9, D, D), slab=4, min_z=5, window=(3, 5, 21, 19))
    assert np.array_equal(zarr_lite.open(win.normals_volume(tmp_path / "win.zarr"))[:], want_n[5:14, 3:24, 5:24])

    # the dataset serves it
    img = np.random.default_rng(0).integers(0, 255, (D, D, D), dtype=np.uint8)
    zarr_lite.write_array(str(tmp_path / "img.zarr"), img, (16, 16, 16))
    tasks = {"sheet": {"channels": 1}, "normals": {"channels": 3}}
    mgr = SimpleNamespace(model_name="m", tasks=tasks, train_patch_size=(16, 16, 16), min_labeled_ratio=0.01, min_bbox_percent=0.1,
                          dilate_label=False, use_cache=False, cache_folder=str(tmp_path / "cache"), dataset_config={"augment": False},
                          volume_paths=[{"input": str(tmp_path / "img.zarr"), "sheet": m_path, "normals": n_path, "ref_label": "sheet"}])
    ds = ZarrSegmentationDataset3D(mgr)
    assert len(ds) > 0
    idx = len(ds) // 2
    it = ds[idx]
    z, y, x = ds.all_valid_patches[idx]["start_pos"]
    sl = np.s_[z:z + 16, y:y + 16, x:x + 16]
    nrm = it["normals"].numpy()
    assert nrm.shape == (3, 16, 16, 16) and nrm.dtype == np.float32
    painted = want_n[sl].any(axis=3)
    assert painted.sum() > 100 and np.array_equal(it["sheet"][0].numpy() > 0, painted)
    # the code truncates (n + 1) * 32767.5, so a decoded component is low by less than 1 / 32767.5 (+ float32 rounding of the decode):
    # | |v| - 1 | <= sqrt(3) / 32767.5 + 4 * 2^-24
    length = np.sqrt((nrm.astype(np.float64) ** 2).sum(axis=0))
    assert np.abs(length[painted] - 1.0).max() <= np.sqrt(3.0) / 32767.5 + 4 * 2.0 ** -24
    assert (nrm[:, ~painted] == -1.0).all()
    assert torch.equal(it["normals"], torch.from_numpy(np.ascontiguousarray((want_n[sl].astype(np.float32) / 32767.5 - 1.0).transpose(3, 0, 1, 2))))
