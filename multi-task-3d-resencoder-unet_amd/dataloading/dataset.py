"""Patch feeders with the reference's item contract (dataloading/dataset.py:103-222): a dict with
"image" (C, Z, Y, X) float32 and one float32 tensor per task.

`SyntheticPatchDataset` generates SURVEY 8(d)'s synthetic patches (what the headline metric is quoted on).
`ZarrSegmentationDataset3D` reads real zarr v2 volumes through `zarr_lite` (the `zarr` package is absent here): same
constructor, valid-patch search, cache file, dtype scaling and item layout as the reference; its augmentations need
albumentations / volumentations (absent): `dataloading/augment.py` restates the stack in numpy (parity unpinned) and is applied
by default with ONE warning saying so (`dataset_config.augment: "restated"` acknowledges it, `false` feeds raw patches, `"device"`
feeds raw patches and leaves the stack to the HIP kernels behind `augment_device.DeviceAugmenter`); remote
(http) stores are refused (no network).

The stage blocks of `dataset_config` -- `geometric` (flips and 90-degree rotations, `geometry_device.py`), `spatial` (small-angle
rotation and scale, `spatial_device.py`), `elastic` (a B-spline deformation, `elastic_device.py`), each absent: off and moving the
image and every target together, a normals target kept consistent; `dilate` under `tr_setup.dilate_label` (absent: `{where: host,
radius: 5}`, the reference's ball, `dilate_device.py`); `ingest` (absent: `{where: host}`: where the float32 conversion, the dtype
scaling and the channels-last transpose run, `ingest_device.py`) and `patch_search` (absent: `{where: host}`: where the
constructor's valid-patch search runs, `patch_search_device.py`; no device is an error, not a fallback) -- are parsed and checked
against each other by ONE call, `stages.parse_stages`; both datasets expose what it returns as `geometric`, `spatial`, ... and
`device_spatial`, ... (the block if it says `where: device`, else None).  `where: host` stages run inside `__getitem__`; `where:
device` ones leave the items alone (`ingest`: hands out `torch.from_numpy` of the raw slices, and `device_ingest` is {key: rule})
and are the trainer's business.  The ORDER of the stages, on either side, is stated once: `stages.DevicePipeline`'s docstring."""
import json
import os
import warnings
from pathlib import Path

import numpy as np
import torch
from torch.utils.data import Dataset

from . import zarr_lite


class SyntheticPatchDataset(Dataset):
    """SURVEY 8(d)'s synthetic patches.  `dataset_config.synthetic_pool` (default 16) distinct patches are generated once per
    process and handed out round-robin: drawing 2 x 128^3 uniform numbers per item costs ~60 ms of one CPU core, which would make
    a 128^3 training run loader-bound at ~8 patches/s; 0 = draw every item afresh.  With a pool the trainer's train / validation
    split (train.py:99-120 mirror) hands out the SAME pool to both sides: synthetic validation numbers measure throughput and
    plumbing, not generalisation (set `synthetic_pool: 0` for disjoint samples)."""

    def __init__(self, mgr, length=None, seed=1234):
        self.mgr = mgr
        self.patch = tuple(mgr.train_patch_size)
        self.cin = mgr.in_channels
        self.tasks = mgr.tasks
        self.length = int(length if length is not None else mgr.dataset_config.get("synthetic_length", 64))
        self.seed = seed
        self.pool = int(mgr.dataset_config.get("synthetic_pool", 16))
        self._cache = {}
        from .stages import parse_stages
        vars(self).update(parse_stages(mgr.dataset_config, self.patch, self.tasks).attributes())
        if self.geometric is not None and self.geometric["where"] != "device":
            raise ValueError("dataset_config.geometric.where: \"host\" is served by the zarr dataset; synthetic patches take \"device\"")
        # `where: host` resamples every item handed out, one draw per item from `spatial_rng` / `elastic_rng` (None: the `random`
        # module, which a DataLoader seeds per worker)
        self.spatial_rng, self.last_spatial_op = None, None
        self.elastic_rng, self.last_elastic_field = None, None

    def __len__(self):
        return self.length

    def __getitem__(self, idx):
        if self.pool > 0:
            key = int(idx) % self.pool
            if key not in self._cache:
                self._cache[key] = self._make(key)
            return self._host_spatial(dict(self._cache[key]))
        return self._host_spatial(self._make(idx))

    def _host_spatial(self, item):
        if self.spatial is not None and self.spatial["where"] == "host":
            item = _host_spatial(self, item)
        if self.elastic is not None and self.elastic["where"] == "host":
            item = _host_elastic(self, item)
        return item

    def _make(self, idx):
        g = torch.Generator().manual_seed(self.seed + int(idx))
        item = {"image": torch.rand((self.cin, *self.patch), generator=g)}
        seg = (torch.rand((1, *self.patch), generator=g) > 0.8).float()
        for name, info in self.tasks.items():
            c = info["channels"]
            if info.get("loss_fn", "BCEDiceLoss") == "MaskedCosineLoss":
                v = torch.randn((c, *self.patch), generator=g)
                item[name] = (v / v.norm(dim=0, keepdim=True).clamp(min=1e-8)) * seg
            else:
                item[name] = seg.expand(c, *self.patch).contiguous()
        return item


def _host_spatial(ds, item):
    """`dataset_config.spatial.where: host`: one draw per item, `affine_numpy` on every array of it (an identity draw: untouched)"""
    import random
    from .spatial_device import apply_item_numpy, draw_affine
    cfg = ds.spatial
    op = draw_affine(ds.spatial_rng if ds.spatial_rng is not None else random, cfg["rotation"], cfg["scale"])
    ds.last_spatial_op = op
    if op.is_identity():
        return item
    return apply_item_numpy(op, item, cfg["normal_keys"], cfg["image_border"])


def _host_elastic(ds, item):
    """`dataset_config.elastic.where: host`: one draw per item, `elastic_numpy` on every array of it (a zero field: untouched)"""
    import random
    from .elastic_device import apply_item_numpy, draw_elastic
    cfg = ds.elastic
    shape = tuple(int(v) for v in item["image"].shape[-3:])
    field = draw_elastic(ds.elastic_rng if ds.elastic_rng is not None else random, shape, cfg["spacing"], cfg["magnitude"], cfg["p"])
    ds.last_elastic_field = field
    if field.is_identity():
        return item
    return apply_item_numpy(field, item, cfg["normal_keys"], cfg["image_border"])


def find_label_bounding_box(arr, chunk_shape=(192, 192, 192)):
    """helpers.py:71-131: (minz, maxz, miny, maxy, minx, maxx) of the non-zero voxels, read chunk by chunk"""
    D, H, W = arr.shape
    lo, hi = [D, H, W], [-1, -1, -1]
    for z0 in range(0, D, chunk_shape[0]):
        for y0 in range(0, H, chunk_shape[1]):
            for x0 in range(0, W, chunk_shape[2]):
                ch = arr[z0:z0 + chunk_shape[0], y0:y0 + chunk_shape[1], x0:x0 + chunk_shape[2]]
                if ch.any():
                    nz = np.argwhere(ch > 0) + np.array([z0, y0, x0])
                    for d in range(3):
                        lo[d], hi[d] = min(lo[d], int(nz[:, d].min())), max(hi[d], int(nz[:, d].max()))
    return lo[0], hi[0], lo[1], hi[1], lo[2], hi[2]


def find_valid_patches(arr, patch_size, bbox_threshold=0.97, label_threshold=0.10):
    """helpers.py:136-198 (+ _check_patch_chunk :38-68), single process: half-patch stride inside the label bounding box; a
    patch is kept when the bounding box of its labelled voxels covers >= bbox_threshold of the patch and >= label_threshold
    of its voxels are labelled."""
    pZ, pY, pX = patch_size
    minz, maxz, miny, maxy, minx, maxx = find_label_bounding_box(arr)
    out = []
    for z in range(minz, maxz - pZ + 2, max(pZ // 2, 1)):
        for y in range(miny, maxy - pY + 2, max(pY // 2, 1)):
            for x in range(minx, maxx - pX + 2, max(pX // 2, 1)):
                patch = arr[z:z + pZ, y:y + pY, x:x + pX]
                nz = np.argwhere(patch > 0)
                if nz.size == 0:
                    continue
                ext = nz.max(axis=0) - nz.min(axis=0) + 1
                if float(ext[0] * ext[1] * ext[2]) / patch.size < bbox_threshold:
                    continue
                if np.count_nonzero(patch) / patch.size < label_threshold:
                    continue
                out.append({"volume_idx": 0, "start_pos": [int(z), int(y), int(x)]})
    return out


def _ball(radius):
    """skimage.morphology.ball: voxels within `radius` of the centre of a (2r+1)^3 cube"""
    r = np.arange(-radius, radius + 1)
    z, y, x = np.meshgrid(r, r, r, indexing="ij")
    return (z * z + y * y + x * x) <= radius * radius


class ZarrSegmentationDataset3D(Dataset):
    """dataloading/dataset.py:18-222; the augmentation stack (:171-205) through `augment.py` (see the module docstring)."""
    _warned = False

    def __init__(self, mgr):
        self.mgr = mgr
        self.model_name = mgr.model_name
        self.volume_paths = mgr.volume_paths
        self.tasks = mgr.tasks
        self.patch_size = tuple(mgr.train_patch_size)
        self.min_labeled_ratio = mgr.min_labeled_ratio
        self.min_bbox_percent = mgr.min_bbox_percent
        self.dilate_label = mgr.dilate_label
        self.use_cache = mgr.use_cache
        self.cache_folder = mgr.cache_folder
        # the reference's recipe augments every item (dataset.py:171-205: brightness / noise / blur OneOf groups,
        # CoarseDropout3D) with albumentations / volumentations, which are not installed here.  `augment.py` restates that
        # stack; say ONCE per process that it is a restatement instead of silently training a slightly different recipe.
        # dataset_config.augment: true (default) = restated stack + the warning, "restated" = acknowledged, false = raw patches,
        # "device" = raw patches here, the same stack as HIP kernels on the batch once it is on the device (augment_device.py;
        # the trainer reads `device_augment`)
        mode = getattr(mgr, "dataset_config", {}).get("augment", True)
        if isinstance(mode, str) and mode.lower() not in ("restated", "true", "false", "device"):
            raise ValueError(f"dataset_config.augment: {mode!r} (true, false, \"restated\" or \"device\")")
        self.device_augment = isinstance(mode, str) and mode.lower() == "device"
        self.augment = (mode.lower() not in ("false", "device")) if isinstance(mode, str) else bool(mode)
        if self.augment and not (isinstance(mode, str) and mode.lower() == "restated") and not ZarrSegmentationDataset3D._warned:
            ZarrSegmentationDataset3D._warned = True
            warnings.warn("ZarrSegmentationDataset3D: the reference's augmentation stack (dataloading/dataset.py:171-205) needs "
                          "albumentations / volumentations, which are absent -- patches go through the numpy RESTATEMENT of it "
                          "(dataloading/augment.py: same structure and probabilities, the members' default parameters as "
                          "documented; not compared with albumentations).  Set dataset_config.augment: \"restated\" to "
                          "acknowledge, or false to feed raw patches.", RuntimeWarning, stacklevel=2)
        # the stage blocks, parsed and checked against each other; "device" stages are the trainer's business
        from .geometry_device import host_transforms
        from .patch_search_device import find_valid_patches_device
        from .stages import parse_stages
        vars(self).update(parse_stages(getattr(mgr, "dataset_config", {}), self.patch_size, self.tasks, self.dilate_label,
                                       self.augment).attributes())
        self._host_geometry = host_transforms(self.geometric) if self.geometric is not None and self.geometric["where"] == "host" else []
        self.device_ingest = None          # {key: rule} once the stores are known (`_ingest_rules`)
        self.spatial_rng, self.last_spatial_op = None, None
        self.elastic_rng, self.last_elastic_field = None, None
        self.volumes = []
        for vol_idx, info in enumerate(self.volume_paths):
            vd = {"input_path": info["input"], "targets_path": {}, "ref_label_key": info.get("ref_label", "sheet")}
            for task in self.tasks:
                if task not in info:
                    raise ValueError(f"Volume {vol_idx} missing path for '{task}'")
                vd["targets_path"][task] = info[task]
            for pth in [vd["input_path"], *vd["targets_path"].values()]:
                if str(pth).startswith("http"):
                    raise ValueError(f"remote zarr store {pth}: no network in this environment, mirror it locally")
            self.volumes.append(vd)
        if self.ingest["where"] == "device":
            self.device_ingest = self._ingest_rules()
        ps = self.patch_size
        self.cache_file = Path(f"{self.cache_folder}/{self.model_name}_{ps[0]}_{ps[1]}_{ps[2]}_cache.json")
        self.all_valid_patches = []
        if self.use_cache and self.cache_file.exists():
            with open(self.cache_file) as f:
                self.all_valid_patches = json.load(f)
        else:
            for vol_idx, vd in enumerate(self.volumes):
                ref = zarr_lite.open(vd["targets_path"][vd["ref_label_key"]])
                if self.patch_search["where"] == "device":
                    found = find_valid_patches_device(ref, ps, self.min_bbox_percent, self.min_labeled_ratio,
                                                      max_device_bytes=self.patch_search["max_device_bytes"])
                else:
                    found = find_valid_patches(ref, ps, self.min_bbox_percent, self.min_labeled_ratio)
                for p in found:
                    p["volume_idx"] = vol_idx
                self.all_valid_patches.extend(found)
            if self.use_cache:
                os.makedirs(os.path.dirname(str(self.cache_file)) or ".", exist_ok=True)
                with open(self.cache_file, "w") as f:
                    json.dump(self.all_valid_patches, f)

    def _ingest_rules(self):
        """opens every volume's input and target stores once: {key: rule} for `DeviceIngest`.  One rule and one layout per key, so
        a key's dtype and dimensionality must agree across volumes."""
        from .ingest_device import DTYPES, MAX_CHANNELS, ingest_rule
        seen = {}
        for vol_idx, vd in enumerate(self.volumes):
            for key, path in [("image", vd["input_path"]), *vd["targets_path"].items()]:
                arr = zarr_lite.open(path)
                dt, nd = np.dtype(arr.dtype), len(arr.shape)
                if dt not in DTYPES:
                    raise ValueError(f"dataset_config.ingest.where: device: '{key}' of volume {vol_idx} is {dt} (uint8, uint16 or float32)")
                if nd != 3 and not (nd == 4 and key.lower() == "normals" and 1 <= arr.shape[3] <= MAX_CHANNELS):
                    raise ValueError(f"dataset_config.ingest.where: device: '{key}' of volume {vol_idx} has shape {tuple(arr.shape)} "
                                     f"((Z, Y, X), or channels-last (Z, Y, X, C <= {MAX_CHANNELS}) for normals)")
                if key in seen and seen[key][:2] != (dt, nd):
                    raise ValueError(f"dataset_config.ingest.where: device: '{key}' is {seen[key][0]} with {seen[key][1]} dimensions in "
                                     f"volume {seen[key][2]} and {dt} with {nd} in volume {vol_idx}")
                seen.setdefault(key, (dt, nd, vol_idx))
        return {key: ingest_rule(key, dt) for key, (dt, _, _) in seen.items()}

    def __len__(self):
        return len(self.all_valid_patches)

    def __getitem__(self, idx):
        info = self.all_valid_patches[idx]
        z0, y0, x0 = info["start_pos"]
        dz, dy, dx = self.patch_size
        sl = np.s_[z0:z0 + dz, y0:y0 + dy, x0:x0 + dx]
        vd = self.volumes[info["volume_idx"]]
        if self.device_ingest is not None:      # what the store holds: no astype, no scaling, no transpose, no channel axis
            item = {"image": torch.from_numpy(np.ascontiguousarray(zarr_lite.open(vd["input_path"])[sl]))}
            for task, path in vd["targets_path"].items():
                item[task] = torch.from_numpy(np.ascontiguousarray(zarr_lite.open(path)[sl]))
            return item
        arr = zarr_lite.open(vd["input_path"])
        img = arr[sl]
        og = img.dtype
        img = img.astype(np.float32)
        if og == np.uint8:
            img /= 255.0
        elif og == np.uint16:
            img /= 65535.0
        item = {"image": img}
        for task, path in vd["targets_path"].items():
            t_arr = zarr_lite.open(path)
            t = t_arr[sl].astype(np.float32)
            if task.lower() == "normals":
                t = (t / 32767.5) - 1.0 if t_arr.dtype == np.uint16 else (t * 2.0) - 1.0
                if t.ndim == 4:
                    t = t.transpose(3, 0, 1, 2).copy()
            else:
                if t_arr.dtype == np.uint8:
                    t /= 255.0
                elif t_arr.dtype == np.uint16:
                    t /= 65535.0
                if self.dilate is not None and self.dilate["where"] == "host":
                    from scipy.ndimage import binary_dilation      # == skimage dilation(t > 0, ball(r)) on a 0/1 volume
                    t = binary_dilation(t > 0, structure=_ball(self.dilate["radius"])).astype(np.float32)
            item[task] = t
        for transform in self._host_geometry:      # image and targets together; (Z, Y, X) and (C, Z, Y, X) arrays alike
            item = transform(item)
        if self.spatial is not None and self.spatial["where"] == "host":      # after the signed permutations, before the intensity stack
            item = _host_spatial(self, item)
        if self.elastic is not None and self.elastic["where"] == "host":      # after the host spatial stage, before the intensity stack
            item = _host_elastic(self, item)
        if self.augment:              # image only; targets untouched (dataset.py:200-205)
            from .augment import augment_image
            item["image"] = augment_image(item["image"])
        if item["image"].ndim == 3:
            item["image"] = item["image"][None, ...]
        item["image"] = torch.from_numpy(np.ascontiguousarray(item["image"]))
        for task in self.tasks:
            t = item[task]
            if t.ndim == 3 and task.lower() != "normals":
                t = t[None, ...]
            item[task] = torch.from_numpy(np.ascontiguousarray(t))
        return item

    def close(self):
        pass
