"""Seeded labels shared by test_patch_search_cpu.py and test_patch_search_gpu.py: (label, patch, bbox_threshold, label_threshold)
per name.  `volume` is the label of test_zarr_dataset._volume (same generator, same draws in the same order); `f32` is a float32
label whose hole is filled with NEGATIVE values (counted by count_nonzero, invisible to `> 0`: candidates inside it are empty
with a nonzero count), with a NaN and a -0.0 planted in a labelled region and a thinly labelled corner."""
import numpy as np


def volume_label():
    rng = np.random.default_rng(1)
    D = 40
    rng.integers(0, 255, size=(D, D, D), dtype=np.uint8)                      # the image is drawn first there
    lab = np.zeros((D, D, D), dtype=np.uint8)
    lab[6:36, 4:38, 5:37] = (rng.random((30, 34, 32)) > 0.6) * 255
    return lab


def f32_label():
    rng = np.random.default_rng(7)
    D, H, W = 40, 36, 44
    lab = np.zeros((D, H, W), np.float32)
    on = rng.random((D - 5, H - 5, W - 6)) < 0.35
    lab[3:D - 2, 2:H - 3, 4:W - 2] = on * rng.uniform(0.25, 2.0, size=on.shape).astype(np.float32)
    lab[10:24, 6:22, 20:38] = -rng.uniform(0.5, 1.5, size=(14, 16, 18)).astype(np.float32)      # the hole: negatives only
    sparse = rng.random((12, 12, 14)) < 0.004
    lab[D - 14:D - 2, 2:14, 4:18] = sparse * np.float32(1.0)                                    # the thin corner
    lab[5, 5, 7] = np.nan
    lab[5, 6, 7] = -0.0
    lab[30, 25, 30] = np.inf
    return lab


def u16_label():
    rng = np.random.default_rng(11)
    lab = np.zeros((33, 45, 38), np.uint16)
    on = rng.random((27, 40, 30)) < 0.3
    lab[2:29, 3:43, 5:35] = on * rng.integers(1, 65536, size=on.shape).astype(np.uint16)
    lab[8:20, 10:30, 5:20] = 0
    return lab


def labels():
    return {
        "volume": (volume_label(), (16, 16, 16), 0.9, 0.1),
        "volume_strict": (volume_label(), (9, 16, 11), 0.9, 0.4),
        "f32": (f32_label(), (8, 8, 8), 0.6, 0.1),
        "u16": (u16_label(), (8, 12, 16), 0.8, 0.2),
    }


def from_stats(stats, label, patch, bbox_threshold, label_threshold):
    """the search with `stats(label, boxes) -> (count, ext)` as its only look at the voxels: (list, {rule: rejected candidates})"""
    from mt3d_amd.dataloading import patch_search_device as P
    count, ext = stats(label, np.array([[0, 0, 0, *label.shape]], np.int32))
    bbox = [int(v) for v in ext[0]]
    zs, ys, xs = P.candidate_starts(bbox, patch)
    cand = [(z, y, x) for z in zs for y in ys for x in xs]
    out, rejected = [], {"empty": 0, "bbox": 0, "label": 0}
    if cand:
        count, ext = stats(label, np.array([[z, y, x, *patch] for z, y, x in cand], np.int32))
        vol = patch[0] * patch[1] * patch[2]
        for (z, y, x), c, e in zip(cand, count.tolist(), ext.tolist()):
            rule = P.decide(c, e, vol, bbox_threshold, label_threshold)
            if rule is None:
                out.append({"volume_idx": 0, "start_pos": [z, y, x]})
            else:
                rejected[rule] += 1
    return out, rejected
