"""Label dilation with ball(r): the device kernel against a torch formulation on the same device, the host scipy call, and the
dataset's per-item cost with `dilate.where: host` and `device`.  Prints ONE JSON line.

    python scripts/bench_dilate.py [--parts kernel,torch,scipy,dataset] [--patch 128] [--batch 2] [--radius 5]

The target batch is `--batch` x 1 x patch^3 fp32 holding a sheet-like label: a wavy surface about 3 voxels thick, roughly 2 % of
the voxels on (the kernel's time does not depend on the data, scipy's does).

  kernel   `rx_label_dilate` in place (pack + dilate launches, scratch from the caching allocator): HIP events around regions of one
           call on each of SETS distinct batches -- more bytes between two uses of the same address than the Infinity Cache holds,
           so the rate is an HBM rate -- after a warm-up, median over the rounds; GB/s against the mandatory 8 bytes per voxel (one
           fp32 read, one fp32 write).  The result is compared with `dilate_numpy` bit for bit first.
  torch    the same on the same device without the kernel: F.conv3d of the 0/1 volume with the ball as weights, then `> 0`; same
           regions, alternated with the kernel's.
  scipy    `scipy.ndimage.binary_dilation(t > 0, structure=ball(r))`, seconds per patch, one process, on this machine's CPU
  dataset  `ZarrSegmentationDataset3D.__getitem__`, ms per item, `where: host` and `where: device`, over a small zarr_lite store
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SETS = 24          # 24 x 16.8 MB at cfg2: 400 MB between two uses of the same batch


def sheet_label(shape, period=128):
    """wavy surfaces about 3 voxels thick, one every `period` voxels of y: 2.3 % on at 128, 19 % at 16"""
    z, y, x = np.meshgrid(*[np.arange(n) for n in shape], indexing="ij")
    return np.abs(((y + 6 * np.sin(x / 9.0) + 4 * np.cos(z / 7.0)) % period) - period // 2) < 1.5


def regions(fns, rounds, warmup=2):
    """every fn of `fns` over all its SETS once per region, the fns ALTERNATED round by round; microseconds per call, per fn"""
    import torch
    times = {k: [] for k in fns}
    for rnd in range(warmup + rounds):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for i in range(SETS):
                fn(i)
            b.record()
            b.synchronize()
            if rnd >= warmup:
                times[k].append(1e3 * a.elapsed_time(b) / SETS)
    return times


def bench_device(patch, batch, radius, parts, rounds=9):
    import torch
    import torch.nn.functional as F
    from mt3d_amd.dataloading import dilate_device as D
    from mt3d_amd.engine import ops as E
    shape = (batch, 1, patch, patch, patch)
    lab = np.broadcast_to(sheet_label((patch,) * 3), shape).astype(np.float32)
    host = torch.from_numpy(np.ascontiguousarray(lab))
    voxels = int(np.prod(shape))
    res = {"fraction_on": round(float(lab.mean()), 4), "mandatory_bytes": 8 * voxels}
    want = torch.from_numpy(np.stack([D.dilate_numpy(s, radius) for s in lab]))
    weight = torch.from_numpy(D.ball(radius).astype(np.float32))[None, None].cuda()

    def torch_dilate(x):
        return (F.conv3d((x > 0).to(torch.float32), weight, padding=radius) > 0).to(torch.float32)
    fns = {}
    if "kernel" in parts:
        got = E.label_dilate(host.cuda(), radius)
        res["kernel_bit_identical_to_dilate_numpy"] = bool(torch.equal(got.cpu().view(torch.int32), want.view(torch.int32)))
        sets = [host.cuda() for _ in range(SETS)]
        fns["kernel"] = lambda i: E.label_dilate(sets[i], radius)
    if "torch" in parts:
        got = torch_dilate(host.cuda())
        res["torch_bit_identical_to_dilate_numpy"] = bool(torch.equal(got.cpu().view(torch.int32), want.view(torch.int32)))
        tsets = [host.cuda() for _ in range(SETS)]
        fns["torch"] = lambda i: torch_dilate(tsets[i])
    for k, ts in regions(fns, rounds).items():
        med = float(np.median(ts))
        res[f"{k}_us"] = round(med, 1)
        res[f"{k}_us_min_max"] = [round(min(ts), 1), round(max(ts), 1)]
        res[f"{k}_GBps_of_mandatory"] = round(8 * voxels / med / 1e3, 1)
    if "kernel_us" in res and "torch_us" in res:
        res["torch_over_kernel"] = round(res["torch_us"] / res["kernel_us"], 2)
    try:
        res["device"] = torch.cuda.get_device_name()
        res["sclk_mhz_after"] = int(torch.cuda.clock_rate())          # the clock is left to the governor; read, never set
    except Exception as e:      # (an optional reading: pynvml / amdsmi may be absent)
        res["sclk_mhz_after"] = f"not read ({type(e).__name__})"
    return res


def bench_scipy(patch, radius, reps=3):
    from scipy.ndimage import binary_dilation
    from mt3d_amd.dataloading import dilate_device as D
    lab = sheet_label((patch,) * 3).astype(np.float32)
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        binary_dilation(lab > 0, structure=D.ball(radius)).astype(np.float32)
        ts.append(time.perf_counter() - t0)
    return {"s_per_patch": round(float(np.median(ts)), 3), "s_min_max": [round(min(ts), 3), round(max(ts), 3)]}


def bench_dataset(patch, radius, items=4):
    from types import SimpleNamespace
    from mt3d_amd.dataloading import zarr_lite
    from mt3d_amd.dataloading.dataset import ZarrSegmentationDataset3D
    shape = (patch, patch, patch + patch // 2)
    sheet = sheet_label(shape, period=16)          # sheets throughout the volume, so the valid-patch search keeps every patch
    rng = np.random.default_rng(0)
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        paths = {k: os.path.join(tmp, f"{k}.zarr") for k in ("img", "sheet")}
        zarr_lite.write_array(paths["img"], rng.integers(0, 255, size=shape, dtype=np.uint8), (64, 64, 64))
        zarr_lite.write_array(paths["sheet"], (sheet * 255).astype(np.uint8), (64, 64, 64))
        for where in ("host", "device"):
            mgr = SimpleNamespace(model_name="m", tasks={"sheet": {"channels": 1}}, train_patch_size=(patch,) * 3, min_labeled_ratio=0.01,
                                  min_bbox_percent=0.5, dilate_label=True, use_cache=False, cache_folder=os.path.join(tmp, "cache"),
                                  dataset_config={"augment": False, "dilate": {"where": where, "radius": radius}},
                                  volume_paths=[{"input": paths["img"], "sheet": paths["sheet"], "ref_label": "sheet"}])
            ds = ZarrSegmentationDataset3D(mgr)
            ts = []
            for i in range(min(items, len(ds))):
                t0 = time.perf_counter()
                ds[i]
                ts.append(time.perf_counter() - t0)
            out[f"{where}_ms_per_item"] = round(1e3 * float(np.median(ts)), 1)
            out["items"], out["fraction_on"] = len(ts), round(float(sheet.mean()), 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="kernel,torch,scipy,dataset")
    ap.add_argument("--patch", type=int, default=128)
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--radius", type=int, default=5)
    a = ap.parse_args()
    import mt3d_amd  # noqa: F401
    parts = a.parts.split(",")
    res = {"patch": a.patch, "batch": a.batch, "radius": a.radius}
    if "kernel" in parts or "torch" in parts:
        res["device_side"] = bench_device(a.patch, a.batch, a.radius, parts)
    if "scipy" in parts:
        res["scipy"] = bench_scipy(a.patch, a.radius)
    if "dataset" in parts:
        res["dataset"] = bench_dataset(a.patch, a.radius)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
