"""Augmentation stack, host against device.  Prints ONE JSON line.

    python scripts/bench_augment.py [--parts host,kernels,trainer] [--patch 128] [--batch 2] [--workers 16] [--runs 3]

  host     `augment.augment_image` patches/s on `--workers` processes (what the loader could deliver at best, zarr reading
           excluded) and ms per member, single process
  kernels  the device stack alone on a cfg2-sized batch: us per launch for the pointwise pass (affine, plane, noise), the downscale
           gather and `rx_aug_filter_zy` at k = 3, 7, 21 with its rate in fp32 FLOP/s (2 k^2 per voxel); HIP events around 20
           launches after a warm-up (per-kernel times from a profiler: run this part under `rocprofv3 --kernel-trace --stats --`)
  trainer  `BaseTrainer` on a zarr volume of random uint8 data written with zarr_lite (raw chunks), the three modes
           `augment: false`, `"restated"` with `--workers` loader workers and `"device"`, alternated, `--runs` runs each after a
           warm-up run, medians of the trainer's patches/s (second epoch of each run)
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


def _host_worker(args):
    seed, n, patch = args
    import mt3d_amd  # noqa: F401
    from mt3d_amd.dataloading import augment as A
    rng = np.random.default_rng(seed)
    x = rng.random((patch, patch, patch), dtype=np.float32)
    t0 = time.perf_counter()
    for _ in range(n):
        A.augment_image(x, rng)
    return time.perf_counter() - t0


def bench_host(patch, workers, per_worker=12):
    import multiprocessing as mp
    import mt3d_amd  # noqa: F401
    from mt3d_amd.dataloading import augment as A
    with mp.get_context("spawn").Pool(workers) as pool:
        pool.map(_host_worker, [(s, 1, 16) for s in range(workers)])          # start the interpreters
        t0 = time.perf_counter()
        pool.map(_host_worker, [(s, per_worker, patch) for s in range(workers)])
        wall = time.perf_counter() - t0
    x = np.random.default_rng(0).random((patch, patch, patch), dtype=np.float32)
    members = {}
    for _, group in A.GROUPS:
        for m in group:
            ts = []
            for s in range(3):
                t0 = time.perf_counter()
                m(x.copy(), np.random.default_rng(s))
                ts.append(time.perf_counter() - t0)
            members[m.__name__] = round(1e3 * float(np.median(ts)), 1)
    t0 = time.perf_counter()
    A.coarse_dropout_3d(x, np.random.default_rng(0))
    members["coarse_dropout_3d"] = round(1e3 * (time.perf_counter() - t0), 1)
    return {"workers": workers, "patches_per_s": round(workers * per_worker / wall, 2), "ms_per_member": members}


def bench_kernels(patch, batch, reps=20):
    import torch
    import mt3d_amd  # noqa: F401
    from mt3d_amd.dataloading import augment_device as D
    x = torch.rand((batch, 1, patch, patch, patch), device="cuda")
    aug = D.DeviceAugmenter(seed=0)
    rng = np.random.default_rng(0)
    P = D.AugmentParams

    def kern(k):
        w = rng.random((k, k)).astype(np.float32)
        return w / w.sum()
    cases = {"pointwise_affine": P(g1=("affine", np.float32(1.1), np.float32(0.05)), boxes=[(1, 2, 3, 20, 20, 20)]),
             "pointwise_plane": P(g1=("affine", D._illumination_factor(rng, patch, patch), np.float32(0))),
             "pointwise_noise": P(g2=("noise", np.float32(0.3), 12345)),
             "downscale": P(g3=("downscale", *D._downscale_tables(patch, patch)))}
    cases.update({f"filter_k{k}": P(g3=("filter", kern(k))) for k in (3, 7, 21)})
    out = {}
    vox = batch * patch ** 3
    for name, p in cases.items():
        params = [p] * batch
        for _ in range(3):
            aug(x, params=params)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            aug(x, params=params)
        e1.record()
        torch.cuda.synchronize()
        out[name + "_us"] = round(1e3 * e0.elapsed_time(e1) / reps, 1)
    # a group-3 sample is the pointwise pass (a copy here) + the second pass: subtract the copy to get the filter kernel alone
    copy_us = out["pointwise_affine_us"]
    for k in (3, 7, 21):
        us = max(out[f"filter_k{k}_us"] - copy_us, 1e-3)
        out[f"filter_k{k}_kernel_us"] = round(us, 1)
        out[f"filter_k{k}_tflops"] = round(2.0 * k * k * vox / us * 1e-6, 2)
    # the whole stack as training draws it
    for _ in range(3):
        aug(x)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(200):
        aug(x)
    e1.record()
    torch.cuda.synchronize()
    out["drawn_stack_us_per_batch"] = round(1e3 * e0.elapsed_time(e1) / 200, 1)
    return out


def bench_trainer(patch, batch, workers, runs, steps):
    import yaml
    import mt3d_amd  # noqa: F401
    from mt3d_amd.dataloading import zarr_lite
    from mt3d_amd.train import BaseTrainer
    tmp = tempfile.mkdtemp(prefix="bench_augment_")
    rng = np.random.default_rng(0)
    dim = 3 * patch                                         # 125 half-stride patches: more batches than an epoch runs
    img = rng.integers(0, 255, size=(dim, dim, dim), dtype=np.uint8)
    lab = np.full((dim, dim, dim), 255, np.uint8)
    zarr_lite.write_array(os.path.join(tmp, "img.zarr"), img, (patch // 2,) * 3, compressor=None)
    zarr_lite.write_array(os.path.join(tmp, "sheet.zarr"), lab, (patch // 2,) * 3, compressor=None)
    base = yaml.safe_load(open(os.path.join(ROOT, "tasks", "synthetic_sheet.yaml")))
    os.chdir(tmp)

    def run(mode, nworkers):
        cfg = json.loads(json.dumps(base))
        cfg["tr_setup"].update(model_name="bench_aug", ckpt_out_base=os.path.join(tmp, "ckpt"), tensorboard_log_dir=os.path.join(tmp, "tb"))
        cfg["tr_config"].update(max_epoch=2, max_steps_per_epoch=steps, max_val_steps_per_epoch=0, patch_size=[patch] * 3,
                                batch_size=batch, num_dataloader_workers=nworkers)
        cfg["dataset_config"].update(synthetic=False, min_labeled_ratio=0.05, min_bbox_percent=0.5, use_cache=True,
                                     cache_folder=os.path.join(tmp, "cache"), augment=mode,
                                     volume_paths=[{"input": os.path.join(tmp, "img.zarr"), "sheet": os.path.join(tmp, "sheet.zarr"),
                                                    "ref_label": "sheet"}])
        path = os.path.join(tmp, "cfg.yaml")
        yaml.safe_dump(cfg, open(path, "w"))
        tr = BaseTrainer(path, verbose=False)
        tr._log = lambda *a: None
        tr.train()
        return tr.last_patches_per_sec
    modes = {"false": (False, 0), "restated": ("restated", workers), "device": ("device", 0)}
    got = {k: [] for k in modes}
    run(False, 0)                                           # warm-up: plans, weight packs, the patch cache
    for _ in range(runs):
        for name, (mode, nw) in modes.items():              # alternated: clocks drift over a session
            got[name].append(round(run(mode, nw), 2))
    return {name: {"runs": v, "median": float(np.median(v)), "spread": round(max(v) - min(v), 2)} for name, v in got.items()}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="host,kernels,trainer")
    ap.add_argument("--patch", type=int, default=128)
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--steps", type=int, default=40)
    a = ap.parse_args()
    res = {"patch": a.patch, "batch": a.batch}
    parts = a.parts.split(",")
    if "host" in parts:
        res["host"] = bench_host(a.patch, a.workers)
    if "kernels" in parts:
        res["kernels"] = bench_kernels(a.patch, a.batch)
    if "trainer" in parts:
        res["trainer"] = bench_trainer(a.patch, a.batch, a.workers, a.runs, a.steps)
    print(json.dumps(res))
