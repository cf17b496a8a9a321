"""Ingest (float32 conversion, dtype scaling, channels-last transpose): the device kernel against the torch formulation on the same
device, the dataset's per-item cost with `ingest.where: host` and `device`, and the trainer's patches/s both ways.
Prints ONE JSON line.

    python scripts/bench_ingest.py [--parts kernel,torch,dataset,trainer] [--patch 128] [--batch 2] [--epochs 3]

  kernel   `rx_ingest` for the three tensors of an image + sheet + normals batch: uint8 (B, p, p, p) under div255 and uint16
           channels-last (B, p, p, p, 3) under normal_u16 (and uint16 / float32 flat, for the other widths).  HIP events around
           regions of one call on each of SETS distinct input / output pairs -- more bytes between two uses of the same address
           than the Infinity Cache holds, so the rate is an HBM rate -- after a warm-up, median over the rounds; GB/s against the
           mandatory bytes (the input at its storage width once, 4 bytes per element out).  Compared with `ingest_numpy` bit for
           bit first.
  torch    the same on the same device without the kernel: `x.to(float32) / 255` and
           `(x.to(float32) / 32767.5 - 1).permute(0, 4, 1, 2, 3).contiguous()`; same regions, alternated with the kernel's.
  dataset  `ZarrSegmentationDataset3D.__getitem__`, ms per item, `where: host` and `where: device`, over an uncompressed zarr_lite
           store of uint8 image, uint8 sheet and uint16 channels-last normals; and the bytes of one item either way
  trainer  `BaseTrainer` on that store (autoconfigured model, batch `--batch`, augment false, no dilation), patches/s of the last
           of `--epochs` epochs, `where: host` then `where: device`, each in a process of its own
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SETS = 16          # 16 x (input + 16.8 MB of output per channel) at 2 x 128^3: at least 330 MB between two uses of the same pair


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


def torch_ingest(x, rule):
    import torch
    t = x.to(torch.float32)
    t = {"copy": lambda: t, "div255": lambda: t / 255.0, "div65535": lambda: t / 65535.0, "normal_u16": lambda: t / 32767.5 - 1.0,
         "normal_mul2": lambda: t * 2.0 - 1.0}[rule]()
    return t.unsqueeze(1) if t.dim() == 4 else t.permute(0, 4, 1, 2, 3).contiguous()


def bench_device(patch, batch, parts, rounds=9):
    import torch
    from mt3d_amd.dataloading import ingest_device as I
    from mt3d_amd.engine import ops as E
    rng = np.random.default_rng(0)
    cases = {"image_u8_div255": (np.uint8, (), "div255"), "normals_u16x3_normal_u16": (np.uint16, (3,), "normal_u16"),
             "image_u16_div65535": (np.uint16, (), "div65535"), "image_f32_copy": (np.float32, (), "copy")}
    res = {}
    for name, (dt, tail, rule) in cases.items():
        shape = (batch, patch, patch, patch) + tail
        a = (rng.random(shape, dtype=np.float32) if dt == np.float32
             else rng.integers(0, np.iinfo(dt).max, size=shape, endpoint=True).astype(dt))
        host = torch.from_numpy(a)
        n = a.size
        mandatory = n * (a.itemsize + 4)
        r = {"mandatory_bytes": mandatory}
        want = np.stack([I.ingest_numpy(s, rule) for s in a[:1]]).view(np.uint32)
        ins = [host.cuda() for _ in range(SETS)]
        outs = [torch.empty((batch, tail[0] if tail else 1, patch, patch, patch), device="cuda") for _ in range(SETS)]
        fns = {}
        if "kernel" in parts:
            got = E.ingest(ins[0], rule, out=outs[0])[:1].cpu().numpy().view(np.uint32)
            r["kernel_bit_identical_to_ingest_numpy"] = bool(np.array_equal(got, want))
            fns["kernel"] = lambda i: E.ingest(ins[i], rule, out=outs[i])
        if "torch" in parts:
            got = torch_ingest(ins[0], rule)[:1].cpu().numpy().view(np.uint32)
            r["torch_bit_identical_to_ingest_numpy"] = bool(np.array_equal(got, want))
            fns["torch"] = lambda i: torch_ingest(ins[i], rule)
        for k, ts in regions(fns, rounds).items():
            med = float(np.median(ts))
            r[f"{k}_us"] = round(med, 1)
            r[f"{k}_us_min_max"] = [round(min(ts), 1), round(max(ts), 1)]
            r[f"{k}_GBps_of_mandatory"] = round(mandatory / med / 1e3, 1)
        if "kernel_us" in r and "torch_us" in r:
            r["torch_over_kernel"] = round(r["torch_us"] / r["kernel_us"], 2)
        res[name] = r
        del ins, outs
        torch.cuda.empty_cache()
    try:
        res["device"] = torch.cuda.get_device_name()
        res["sclk_mhz_after"] = int(torch.cuda.clock_rate())          # the clock is left to the governor; read, never set
    except Exception as e:      # (an optional reading: pynvml / amdsmi may be absent)
        res["sclk_mhz_after"] = f"not read ({type(e).__name__})"
    return res


def write_store(tmp, patch):
    """uint8 image, uint8 sheet (sheets throughout, so the valid-patch search keeps every patch) and uint16 channels-last normals,
    uncompressed: (1.5 p, 1.5 p, 2 p) holds 2 x 2 x 3 = 12 patches at the half-patch stride"""
    from mt3d_amd.dataloading import zarr_lite
    shape = (patch + patch // 2, patch + patch // 2, 2 * patch)
    z, y, x = np.meshgrid(*[np.arange(n) for n in shape], indexing="ij")
    sheet = np.abs(((y + 6 * np.sin(x / 9.0) + 4 * np.cos(z / 7.0)) % 16) - 8) < 1.5
    rng = np.random.default_rng(0)
    paths = {k: os.path.join(tmp, f"{k}.zarr") for k in ("img", "sheet", "normals")}
    ch = (min(64, patch),) * 3
    zarr_lite.write_array(paths["img"], rng.integers(0, 255, size=shape, dtype=np.uint8), ch)
    zarr_lite.write_array(paths["sheet"], (sheet * 255).astype(np.uint8), ch)
    zarr_lite.write_array(paths["normals"], rng.integers(0, 65535, size=shape + (3,), dtype=np.uint16), ch + (3,))
    return paths


def bench_dataset(patch, items=8):
    from types import SimpleNamespace
    from mt3d_amd.dataloading.dataset import ZarrSegmentationDataset3D
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        paths = write_store(tmp, patch)
        for where in ("host", "device"):
            mgr = SimpleNamespace(model_name="m", tasks={"sheet": {"channels": 1}, "normals": {"channels": 3}}, train_patch_size=(patch,) * 3,
                                  min_labeled_ratio=0.01, min_bbox_percent=0.5, dilate_label=False, use_cache=False,
                                  cache_folder=os.path.join(tmp, "cache"), dataset_config={"augment": False, "ingest": {"where": where}},
                                  volume_paths=[{"input": paths["img"], "sheet": paths["sheet"], "normals": paths["normals"],
                                                 "ref_label": "sheet"}])
            ds = ZarrSegmentationDataset3D(mgr)
            ds[0]
            ts = []
            for i in range(min(items, len(ds))):
                t0 = time.perf_counter()
                item = ds[i]
                ts.append(time.perf_counter() - t0)
            out[f"{where}_ms_per_item"] = round(1e3 * float(np.median(ts)), 2)
            out[f"{where}_ms_min_max"] = [round(1e3 * min(ts), 2), round(1e3 * max(ts), 2)]
            out[f"{where}_item_bytes"] = int(sum(v.numel() * v.element_size() for v in item.values()))
            out["items"] = len(ts)
    return out


def trainer_child(tmp, where, patch, batch, epochs):
    """one BaseTrainer run in this process; prints the patches/s of every epoch"""
    import yaml
    import torch
    import mt3d_amd  # noqa: F401
    from mt3d_amd.train import BaseTrainer
    paths = {k: os.path.join(tmp, f"{k}.zarr") for k in ("img", "sheet", "normals")}
    cfg = yaml.safe_load(open(os.path.join(ROOT, "tasks", "synthetic_sheet.yaml")))
    run = os.path.join(tmp, f"run_{where}")
    cfg["tr_setup"].update(model_name=f"ingest_{where}", ckpt_out_base=os.path.join(run, "ckpt"), tensorboard_log_dir=os.path.join(run, "tb"))
    cfg["tr_config"].update(max_epoch=epochs, max_steps_per_epoch=1000, max_val_steps_per_epoch=1, patch_size=[patch] * 3,
                            batch_size=batch, compile=False)
    cfg["dataset_config"]["targets"]["normals"] = {"channels": 3, "activation": "none", "weight": 1, "loss_fn": "MaskedCosineLoss"}
    cfg["dataset_config"].update(synthetic=False, min_labeled_ratio=0.01, min_bbox_percent=0.5, use_cache=False,
                                 cache_folder=os.path.join(run, "cache"), augment=False, ingest={"where": where},
                                 volume_paths=[{"input": paths["img"], "sheet": paths["sheet"], "normals": paths["normals"],
                                                "ref_label": "sheet"}])
    os.makedirs(run, exist_ok=True)
    p = os.path.join(run, "cfg.yaml")
    yaml.safe_dump(cfg, open(p, "w"))
    os.chdir(run)
    rates = []

    class Rec(BaseTrainer):
        def _log(self, *a):
            if self.last_patches_per_sec is not None and (not rates or rates[-1] != self.last_patches_per_sec):
                rates.append(self.last_patches_per_sec)

    torch.manual_seed(0)
    Rec(p, verbose=False).train()
    print("RATES", json.dumps([round(r, 2) for r in rates]), flush=True)


def bench_trainer(patch, batch, epochs):
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        write_store(tmp, patch)
        for where in ("host", "device"):
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--trainer-child", tmp, where, "--patch", str(patch), "--batch",
                                str(batch), "--epochs", str(epochs)], capture_output=True, text=True, timeout=900)
            if r.returncode != 0:
                raise RuntimeError(f"trainer run ({where}) failed:\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}")
            rates = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RATES ")][-1][6:])
            out[f"{where}_patches_per_s_by_epoch"] = rates
            out[f"{where}_patches_per_s"] = rates[-1]
    out["device_over_host"] = round(out["device_patches_per_s"] / out["host_patches_per_s"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="kernel,torch,dataset,trainer")
    ap.add_argument("--patch", type=int, default=128)
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--trainer-child", nargs=2, metavar=("STORE", "WHERE"), default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.trainer_child:
        return trainer_child(a.trainer_child[0], a.trainer_child[1], a.patch, a.batch, a.epochs)
    import mt3d_amd  # noqa: F401
    parts = a.parts.split(",")
    res = {"patch": a.patch, "batch": a.batch}
    if "kernel" in parts or "torch" in parts:
        res["device_side"] = bench_device(a.patch, a.batch, parts)
    if "dataset" in parts:
        res["dataset"] = bench_dataset(a.patch)
    if "trainer" in parts:
        res["trainer"] = bench_trainer(a.patch, a.batch, a.epochs)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
