#!/usr/bin/env python3
"""What the trainer feeds the network and the losses, as SHA-256 digests: the check that a change to the input side (the dataset's
stage blocks, `DeviceFeeder`, `forward_loss`) leaves every batch as it was, byte for byte.

One epoch of `BaseTrainer` -- 3 training steps and 1 validation step, patch 16^3, seeded -- over a small zarr store written to a
temporary directory, with all seven stage blocks on the device (ingest, dilate, geometric, spatial, elastic, augment, patch_search).
A forward pre-hook on the model records the digest of every input batch; every loss function is wrapped to record the digest of
its target.  The run is made twice, each in a fresh child process: behind the feeder and with RX_DEVICE_FEEDER=0.

    python scripts/pipeline_digest.py > digests.txt          # at two commits: the files must not differ

It uses nothing but `BaseTrainer`, its `_build_model` / `_build_loss` hooks and a config file, so it runs unchanged on either side
of such a change."""
import hashlib
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BLOCKS = {
    "augment": "device",
    "ingest": {"where": "device"},
    "dilate": {"where": "device", "radius": 2},
    "geometric": {"flip": {"p": 0.5}, "rot90": {"p": 0.7}, "normal_keys": ["normals"], "where": "device"},
    "spatial": {"rotation": {"axes": ["z", "y", "x"], "max_degrees": 30, "p": 0.8}, "scale": {"range": [0.8, 1.25], "p": 0.5},
                "normal_keys": ["normals"], "image_border": "constant", "where": "device"},
    "elastic": {"spacing": 8, "magnitude": [0.0, 1.25], "p": 0.8, "normal_keys": ["normals"], "image_border": "constant",
                "where": "device"},
    "patch_search": {"where": "device"},
}


def write_volume(tmp):
    """a 40 x 40 x 48 volume: a wavy sheet (uint8 0 / 255), a uint8 image, channels-last uint16 normals on the sheet"""
    import numpy as np
    from mt3d_amd.dataloading import zarr_lite
    rng = np.random.default_rng(0)
    shape = (40, 40, 48)
    z, y, x = np.meshgrid(*[np.arange(n) for n in shape], indexing="ij")
    sheet = np.abs(((y + 4 * np.sin(x / 7.0) + 3 * np.cos(z / 5.0)) % 10) - 5) < 1.0
    img = (sheet * 140 + rng.integers(0, 80, size=shape)).astype(np.uint8)
    nrm = (rng.integers(1, 65535, size=shape + (3,)) * sheet[..., None]).astype(np.uint16)
    paths = {k: os.path.join(tmp, f"{k}.zarr") for k in ("img", "sheet", "normals")}
    zarr_lite.write_array(paths["img"], img, (16, 16, 16), compressor="zlib")
    zarr_lite.write_array(paths["sheet"], (sheet * 255).astype(np.uint8), (16, 16, 16), compressor="zlib")
    zarr_lite.write_array(paths["normals"], nrm, (16, 16, 16, 3), compressor="zlib")
    return paths


def child(tmp):
    import numpy as np
    import torch
    import yaml
    from mt3d_amd.train import BaseTrainer
    paths = write_volume(tmp)
    cfg = yaml.safe_load(open(os.path.join(ROOT, "tasks", "synthetic_sheet.yaml")))
    cfg["tr_setup"].update(model_name="digest", dilate_label=True, ckpt_out_base=os.path.join(tmp, "ckpt"),
                           tensorboard_log_dir=os.path.join(tmp, "tb"))
    cfg["tr_config"].update(max_epoch=1, max_steps_per_epoch=3, max_val_steps_per_epoch=1, patch_size=[16, 16, 16], compile=False)
    cfg["dataset_config"]["targets"]["normals"] = {"channels": 3, "activation": "none", "weight": 1, "loss_fn": "MaskedCosineLoss"}
    cfg["dataset_config"].update(synthetic=False, min_labeled_ratio=0.05, min_bbox_percent=0.5, use_cache=False,
                                 cache_folder=os.path.join(tmp, "cache"),
                                 volume_paths=[{"input": paths["img"], "sheet": paths["sheet"], "normals": paths["normals"],
                                                "ref_label": "sheet"}], **BLOCKS)
    path = os.path.join(tmp, "cfg.yaml")
    yaml.safe_dump(cfg, open(path, "w"))
    os.chdir(tmp)
    lines = []

    def digest(what, t):
        a = t.detach().contiguous().cpu()
        lines.append(f"{what} {a.dtype} {tuple(a.shape)} {hashlib.sha256(a.view(torch.uint8).numpy().tobytes()).hexdigest()}")

    class Rec(BaseTrainer):
        def _build_model(self):
            model = super()._build_model()
            model.register_forward_pre_hook(lambda module, args: digest("input", args[0]))
            return model

        def _build_loss(self):
            def wrap(name, fn):
                def f(pred, gt):
                    digest(f"target {name}", gt)
                    return fn(pred, gt)
                return f
            return {k: wrap(k, v) for k, v in super()._build_loss().items()}

    torch.manual_seed(1234)
    np.random.seed(1234)
    Rec(path, verbose=False).train()
    torch.cuda.synchronize()
    assert len(lines) == 3 * (3 + 1), lines          # per step: the input and the two targets
    for i, ln in enumerate(lines):
        print(f"DIGEST {i:02d} {ln}")


def main():
    if len(sys.argv) == 3 and sys.argv[1] == "--child":
        return child(sys.argv[2])
    for feeder in ("1", "0"):
        with tempfile.TemporaryDirectory() as tmp:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", tmp], capture_output=True, text=True, timeout=900,
                               env=dict(os.environ, RX_DEVICE_FEEDER=feeder))
        if r.returncode != 0:
            sys.exit(f"RX_DEVICE_FEEDER={feeder}: exit {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}")
        for ln in r.stdout.splitlines():
            if ln.startswith("DIGEST "):
                print(f"feeder={feeder} {ln[7:]}")


if __name__ == "__main__":
    main()
