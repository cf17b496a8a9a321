"""Rotation / scaling with normals: the device kernel against a plain device copy, the torch formulation and the host statement
(DESIGN §19).  Prints ONE JSON line.

    python scripts/bench_spatial.py [--parts kernels,host,trainer] [--patch 128] [--batch 2] [--runs 3]

  kernels  per op class on the cfg2 batch (`--batch` x {image 1 ch linear, sheet 1 ch nearest, normals 3 ch nearest + vector rule}
           x patch^3 fp32): `rx_affine_apply` per tensor, a plain device copy of the same tensor (`out.copy_(t)`: the floor of any
           pass that reads and writes it once), and the same resampling written with torch on the same device (`affine_grid` +
           `grid_sample`, align_corners=True; normals: the component matrix applied with an einsum afterwards).  Device-synchronised
           regions of 10 applications after a warm-up, the three sides ALTERNATED, medians over 7 rounds, rotating through 4 input
           batches with the last 4 outputs kept alive (more bytes between two uses of the same address than the Infinity Cache
           holds).  The torch side is compared with the kernel within a tolerance (it is not bit-exact: float32 normalised
           coordinates); the kernel's bits are the GPU tests' business.
  host     `affine_numpy` (the `where: host` path), ms per item of the same three arrays, one thread, per op class
  trainer  `BaseTrainer` on synthetic patches with a sheet and a normals task, `spatial` absent and `where: device`, alternated,
           `--runs` runs each after a warm-up run: the trainer's patches/s of the last epoch, medians and the spread
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

# per key: channels, interp, border, vector
KEYS = {"image": (1, "linear", "constant", False), "sheet": (1, "nearest", "constant", False), "normals": (3, "nearest", "constant", True)}


def op_classes():
    import mt3d_amd  # noqa: F401
    from mt3d_amd.dataloading import spatial_device as S
    return {"rot_z_30": S.rotation_op("z", 30.0), "rot_y_30": S.rotation_op("y", 30.0), "rot_x_30": S.rotation_op("x", 30.0),
            "rot_zyx_30_20_10": S.compose(S.compose(S.rotation_op("z", 30.0), S.rotation_op("y", 20.0)), S.rotation_op("x", 10.0)),
            "rot_y_45": S.rotation_op("y", 45.0), "scale_0.8": S.scale_op(0.8), "scale_1.25": S.scale_op(1.25),
            "rot_zyx_scale_1.25": S.compose(S.compose(S.compose(S.rotation_op("z", 30.0), S.rotation_op("y", 20.0)), S.rotation_op("x", 10.0)),
                                            S.scale_op(1.25))}


def torch_theta(op, shape, batch, device):
    """`point` as the theta of affine_grid (align_corners=True): (x, y, z) order, rescaled by the half extents"""
    import torch
    n = np.array(shape, dtype=np.float64)
    half = (n[::-1] - 1.0) / 2.0
    theta = np.zeros((3, 4))
    theta[:, :3] = op.point.astype(np.float64)[::-1, ::-1] * half[None, :] / half[:, None]
    return torch.tensor(theta, dtype=torch.float32, device=device).expand(batch, 3, 4).contiguous()


def torch_apply(t, theta, mode, vec):
    """what a user would write without the kernel (`vec`: the (3, 3) device matrix of a vector tensor, None otherwise)"""
    import torch
    grid = torch.nn.functional.affine_grid(theta, list(t.shape), align_corners=True)
    y = torch.nn.functional.grid_sample(t, grid, mode=mode, padding_mode="zeros", align_corners=True)
    if vec is not None:
        y = torch.einsum("ck,bkzyx->bczyx", vec, y)
    return y


def bench_kernels(patch, batch, rounds=7, reps=10):
    import torch
    from mt3d_amd.engine import ops as E
    g = torch.Generator(device="cuda").manual_seed(0)
    SETS = 4
    sets = [{k: torch.randn((batch, c, patch, patch, patch), device="cuda", generator=g) for k, (c, _, _, _) in KEYS.items()}
            for _ in range(SETS)]
    nbytes = {k: 2 * t.numel() * 4 for k, t in sets[0].items()}
    turn, alive = [0], []

    def rotating(fn, key):
        def run():
            alive.append(fn(sets[turn[0] % SETS][key]))
            turn[0] += 1
            if len(alive) > SETS:
                alive.pop(0)
        return run

    def region(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / reps

    def copy(t):
        return torch.empty_like(t).copy_(t)
    out = {}
    for name, op in op_classes().items():
        table = E.affine_table([op] * batch)
        theta = torch_theta(op, (patch,) * 3, batch, "cuda")
        vec = torch.tensor(op.vector, device="cuda")
        res = {}
        for key, (c, interp, border, vector) in KEYS.items():
            def ours(t):
                return E.affine_apply(t, table, interp, border, 0.0, vector)

            def theirs(t):
                return torch_apply(t, theta, "bilinear" if interp == "linear" else "nearest", vec if vector else None)
            a0, b0 = ours(sets[0][key]), theirs(sets[0][key])
            diff = (a0 - b0).abs()
            # nearest: a coordinate within float32 rounding of a half-integer may pick the neighbour; report the share that differs
            agree = {"max_abs_diff": float(diff.max()), "share_differing": float((diff > 1e-3).float().mean())}
            del a0, b0, diff
            for _ in range(3):
                ours(sets[1][key]), theirs(sets[1][key]), copy(sets[1][key])
            ta, tb, tc = [], [], []
            for _ in range(rounds):
                for fn, acc in ((ours, ta), (copy, tc), (theirs, tb)):
                    acc.append(region(rotating(fn, key)))
                    alive.clear()
            ka, kb, kc = float(np.median(ta)), float(np.median(tb)), float(np.median(tc))
            res[key] = {"kernel_us": round(1e6 * ka, 1), "copy_us": round(1e6 * kc, 1), "torch_us": round(1e6 * kb, 1),
                        "kernel_over_copy": round(ka / kc, 2), "torch_over_kernel": round(kb / ka, 2),
                        "kernel_GBps": round(nbytes[key] / ka / 1e9, 1), "copy_GBps": round(nbytes[key] / kc / 1e9, 1),
                        "kernel_us_min_max": [round(1e6 * min(ta), 1), round(1e6 * max(ta), 1)], "torch_vs_kernel": agree}
        res["batch_kernel_us"] = round(sum(res[k]["kernel_us"] for k in KEYS), 1)
        res["batch_copy_us"] = round(sum(res[k]["copy_us"] for k in KEYS), 1)
        res["batch_torch_us"] = round(sum(res[k]["torch_us"] for k in KEYS), 1)
        out[name] = res
    return {"bytes_read_plus_written": nbytes, "library": os.environ.get("RX_LIBRARY", "default"), "ops": out}


def bench_host(patch):
    from mt3d_amd.dataloading import spatial_device as S
    rng = np.random.default_rng(0)
    item = {"image": rng.random((1, *(patch,) * 3), dtype=np.float32), "sheet": rng.random((1, *(patch,) * 3), dtype=np.float32),
            "normals": rng.standard_normal((3, *(patch,) * 3)).astype(np.float32)}
    out = {}
    for name, op in list(op_classes().items())[:4]:
        ts = []
        for _ in range(3):
            t0 = time.perf_counter()
            S.apply_item_numpy(op, item)
            ts.append(time.perf_counter() - t0)
        out[name] = round(1e3 * float(np.median(ts)), 1)
    return {"ms_per_item": out}


def _trainer_once(tmp, patch, batch, steps, spatial):
    import yaml
    from mt3d_amd.train import BaseTrainer
    cfg = yaml.safe_load(open(os.path.join(ROOT, "tasks", "synthetic_sheet.yaml")))
    cfg["tr_setup"].update(model_name="spatial_bench", ckpt_out_base=os.path.join(tmp, "ckpt"), tensorboard_log_dir=os.path.join(tmp, "tb"))
    cfg["tr_config"].update(max_epoch=2, max_steps_per_epoch=steps, max_val_steps_per_epoch=1, patch_size=[patch] * 3,
                            batch_size=batch, compile=False)
    cfg["dataset_config"]["targets"]["normals"] = {"channels": 3, "activation": "none", "weight": 1, "loss_fn": "MaskedCosineLoss"}
    cfg["dataset_config"].update(synthetic_length=max(64, 2 * steps * batch))
    if spatial:          # every sample rotated and scaled: the stage's full cost on every batch
        cfg["dataset_config"]["spatial"] = {"rotation": {"axes": ["z", "y", "x"], "max_degrees": 30, "p": 1.0},
                                            "scale": {"range": [0.8, 1.25], "p": 1.0}, "normal_keys": ["normals"], "where": "device"}
    p = os.path.join(tmp, f"cfg_{int(spatial)}.yaml")
    yaml.safe_dump(cfg, open(p, "w"))
    tr = BaseTrainer(p, verbose=False)
    tr.train()
    return float(tr.last_patches_per_sec)


def bench_trainer(patch, batch, runs, steps=24):
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)
        _trainer_once(tmp, patch, batch, 4, True)          # warm-up: library, allocator, kernels
        off, on = [], []
        for _ in range(runs):
            off.append(_trainer_once(tmp, patch, batch, steps, False))
            on.append(_trainer_once(tmp, patch, batch, steps, True))
    return {"patches_per_s_off": [round(v, 2) for v in off], "patches_per_s_on": [round(v, 2) for v in on],
            "median_off": round(float(np.median(off)), 2), "median_on": round(float(np.median(on)), 2),
            "spread_off": round(max(off) - min(off), 2), "spread_on": round(max(on) - min(on), 2), "steps_per_epoch": steps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="kernels,host,trainer")
    ap.add_argument("--patch", type=int, default=128)
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--runs", type=int, default=3)
    a = ap.parse_args()
    import mt3d_amd  # noqa: F401
    res = {"patch": a.patch, "batch": a.batch}
    parts = a.parts.split(",")
    if "kernels" in parts:
        res["kernels"] = bench_kernels(a.patch, a.batch)
    if "host" in parts:
        res["host"] = bench_host(a.patch)
    if "trainer" in parts:
        res["trainer"] = bench_trainer(a.patch, a.batch, a.runs)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
