"""Flip / rot90 with normals, device kernel against the torch formulation and the host classes.  Prints ONE JSON line.

    python scripts/bench_geometry.py [--parts kernels,host,trainer] [--patch 128] [--batch 2] [--runs 3]

  kernels  per op class on the cfg2 batch (`--batch` x {image 1 ch, sheet 1 ch, normals 3 ch} x patch^3 fp32): `rx_geom_apply`
           on the three tensors against the same op written with torch on the same device (permute / flip / component index /
           sign constant built once / contiguous).  Device-synchronised regions of 10 applications after a warm-up, the two sides
           ALTERNATED, medians over 7 rounds, rotating through 4 input batches with the last 4 outputs kept alive (more bytes
           between two uses of the same address than the Infinity Cache holds); GB/s counts one read and one write of the batch.
           The results of both sides are compared bit for bit.
  host     the host classes (numpy), ms per item of the same three arrays, one thread, per op class
  trainer  `BaseTrainer` on synthetic patches with a sheet and a normals task, `geometric` absent and `where: device`, alternated,
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


def op_classes():
    import mt3d_amd  # noqa: F401
    from mt3d_amd.dataloading import geometry_device as G
    return {"flip_z": G.flip_op(0), "flip_y": G.flip_op(1), "flip_x": G.flip_op(2), "rot_x_90": G.rot90_op("x", 1),
            "rot_z_90": G.rot90_op("z", 1), "rot_y_90": G.rot90_op("y", 1), "rot_z_180": G.rot90_op("z", 2),
            "flip_zx_rot_y_270": G.compose(G.compose(G.flip_op(0), G.flip_op(2)), G.rot90_op("y", 3)),
            "flip_y_rot_z_90_rot_x_90": G.compose(G.compose(G.flip_op(1), G.rot90_op("z", 1)), G.rot90_op("x", 1))}


def torch_apply(t, op, vector, sign=None):
    """the op in torch: what a user would write without the kernel (`sign`: the (1, 3, 1, 1, 1) device constant of `ch_neg`,
    built once by the caller)"""
    y = t.permute(0, 1, 2 + op.src_axis[0], 2 + op.src_axis[1], 2 + op.src_axis[2])
    dims = [2 + d for d in range(3) if op.flip[d]]
    if dims:
        y = y.flip(dims)
    if vector:
        if op.ch_src != (0, 1, 2):
            y = y[:, list(op.ch_src)]
        if any(op.ch_neg):
            y = y * sign
    return y.contiguous()


def bench_kernels(patch, batch, rounds=7, reps=10):
    import torch
    from mt3d_amd.engine import ops as E
    g = torch.Generator(device="cuda").manual_seed(0)
    # SETS distinct input batches in turn, and the outputs of the last SETS applications kept alive so that the allocator hands
    # out other addresses: at cfg2 sizes 4 x (84 MB in + 84 MB out) pass between two uses of the same bytes, more than the
    # 256 MiB Infinity Cache holds -- the rates below are HBM rates, not cache rates
    SETS = 4
    sets = [{k: torch.randn((batch, c, patch, patch, patch), device="cuda", generator=g) for k, c in
             (("image", 1), ("sheet", 1), ("normals", 3))} for _ in range(SETS)]
    tensors = sets[0]
    nbytes = 2 * sum(t.numel() * 4 for t in tensors.values())
    turn, alive = [0], []

    def rotating(fn):
        def run():
            alive.append(fn(sets[turn[0] % SETS]))
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
    out = {}
    for name, op in op_classes().items():
        table = E.geom_table([op] * batch)

        sign = torch.tensor([-1.0 if n else 1.0 for n in op.ch_neg], device="cuda").view(1, 3, 1, 1, 1)

        def ours(ts=tensors):
            return [E.geom_apply(t, table, k == "normals") for k, t in ts.items()]

        def theirs(ts=tensors):
            return [torch_apply(t, op, k == "normals", sign) for k, t in ts.items()]
        same = all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(ours(), theirs()))
        for _ in range(3):
            ours(), theirs()
        a, b = [], []
        for _ in range(rounds):
            a.append(region(rotating(ours)))
            alive.clear()
            b.append(region(rotating(theirs)))
            alive.clear()
        ka, kb = float(np.median(a)), float(np.median(b))
        out[name] = {"kernel_us": round(1e6 * ka, 1), "kernel_GBps": round(nbytes / ka / 1e9, 1), "torch_us": round(1e6 * kb, 1),
                     "torch_GBps": round(nbytes / kb / 1e9, 1), "torch_over_kernel": round(kb / ka, 2), "bit_identical": bool(same),
                     "kernel_us_min_max": [round(1e6 * min(a), 1), round(1e6 * max(a), 1)]}
    return {"batch_bytes_read_plus_written": nbytes, "ops": out}


def bench_host(patch):
    from mt3d_amd.dataloading import geometry_device as G
    rng = np.random.default_rng(0)
    item = {"image": rng.random((patch,) * 3, dtype=np.float32), "sheet": rng.random((1, *(patch,) * 3), dtype=np.float32),
            "normals": rng.standard_normal((3, *(patch,) * 3)).astype(np.float32)}
    out = {}
    for name, op in op_classes().items():
        ts = []
        for _ in range(3):
            t0 = time.perf_counter()
            for k, v in item.items():
                G.apply_op_numpy(op, v, k == "normals")
            ts.append(time.perf_counter() - t0)
        out[name] = round(1e3 * float(np.median(ts)), 1)
    return {"ms_per_item": out}


def _trainer_once(tmp, patch, batch, steps, geometric):
    import yaml
    from mt3d_amd.train import BaseTrainer
    cfg = yaml.safe_load(open(os.path.join(ROOT, "tasks", "synthetic_sheet.yaml")))
    cfg["tr_setup"].update(model_name="geom_bench", ckpt_out_base=os.path.join(tmp, "ckpt"), tensorboard_log_dir=os.path.join(tmp, "tb"))
    cfg["tr_config"].update(max_epoch=2, max_steps_per_epoch=steps, max_val_steps_per_epoch=1, patch_size=[patch] * 3,
                            batch_size=batch, compile=False)
    cfg["dataset_config"]["targets"]["normals"] = {"channels": 3, "activation": "none", "weight": 1, "loss_fn": "MaskedCosineLoss"}
    cfg["dataset_config"].update(synthetic_length=max(64, 2 * steps * batch))
    if geometric:
        cfg["dataset_config"]["geometric"] = {"flip": {"p": 0.5}, "rot90": {"p": 0.5}, "normal_keys": ["normals"], "where": "device"}
    p = os.path.join(tmp, f"cfg_{int(geometric)}.yaml")
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
