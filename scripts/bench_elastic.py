"""Elastic deformation with normals: the device kernel against a plain device copy, a torch formulation and the host statement
(DESIGN §21).  Prints ONE JSON line.

    python scripts/bench_elastic.py [--parts kernels,host] [--patch 128] [--batch 2] [--spacing 32]

  kernels  on the cfg2 batch (`--batch` x {image 1 ch linear, sheet 1 ch nearest, normals 3 ch nearest + vector rule} x patch^3
           fp32, nodes at the largest magnitude the parser allows): `rx_elastic_apply` per tensor, a plain device copy of the same
           tensor (`out.copy_(t)`: the floor of any pass that reads and writes it once), and the same deformation written with
           torch on the same device (the dense field from the same nodes as three small matrix products per component, then
           `grid_sample`, align_corners=True; normals: the Jacobian the same way and the covector rule in tensor ops).
           Device-synchronised regions of 10 applications after a warm-up, the three sides ALTERNATED, medians over 7 rounds,
           rotating through 4 input batches with the last 4 outputs kept alive (more bytes between two uses of the same address
           than the Infinity Cache holds).  The torch side is compared with the kernel within a tolerance (it is not bit-exact);
           the kernel's bits are the GPU tests' business.
  host     `elastic_numpy` (the `where: host` path), ms per item of the same three arrays, one thread
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# per key: channels, interp, border, vector
KEYS = {"image": (1, "linear", "constant", False), "sheet": (1, "nearest", "constant", False), "normals": (3, "nearest", "constant", True)}


def make_fields(patch, batch, spacing):
    import mt3d_amd  # noqa: F401
    from mt3d_amd.dataloading import elastic_device as M
    sp = (spacing,) * 3
    amp = spacing / 6.0 * 0.999
    rng = np.random.default_rng(0)
    return [M.ElasticField(rng.uniform(-amp, amp, (3,) + M.grid_shape((patch,) * 3, sp)), sp) for _ in range(batch)]


def dense_basis(n, s, device):
    """[n, G] weight and derivative matrices of one axis, from the kernel's own tables"""
    import torch
    from mt3d_amd.dataloading.elastic_device import bspline_tables
    idx, w, dw = bspline_tables(n, s)
    G = (n - 1) // s + 4
    W, DW = np.zeros((n, G), dtype=np.float32), np.zeros((n, G), dtype=np.float32)
    for a in range(4):
        W[np.arange(n), idx + a], DW[np.arange(n), idx + a] = w[:, a], dw[:, a]
    return torch.from_numpy(W).to(device), torch.from_numpy(DW).to(device)


def torch_apply(t, nodes, basis, mode, vector):
    """what a user would write without the kernel"""
    import torch
    (Wz, DWz), (Wy, DWy), (Wx, DWx) = basis
    Z, Y, X = t.shape[2:]

    def field(bz, by, bx):
        return torch.einsum("bcijk,zi,yj,xk->bczyx", nodes, bz, by, bx)
    D = field(Wz, Wy, Wx)
    base = torch.stack(torch.meshgrid(torch.arange(Z, device=t.device, dtype=torch.float32), torch.arange(Y, device=t.device, dtype=torch.float32),
                                      torch.arange(X, device=t.device, dtype=torch.float32), indexing="ij"))
    p = base[None] + D                                                       # (B, 3, Z, Y, X), (z, y, x)
    half = torch.tensor([(Z - 1) / 2.0, (Y - 1) / 2.0, (X - 1) / 2.0], device=t.device).view(1, 3, 1, 1, 1)
    grid = (p / half - 1.0).flip(1).permute(0, 2, 3, 4, 1)                   # (x, y, z) last
    y = torch.nn.functional.grid_sample(t, grid, mode=mode, padding_mode="zeros", align_corners=True)
    if vector:
        E = torch.stack([field(DWz, Wy, Wx), field(Wz, DWy, Wx), field(Wz, Wy, DWx)], dim=2)      # [b][d][e]
        n = y.flip(1)                                                                             # (n_z, n_y, n_x)
        tt = n + torch.einsum("bdezyx,bdzyx->bezyx", E, n)
        q, r = (y * y).sum(1, keepdim=True), (tt * tt).sum(1, keepdim=True)
        k = torch.where(r > 0, torch.sqrt(q / torch.where(r > 0, r, torch.ones_like(r))), torch.zeros_like(r))
        y = (tt * k).flip(1)
    return y


def bench_kernels(patch, batch, spacing, rounds=7, reps=10):
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
    fields = make_fields(patch, batch, spacing)
    sp = fields[0].spacing
    nodes, tables = E.elastic_nodes(fields), E.elastic_tables((patch,) * 3, sp)
    basis = [dense_basis(patch, spacing, "cuda") for _ in range(3)]
    res = {}
    for key, (c, interp, border, vector) in KEYS.items():
        def ours(t):
            return E.elastic_apply(t, nodes, tables, sp, interp, border, 0.0, vector)

        def theirs(t):
            return torch_apply(t, nodes, basis, "bilinear" if interp == "linear" else "nearest", vector)
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
    t0 = time.perf_counter()
    for _ in range(20):
        E.elastic_nodes(fields)
    torch.cuda.synchronize()
    res["nodes_upload_us"] = round(1e6 * (time.perf_counter() - t0) / 20, 1)
    return {"bytes_read_plus_written": nbytes, "library": os.environ.get("RX_LIBRARY", "default"), "keys": res}


def bench_host(patch, spacing):
    from mt3d_amd.dataloading import elastic_device as M
    rng = np.random.default_rng(0)
    item = {"image": rng.random((1, *(patch,) * 3), dtype=np.float32), "sheet": rng.random((1, *(patch,) * 3), dtype=np.float32),
            "normals": rng.standard_normal((3, *(patch,) * 3)).astype(np.float32)}
    field = make_fields(patch, 1, spacing)[0]
    ts = []
    for _ in range(3):
        t0 = time.perf_counter()
        M.apply_item_numpy(field, item)
        ts.append(time.perf_counter() - t0)
    return {"ms_per_item": round(1e3 * float(np.median(ts)), 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="kernels,host")
    ap.add_argument("--patch", type=int, default=128)
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--spacing", type=int, default=32)
    a = ap.parse_args()
    import mt3d_amd  # noqa: F401
    res = {"patch": a.patch, "batch": a.batch, "spacing": a.spacing}
    parts = a.parts.split(",")
    if "kernels" in parts:
        res["kernels"] = bench_kernels(a.patch, a.batch, a.spacing)
    if "host" in parts:
        res["host"] = bench_host(a.patch, a.spacing)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
