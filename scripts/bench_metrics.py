"""Validation-metric kernels against the torch formulation of the same counts and sums on the same device.  Prints ONE
JSON line.

    python scripts/bench_metrics.py [--patch 128] [--batch 2] [--classes 4] [--rounds 9]

A cfg2-sized validation batch: `--batch` x C x patch^3 fp32 predictions and targets (C = 1 for seg_counts, `--classes` for
class_counts, 3 for normal_stats).  Per kernel and per torch formulation: HIP events around regions of one call on each of SETS
distinct batches -- more bytes between two uses of the same address than the Infinity Cache holds, so the rate is an HBM rate --
kernel and torch regions alternated, after a warm-up, median over the rounds; GB/s against the bytes streamed (every operand once
at its storage type).  Each kernel's result is compared with its numpy statement first (counts with ==).

The torch formulations are what one would write without the kernels, kept on the device (no .item()):
  seg     p = pred > thr; t = target > thr; stack([(p & t), (p & ~t), (~p & t)]).sum over the voxels
  class   pc = pred.argmax(1); lab = target.argmax(1); per class k: (pc == k) & (lab == k) etc., summed
  normal  the masked cosine and acos of MaskedCosineLoss' formula with elementwise torch ops, summed in float64
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SETS = 12


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


def torch_seg(p, t, thr_p, thr_t):
    import torch
    a, b = p > thr_p, t > thr_t
    return torch.stack([(a & b).flatten(2).sum(-1), (a & ~b).flatten(2).sum(-1), (~a & b).flatten(2).sum(-1)], dim=-1)


def torch_class(p, t):
    import torch
    c = p.shape[1]
    pc, lab = p.argmax(1).flatten(1), t.argmax(1).flatten(1)
    hit = pc == lab
    tp = torch.stack([((lab == k) & hit).sum(-1) for k in range(c)], dim=-1)
    fp = torch.stack([((pc == k) & ~hit).sum(-1) for k in range(c)], dim=-1)
    fn = torch.stack([((lab == k) & ~hit).sum(-1) for k in range(c)], dim=-1)
    return torch.stack([tp, fp, fn], dim=-1)


def torch_normal(p, t):
    import torch
    pn, tn = p.norm(dim=1), t.norm(dim=1)
    mask = tn > 1e-6
    cos = ((p * t).sum(1) / (pn.clamp(min=1e-8) * tn.clamp(min=1e-8))).clamp(-1.0, 1.0)
    deg = torch.acos(cos) * (180.0 / np.pi)
    m = mask.flatten(1)
    return m.sum(-1), torch.stack([(cos.flatten(1) * m).sum(-1, dtype=torch.float64), (deg.flatten(1) * m).sum(-1, dtype=torch.float64)], dim=-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--patch", type=int, default=128)
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--classes", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=9)
    a = ap.parse_args()
    import torch
    import mt3d_amd  # noqa: F401
    from mt3d_amd.engine import ops as E
    from mt3d_amd.training import metrics as M
    g = torch.Generator().manual_seed(0)
    sp = (a.patch,) * 3
    vox = a.batch * a.patch ** 3
    res = {"patch": a.patch, "batch": a.batch, "classes": a.classes, "sets": SETS}

    def report(name, fns, nbytes):
        out = {"bytes_streamed": nbytes}
        for k, ts in regions(fns, a.rounds).items():
            med = float(np.median(ts))
            out[f"{k}_us"] = round(med, 1)
            out[f"{k}_us_min_max"] = [round(min(ts), 1), round(max(ts), 1)]
            out[f"{k}_GBps"] = round(nbytes / med / 1e3, 1)
        res[name].update(out)

    # seg_counts: C = 1, a sheet-like fifth of the voxels labelled
    pred = [torch.randn((a.batch, 1) + sp, generator=g).cuda() for _ in range(SETS)]
    targ = [(torch.rand((a.batch, 1) + sp, generator=g) > 0.8).float().cuda() for _ in range(SETS)]
    out = torch.zeros((a.batch, 1, 3), dtype=torch.int64, device="cuda")
    want = M.seg_counts_numpy(pred[0].cpu().numpy(), targ[0].cpu().numpy(), 0.0, 0.5)
    res["seg_counts"] = {"kernel_equals_statement": bool(np.array_equal(E.seg_counts(pred[0], targ[0], 0.0, 0.5).cpu().numpy(), want)),
                         "torch_equals_statement": bool(np.array_equal(torch_seg(pred[0], targ[0], 0.0, 0.5).cpu().numpy(), want))}
    report("seg_counts", {"kernel": lambda i: E.seg_counts(pred[i], targ[i], 0.0, 0.5, out=out),
                          "torch": lambda i: torch_seg(pred[i], targ[i], 0.0, 0.5)}, vox * 8)
    del pred, targ

    # class_counts: probability targets of the prediction's shape (what the trainer's float32 cast of a multi-channel mask gives)
    c = a.classes
    pred = [torch.randn((a.batch, c) + sp, generator=g).cuda() for _ in range(SETS)]
    targ = [torch.rand((a.batch, c) + sp, generator=g).cuda() for _ in range(SETS)]
    out = torch.zeros((a.batch, c, 3), dtype=torch.int64, device="cuda")
    want = M.class_counts_numpy(pred[0].cpu().numpy(), targ[0].cpu().numpy())
    res["class_counts"] = {"kernel_equals_statement": bool(np.array_equal(E.class_counts(pred[0], targ[0]).cpu().numpy(), want)),
                           "torch_equals_statement": bool(np.array_equal(torch_class(pred[0], targ[0]).cpu().numpy(), want))}
    report("class_counts", {"kernel": lambda i: E.class_counts(pred[i], targ[i], out=out),
                            "torch": lambda i: torch_class(pred[i], targ[i])}, vox * c * 8)
    del pred, targ

    # normal_stats: unit targets on a fifth of the voxels, zero elsewhere
    pred = [torch.randn((a.batch, 3) + sp, generator=g).cuda() for _ in range(SETS)]
    targ = []
    for _ in range(SETS):
        v = torch.randn((a.batch, 3) + sp, generator=g)
        targ.append((v / v.norm(dim=1, keepdim=True).clamp(min=1e-8) * (torch.rand((a.batch, 1) + sp, generator=g) > 0.8)).cuda())
    outn = (torch.zeros(a.batch, dtype=torch.int64, device="cuda"), torch.zeros((a.batch, 2), dtype=torch.float64, device="cuda"))
    ws = torch.empty(E.load().rx_normal_stats_workspace(a.batch, a.patch ** 3) // 8, dtype=torch.float64, device="cuda")
    count, sums = M.normal_stats_numpy(pred[0].cpu().numpy(), targ[0].cpu().numpy())
    e0 = np.abs(M.normal_stats_numpy(pred[0].cpu().numpy(), targ[0].cpu().numpy(), dtype=np.float32)[1] - sums)
    kc, ks = E.normal_stats(pred[0], targ[0])
    tc, ts = torch_normal(pred[0], targ[0])
    res["normal_stats"] = {"kernel_count_equals_statement": bool(np.array_equal(kc.cpu().numpy(), count)),
                           "kernel_sums_deviation": np.abs(ks.cpu().numpy() - sums).max(0).tolist(),
                           "torch_count_equals_statement": bool(np.array_equal(tc.cpu().numpy(), count)),
                           "torch_sums_deviation": np.abs(ts.cpu().numpy() - sums).max(0).tolist(), "e0": e0.max(0).tolist()}
    report("normal_stats", {"kernel": lambda i: E.normal_stats(pred[i], targ[i], out=outn, ws=ws),
                            "torch": lambda i: torch_normal(pred[i], targ[i])}, vox * 3 * 8)
    for k in ("seg_counts", "class_counts", "normal_stats"):
        res[k]["torch_over_kernel"] = round(res[k]["torch_us"] / res[k]["kernel_us"], 2)
    try:
        res["device"] = torch.cuda.get_device_name()
        res["sclk_mhz_after"] = int(torch.cuda.clock_rate())          # the clock is left to the governor; read, never set
    except Exception as e:      # (an optional reading: pynvml / amdsmi may be absent)
        res["sclk_mhz_after"] = f"not read ({type(e).__name__})"
    print(json.dumps(res))


if __name__ == "__main__":
    main()
