"""Times the validation preview at the cfg2 validation shape (128^3, a 1-channel and a 3-channel task: 9 float32 channel volumes):

  kernel   engine.ops.preview_frames (one rx_preview_panel launch per panel) + the copy of the uint8 frames to pinned memory
  torch    the same panels as torch ops on the device (amin / amax per slice, subtract, divide, multiply, cast) + the same copy
  host     the float32 volumes copied to the host, then training.visualization.frames_numpy
  gif      training.visualization.write_gif on the finished frames, on its own

    python scripts/bench_preview.py [--size 128] [--iters 20]

Prints one JSON line.  Needs the GPU; there is no fallback."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mt3d_amd  # noqa: E402,F401
from mt3d_amd.engine import lib, ops  # noqa: E402
from mt3d_amd.training import visualization as V  # noqa: E402


def torch_panel(vol):
    """(C, Z, H, W) device float32 -> uint8 (Z, H, W, 3): the statement as torch ops (finite inputs)"""
    v = vol[:3] if vol.shape[0] == 3 else vol[:1]
    lo, hi = v.amin(dim=(2, 3), keepdim=True), v.amax(dim=(2, 3), keepdim=True)
    r = hi - lo
    q = ((v - lo) / r) * 255.0
    b = torch.where(r > 1e-6, q, torch.full_like(q, 127.0)).to(torch.uint8)
    if b.shape[0] == 1:
        b = b.expand(3, -1, -1, -1)
    return b.permute(1, 2, 3, 0)


def torch_frames(image, targets, preds):
    names = sorted(targets)
    top = torch.cat([torch_panel(image)] + [torch_panel(targets[n]) for n in names], dim=2)
    bottom = torch.cat([torch.zeros_like(torch_panel(image))] + [torch_panel(preds[n]) for n in names], dim=2)
    return torch.cat([top, bottom], dim=1).contiguous()


def timed(fn, iters, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    lib.require_device()
    s = a.size
    g = torch.Generator().manual_seed(0)
    image = torch.randn(1, 1, s, s, s, generator=g).cuda()
    targets = {"sheet": (torch.randn(1, 1, s, s, s, generator=g) > 0).float().cuda(), "normals": torch.randn(1, 3, s, s, s, generator=g).cuda()}
    preds = {"sheet": torch.rand(1, 1, s, s, s, generator=g).cuda(), "normals": torch.randn(1, 3, s, s, s, generator=g).cuda()}
    out = ops.preview_frames(image, targets, preds)
    pinned = torch.empty(out.shape, dtype=torch.uint8, pin_memory=True)

    def kernel_only():
        ops.preview_frames(image, targets, preds, out=out)

    def kernel():
        ops.preview_frames(image, targets, preds, out=out)
        pinned.copy_(out, non_blocking=True)

    def torch_path():
        pinned.copy_(torch_frames(image[0], {k: v[0] for k, v in targets.items()}, {k: v[0] for k, v in preds.items()}), non_blocking=True)

    host_frames = []

    def host():
        torch.cuda.synchronize()      # the reference drains the queue with its .cpu() copies
        host_frames[:] = [V.frames_numpy(image[0].cpu().numpy(), {k: v[0].cpu().numpy() for k, v in targets.items()},
                                         {k: v[0].cpu().numpy() for k, v in preds.items()})]
    res = {"shape": [s, s, s], "float_bytes": 9 * s ** 3 * 4, "frame_bytes": int(out.numel())}
    res["kernel_only_ms"] = round(timed(kernel_only, a.iters), 4)
    res["kernel_ms"] = round(timed(kernel, a.iters), 4)
    res["torch_ms"] = round(timed(torch_path, a.iters), 4)
    res["host_ms"] = round(timed(host, max(a.iters // 10, 2), warmup=1), 3)
    kernel()
    torch.cuda.synchronize()
    frames = pinned.numpy().copy()
    res["kernel_equals_host"] = bool(np.array_equal(frames, host_frames[0]))
    res["torch_equals_host"] = bool(np.array_equal(torch_frames(image[0], {k: v[0] for k, v in targets.items()},
                                                                {k: v[0] for k, v in preds.items()}).cpu().numpy(), host_frames[0]))
    with tempfile.TemporaryDirectory() as tmp:
        t0 = time.perf_counter()
        V.write_gif(frames, os.path.join(tmp, "bench_debug.gif"), 5)
        res["gif_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
        res["gif_bytes"] = os.path.getsize(os.path.join(tmp, "bench_debug.gif"))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
