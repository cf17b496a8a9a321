"""Forward + backward of the six task losses of csrc/rx_loss.hip's element-wise and cross-entropy families: the HIP path against
the torch formulation on the same device, at cfg2's head shapes (2,1,128^3) and (2,4,128^3), cross entropy also at (1,32,128^3).

    python scripts/bench_losses.py [filter ...] [--reps N] [--inner N]

Per case one JSON line: median over `reps` windows of `inner` forward+backward calls (HIP events around each window, after a
warm-up window per arm; the two arms alternate window by window).  `gbs` is ALGORITHMIC bytes over time: every operand the kernels
touch once per direction (the table in DESIGN, "The remaining task losses"); the same byte count is used for the torch arm, so
its figure is an equivalent rate, not its real traffic."""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
import torch
import torch.nn as nn
import torch.nn.functional as F
import mt3d_amd  # noqa: F401
from mt3d_amd.engine import lib
from mt3d_amd.training.losses import losses as L

args = sys.argv[1:]
flt = [a for i, a in enumerate(args) if not a.startswith("--") and not (i and args[i - 1] in ("--reps", "--inner"))]
reps = int(args[args.index("--reps") + 1]) if "--reps" in args else 15
inner = int(args[args.index("--inner") + 1]) if "--inner" in args else 10


def zsmooth_torch(x, t, center=0.1, edge=0.4):
    d = x.shape[2]
    z = torch.arange(d, device=x.device, dtype=x.dtype)
    alpha = (center + (edge - center) * ((z - (d - 1) / 2.0).abs() / (d // 2))).view(1, 1, d, 1, 1)
    return F.binary_cross_entropy_with_logits(x, t * (1.0 - 2.0 * alpha) + alpha)


def smoothing_torch(x, t, s=0.1):
    return F.binary_cross_entropy_with_logits(x, t * (1.0 - 2.0 * s) + s)


def elem_bytes(e, p):       # forward 8E, backward 8E + 4E
    return 20 * e


def ce_prob_bytes(e, p):    # forward 8E + 8P, backward 8E + 8P + 4E
    return 20 * e + 16 * p


def ce_index_bytes(e, p):   # forward 4E + 8P + 4P, backward 4E + 12P + 4E
    return 12 * e + 24 * p


HEADS = [(2, 1, 128, 128, 128), (2, 4, 128, 128, 128)]
CASES = []      # (name, shape, target mode, HIP module, torch callable, byte model)
for shape in HEADS:
    CASES += [
        ("BCEWithLogitsLoss", shape, "binary", L.BCEWithLogitsLoss(), nn.BCEWithLogitsLoss(), elem_bytes),
        ("BCEWithLogitsLossLabelSmoothing", shape, "binary", L.BCEWithLogitsLossLabelSmoothing(), smoothing_torch, elem_bytes),
        ("BCEWithLogitsLossZSmooth", shape, "binary", L.BCEWithLogitsLossZSmooth(), zsmooth_torch, elem_bytes),
        ("BCELoss", shape, "binary_prob", L.BCELoss(), nn.BCELoss(), elem_bytes),
        ("MSELoss", shape, "binary", L.MSELoss(), nn.MSELoss(), elem_bytes),
    ]
for shape in HEADS + [(1, 32, 128, 128, 128)]:
    CASES += [
        ("CrossEntropyLoss/prob", shape, "prob", L.CrossEntropyLoss(), nn.CrossEntropyLoss(), ce_prob_bytes),
        ("CrossEntropyLoss/index", shape, "index", L.CrossEntropyLoss(), nn.CrossEntropyLoss(), ce_index_bytes),
    ]


def window(fn, x, t):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        x.grad = None
        fn(x, t).backward()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / inner


def main():
    lib.require_device()
    for name, shape, mode, hip, ref, nbytes in CASES:
        label = f"{name}@{'x'.join(map(str, shape[:2]))}x128^3"
        if flt and not any(f in label for f in flt):
            continue
        g = torch.Generator(device="cuda").manual_seed(1)
        x = torch.randn(shape, device="cuda", generator=g)
        if mode == "binary_prob":
            x = torch.sigmoid(x)
        x.requires_grad_(True)
        if mode == "prob":
            t = torch.softmax(torch.randn(shape, device="cuda", generator=g), dim=1)
        elif mode == "index":
            t = torch.randint(0, shape[1], (shape[0], *shape[2:]), device="cuda", generator=g)
        else:
            t = (torch.rand(shape, device="cuda", generator=g) > 0.8).float()
        l_hip = hip(x, t)
        assert "_ElemLossFn" in type(l_hip.grad_fn).__name__ or "_CrossEntropyFn" in type(l_hip.grad_fn).__name__
        window(hip, x, t), window(ref, x, t)                # warm-up: code objects, allocator
        ms = {"hip": [], "torch": []}
        for _ in range(reps):                               # alternate the arms: same clocks, same neighbours
            ms["hip"].append(window(hip, x, t))
            ms["torch"].append(window(ref, x, t))
        e, p = x.numel(), x.numel() // shape[1]
        hip_ms, torch_ms = statistics.median(ms["hip"]), statistics.median(ms["torch"])
        print(json.dumps({"case": label, "hip_ms": round(hip_ms, 4), "torch_ms": round(torch_ms, 4),
                          "hip_min_ms": round(min(ms["hip"]), 4), "torch_min_ms": round(min(ms["torch"]), 4),
                          "speedup": round(torch_ms / hip_ms, 2), "algorithmic_mb": round(nbytes(e, p) / 1e6, 1),
                          "hip_gbs": round(nbytes(e, p) / hip_ms / 1e6, 1), "torch_equiv_gbs": round(nbytes(e, p) / torch_ms / 1e6, 1),
                          "loss_hip": round(l_hip.item(), 6), "loss_torch": round(ref(x, t).item(), 6)}), flush=True)
        del x, t


if __name__ == "__main__":
    main()
