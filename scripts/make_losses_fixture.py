"""Writes `tests/golden/losses_extra.npz`, the vectors the element-wise and cross-entropy loss kernels (csrc/rx_loss.hip) are
pinned against (tests/test_losses_extra.py).  Needs the reference tree (oracle/ref_shim.py) at generation time only:

    python scripts/make_losses_fixture.py

`BCEWithLogitsLossLabelSmoothing` and `BCEWithLogitsLossZSmooth` are the REAL reference classes (training/losses/losses.py
:217-304); the other four names of the reference's loss map are `torch.nn` classes there too.  Everything runs on the CPU in
fp32.  Per case: `pred`, `target`, `loss`, `grad` (d(weight * loss)/d(pred)), and `loss64`, the same module on float64 copies of
the inputs -- the value both fp32 results (torch's and the kernels') are judged against where the bound is relative.

Logits are drawn as randn * 2 rounded to multiples of 1/64: still arbitrary fp32 inputs for exp / log, but the file stays small."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "losses_extra.npz")

ELEMENTWISE = ("BCEWithLogitsLoss", "BCEWithLogitsLossLabelSmoothing", "BCEWithLogitsLossZSmooth", "BCELoss", "MSELoss")
_SHORT = {"BCEWithLogitsLoss": "bcel", "BCEWithLogitsLossLabelSmoothing": "bcels", "BCEWithLogitsLossZSmooth": "zs", "BCELoss": "bce",
          "MSELoss": "mse"}


def _cases():
    """name -> (kind, shape, seed, kwargs, upstream weight, target mode)"""
    c = {}
    seed = 100
    for kind in ELEMENTWISE:
        p = _SHORT[kind]
        kw_ragged = {"BCEWithLogitsLossLabelSmoothing": {"smoothing": 0.2},
                     "BCEWithLogitsLossZSmooth": {"center_smoothing": 0.05, "edge_smoothing": 0.3}}.get(kind, {})
        c[f"{p}_vec"] = (kind, (1, 1, 8, 8, 8), seed, {}, 1.0, "binary")                     # 16-byte path; Z = 8 (even)
        c[f"{p}_ragged"] = (kind, (1, 3, 5, 7, 9), seed + 1, kw_ragged, 0.25, "binary")      # odd planes, scalar path; Z = 5 (odd)
        c[f"{p}_multiblock"] = (kind, (1, 2, 21, 20, 20), seed + 2, {}, 1.0, "binary")       # 8400 > 8192 elements per plane
        if kind != "BCEWithLogitsLossZSmooth":
            c[f"{p}_2d"] = (kind, (2, 2, 24, 20), seed + 3, {}, 1.0, "binary")
        seed += 10
    for kind in ("BCEWithLogitsLoss", "BCEWithLogitsLossZSmooth", "BCELoss", "MSELoss"):    # one per kernel kind (+ the table mode)
        c[f"{_SHORT[kind]}_sum"] = (kind, (1, 3, 5, 7, 9), seed, {"reduction": "sum"}, 0.5, "binary")
        seed += 1
    c["bce_clamp"] = ("BCELoss", (1, 1, 8, 8, 8), seed, {}, 1.0, "clamp")                   # exact 0.0 / 1.0 against opposite targets
    ce = "CrossEntropyLoss"
    c["ce_prob_c2"] = (ce, (1, 2, 8, 8, 8), 201, {}, 1.0, "prob")
    c["ce_prob_c5"] = (ce, (2, 5, 5, 7, 9), 202, {}, 0.5, "prob")
    c["ce_prob_c70"] = (ce, (1, 70, 3, 5, 7), 203, {}, 1.0, "prob")
    c["ce_prob_multiblock_onehot"] = (ce, (1, 3, 21, 20, 20), 204, {}, 1.0, "onehot")       # 8400 voxels: 5 blocks of 2048
    c["ce_prob_mask"] = (ce, (2, 5, 5, 7, 9), 205, {}, 1.0, "mask")                         # channel sums != 1 (a mask cast to float)
    c["ce_prob_sum"] = (ce, (2, 5, 5, 7, 9), 206, {"reduction": "sum"}, 0.5, "prob")
    c["ce_prob_2d"] = (ce, (2, 3, 24, 20), 207, {}, 1.0, "prob")
    c["ce_idx"] = (ce, (2, 5, 5, 7, 9), 211, {}, 1.0, "index")                              # ~30 % at ignore_index = -100
    c["ce_idx_ignore255"] = (ce, (2, 5, 5, 7, 9), 212, {"ignore_index": 255}, 0.5, "index")
    c["ce_idx_sum"] = (ce, (2, 5, 5, 7, 9), 213, {"reduction": "sum"}, 1.0, "index")
    c["ce_idx_vec"] = (ce, (1, 4, 8, 8, 8), 214, {}, 2.0, "index")
    c["ce_idx_multiblock"] = (ce, (1, 2, 21, 20, 20), 215, {}, 1.0, "index")
    return c


CASES = _cases()


def inputs(name):
    kind, shape, seed, kw, _, mode = CASES[name]
    g = torch.Generator().manual_seed(seed)
    pred = torch.round(torch.randn(shape, generator=g) * 2.0 * 64.0) / 64.0
    if kind == "BCELoss":
        pred = torch.sigmoid(pred)
    if mode == "binary":
        target = (torch.rand(shape, generator=g) > 0.7).float()
    elif mode == "clamp":
        target = (torch.rand(shape, generator=g) > 0.5).float()
        flat, tf = pred.view(-1), target.view(-1)
        flat[0:64:4] = 0.0; tf[0:64:4] = 1.0            # log(0) -> -100;  (0 - 1) / max(0, 1e-12)
        flat[1:64:4] = 1.0; tf[1:64:4] = 0.0            # log(1 - 1) -> -100
        flat[2:64:4] = 0.0; tf[2:64:4] = 0.0            # 0 * -100: no contribution, gradient 0 / 1e-12
        flat[3:64:4] = 1.0; tf[3:64:4] = 1.0
    elif mode == "prob":
        target = torch.softmax(torch.randn(shape, generator=g) * 2.0, dim=1)
    elif mode == "onehot":
        idx = torch.randint(0, shape[1], (shape[0], *shape[2:]), generator=g)
        target = torch.nn.functional.one_hot(idx, shape[1]).movedim(-1, 1).float().contiguous()
    elif mode == "mask":
        target = (torch.rand(shape, generator=g) > 0.7).float()
    elif mode == "index":
        target = torch.randint(0, shape[1], (shape[0], *shape[2:]), generator=g)
        target[torch.rand(target.shape, generator=g) < 0.3] = kw.get("ignore_index", -100)
    else:
        raise ValueError(mode)
    return pred, target


def generate(classes):
    """classes: name -> loss class.  -> dict of arrays, as stored in the fixture"""
    arrays = {}
    for name, (kind, shape, seed, kw, weight, mode) in CASES.items():
        pred, target = inputs(name)
        fn = classes[kind](**kw)
        p = pred.clone().requires_grad_(True)
        loss = fn(p, target)
        (loss * weight).backward()
        loss64 = fn(pred.double(), target if target.dtype == torch.int64 else target.double())
        arrays[f"{name}.pred"] = pred.numpy()
        arrays[f"{name}.target"] = target.numpy()
        arrays[f"{name}.loss"] = np.float64(loss.item())
        arrays[f"{name}.loss64"] = np.float64(loss64.item())
        arrays[f"{name}.grad"] = p.grad.numpy()
    return arrays


def reference_classes():
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import ref_shim
    _, ref_losses = ref_shim.import_reference()
    import torch.nn as nn
    return {"BCEWithLogitsLossLabelSmoothing": ref_losses.BCEWithLogitsLossLabelSmoothing,
            "BCEWithLogitsLossZSmooth": ref_losses.BCEWithLogitsLossZSmooth,
            "BCEWithLogitsLoss": nn.BCEWithLogitsLoss, "BCELoss": nn.BCELoss, "MSELoss": nn.MSELoss,
            "CrossEntropyLoss": nn.CrossEntropyLoss}


def sum_margin(loss, loss64):
    """bound of the sum-reduced cases, relative to loss64: 4x the relative error of torch's own fp32 result (another summation
    order of the same fp32 terms), never below 2e-6"""
    return max(4.0 * abs(loss - loss64) / abs(loss64), 2e-6)


def main():
    arrays = generate(reference_classes())
    for name, (kind, shape, seed, kw, weight, mode) in CASES.items():
        loss, loss64 = float(arrays[f"{name}.loss"]), float(arrays[f"{name}.loss64"])
        rel = abs(loss - loss64) / abs(loss64)
        extra = f"  sum margin {sum_margin(loss, loss64):.2e}" if kw.get("reduction") == "sum" else ""
        print(f"{name:28s} {str(shape):18s} loss={loss:.6f} loss64={loss64:.9f} fp32 rel err {rel:.2e}{extra}")
    np.savez_compressed(OUT, **arrays)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
