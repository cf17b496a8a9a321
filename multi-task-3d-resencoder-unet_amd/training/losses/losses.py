"""Task losses consumed by the train step (reference: training/losses/losses.py).  Same class names, constructor
arguments and arithmetic as the reference so `_build_loss` (train.py:43-66) maps YAML names 1:1.

`BCEDiceLoss` and `MaskedCosineLoss` -- the two losses of the BASELINE configs -- run as single-pass HIP kernels
(csrc/rx_loss.hip) whenever they are handed HIP tensors: one read of logits + target forward, one
read + one write backward, loss value and upstream gradient kept as device scalars (the torch formulation makes 5-8
passes per direction).  On a HIP device a missing librxunet.so is an error, not a fallback; tensors that live on the
CPU (the host-side unit tests of the trainer plumbing) take the torch formulation, which is also what the GPU tests
compare the kernels against.

The other six names of the map run natively as well, on two more kernel families of the same file: the element-wise family
(`_ElemLossFn`: `BCEWithLogitsLoss`, `BCEWithLogitsLossLabelSmoothing`, `BCEWithLogitsLossZSmooth`, `BCELoss`, `MSELoss`) and
cross entropy over the channel axis (`_CrossEntropyFn`: `CrossEntropyLoss`, probability or class-index targets).  The four
`torch.nn` names are subclasses of the torch classes (same constructor, `isinstance` holds); they take the HIP branch for
device tensors with `reduction` "mean" or "sum" and none of `weight` / `pos_weight` / `label_smoothing`, and call
`super().forward` for everything else (CPU tensors, `reduction="none"`, those keyword arguments)."""
import torch
import torch.nn as nn
import torch.nn.functional as F


def _hip_eligible(pred, target):
    return pred.is_cuda and target.is_cuda and pred.shape == target.shape and pred.dim() >= 3


def _as_f32c(t):
    t = t if t.dtype == torch.float32 else t.float()
    return t if t.is_contiguous() else t.contiguous()


class _BCEDiceFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, target, alpha, beta, smoothing):
        from ...engine import ops
        x, t = _as_f32c(logits.detach()), _as_f32c(target.detach())
        loss, coef = ops.bce_dice_loss_fwd(x, t, alpha, beta, smoothing, 1e-6)
        ctx.save_for_backward(x, t, coef)
        ctx.hp = (alpha, beta, smoothing, logits.dtype)
        return loss

    @staticmethod
    def backward(ctx, g):
        from ...engine import ops
        x, t, coef = ctx.saved_tensors
        alpha, beta, smoothing, dtype = ctx.hp
        g = _as_f32c(g)
        d = ops.bce_dice_loss_bwd(x, t, coef, g, alpha, beta, smoothing)
        return (d if dtype == torch.float32 else d.to(dtype)), None, None, None, None


class _MaskedCosineFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, target):
        from ...engine import ops
        x, t = _as_f32c(pred.detach()), _as_f32c(target.detach())
        loss, coef = ops.masked_cosine_loss_fwd(x, t)
        ctx.save_for_backward(x, t, coef)
        ctx.dtype = pred.dtype
        return loss

    @staticmethod
    def backward(ctx, g):
        from ...engine import ops
        x, t, coef = ctx.saved_tensors
        d = ops.masked_cosine_loss_bwd(x, t, coef, _as_f32c(g))
        return (d if ctx.dtype == torch.float32 else d.to(ctx.dtype)), None


class _ElemLossFn(torch.autograd.Function):
    """mean / sum of a per-element term (csrc/rx_loss.hip, element-wise family); nothing but the inputs is saved"""

    @staticmethod
    def forward(ctx, pred, target, kind, reduction, smoothing, alpha_z):
        from ...engine import ops
        x, t = _as_f32c(pred.detach()), _as_f32c(target.detach())
        loss = ops.elem_loss_fwd(kind, x, t, reduction, smoothing, alpha_z)
        ctx.save_for_backward(x, t)
        ctx.hp = (kind, reduction, smoothing, alpha_z, pred.dtype)
        return loss

    @staticmethod
    def backward(ctx, g):
        from ...engine import ops
        x, t = ctx.saved_tensors
        kind, reduction, smoothing, alpha_z, dtype = ctx.hp
        d = ops.elem_loss_bwd(kind, x, t, _as_f32c(g), reduction, smoothing, alpha_z)
        return (d if dtype == torch.float32 else d.to(dtype)), None, None, None, None, None


class _CrossEntropyFn(torch.autograd.Function):
    """cross entropy over dim 1; the forward leaves the per-voxel log-sum-exp (and target sum) for the backward"""

    @staticmethod
    def forward(ctx, logits, target, reduction, ignore_index):
        from ...engine import ops
        x = _as_f32c(logits.detach())
        t = target.detach()
        t = t.contiguous() if t.dtype == torch.int64 else _as_f32c(t)
        loss, coef, saved = ops.cross_entropy_loss_fwd(x, t, reduction, ignore_index)
        ctx.save_for_backward(x, t, coef, saved)
        ctx.hp = (ignore_index, logits.dtype)
        return loss

    @staticmethod
    def backward(ctx, g):
        from ...engine import ops
        x, t, coef, saved = ctx.saved_tensors
        ignore_index, dtype = ctx.hp
        d = ops.cross_entropy_loss_bwd(x, t, coef, saved, _as_f32c(g), ignore_index)
        return (d if dtype == torch.float32 else d.to(dtype)), None, None, None


_BCE_LOGITS, _BCE_PROB, _MSE = 0, 1, 2      # engine/lib.py RX_LOSS_*
_CE_MAX_CLASSES = 1024


def _elem_eligible(pred, target, reduction):
    # a target that wants a gradient of its own (nn.MSELoss gives one) keeps torch's graph
    return reduction in ("mean", "sum") and _hip_eligible(pred, target) and not target.requires_grad


def flatten(tensor):
    """(N, C, *spatial) -> (C, N * prod(spatial))   (losses.py:321-333)"""
    c = tensor.size(1)
    return tensor.transpose(0, 1).reshape(c, -1)


def compute_per_channel_dice(input, target, epsilon=1e-6, weight=None):
    """V-Net dice per channel: 2 * sum(p t) / (sum(p^2) + sum(t^2))   (losses.py:17-43)"""
    assert input.size() == target.size(), "'input' and 'target' must have the same shape"
    p, t = flatten(input), flatten(target).float()
    inter = (p * t).sum(-1)
    if weight is not None:
        inter = weight * inter
    den = (p * p).sum(-1) + (t * t).sum(-1)
    return 2 * (inter / den.clamp(min=epsilon))


class DiceLoss(nn.Module):
    """1 - mean_c dice_c on sigmoid / softmax / raw inputs   (losses.py:95-138)"""

    def __init__(self, weight=None, normalization="sigmoid"):
        super().__init__()
        assert normalization in ("sigmoid", "softmax", "none")
        self.register_buffer("weight", weight)
        self.normalization = normalization

    def forward(self, input, target):
        if self.normalization == "sigmoid":
            input = torch.sigmoid(input)
        elif self.normalization == "softmax":
            input = torch.softmax(input, dim=1)
        return 1.0 - compute_per_channel_dice(input, target, weight=self.weight).mean()


class BCEWithLogitsLossLabelSmoothing(nn.Module):
    """targets y -> y (1 - 2 s) + s, then BCE-with-logits   (losses.py:217-238)"""

    def __init__(self, smoothing=0.1, reduction="mean"):
        super().__init__()
        self.smoothing, self.reduction = smoothing, reduction

    def forward(self, logits, targets):
        if _elem_eligible(logits, targets, self.reduction):
            return _ElemLossFn.apply(logits, targets, _BCE_LOGITS, self.reduction, float(self.smoothing), None)
        with torch.no_grad():
            smoothed = targets * (1.0 - 2.0 * self.smoothing) + self.smoothing
        return F.binary_cross_entropy_with_logits(logits, smoothed, reduction=self.reduction)


_ZSMOOTH_TABLES = {}


def _zsmooth_table(d, center, edge, device, dtype=torch.float32):
    """per-slice smoothing, the reference's own expression (losses.py:277-288)"""
    z = torch.arange(d, device=device, dtype=dtype)
    ratio = (z - (d - 1) / 2.0).abs() / (d // 2)
    return center + (edge - center) * ratio


class BCEWithLogitsLossZSmooth(nn.Module):
    """label smoothing that grows linearly with the distance from the central Z slice (losses.py:240-304)"""

    def __init__(self, center_smoothing=0.1, edge_smoothing=0.4, reduction="mean"):
        super().__init__()
        self.center_smoothing, self.edge_smoothing, self.reduction = center_smoothing, edge_smoothing, reduction

    def forward(self, logits, targets):
        assert logits.shape == targets.shape, "Logits and targets must match in shape."
        d = logits.shape[2]
        if logits.dim() == 5 and d >= 2 and _elem_eligible(logits, targets, self.reduction):
            key = (d, self.center_smoothing, self.edge_smoothing, logits.device)
            table = _ZSMOOTH_TABLES.get(key)
            if table is None:       # fp32 torch expression, evaluated once per (Z, center, edge, device)
                table = _ZSMOOTH_TABLES[key] = _zsmooth_table(d, self.center_smoothing, self.edge_smoothing, logits.device).contiguous()
            return _ElemLossFn.apply(logits, targets, _BCE_LOGITS, self.reduction, 0.0, table)
        alpha = _zsmooth_table(d, self.center_smoothing, self.edge_smoothing, logits.device, logits.dtype).view(1, 1, d, 1, 1)
        return F.binary_cross_entropy_with_logits(logits, targets * (1.0 - 2.0 * alpha) + alpha,
                                                  reduction=self.reduction)


class BCEWithLogitsLoss(nn.BCEWithLogitsLoss):
    """nn.BCEWithLogitsLoss; without `weight` / `pos_weight` the element-wise HIP kernel on device tensors"""

    def forward(self, input, target):
        if self.weight is None and self.pos_weight is None and _elem_eligible(input, target, self.reduction):
            return _ElemLossFn.apply(input, target, _BCE_LOGITS, self.reduction, 0.0, None)
        return super().forward(input, target)


class BCELoss(nn.BCELoss):
    """nn.BCELoss (probabilities in, torch's -100 / 1e-12 clamps); without `weight` the element-wise HIP kernel"""

    def forward(self, input, target):
        if self.weight is None and _elem_eligible(input, target, self.reduction):
            return _ElemLossFn.apply(input, target, _BCE_PROB, self.reduction, 0.0, None)
        return super().forward(input, target)


class MSELoss(nn.MSELoss):
    """nn.MSELoss; the element-wise HIP kernel on device tensors"""

    def forward(self, input, target):
        if _elem_eligible(input, target, self.reduction):
            return _ElemLossFn.apply(input, target, _MSE, self.reduction, 0.0, None)
        return super().forward(input, target)


class CrossEntropyLoss(nn.CrossEntropyLoss):
    """nn.CrossEntropyLoss over dim 1.  HIP kernel for device tensors with float targets of the logits' shape (class
    probabilities -- what the trainer's float32 cast of a multi-channel mask gives) or int64 targets (N, *spatial), when
    `weight is None`, `label_smoothing == 0`, C <= 1024 and reduction is mean / sum"""

    def _hip(self, input, target):
        if not (input.is_cuda and target.is_cuda and input.dim() >= 3 and self.reduction in ("mean", "sum")) or target.requires_grad:
            return False
        if self.weight is not None or self.label_smoothing != 0.0 or input.shape[1] > _CE_MAX_CLASSES or input.numel() == 0:
            return False
        if target.dtype == torch.int64:
            return target.shape == input.shape[:1] + input.shape[2:]
        return target.is_floating_point() and target.shape == input.shape

    def forward(self, input, target):
        if self._hip(input, target):
            return _CrossEntropyFn.apply(input, target, self.reduction, int(self.ignore_index))
        return super().forward(input, target)


class BCEDiceLoss(nn.Module):
    """alpha * smoothed BCE + beta * Dice   (losses.py:307-318)"""

    def __init__(self, alpha, beta):
        super().__init__()
        self.alpha, self.beta = alpha, beta
        self.bce = BCEWithLogitsLossLabelSmoothing(smoothing=0.1, reduction="mean")
        self.dice = DiceLoss()

    def forward(self, input, target):
        if _hip_eligible(input, target):
            return _BCEDiceFn.apply(input, target, float(self.alpha), float(self.beta), float(self.bce.smoothing))
        return self.alpha * self.bce(input, target) + self.beta * self.dice(input, target)


class MaskedCosineLoss(nn.Module):
    """1 - mean cosine similarity over voxels whose target normal is non-zero   (losses.py:187-215)"""

    def forward(self, pred, target):
        if _hip_eligible(pred, target) and pred.shape[1] <= 8:
            return _MaskedCosineFn.apply(pred, target)
        mask = (torch.norm(target, dim=1) > 1e-6).float()
        unit = pred / torch.norm(pred, dim=1, keepdim=True).clamp(min=1e-8)
        cos = F.cosine_similarity(unit, target, dim=1, eps=1e-8)
        return 1.0 - (cos * mask).sum() / (mask.sum() + 1e-8)


LOSS_FN_MAP = {
    "BCEDiceLoss": BCEDiceLoss,
    "BCEWithLogitsLossLabelSmoothing": BCEWithLogitsLossLabelSmoothing,
    "BCEWithLogitsLossZSmooth": BCEWithLogitsLossZSmooth,
    "BCEWithLogitsLoss": BCEWithLogitsLoss,
    "BCELoss": BCELoss,
    "CrossEntropyLoss": CrossEntropyLoss,
    "MSELoss": MSELoss,
    "MaskedCosineLoss": MaskedCosineLoss,
}
