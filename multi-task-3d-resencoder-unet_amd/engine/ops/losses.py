"""Task losses: single-pass kernels; the loss value and the upstream gradient stay on the device."""
import torch

from .. import lib as _l
from ..lib import check, load, stream_ptr
from .core import _ncv, _ptr, _ws_args, workspace


def bce_dice_loss_fwd(logits, target, alpha, beta, smoothing=0.1, eps=1e-6):
    """-> (loss: 0-dim fp32 device tensor, coef: (2*C,) fp32 for the backward)"""
    n, c, v = _ncv(logits)
    loss = torch.empty((), dtype=torch.float32, device=logits.device)
    coef = torch.empty(2 * c, dtype=torch.float32, device=logits.device)
    ws = workspace(load().rx_loss_workspace(n, c, v))
    check(load().rx_bce_dice_loss_fwd(_ptr(logits), _ptr(target), n, c, v, alpha, beta, smoothing, eps, _ptr(loss), _ptr(coef),
                                      *_ws_args(ws), stream_ptr()), "rx_bce_dice_loss_fwd")
    return loss, coef


def bce_dice_loss_bwd(logits, target, coef, grad_loss, alpha, beta, smoothing=0.1):
    n, c, v = _ncv(logits)
    dlogits = torch.empty_like(logits)
    check(load().rx_bce_dice_loss_bwd(_ptr(logits), _ptr(target), n, c, v, alpha, beta, smoothing, _ptr(coef), _ptr(grad_loss),
                                      _ptr(dlogits), stream_ptr()), "rx_bce_dice_loss_bwd")
    return dlogits


def masked_cosine_loss_fwd(pred, target):
    n, c, v = _ncv(pred)
    loss = torch.empty((), dtype=torch.float32, device=pred.device)
    coef = torch.empty(1, dtype=torch.float32, device=pred.device)
    ws = workspace(load().rx_loss_workspace(n, c, v))
    check(load().rx_masked_cosine_loss_fwd(_ptr(pred), _ptr(target), n, c, v, _ptr(loss), _ptr(coef), *_ws_args(ws), stream_ptr()),
          "rx_masked_cosine_loss_fwd")
    return loss, coef


def masked_cosine_loss_bwd(pred, target, coef, grad_loss):
    n, c, v = _ncv(pred)
    dpred = torch.empty_like(pred)
    check(load().rx_masked_cosine_loss_bwd(_ptr(pred), _ptr(target), n, c, v, _ptr(coef), _ptr(grad_loss), _ptr(dpred),
                                           stream_ptr()), "rx_masked_cosine_loss_bwd")
    return dpred


_REDUCTION = {"mean": _l.RX_REDUCE_MEAN, "sum": _l.RX_REDUCE_SUM}


def elem_loss_fwd(kind, x, target, reduction="mean", smoothing=0.0, alpha_z=None):
    """element-wise family (kind: lib.RX_LOSS_*) on contiguous fp32 (N, C, *spatial); `alpha_z`: optional (Z,) fp32 device table of
    per-slice smoothing, Z = x.shape[2].  -> loss: 0-dim fp32 device tensor"""
    n, c, v = _ncv(x)
    loss = torch.empty((), dtype=torch.float32, device=x.device)
    ws = workspace(load().rx_loss_workspace(n, c, v))
    check(load().rx_elem_loss_fwd(kind, _ptr(x), _ptr(target), n, c, v, smoothing, _ptr(alpha_z), alpha_z.numel() if alpha_z is not None else 0,
                                  _REDUCTION[reduction], _ptr(loss), *_ws_args(ws), stream_ptr()), "rx_elem_loss_fwd")
    return loss


def elem_loss_bwd(kind, x, target, grad_loss, reduction="mean", smoothing=0.0, alpha_z=None):
    n, c, v = _ncv(x)
    dx = torch.empty_like(x)
    check(load().rx_elem_loss_bwd(kind, _ptr(x), _ptr(target), n, c, v, smoothing, _ptr(alpha_z), alpha_z.numel() if alpha_z is not None else 0,
                                  _REDUCTION[reduction], _ptr(grad_loss), _ptr(dx), stream_ptr()), "rx_elem_loss_bwd")
    return dx


def _ce_targets(target):
    """(target_prob, target_index): float targets are class probabilities, int64 targets class indices"""
    return (None, target) if target.dtype == torch.int64 else (target, None)


def cross_entropy_loss_fwd(logits, target, reduction="mean", ignore_index=-100):
    """logits: contiguous fp32 (N, C, *spatial); target: fp32 of the same shape, or int64 (N, *spatial).
    -> (loss: 0-dim fp32 device tensor, coef: (1,) backward scale, saved: per-voxel lse [and target sum] for the backward)"""
    n, c, v = _ncv(logits)
    tp, ti = _ce_targets(target)
    loss = torch.empty((), dtype=torch.float32, device=logits.device)
    coef = torch.empty(1, dtype=torch.float32, device=logits.device)
    saved = torch.empty((1 if tp is None else 2, n, v), dtype=torch.float32, device=logits.device)
    ws = workspace(load().rx_cross_entropy_loss_workspace(n, c, v))
    check(load().rx_cross_entropy_loss_fwd(_ptr(logits), _ptr(tp), _ptr(ti), ignore_index, n, c, v, _REDUCTION[reduction], _ptr(loss),
                                           _ptr(coef), _ptr(saved), *_ws_args(ws), stream_ptr()), "rx_cross_entropy_loss_fwd")
    return loss, coef, saved


def cross_entropy_loss_bwd(logits, target, coef, saved, grad_loss, ignore_index=-100):
    n, c, v = _ncv(logits)
    tp, ti = _ce_targets(target)
    dlogits = torch.empty_like(logits)
    check(load().rx_cross_entropy_loss_bwd(_ptr(logits), _ptr(tp), _ptr(ti), ignore_index, n, c, v, _ptr(coef), _ptr(saved),
                                           _ptr(grad_loss), _ptr(dlogits), stream_ptr()), "rx_cross_entropy_loss_bwd")
    return dlogits
