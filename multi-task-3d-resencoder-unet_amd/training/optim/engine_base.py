"""What the engine's optimizers share: the device-side gradient norm + clip coefficient (`clip_grad_norm`, `take_clip`), the lookup
of the model's training plan whose packs a fused update rewrites (`_plan`), the parameter checks, and the loss-scaling protocol of
`torch.amp.GradScaler` (`_step_supports_amp_scaling`: the scaler sets `optimizer.grad_scale` / `optimizer.found_inf` around `step()`).

The update kernels take ONE device scalar that they multiply into every gradient.  `_amp_begin` folds the scaler's `1 / grad_scale`
into the clip coefficient left by `clip_grad_norm` (the norm there is taken on the still-scaled gradients: clip first, unscale
after, the order of the trainer's plain path), and reads `found_inf` on the host once -- the same sync `GradScaler._maybe_opt_step`
performs for an optimizer without this protocol."""
import ctypes
from ctypes import c_void_p

import torch

from ...engine import lib as _l
from ...engine.lib import check, load, stream_ptr


def _p(t):
    return c_void_p(t.data_ptr()) if t is not None else c_void_p(0)


class EngineOptimizerBase(torch.optim.Optimizer):
    _step_supports_amp_scaling = True

    def __init__(self, params, defaults, model=None):
        super().__init__(params, defaults)
        self.model = model            # NetworkFromConfig whose training plan's packs are rewritten (optional)
        self._clip = None             # device scalar set by clip_grad_norm(), consumed by the next step()
        self._norm_ws = None          # scratch of rx_grad_norm_clip

    # ---- gradient clipping without touching the gradients -------------------------------------------------------
    @torch.no_grad()
    def clip_grad_norm(self, max_norm, norm_type=2.0):
        """same value as torch.nn.utils.clip_grad_norm_ (returned); the scale is applied inside the next step()"""
        grads = [p.grad for g in self.param_groups for p in g["params"] if p.grad is not None]
        if not grads:
            return torch.zeros(())
        if (float(norm_type) == 2.0
                and all(g.is_cuda and g.dtype == torch.float32 and g.is_contiguous() for g in grads)):
            # two launches (table kernel + one-workgroup finalize) instead of torch's ~20: norm AND coefficient on the device
            n = len(grads)
            VP, LP = ctypes.c_void_p * n, ctypes.c_long * n
            numel = LP(*[g.numel() for g in grads])
            need = load().rx_grad_norm_clip_partials(n, numel)
            if self._norm_ws is None or self._norm_ws.numel() < need or self._norm_ws.device != grads[0].device:
                self._norm_ws = torch.empty(int(need), dtype=torch.float32, device=grads[0].device)
            out = torch.empty(2, dtype=torch.float32, device=grads[0].device)
            from ...engine import ops as _ops
            _ops.timed_bytes("grad_norm_clip", 4 * sum(g.numel() for g in grads), lambda: check(
                load().rx_grad_norm_clip(n, VP(*[g.data_ptr() for g in grads]), numel, float(max_norm), _p(self._norm_ws),
                                         self._norm_ws.numel(), _p(out), stream_ptr()), "rx_grad_norm_clip"))
            self._clip = out[1:2]
            return out[0]
        norms = torch._foreach_norm(grads, norm_type)
        total = torch.linalg.vector_norm(torch.stack(norms), norm_type)
        self._clip = torch.clamp(max_norm / (total + 1e-6), max=1.0).to(torch.float32).reshape(1)
        return total

    def take_clip(self):
        """the device scalar left by clip_grad_norm() (None if it was not called); consumed"""
        clip, self._clip = self._clip, None
        return clip

    def _plan(self):
        plans = [p for p in getattr(self.model, "_plans", {}).values() if p.needs_grad and p.device.type == "cuda"] \
            if self.model is not None else []
        # (a plan with padded channel extents packs from zero-padded SHADOW tensors: the fused update-and-pack kernel would write
        # un-padded layouts -- such plans take the plain update and re-pack in their next forward)
        return plans[0] if len(plans) == 1 and not plans[0]._shadows else None

    def _checked_grad(self, p):
        """the contiguous gradient of a parameter the kernels can update; RxError for anything else"""
        if not p.is_cuda or p.dtype != torch.float32 or not p.is_contiguous():
            raise _l.RxError(f"{type(self).__name__} updates contiguous fp32 parameters on the HIP device only")
        return p.grad if p.grad.is_contiguous() else p.grad.contiguous()

    def _amp_begin(self):
        """-> (skip, clip): consumes clip_grad_norm()'s scalar and the GradScaler's `found_inf` / `grad_scale`, if it set them."""
        return amp_fold(self, self.take_clip())


def amp_fold(opt, clip):
    """(skip, scalar for the kernels): skip when the GradScaler found an inf / NaN gradient (ONE host read); otherwise
    clip * (1 / grad_scale), formed on the device in fp32 with one-element ops (1 / grad_scale when there is no clip)."""
    found_inf = getattr(opt, "found_inf", None)
    if found_inf is not None and float(found_inf) != 0.0:
        return True, None
    scale = getattr(opt, "grad_scale", None)
    if scale is not None:
        inv = torch.reciprocal(scale.to(torch.float32).reshape(1))
        clip = inv if clip is None else clip.to(torch.float32).reshape(1) * inv
    return False, clip
