"""SGD with momentum / Nesterov for the HIP engine: update, gradient clipping, loss un-scaling and weight re-pack in one pass.

The reference's other optimizer (train.py:70-77 builds `torch.optim.SGD(momentum=0.9, nesterov=True)`).  `EngineSGD` keeps torch's
`Optimizer` interface -- param_groups with every key `torch.optim.SGD` writes, per-parameter state `{"momentum_buffer": tensor}`, so
a `state_dict()` of either class loads into the other and lr schedulers work unchanged -- and torch's `_single_tensor_sgd`
arithmetic in fp32, but its `step()`

  * multiplies the gradient by a DEVICE scalar on the fly: the clip coefficient of `clip_grad_norm(max_norm)` (gradients stay
    untouched), times `1 / grad_scale` under a `torch.amp.GradScaler`,
  * updates a conv / convT weight and rewrites BOTH packed compute-dtype copies of the model's training plan in the same kernel
    (`rx_sgd_pack`), so the next forward finds fresh packs and re-packs nothing,
  * updates everything else with one table-kernel call (`rx_sgd_flat_multi`) per param group and `first` set: 16 bytes per
    parameter with momentum, 12 without.

CPU, non-fp32 or non-contiguous parameters are refused: this optimizer only exists for the engine."""
import ctypes

import torch

from ...engine import lib as _l
from ...engine.lib import check, load, stream_ptr
from .engine_base import EngineOptimizerBase, _p


class EngineSGD(EngineOptimizerBase):
    def __init__(self, params, model=None, lr=1e-3, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False):
        if lr < 0.0:
            raise ValueError(f"Invalid learning rate: {lr}")
        if momentum < 0.0:
            raise ValueError(f"Invalid momentum value: {momentum}")
        if weight_decay < 0.0:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        if nesterov and (momentum <= 0 or dampening != 0):
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")
        # (maximize / foreach / differentiable / fused: the keys torch.optim.SGD writes, at its defaults, so that state_dicts interchange)
        defaults = dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=nesterov,
                        maximize=False, foreach=None, differentiable=False, fused=None)
        super().__init__(params, defaults, model=model)

    @staticmethod
    def _check_group(group):
        if group.get("maximize", False):
            raise ValueError("EngineSGD does not support maximize=True (param group key 'maximize')")
        if group["nesterov"] and (group["momentum"] <= 0 or group["dampening"] != 0):
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")

    def _item(self, p, group):
        """(param, grad, buf or None, first) with the momentum buffer allocated (not initialised: a first step only writes it)"""
        g = self._checked_grad(p)
        if group["momentum"] == 0:
            return p, g, None, False
        st = self.state[p]
        first = st.get("momentum_buffer") is None
        if first:
            st["momentum_buffer"] = torch.empty_like(p, memory_format=torch.contiguous_format)
        return p, g, st["momentum_buffer"], first

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for group in self.param_groups:
            self._check_group(group)
        skip, clip = self._amp_begin()
        if skip:                           # the GradScaler found an inf / NaN: no launch, no state
            return loss
        plan = self._plan()
        packed = plan.packs.by_param() if plan is not None else {}      # (waits for the side stream)
        lib = load()
        for group in self.param_groups:
            flat = []                      # un-packed parameters of this group: one C call per `first` set (rx_sgd_flat_multi)
            for p in group["params"]:
                if p.grad is None:
                    continue
                p, g, buf, first = self._item(p, group)
                ent = packed.get(id(p))
                # (rx_sgd_pack holds a [taps][32][40] tile in LDS: up to 27 taps; wider kernels take the flat update, their pack
                # entry stays stale and the next forward re-packs it)
                if ent is not None and p[0, 0].numel() <= 27:
                    kind = 0 if ent.kind == "conv" else 1
                    check(lib.rx_sgd_pack(_l.DTYPE_CODE[plan.dtype], _p(p), _p(g), _p(buf), _p(clip), group["lr"], group["momentum"],
                                          group["dampening"], group["weight_decay"], int(group["nesterov"]), int(first), kind,
                                          p.shape[0], p.shape[1], p[0, 0].numel(), _p(ent.w_fwd), _p(ent.w_bwd), stream_ptr()),
                          "rx_sgd_pack")
                    ent.mark_fresh(plan._epoch())
                else:
                    flat.append((p, g, buf, first))
            self._flat_update(group, flat, clip)
        return loss

    def _flat_update(self, group, items, clip):
        """items: (param, grad, buf, first) of ONE param group -> rx_sgd_flat_multi on the current stream (tensors that share `first`
        go in one call: normally all of them)"""
        mom = group["momentum"] != 0
        for first in (True, False):
            its = [it for it in items if it[3] == first]
            if not its:
                continue
            n = len(its)
            VP, LP = ctypes.c_void_p * n, ctypes.c_long * n
            bufs = VP(*[b.data_ptr() for _, _, b, _ in its]) if mom else None
            nbytes = (16 if mom and not first else 12) * sum(p.numel() for p, _, _, _ in its)
            from ...engine import ops as _ops
            _ops.timed_bytes("sgd", nbytes, lambda: check(
                load().rx_sgd_flat_multi(n, VP(*[p.data_ptr() for p, _, _, _ in its]), VP(*[g.data_ptr() for _, g, _, _ in its]), bufs,
                                         LP(*[p.numel() for p, _, _, _ in its]), _p(clip), group["lr"], group["momentum"],
                                         group["dampening"], group["weight_decay"], int(group["nesterov"]), int(first), stream_ptr()),
                "rx_sgd_flat_multi"))

    # ---- the same update for a SUBSET of the parameters, on the current stream (the meaning of EngineAdamW.update_subset) ----
    @torch.no_grad()
    def update_subset(self, params, clip):
        group_of = {id(p): g for g in self.param_groups for p in g["params"]}
        per_group = {}
        for p in params:
            if p.grad is None:
                continue
            grp = group_of[id(p)]
            self._check_group(grp)
            per_group.setdefault(id(grp), (grp, []))[1].append(self._item(p, grp))
        for grp, items in per_group.values():
            self._flat_update(grp, items, clip)
