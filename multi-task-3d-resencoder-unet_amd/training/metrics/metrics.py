"""Validation metrics: overlap scores of the segmentation heads and the angular error of a normals head.

Three layers:
  * the numpy statements `seg_counts_numpy`, `class_counts_numpy`, `normal_stats_numpy` -- what the HIP kernels of
    csrc/rx_metrics.hip (engine.ops.seg_counts / class_counts / normal_stats) compute, and the oracles of their tests;
  * `scores_from_counts`: Dice, IoU, precision and recall from (TP, FP, FN);
  * `ValidationMetrics`: the per-epoch accumulator the trainer drives (`tr_config.val_metrics`, parsed by `parse_config`).
The opt-in surface-distance metrics (`tr_config.val_metrics.surface`) have their statements and scores in surface.py.

The values compared are the ones the model hands over in eval mode: `NetworkFromConfig.forward` applies the task activation there,
so a `sigmoid` head yields probabilities and the threshold applies as it is, while an `activation: none` head yields logits and
the threshold is moved to logit space (`pred_threshold`): the same voxels are positive either way.
"""
import math

import numpy as np

from .surface import default_bins, parse_surface, surface_metric_names, surface_scores

KINDS = ("binary", "multiclass", "normals", "none")
RATES = ("dice", "iou", "precision", "recall")
MAX_CLASSES = 64
_TOP_KEYS = ("threshold", "target_threshold", "tasks", "best", "surface")
_TASK_KEYS = ("kind",)
_BEST_KEYS = ("task", "metric", "mode")


# ---- the numpy statements ---------------------------------------------------------------------------------------------------------
def _f32(a):
    """float32 view of what the kernel sees: a bfloat16 / float16 value converts exactly"""
    return np.asarray(a).astype(np.float32)


def seg_counts_numpy(pred, target, thr_pred=0.5, thr_target=0.5):
    """(N, C, *spatial) -> int64 (N, C, 3) = (TP, FP, FN) of `pred > thr_pred` against `target > thr_target`: float32 comparisons
    (the thresholds are rounded to float32 first), so a NaN on either side is negative"""
    p, t = _f32(pred), _f32(target)
    n, c = p.shape[:2]
    a = (p > np.float32(thr_pred)).reshape(n, c, -1)
    b = (t > np.float32(thr_target)).reshape(n, c, -1)
    return np.stack([(a & b).sum(-1), (a & ~b).sum(-1), (~a & b).sum(-1)], axis=-1).astype(np.int64)


def argmax_numpy(x):
    """arg-max over axis 1 of (N, C, V) by the kernels' rule: best = 0; for k = 1 .. C-1: if x[k] > x[best], or x[best] is a NaN
    and x[k] is not: best = k.  The first maximum wins, a NaN is never chosen over a number, all-NaN gives class 0."""
    x = _f32(x)
    best = np.zeros((x.shape[0], x.shape[2]), dtype=np.int64)
    val = x[:, 0].copy()
    for k in range(1, x.shape[1]):
        xk = x[:, k]
        with np.errstate(invalid="ignore"):
            better = ~(xk <= val) & ~np.isnan(xk)
        best[better] = k
        val = np.where(better, xk, val)
    return best


def class_counts_numpy(pred, target, ignore_index=-100):
    """(N, C, *spatial) prediction, and a float target of the same shape (class probabilities, arg-max by the same rule) or an
    integer target (N, *spatial) of class indices -> int64 (N, C, 3) = per-class (TP, FP, FN).  A voxel with label l predicted as p
    adds TP[l] if p == l, else FP[p] and FN[l]; index voxels equal to `ignore_index`, or outside [0, C), are skipped."""
    p = _f32(pred)
    n, c = p.shape[:2]
    p = p.reshape(n, c, -1)
    pc = argmax_numpy(p)
    target = np.asarray(target)
    if target.dtype.kind in "iu":
        lab = target.reshape(n, -1).astype(np.int64)
        keep = (lab != ignore_index) & (lab >= 0) & (lab < c)
    else:
        lab = argmax_numpy(target.reshape(n, c, -1))
        keep = np.ones_like(lab, dtype=bool)
    out = np.zeros((n, c, 3), dtype=np.int64)
    for i in range(n):
        l, q = lab[i][keep[i]], pc[i][keep[i]]
        out[i, :, 0] = np.bincount(l[l == q], minlength=c)
        out[i, :, 1] = np.bincount(q[l != q], minlength=c)
        out[i, :, 2] = np.bincount(l[l != q], minlength=c)
    return out


def normal_mask_numpy(target):
    """(N, 3, V) -> bool (N, V): sqrt((tx*tx + ty*ty) + tz*tz) > 1e-6 in float32, one rounding per operation -- the mask of
    MaskedCosineLoss.  It is a predicate like the thresholds above, so it is taken in the kernel's own precision."""
    t = _f32(target)
    tt = (t[:, 0] * t[:, 0] + t[:, 1] * t[:, 1]) + t[:, 2] * t[:, 2]
    return np.sqrt(tt) > np.float32(1e-6)


def _normal_terms(pred, target, dtype):
    p, t = _f32(pred).astype(dtype), _f32(target).astype(dtype)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        pn = np.sqrt((p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1]) + p[:, 2] * p[:, 2])
        tn = np.sqrt((t[:, 0] * t[:, 0] + t[:, 1] * t[:, 1]) + t[:, 2] * t[:, 2])
        dot = (p[:, 0] * t[:, 0] + p[:, 1] * t[:, 1]) + p[:, 2] * t[:, 2]
        cos = dot / (np.maximum(pn, dtype(1e-8)) * np.maximum(tn, dtype(1e-8)))
        cos = np.minimum(np.maximum(cos, dtype(-1)), dtype(1))
        deg = np.arccos(cos) * dtype(180.0 / math.pi)
    return cos, deg


def normal_stats_numpy(pred, target, dtype=np.float64):
    """(N, 3, *spatial) -> (count int64 (N,), sums float64 (N, 2)): over the voxels of `normal_mask_numpy`,
    cos = dot / (max(|p|, 1e-8) * max(|t|, 1e-8)) clamped to [-1, 1] and deg = acos(cos) * 180 / pi, evaluated in float64 from the
    float32 inputs and summed in float64.  `dtype=np.float32` evaluates the per-voxel formula in float32 instead (still summed in
    float64): what the kernel does up to a few ulp per voxel, and the measure of how far float32 can be from this statement."""
    n = np.asarray(pred).shape[0]
    p, t = _f32(pred).reshape(n, 3, -1), _f32(target).reshape(n, 3, -1)
    mask = normal_mask_numpy(t)
    cos, deg = _normal_terms(p, t, dtype)
    count = mask.sum(-1).astype(np.int64)
    sums = np.stack([np.where(mask, cos, 0).astype(np.float64).sum(-1), np.where(mask, deg, 0).astype(np.float64).sum(-1)], axis=-1)
    return count, sums


# ---- scores -----------------------------------------------------------------------------------------------------------------------
def scores_from_counts(tp, fp, fn):
    """dice = 2TP / (2TP + FP + FN), iou = TP / (TP + FP + FN), precision = TP / (TP + FP), recall = TP / (TP + FN); scalars or
    arrays.  A zero denominator gives nan: nothing to score is not a score of 0 or 1."""
    tp, fp, fn = (np.asarray(a, dtype=np.float64) for a in (tp, fp, fn))

    def ratio(num, den):
        with np.errstate(invalid="ignore", divide="ignore"):
            r = np.where(den > 0, num / np.where(den > 0, den, 1.0), np.nan)
        return float(r) if r.ndim == 0 else r
    return {"dice": ratio(2 * tp, 2 * tp + fp + fn), "iou": ratio(tp, tp + fp + fn), "precision": ratio(tp, tp + fp),
            "recall": ratio(tp, tp + fn)}


# ---- configuration ----------------------------------------------------------------------------------------------------------------
def infer_kind(name, info, normal_keys=None):
    """`normals`: 3 channels and the task is in `normal_keys` (default: tasks named "normals"); `multiclass`: CrossEntropyLoss, or a
    softmax head with more than one channel; anything else `binary`, per channel"""
    keys = ("normals",) if normal_keys is None else tuple(normal_keys)
    channels = int(info.get("channels", 1))
    if channels == 3 and name in keys:
        return "normals"
    if info.get("loss_fn") == "CrossEntropyLoss" or (str(info.get("activation", "none")).lower() == "softmax" and channels > 1):
        return "multiclass"
    return "binary"


def pred_threshold(info, threshold):
    """the probability-space `threshold` in the space of the values the model hands over in eval mode: an `activation: none` head
    yields logits, so log(threshold / (1 - threshold)); any activated head yields probabilities"""
    if str(info.get("activation", "none")).lower() == "none":
        return math.log(threshold / (1.0 - threshold))
    return float(threshold)


def metric_names(kind, surface=None):
    """the metrics of a task of `kind`; `surface`: the parsed `surface` block when it covers the task (binary tasks only), which
    appends surface_dice_<t> per tolerance, assd, hd95 and surface_voxels"""
    if kind == "binary":
        return RATES + ("dice_per_patch",) + (surface_metric_names(surface["tolerances"]) if surface else ())
    if kind == "multiclass":
        return RATES + tuple(f"{r}_class_mean" for r in RATES) + ("dice_per_patch",)
    if kind == "normals":
        return ("mean_cos", "mean_angle_deg", "masked_voxels")
    return ()


def _surface_of(surface, name):
    """the parsed surface block if it covers task `name`, else None"""
    return surface if surface and name in surface["tasks"] else None


def parse_config(cfg, tasks, normal_keys=None, patch_size=None):
    """`tr_config.val_metrics` -> None (absent / false) or {"threshold", "target_threshold", "kinds": {task: kind}, "best": None |
    {"task", "metric", "mode"}, "surface": None | {"tolerances", "tasks"}}.  `patch_size`: the train patch size when known (the
    surface block refuses 2-D patches).  A ValueError names the offending key."""
    if cfg is None or cfg is False:
        return None
    if cfg is True:
        cfg = {}
    if not isinstance(cfg, dict):
        raise ValueError(f"tr_config.val_metrics: expected true / false or a mapping, got {type(cfg).__name__}")
    for k in cfg:
        if k not in _TOP_KEYS:
            raise ValueError(f"tr_config.val_metrics: unknown key '{k}' (known: {', '.join(_TOP_KEYS)})")
    out = {}
    for key in ("threshold", "target_threshold"):
        v = cfg.get(key, 0.5)
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not 0.0 < float(v) < 1.0:
            raise ValueError(f"tr_config.val_metrics.{key}: must lie in (0, 1), got {v!r}")
        out[key] = float(v)
    kinds = {name: infer_kind(name, info, normal_keys) for name, info in tasks.items()}
    overrides = cfg.get("tasks") or {}
    if not isinstance(overrides, dict):
        raise ValueError("tr_config.val_metrics.tasks: expected a mapping of task name to {kind: ...}")
    for name, spec in overrides.items():
        if name not in tasks:
            raise ValueError(f"tr_config.val_metrics.tasks: unknown task '{name}' (the targets are: {', '.join(tasks)})")
        spec = spec or {}
        if not isinstance(spec, dict):
            raise ValueError(f"tr_config.val_metrics.tasks.{name}: expected a mapping")
        for k in spec:
            if k not in _TASK_KEYS:
                raise ValueError(f"tr_config.val_metrics.tasks.{name}: unknown key '{k}' (known: {', '.join(_TASK_KEYS)})")
        if "kind" in spec:
            if spec["kind"] not in KINDS:
                raise ValueError(f"tr_config.val_metrics.tasks.{name}.kind: unknown kind '{spec['kind']}' (known: {', '.join(KINDS)})")
            kinds[name] = spec["kind"]
    for name, kind in kinds.items():
        channels = int(tasks[name].get("channels", 1))
        if kind == "multiclass" and channels > MAX_CLASSES:
            raise ValueError(f"tr_config.val_metrics.tasks.{name}.kind: multiclass takes at most {MAX_CLASSES} classes, "
                             f"the task has {channels}")
        if kind == "multiclass" and channels < 2:
            raise ValueError(f"tr_config.val_metrics.tasks.{name}.kind: multiclass needs at least 2 channels, the task has {channels}")
        if kind == "normals" and channels != 3:
            raise ValueError(f"tr_config.val_metrics.tasks.{name}.kind: normals needs 3 channels, the task has {channels}")
    out["kinds"] = kinds
    out["surface"] = parse_surface(cfg.get("surface"), kinds, patch_size)
    best = cfg.get("best")
    if best is not None:
        if not isinstance(best, dict):
            raise ValueError("tr_config.val_metrics.best: expected a mapping {task, metric, mode}")
        for k in best:
            if k not in _BEST_KEYS:
                raise ValueError(f"tr_config.val_metrics.best: unknown key '{k}' (known: {', '.join(_BEST_KEYS)})")
        for k in ("task", "metric"):
            if k not in best:
                raise ValueError(f"tr_config.val_metrics.best.{k}: missing")
        if best["task"] not in tasks:
            raise ValueError(f"tr_config.val_metrics.best.task: unknown task '{best['task']}' (the targets are: {', '.join(tasks)})")
        names = metric_names(kinds[best["task"]], _surface_of(out["surface"], best["task"]))
        if best["metric"] not in names:
            raise ValueError(f"tr_config.val_metrics.best.metric: unknown metric '{best['metric']}' for the {kinds[best['task']]} task "
                             f"'{best['task']}' (known: {', '.join(names) or 'none'})")
        mode = best.get("mode", "max")
        if mode not in ("max", "min"):
            raise ValueError(f"tr_config.val_metrics.best.mode: unknown mode '{mode}' (max or min)")
        best = {"task": best["task"], "metric": best["metric"], "mode": mode}
    out["best"] = best
    return out


# ---- the accumulator --------------------------------------------------------------------------------------------------------------
class ValidationMetrics:
    """Accumulates a validation epoch on the device.  `tasks`: the config's target table {name: {channels, activation, loss_fn,
    ...}}; `config`: `tr_config.val_metrics` (true or the mapping) or what `parse_config` made of it.

    update(outputs, targets)   one kernel per task on the current stream plus a few small torch ops on the per-sample rows; no host
                               synchronisation, and no buffer is created after the first call for a given shape
    compute()                  ONE device-to-host copy of the state -> {task: {metric: float}}
    reset()                    clears the state

    State, one int64 buffer (float64 words are views of it): per counting task C*3 summed (TP, FP, FN), the sum of the per-patch
    Dice values and the number of patches that had one; per normals task the masked voxels, the sum of cos and the sum of degrees.

    With a `surface` block, every covered binary task also owns 4 counts and a (2, bins) histogram of squared surface distances
    (engine.ops.surface_hist), pooled over the epoch.  `bins` follows from the first patch shape the accumulator sees, so these
    words are appended to the state then, and a second patch shape raises ValueError."""

    def __init__(self, tasks, config=True, normal_keys=None):
        cfg = config if isinstance(config, dict) and "kinds" in config else parse_config(config, tasks, normal_keys)
        if cfg is None:
            raise ValueError("ValidationMetrics: val_metrics is off")
        self.tasks = {k: dict(v) for k, v in tasks.items()}
        self.kinds = {k: v for k, v in cfg["kinds"].items() if v != "none"}
        self.threshold, self.target_threshold = cfg["threshold"], cfg["target_threshold"]
        self.thr_pred = {k: pred_threshold(self.tasks[k], self.threshold) for k, v in self.kinds.items() if v == "binary"}
        self.ignore_index = {k: int(self.tasks[k].get("loss_kwargs", {}).get("ignore_index", -100)) for k in self.kinds}
        self._slots, n = {}, 0
        for k, kind in self.kinds.items():
            words = 3 if kind == "normals" else int(self.tasks[k].get("channels", 1)) * 3 + 2
            self._slots[k] = (n, words)
            n += words
        self._words = max(n, 1)
        self._state = None
        self._scratch = {}
        self.surface = cfg.get("surface")
        self._surface_tasks = tuple(k for k in self.kinds if _surface_of(self.surface, k))
        self._surface_shape = None      # the patch shape (Z, Y, X) that fixed `bins`
        self._surface_slots = {}        # task -> offset of its 4 counts, followed by 2 * bins histogram words

    def _names(self, name):
        return metric_names(self.kinds[name], _surface_of(self.surface, name))

    def _surface_views(self, name):
        o, bins = self._surface_slots[name], default_bins(self._surface_shape)
        return self._state[o + 4:o + 4 + 2 * bins].view(2, bins), self._state[o:o + 4]

    def _surface_check(self, outputs):
        """refuses, before anything is added, a batch the histogram cannot take"""
        for name in self._surface_tasks:
            if name not in outputs:
                continue
            shape = tuple(outputs[name].shape)
            if len(shape) != 5:
                raise ValueError(f"ValidationMetrics: surface metrics need (N, C, Z, Y, X) batches, task '{name}' has shape {shape}")
            if self._surface_shape is not None and shape[2:] != self._surface_shape:
                raise ValueError(f"ValidationMetrics: surface metrics were started on patches of shape {self._surface_shape}, task "
                                 f"'{name}' now has {shape[2:]}: the histogram length is fixed by the first shape")

    def _surface_update(self, name, pred, target):
        import torch
        from ...engine import ops as E
        shape = tuple(pred.shape[2:])
        if self._surface_shape is None:      # the state grows once, before anything was added to the new words
            self._surface_shape = shape
            n = self._words
            for k in self._surface_tasks:
                self._surface_slots[k] = n
                n += 4 + 2 * default_bins(shape)
            grown = torch.zeros(n, dtype=torch.int64, device=self._state.device)
            grown[:self._words].copy_(self._state)
            self._state, self._words = grown, n
        key = ("surface", name, tuple(pred.shape), pred.device)
        scratch = self._scratch.get(key)
        if scratch is None:
            scratch = self._scratch[key] = E.surface_scratch(pred.shape, pred.device)
        hist, counts = self._surface_views(name)
        E.surface_hist(pred, target, self.thr_pred[name], self.target_threshold, hist=hist, counts=counts, scratch=scratch)

    def _views(self, name):
        o, w = self._slots[name]
        s = self._state[o:o + w]
        if self.kinds[name] == "normals":
            return s[0:1], s[1:3].view(self._f64)
        return s[:w - 2], s[w - 2:w - 1].view(self._f64), s[w - 1:w]

    def _buffers(self, name, kind, pred):
        import torch
        key = (name, tuple(pred.shape), pred.device)
        b = self._scratch.get(key)
        if b is None:
            n, c = pred.shape[:2]
            if kind == "normals":
                v = pred.numel() // (n * 3)
                from ...engine.lib import load
                b = (torch.zeros(n, dtype=torch.int64, device=pred.device), torch.zeros((n, 2), dtype=torch.float64, device=pred.device),
                     torch.empty(max(load().rx_normal_stats_workspace(n, v) // 8, 1), dtype=torch.float64, device=pred.device))
            else:
                b = (torch.zeros((n, c, 3), dtype=torch.int64, device=pred.device), torch.zeros((n, 3), dtype=torch.int64, device=pred.device),
                     torch.zeros(n, dtype=torch.float64, device=pred.device), torch.zeros(n, dtype=torch.float64, device=pred.device),
                     torch.zeros(n, dtype=torch.bool, device=pred.device))
            self._scratch[key] = b
        return b

    def update(self, outputs, targets):
        import torch
        from ...engine import ops as E
        self._f64 = torch.float64
        self._surface_check(outputs)
        for name, kind in self.kinds.items():
            if name not in outputs or name not in targets:
                continue
            pred, target = outputs[name].detach(), targets[name]
            if self._state is None:
                self._state = torch.zeros(self._words, dtype=torch.int64, device=pred.device)
            if kind == "normals":
                count, sums, ws = self._buffers(name, kind, pred)
                count.zero_(), sums.zero_()
                E.normal_stats(pred, target, out=(count, sums), ws=ws)
                total, fsum = self._views(name)
                total.add_(count.sum()), fsum.add_(sums.sum(0))
                continue
            rows, per, num, den, valid = self._buffers(name, kind, pred)
            rows.zero_()
            if kind == "binary":
                E.seg_counts(pred, target, self.thr_pred[name], self.target_threshold, out=rows)
            else:
                E.class_counts(pred, target, self.ignore_index[name], out=rows)
            total, dsum, dcnt = self._views(name)
            total.add_(rows.sum(0).view(-1))
            # per-patch Dice over the patches that have anything to score: 2TP / (2TP + FP + FN) of the patch's summed channels
            torch.sum(rows, dim=1, out=per)
            torch.mul(per[:, 0], 2.0, out=num)
            torch.add(num, per[:, 1] + per[:, 2], out=den)
            torch.gt(den, 0, out=valid)
            den.masked_fill_(~valid, 1.0)
            num.div_(den).masked_fill_(~valid, 0.0)
            dsum.add_(num.sum()), dcnt.add_(valid.sum())
            if name in self._surface_tasks:      # last: it may move the state, and the views above are of the old one
                self._surface_update(name, pred, target)

    def reset(self):
        if self._state is not None:
            self._state.zero_()

    def compute(self):
        out = {name: {m: float("nan") for m in self._names(name)} for name in self.kinds}
        if self._state is None:
            return out
        host = self._state.cpu().numpy()      # the one copy (and the one synchronisation) of the epoch
        for name, kind in self.kinds.items():
            o, w = self._slots[name]
            s = host[o:o + w]
            if kind == "normals":
                cnt, sums = int(s[0]), s[1:3].view(np.float64)
                out[name] = {"mean_cos": float(sums[0] / cnt) if cnt else float("nan"),
                             "mean_angle_deg": float(sums[1] / cnt) if cnt else float("nan"), "masked_voxels": float(cnt)}
                continue
            counts = s[:w - 2].reshape(-1, 3)
            dsum, dcnt = float(s[w - 2:w - 1].view(np.float64)[0]), int(s[w - 1])
            res = scores_from_counts(counts[:, 0].sum(), counts[:, 1].sum(), counts[:, 2].sum())
            if kind == "multiclass":
                per_class = scores_from_counts(counts[:, 0], counts[:, 1], counts[:, 2])
                for r in RATES:
                    ok = ~np.isnan(per_class[r])
                    res[f"{r}_class_mean"] = float(per_class[r][ok].mean()) if ok.any() else float("nan")
            res["dice_per_patch"] = dsum / dcnt if dcnt else float("nan")
            if name in self._surface_slots:
                so, bins = self._surface_slots[name], default_bins(self._surface_shape)
                res.update(surface_scores(host[so + 4:so + 4 + 2 * bins].reshape(2, bins), host[so:so + 4], self.surface["tolerances"]))
            elif name in self._surface_tasks:      # covered, but no batch seen yet
                res.update({m: float("nan") for m in surface_metric_names(self.surface["tolerances"])})
            out[name] = res
        return out

    def counts(self, name):
        """the epoch's summed (TP, FP, FN) rows of a counting task, int64 (C, 3) on the host (synchronises)"""
        o, w = self._slots[name]
        return self._state[o:o + w - 2].cpu().numpy().reshape(-1, 3)
