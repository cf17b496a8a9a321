"""Validation preview: the slice-by-slice debug GIF of input, targets and predictions (`tr_config.val_preview`).

Three layers:
  * the numpy statements `panel_numpy` / `minmax_numpy` -- what the HIP kernel of csrc/rx_preview.hip (engine.ops.preview_panel)
    computes, and the oracle of its tests -- and `frames_numpy`, the layout engine.ops.preview_frames fills;
  * `parse_config`: `tr_config.val_preview` -> None or the checked settings;
  * `write_gif`: the finished uint8 frames -> an animated GIF through PIL (skipped, with one log line, when PIL is missing).

A panel scales every z-slice of every drawn channel to its own range: lo -> 0, hi -> 255, truncated.  All of it is float32, one
operation at a time.  Two rules are this project's own, because the float -> uint8 cast they replace is undefined: a slice that
holds a NaN or an infinity, and a slice whose range hi - lo overflows float32, are drawn like a flat slice, 127 throughout.
"""
import logging
import os

import numpy as np

EPS = np.float32(1e-6)
FLAT = 127                      # trunc(0.5 * 255): a slice without a range
DEFAULTS = {"sample": 0, "every": 1, "fps": 5, "tasks": None, "reference_sigmoid": False, "path": None}
_log = logging.getLogger(__name__)
_warned_no_pil = False


# ---- the numpy statements ---------------------------------------------------------------------------------------------------------
def _f32(a):
    """float32 array of what the kernel sees: float16 and bfloat16 values convert exactly (a bfloat16 volume arrives as a torch
    tensor, numpy has no such type)"""
    if hasattr(a, "detach"):
        a = a.detach().float().cpu().numpy()
    return np.asarray(a).astype(np.float32)


def _drawn(vol, sigmoid, dtype=np.float32):
    """(C, Z, H, W) -> `dtype` (c_drawn, Z, H * W): channels 0..2 when C == 3, else channel 0, after the optional activation"""
    v = _f32(vol).astype(dtype)
    if v.ndim != 4:
        raise ValueError(f"expected a (C, Z, H, W) volume, got {v.shape}")
    v = v[:3] if v.shape[0] == 3 else v[:1]
    if sigmoid:
        with np.errstate(over="ignore"):
            v = dtype(1) / (dtype(1) + np.exp(-v))
    return v.reshape(v.shape[0], v.shape[1], -1)


def _ranges(s):
    with np.errstate(invalid="ignore", over="ignore"):
        finite = np.isfinite(s).all(-1)
        lo, hi = s.min(-1), s.max(-1)
        r = hi - lo
        ok = finite & (r > s.dtype.type(EPS)) & np.isfinite(r)
    return lo, hi, r, finite, ok


def minmax_numpy(vol, sigmoid=False):
    """(C, Z, H, W) -> float32 (c_drawn, Z, 2) = (lo, hi) per drawn channel and slice; (nan, nan) for a slice that holds a NaN or an
    infinity"""
    lo, hi, _, finite, _ = _ranges(_drawn(vol, sigmoid))
    return np.stack([np.where(finite, lo, np.nan), np.where(finite, hi, np.nan)], axis=-1).astype(np.float32)


def panel_numpy(vol, sigmoid=False, dtype=np.float32):
    """(C, Z, H, W) float32 / float16 / bfloat16 -> uint8 (Z, H, W, 3).  Per drawn channel and z-slice, in float32:
    v = 1 / (1 + exp(-v)) if `sigmoid`; lo = min, hi = max, r = hi - lo; the byte is trunc(((v - lo) / r) * 255) if r > 1e-6, else
    127 for the whole slice -- also when the slice holds a NaN or an infinity or r is not finite (this project's rule).  C == 1:
    the grey value in all three bytes.  C == 3: channel k, scaled by its own range, in byte k.  Any other C: channel 0 as grey.
    `dtype=np.float64` evaluates the same statement in float64 from the float32 inputs: the measure of how far one float32 rounding
    can move a byte."""
    s = _drawn(vol, sigmoid, dtype)
    _, z, h, w = _f32(vol).shape
    lo, _, r, _, ok = _ranges(s)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        q = ((s - lo[..., None]) / r[..., None]) * dtype(255)
    q = np.where(ok[..., None], q, dtype(FLAT))
    b = np.trunc(q).astype(np.uint8).reshape(s.shape[0], z, h, w)
    if b.shape[0] == 1:
        b = np.repeat(b, 3, axis=0)
    return np.ascontiguousarray(np.moveaxis(b, 0, -1))


def frames_numpy(image, targets, preds, sigmoid_tasks=(), every=1):
    """image (C, Z, H, W), targets / preds {task: (C, Z, H, W)} -> uint8 (Zk, 2H, (1 + T)W, 3), Zk = ceil(Z / every) (slices 0, every,
    2 * every, ...).  Top row: the input panel, then one target panel per task in sorted task-name order; bottom row: an all-zero
    tile, then the prediction panels in the same order.  A one-channel prediction of a task in `sigmoid_tasks` is drawn through a
    sigmoid."""
    names = sorted(targets)
    top = [panel_numpy(image)] + [panel_numpy(targets[n]) for n in names]
    bottom = [np.zeros_like(top[0])]
    for n in names:
        p = preds[n]
        bottom.append(panel_numpy(p, sigmoid=n in sigmoid_tasks and p.shape[0] == 1))
    full = np.concatenate([np.concatenate(top, axis=2), np.concatenate(bottom, axis=2)], axis=1)
    return np.ascontiguousarray(full[::int(every)])


# ---- configuration ----------------------------------------------------------------------------------------------------------------
def parse_config(value, tasks, model_name=None):
    """`tr_config.val_preview` -> None (absent / false) or {"sample", "every", "fps", "tasks" (sorted names), "reference_sigmoid",
    "path"}.  `path` defaults to `<model_name>_debug.gif` (None when no model name is given).  A ValueError names the offending
    key."""
    if value is None or value is False:
        return None
    if value is True:
        value = {}
    if not isinstance(value, dict):
        raise ValueError(f"tr_config.val_preview: expected true / false or a mapping, got {type(value).__name__}")
    for k in value:
        if k not in DEFAULTS:
            raise ValueError(f"tr_config.val_preview: unknown key '{k}' (known: {', '.join(DEFAULTS)})")
    cfg = {**DEFAULTS, **value}

    def is_int(v):
        return isinstance(v, int) and not isinstance(v, bool)
    if not is_int(cfg["sample"]) or cfg["sample"] < 0:
        raise ValueError(f"tr_config.val_preview.sample: an index >= 0 into the first validation batch, got {cfg['sample']!r}")
    if not is_int(cfg["every"]) or cfg["every"] < 1:
        raise ValueError(f"tr_config.val_preview.every: an integer >= 1, got {cfg['every']!r}")
    if isinstance(cfg["fps"], bool) or not isinstance(cfg["fps"], (int, float)) or not cfg["fps"] > 0:
        raise ValueError(f"tr_config.val_preview.fps: must be > 0, got {cfg['fps']!r}")
    names = cfg["tasks"]
    if names is None:
        names = list(tasks)
    elif isinstance(names, str) or not isinstance(names, (list, tuple)):
        raise ValueError(f"tr_config.val_preview.tasks: expected a list of task names, got {names!r}")
    for n in names:
        if n not in tasks:
            raise ValueError(f"tr_config.val_preview.tasks: unknown task '{n}' (the targets are: {', '.join(tasks)})")
    if not isinstance(cfg["reference_sigmoid"], bool):
        raise ValueError(f"tr_config.val_preview.reference_sigmoid: true or false, got {cfg['reference_sigmoid']!r}")
    path = cfg["path"]
    if path is None:
        path = f"{model_name}_debug.gif" if model_name is not None else None
    elif not isinstance(path, str) or not path:
        raise ValueError(f"tr_config.val_preview.path: a file name, got {path!r}")
    return {"sample": cfg["sample"], "every": cfg["every"], "fps": cfg["fps"], "tasks": sorted(set(names)),
            "reference_sigmoid": cfg["reference_sigmoid"], "path": path}


def sigmoid_tasks_of(tasks, config):
    """the tasks whose prediction is drawn through a sigmoid: none by default (in eval mode the model already hands over activated
    values); with `reference_sigmoid` every previewed one-channel `activation: sigmoid` head -- the reference's second sigmoid"""
    if not config["reference_sigmoid"]:
        return ()
    return tuple(n for n in config["tasks"] if int(tasks[n].get("channels", 1)) == 1
                 and str(tasks[n].get("activation", "none")).lower() == "sigmoid")


# ---- the file ---------------------------------------------------------------------------------------------------------------------
def write_gif(frames, path, fps=5):
    """uint8 (Z, H, W, 3) frames -> an endlessly looping GIF at `path` (its directory is created), 1000 / fps ms per frame.  Returns
    the path, or None when PIL is not installed (logged once; nothing is written)."""
    global _warned_no_pil
    try:
        from PIL import Image
    except ImportError:
        if not _warned_no_pil:
            _log.warning("val_preview: PIL is not installed, no GIF is written")
            _warned_no_pil = True
        return None
    frames = np.asarray(frames)
    if frames.dtype != np.uint8 or frames.ndim != 4 or frames.shape[-1] != 3 or frames.shape[0] < 1:
        raise ValueError(f"write_gif: expected uint8 (Z, H, W, 3) frames, got {frames.dtype} {frames.shape}")
    parent = os.path.dirname(os.path.abspath(path))
    os.makedirs(parent, exist_ok=True)
    images = [Image.fromarray(f, "RGB") for f in frames]
    images[0].save(path, format="GIF", save_all=True, append_images=images[1:], duration=1000.0 / float(fps), loop=0)
    return path
