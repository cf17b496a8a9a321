"""Surface-distance validation metrics: surface Dice at a tolerance, average symmetric surface distance, 95 % Hausdorff distance.

Two layers:
  * the numpy statements `edges_numpy`, `edt_sq_numpy`, `surface_hist_numpy` -- what the HIP kernels of csrc/rx_surface.hip
    (engine.ops.mask_edges / edt_sq / surface_hist) compute bit for bit, and the oracles of their tests.  Plain numpy, no scipy;
  * `surface_scores`: the scores, on the host in float64, as a function of the histogram alone.

A volume is (Z, Y, X); distances are in voxels and isotropic.  Everything a kernel produces is an integer: the squared distance
from an edge voxel of one mask to the nearest edge voxel of the other is the histogram's bin index.  `ValidationMetrics` adds every
validation batch of an epoch into one histogram per task, so the scores are POOLED over the epoch's voxels, as `dice` is -- not a
mean of per-patch scores.
"""
import math

import numpy as np

EDT_NONE = 1 << 30      # "no feature anywhere": larger than any squared distance in a volume of extents <= MAX_EXTENT
MAX_EXTENT = 1024       # EDT_NONE + (MAX_EXTENT - 1)^2 fits int32
DEFAULT_TOLERANCES = (1.0, 2.0)
SURFACE_KEYS = ("tolerances", "tasks")


def _f32(a):
    """float32 view of what the kernel sees: a bfloat16 / float16 value converts exactly"""
    return np.asarray(a).astype(np.float32)


def _volume(a, what):
    a = np.asarray(a)
    if a.ndim != 3:
        raise ValueError(f"{what}: expected a (Z, Y, X) volume, got shape {a.shape} (2-D patches have no surface distance here)")
    return a


# ---- the numpy statements ---------------------------------------------------------------------------------------------------------
def edges_numpy(mask):
    """bool (Z, Y, X) -> bool (Z, Y, X): mask & ~erode6(mask), erode6 = the AND of the mask with its six face neighbours, everything
    outside the volume being background -- so a mask voxel on the volume's border is an edge.  (scipy's
    mask & ~binary_erosion(mask) with the default structure and border_value=0.)"""
    m = _volume(mask, "edges_numpy").astype(bool)
    er = m.copy()
    for ax in range(3):
        lo = np.zeros_like(m)      # lo[i] = m[i - 1], background at i = 0
        hi = np.zeros_like(m)      # hi[i] = m[i + 1], background at the far end
        src = [slice(None)] * 3
        dst = [slice(None)] * 3
        src[ax], dst[ax] = slice(0, -1), slice(1, None)
        lo[tuple(dst)] = m[tuple(src)]
        hi[tuple(src)] = m[tuple(dst)]
        er &= lo & hi
    return m & ~er


def _edt_pass(g, axis):
    """g'[i] = min(EDT_NONE, min_j (g[j] + (i - j)^2)) along `axis`, int64 arithmetic"""
    g = np.moveaxis(g, axis, -1)
    n = g.shape[-1]
    out = np.full(g.shape, EDT_NONE, dtype=np.int64)
    idx = np.arange(n, dtype=np.int64)
    for j in range(n):
        np.minimum(out, g[..., j:j + 1] + (idx - j) ** 2, out=out)
    return np.moveaxis(out, -1, axis)


def edt_sq_numpy(feature):
    """bool (Z, Y, X) -> int32 (Z, Y, X): the exact squared Euclidean distance to the nearest True voxel, EDT_NONE everywhere if
    there is none.  Separable, in the kernel's order x, then y, then z (the order does not change the result): from g0 = 0 on a
    feature and EDT_NONE elsewhere, per axis g'[i] = min_j (g[j] + (i - j)^2), clamped to EDT_NONE, in integers."""
    f = _volume(feature, "edt_sq_numpy").astype(bool)
    if max(f.shape) > MAX_EXTENT:
        raise ValueError(f"edt_sq_numpy: an extent above {MAX_EXTENT} (shape {f.shape})")
    g = np.where(f, 0, EDT_NONE).astype(np.int64)
    for axis in (2, 1, 0):
        g = _edt_pass(g, axis)
    return g.astype(np.int32)


def default_bins(shape):
    """(Z - 1)^2 + (Y - 1)^2 + (X - 1)^2 + 1: no finite squared distance inside the volume can overflow it"""
    z, y, x = (int(s) for s in shape)
    return (z - 1) ** 2 + (y - 1) ** 2 + (x - 1) ** 2 + 1


def surface_hist_numpy(pred, target, thr_pred, thr_target, bins=None):
    """one (Z, Y, X) pair -> (hist int64 (2, bins), counts int64 (4,)).  Masks: pred > thr_pred and target > thr_target, the
    float32 comparisons of `seg_counts_numpy` (a NaN is negative; bf16 / fp16 values are widened first).  With Ep, Et the edges of
    the two masks: hist[0] counts the voxels of Ep by d2 = edt_sq(Et) there, hist[1] the voxels of Et by edt_sq(Ep);
    counts = (|Ep|, |Et|, unmatched_pred, unmatched_target), where an edge voxel whose distance is EDT_NONE (the other edge set is
    empty) is unmatched and goes to no bin.  `bins` defaults to `default_bins(shape)`; with a smaller caller-given `bins`, a
    distance >= bins that is not EDT_NONE goes to the LAST bin."""
    p, t = _f32(_volume(pred, "surface_hist_numpy")), _f32(_volume(target, "surface_hist_numpy"))
    if p.shape != t.shape:
        raise ValueError(f"surface_hist_numpy: prediction {p.shape} against target {t.shape}")
    bins = default_bins(p.shape) if bins is None else int(bins)
    if bins < 1:
        raise ValueError(f"surface_hist_numpy: bins must be positive (got {bins})")
    ep, et = edges_numpy(p > np.float32(thr_pred)), edges_numpy(t > np.float32(thr_target))
    hist = np.zeros((2, bins), dtype=np.int64)
    counts = np.zeros(4, dtype=np.int64)
    for row, (e, other) in enumerate(((ep, et), (et, ep))):
        d = edt_sq_numpy(other)[e].astype(np.int64)
        counts[row] = d.size
        counts[2 + row] = int((d >= EDT_NONE).sum())
        hist[row] = np.bincount(np.minimum(d[d < EDT_NONE], bins - 1), minlength=bins)
    return hist, counts


# ---- scores -----------------------------------------------------------------------------------------------------------------------
def tolerance_name(tau):
    return "surface_dice_%g" % tau


def surface_metric_names(tolerances):
    return tuple(tolerance_name(t) for t in tolerances) + ("assd", "hd95", "surface_voxels")


def surface_scores(hist, counts, tolerances):
    """hist int64 (2, bins), counts (|Ep|, |Et|, unmatched_pred, unmatched_target) -> {name: float}, float64 on the host.
    With n0 = hist[0].sum(), n1 = hist[1].sum(), u = unmatched_pred + unmatched_target:

      surface_dice_<t>  (sum_{k <= t^2} hist[0][k] + sum_{k <= t^2} hist[1][k]) / (n0 + n1 + u): an edge with nothing to match is
                        a miss at every tolerance; <t> is formatted with %g
      assd              (sum_k hist[0][k] sqrt(k) + sum_k hist[1][k] sqrt(k)) / (n0 + n1), summed in ascending k
      hd95              the larger of the two rows' 95th percentiles BY NEAREST RANK: for a row, sqrt(k*) with k* the smallest k
                        whose cumulative count reaches ceil(0.95 n_row); an empty row contributes nothing.  Nearest rank on purpose:
                        numpy's interpolating percentile needs the sorted distances, and this must be a function of the histogram
                        alone
      surface_voxels    float(n0 + n1 + u)

    A zero denominator gives nan (`scores_from_counts` does the same).  The scores are pooled over whatever was added into the
    histogram."""
    hist = np.asarray(hist, dtype=np.int64)
    counts = np.asarray(counts, dtype=np.int64)
    if hist.ndim != 2 or hist.shape[0] != 2 or counts.shape != (4,):
        raise ValueError(f"surface_scores: hist (2, bins) and counts (4,), got {hist.shape} and {counts.shape}")
    n0, n1 = int(hist[0].sum()), int(hist[1].sum())
    u = int(counts[2]) + int(counts[3])
    nan = float("nan")
    out = {}
    cum = np.cumsum(hist, axis=1)
    last = hist.shape[1] - 1
    for tau in tolerances:
        k = min(int(math.floor(float(tau) ** 2)), last)      # the bins k <= tau^2
        out[tolerance_name(tau)] = float(cum[0, k] + cum[1, k]) / float(n0 + n1 + u) if n0 + n1 + u else nan
    root = np.sqrt(np.arange(hist.shape[1], dtype=np.float64))
    total = 0.0
    for k in np.nonzero(hist[0] + hist[1])[0]:      # ascending k
        total += (float(hist[0, k]) + float(hist[1, k])) * root[k]
    out["assd"] = float(total) / float(n0 + n1) if n0 + n1 else nan
    hd = nan
    for row, n in ((0, n0), (1, n1)):
        if n:
            rank = int(math.ceil(0.95 * n))
            k_star = int(np.searchsorted(cum[row], rank, side="left"))
            v = float(math.sqrt(k_star))
            hd = v if hd != hd else max(hd, v)
    out["hd95"] = hd
    out["surface_voxels"] = float(n0 + n1 + u)
    return out


# ---- configuration ----------------------------------------------------------------------------------------------------------------
def parse_surface(cfg, kinds, patch_size=None):
    """`tr_config.val_metrics.surface` -> None (absent / false) or {"tolerances": (floats), "tasks": (names)}; `true` means
    tolerances (1, 2) and every binary task.  `kinds`: {task: kind} as `parse_config` resolved them; `patch_size`: the train patch
    size when known (a 2-D one is refused).  A ValueError names the offending key."""
    key = "tr_config.val_metrics.surface"
    if cfg is None or cfg is False:
        return None
    if cfg is True:
        cfg = {}
    if not isinstance(cfg, dict):
        raise ValueError(f"{key}: expected true / false or a mapping, got {type(cfg).__name__}")
    for k in cfg:
        if k not in SURFACE_KEYS:
            raise ValueError(f"{key}: unknown key '{k}' (known: {', '.join(SURFACE_KEYS)})")
    tol = cfg.get("tolerances", DEFAULT_TOLERANCES)
    if not isinstance(tol, (list, tuple)) or not tol:
        raise ValueError(f"{key}.tolerances: expected a non-empty list of numbers, got {tol!r}")
    out_tol = []
    for t in tol:
        if isinstance(t, bool) or not isinstance(t, (int, float)) or not math.isfinite(float(t)) or float(t) < 0:
            raise ValueError(f"{key}.tolerances: every tolerance must be a finite number >= 0, got {t!r}")
        if float(t) in out_tol:
            raise ValueError(f"{key}.tolerances: duplicate tolerance {t!r}")
        out_tol.append(float(t))
    binary = tuple(n for n, k in kinds.items() if k == "binary")
    names = cfg.get("tasks")
    if names is None:
        names = binary
    else:
        if isinstance(names, str) or not isinstance(names, (list, tuple)):
            raise ValueError(f"{key}.tasks: expected a list of task names, got {names!r}")
        for n in names:
            if n not in kinds:
                raise ValueError(f"{key}.tasks: unknown task '{n}' (the targets are: {', '.join(kinds)})")
            if kinds[n] != "binary":
                raise ValueError(f"{key}.tasks: task '{n}' is of kind '{kinds[n]}', surface metrics take binary tasks only")
    if patch_size is not None and len(tuple(patch_size)) != 3:
        raise ValueError(f"{key}: needs 3-D patches, train_patch_size is {tuple(patch_size)}")
    return {"tolerances": tuple(out_tol), "tasks": tuple(names)}
