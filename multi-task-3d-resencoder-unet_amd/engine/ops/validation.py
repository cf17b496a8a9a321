"""Validation on the device: the metric counts (training/metrics/metrics.py holds the numpy statements and `ValidationMetrics`), the
surface-distance histograms (training/metrics/surface.py holds the numpy statements and the scores) and the preview panels
(training/visualization/preview.py holds the numpy statements, the config and the GIF writer)."""
import torch

from .. import lib as _l
from ..lib import check, load, stream_ptr
from .core import FLOATS, _code, _ncv, _ptr, device_batch, result_tensor, timed_bytes


# ---- validation metrics ------------------------------------------------------------------------------------------------------------
def _metric_pred(fn, pred, min_dim=3):
    return device_batch(fn, pred, f"the host statement is training.metrics.{fn}_numpy", what="prediction", dtypes=FLOATS,
                        rank=min_dim, or_more=True, layout="(N, C, *spatial)")


def _metric_f32_target(fn, pred, target):
    if not isinstance(target, torch.Tensor) or target.device != pred.device:
        raise _l.RxError(f"{fn}: the target must be a tensor on the prediction's device")
    if target.dtype != torch.float32:
        raise _l.RxError(f"{fn}: target dtype {target.dtype} (float32)")
    if target.shape != pred.shape:
        raise _l.RxError(f"{fn}: target shape {tuple(target.shape)} against prediction shape {tuple(pred.shape)}")
    return target.contiguous()


def seg_counts(pred, target, thr_pred=0.5, thr_target=0.5, out=None):
    """binary confusion per (sample, channel) of a float32 / bfloat16 / float16 (N, C, *spatial) device prediction against a float32
    target of the same shape: int64 (N, C, 3) = (TP, FP, FN) of `pred > thr_pred` against `target > thr_target`, float32 compares,
    a NaN is negative (training.metrics.seg_counts_numpy is the statement).  ADDED into `out` when given (the caller zeroes it),
    else returned in a fresh zeroed tensor; on the current stream, no synchronisation."""
    p = _metric_pred("seg_counts", pred, 2)
    t = _metric_f32_target("seg_counts", p, target)
    n, c, v = _ncv(p)
    out = result_tensor("seg_counts", "out", out, (n, c, 3), torch.int64, p.device, torch.zeros)
    timed_bytes("seg_counts", p.numel() * (p.element_size() + 4),
                lambda: check(load().rx_seg_counts(_ptr(p), _code(p.dtype), _ptr(t), n, c, v, float(thr_pred), float(thr_target), _ptr(out),
                                                   stream_ptr()), "rx_seg_counts"))
    return out


def class_counts(pred, target, ignore_index=-100, out=None):
    """multi-class confusion by arg-max over the 2..64 channels of an (N, C, *spatial) device prediction; `target` is float32 class
    probabilities of the same shape or int64 class indices (N, *spatial), where `ignore_index` voxels are skipped: int64 (N, C, 3)
    = per-class (TP, FP, FN) (training.metrics.class_counts_numpy is the statement).  ADDED into `out` when given."""
    p = _metric_pred("class_counts", pred)
    n, c, v = _ncv(p)
    if isinstance(target, torch.Tensor) and target.dtype == torch.int64:
        if target.device != p.device or tuple(target.shape) != (n,) + tuple(p.shape[2:]):
            raise _l.RxError(f"class_counts: index target {tuple(target.shape)} on {target.device} against prediction {tuple(p.shape)} "
                             f"on {p.device}")
        tp, ti, tbytes = None, target.contiguous(), n * v * 8
    else:
        tp, ti, tbytes = _metric_f32_target("class_counts", p, target), None, p.numel() * 4
    out = result_tensor("class_counts", "out", out, (n, c, 3), torch.int64, p.device, torch.zeros)
    timed_bytes("class_counts", p.numel() * p.element_size() + tbytes,
                lambda: check(load().rx_class_counts(_ptr(p), _code(p.dtype), _ptr(tp), _ptr(ti), int(ignore_index), n, c, v, _ptr(out),
                                                     stream_ptr()), "rx_class_counts"))
    return out


def normal_stats(pred, target, out=None, ws=None):
    """angular agreement of a 3-channel (N, 3, *spatial) device prediction with a float32 target over the voxels where |target| >
    1e-6: (count int64 (N,), sums float64 (N, 2) = (sum of cos, sum of the angle in degrees)), float32 per voxel, float64 sums in a
    fixed order (training.metrics.normal_stats_numpy is the statement).  ADDED into `out=(count, sums)` when given.  `ws`: a float64
    device tensor of at least `rx_normal_stats_workspace(N, V) / 8` elements for the partials, else one is taken from the allocator."""
    p = _metric_pred("normal_stats", pred)
    t = _metric_f32_target("normal_stats", p, target)
    n, c, v = _ncv(p)
    if c != 3:
        raise _l.RxError(f"normal_stats: expected 3 channels, got {tuple(p.shape)}")
    if out is not None and (not isinstance(out, (tuple, list)) or len(out) != 2):
        raise _l.RxError("normal_stats: `out` must be the pair (count, sums)")
    count = result_tensor("normal_stats", "out[0]", None if out is None else out[0], (n,), torch.int64, p.device, torch.zeros)
    sums = result_tensor("normal_stats", "out[1]", None if out is None else out[1], (n, 2), torch.float64, p.device, torch.zeros)
    nbytes = load().rx_normal_stats_workspace(n, v)
    if ws is None:
        ws = torch.empty(nbytes // 8, dtype=torch.float64, device=p.device)
    elif not isinstance(ws, torch.Tensor) or ws.device != p.device or ws.dtype != torch.float64 or not ws.is_contiguous():
        raise _l.RxError(f"normal_stats: `ws` must be a contiguous float64 tensor on {p.device}")
    timed_bytes("normal_stats", p.numel() * (p.element_size() + 4),
                lambda: check(load().rx_normal_stats(_ptr(p), _code(p.dtype), _ptr(t), n, v, _ptr(count), _ptr(sums), _ptr(ws), ws.numel() * 8,
                                                     stream_ptr()), "rx_normal_stats"))
    return count, sums


# ---- surface-distance metrics (csrc/rx_surface.hip; training/metrics/surface.py holds the numpy statements) ---------------------------
def _surface_volumes(fn, t, what, dtypes, statement):
    """a device (N, C, Z, Y, X) batch of `dtypes`, every extent within the library's limit -> it made contiguous"""
    t = device_batch(fn, t, f"the host statement is training.metrics.{statement}", what=what, dtypes=dtypes, rank=5,
                     layout="(N, C, Z, Y, X)")
    if max(t.shape[2:]) > _l.RX_EDT_MAX_EXTENT:
        raise _l.RxError(f"{fn}: an extent above {_l.RX_EDT_MAX_EXTENT} in {tuple(t.shape)}")
    return t


def _mask_edges_launch(v, threshold, out):
    n, c, z, y, x = v.shape
    check(load().rx_mask_edges(_ptr(v), _code(v.dtype), float(threshold), n * c, z, y, x, _ptr(out), stream_ptr()), "rx_mask_edges")


def _edt_sq_launch(f, out):
    n, c, z, y, x = f.shape
    check(load().rx_edt_sq(_ptr(f), n * c, z, y, x, _ptr(out), stream_ptr()), "rx_edt_sq")


def _surface_hist_launch(edges, dist, hist_row, count, unmatched):
    check(load().rx_surface_hist(_ptr(edges), _ptr(dist), edges.numel(), hist_row.numel(), _ptr(hist_row), _ptr(count), _ptr(unmatched),
                                 stream_ptr()), "rx_surface_hist")


def mask_edges(values, threshold, out=None):
    """the edge voxels of `values > threshold` per (sample, channel) volume of a float32 / bfloat16 / float16 (N, C, Z, Y, X) device
    batch -> uint8 (N, C, Z, Y, X), 1 on a mask voxel that lies on its volume's border or has a face neighbour outside the mask
    (float32 compare, a NaN is outside; training.metrics.edges_numpy is the statement).  On the current stream, no synchronisation."""
    v = _surface_volumes("mask_edges", values, "values", FLOATS, "edges_numpy")
    out = result_tensor("mask_edges", "out", out, v.shape, torch.uint8, v.device)
    timed_bytes("mask_edges", v.numel() * (v.element_size() + 1), lambda: _mask_edges_launch(v, threshold, out))
    return out


def edt_sq(feature, out=None):
    """the exact squared Euclidean distance transform per (sample, channel) volume of a uint8 or bool (N, C, Z, Y, X) device batch ->
    int32 (N, C, Z, Y, X): the squared distance in voxels to the volume's nearest non-zero voxel, EDT_NONE = 1 << 30 throughout a
    volume that has none (training.metrics.edt_sq_numpy is the statement).  Extents up to 1024.  On the current stream, no
    synchronisation, no workspace."""
    f = _surface_volumes("edt_sq", feature, "feature", (torch.uint8, torch.bool), "edt_sq_numpy")
    out = result_tensor("edt_sq", "out", out, f.shape, torch.int32, f.device)
    timed_bytes("edt_sq", f.numel() * (1 + 4), lambda: _edt_sq_launch(f, out))      # the y and z passes are extra time, not bytes
    return out


def surface_scratch(shape, device):
    """the buffers `surface_hist` works in for batches of `shape` (N, C, Z, Y, X): (prediction edges uint8, target edges uint8,
    distances int32)"""
    shape = tuple(shape)
    return (torch.empty(shape, dtype=torch.uint8, device=device), torch.empty(shape, dtype=torch.uint8, device=device),
            torch.empty(shape, dtype=torch.int32, device=device))


def surface_hist(pred, target, thr_pred, thr_target, hist=None, counts=None, scratch=None):
    """the histograms of squared surface distances between `pred > thr_pred` and `target > thr_target`, pooled over the N * C volumes
    of a float32 / bfloat16 / float16 (N, C, Z, Y, X) device prediction and a float32 target of the same shape
    (training.metrics.surface_hist_numpy, summed over the volumes, is the statement): with Ep, Et the edges of the two masks,
    hist[0] counts the voxels of Ep by their squared distance to Et and hist[1] those of Et by their squared distance to Ep;
    counts = (|Ep|, |Et|, unmatched_pred, unmatched_target), where an edge voxel is unmatched, and goes to no bin, when the other
    edge set of its volume is empty.  ADDED into `hist` int64 (2, bins) and `counts` int64 (4,) when given (the caller zeroes
    them); else fresh zeroed tensors with bins = (Z-1)^2 + (Y-1)^2 + (X-1)^2 + 1, which no distance can overflow.  With a smaller
    caller-given `bins`, a distance >= bins goes to the LAST bin.  `scratch`: what `surface_scratch(pred.shape, device)` returned,
    kept across calls; with it the call allocates nothing.  Ten kernel launches on the current stream, no synchronisation.
    Returns (hist, counts)."""
    p = _surface_volumes("surface_hist", pred, "prediction", FLOATS, "surface_hist_numpy")
    t = _metric_f32_target("surface_hist", p, target)
    z, y, x = p.shape[2:]
    if hist is None:
        hist = torch.zeros((2, (z - 1) ** 2 + (y - 1) ** 2 + (x - 1) ** 2 + 1), dtype=torch.int64, device=p.device)
    elif (not isinstance(hist, torch.Tensor) or hist.device != p.device or hist.dtype != torch.int64 or hist.dim() != 2
          or hist.shape[0] != 2 or hist.shape[1] < 1 or not hist.is_contiguous()):
        raise _l.RxError(f"surface_hist: `hist` must be a contiguous int64 tensor of shape (2, bins) on {p.device}")
    counts = result_tensor("surface_hist", "counts", counts, (4,), torch.int64, p.device, torch.zeros)
    if scratch is None:
        scratch = surface_scratch(p.shape, p.device)
    elif not isinstance(scratch, (tuple, list)) or len(scratch) != 3:
        raise _l.RxError("surface_hist: `scratch` must be what surface_scratch(pred.shape, device) returned")
    ep = result_tensor("surface_hist", "scratch[0]", scratch[0], p.shape, torch.uint8, p.device)
    et = result_tensor("surface_hist", "scratch[1]", scratch[1], p.shape, torch.uint8, p.device)
    dist = result_tensor("surface_hist", "scratch[2]", scratch[2], p.shape, torch.int32, p.device)

    def run():
        _mask_edges_launch(p, thr_pred, ep)
        _mask_edges_launch(t, thr_target, et)
        _edt_sq_launch(et, dist)
        _surface_hist_launch(ep, dist, hist[0], counts[0:1], counts[2:3])
        _edt_sq_launch(ep, dist)
        _surface_hist_launch(et, dist, hist[1], counts[1:2], counts[3:4])
    # each value once, each edge byte written once and read twice, each distance word written and read once per direction
    timed_bytes("surface_hist", p.numel() * (p.element_size() + 4 + 2 * (1 + 1 + 1) + 2 * (4 + 4)), run)
    return hist, counts


# ---- validation preview ------------------------------------------------------------------------------------------------------------
def _preview_vol(fn, vol):
    device_batch(fn, vol, "the host statement is training.visualization.panel_numpy", what="volume", dtypes=FLOATS, rank=4,
                 layout="one sample's (C, Z, H, W)")
    if not vol.is_contiguous():      # never copied: a panel is drawn from the batch's own storage
        raise _l.RxError(f"{fn}: the sample must be contiguous (strides {vol.stride()} for shape {tuple(vol.shape)})")
    return vol


def _preview_launch(vol, frames, y0, x0, z_step, sigmoid, minmax):
    c, z, h, w = vol.shape
    check(load().rx_preview_panel(_ptr(vol), _code(vol.dtype), c, z, h, w, z_step, 1 if sigmoid else 0, _ptr(frames), frames.stride(0),
                                  frames.stride(1), y0, x0, _ptr(minmax), stream_ptr()), "rx_preview_panel")


def _preview_bytes(vol, z_step):
    c, z, h, w = vol.shape
    zk = -(-z // z_step)
    return zk * h * w * ((3 if c == 3 else 1) * vol.element_size() + 3)


def preview_panel(vol4, frames, y0, x0, z_step=1, sigmoid=False, minmax=None):
    """draws one sample's (C, Z, H, W) float32 / bfloat16 / float16 device volume into the uint8 device frames (Zf, Hf, Wf, 3) (rows and
    pixels packed: strides (*, *, 3, 1)): the panel of kept slice j = source slice j * z_step occupies rows y0 .. y0 + H and
    columns x0 .. x0 + W of frame j; nothing else is written.  Every slice of every drawn channel is scaled to its own range
    (training.visualization.panel_numpy is the statement; `sigmoid` draws 1 / (1 + exp(-v))).  `minmax`: an optional contiguous
    float32 (c_drawn, Zk, 2) device tensor that receives (lo, hi).  On the current stream, no synchronisation; returns `frames`."""
    vol = _preview_vol("preview_panel", vol4)
    c, z, h, w = vol.shape
    z_step, y0, x0 = int(z_step), int(y0), int(x0)
    if z_step < 1 or y0 < 0 or x0 < 0:
        raise _l.RxError(f"preview_panel: z_step must be >= 1 and y0, x0 >= 0 (got z_step={z_step} y0={y0} x0={x0})")
    zk = -(-z // z_step)
    if (not isinstance(frames, torch.Tensor) or frames.device != vol.device or frames.dtype != torch.uint8 or frames.dim() != 4
            or frames.shape[3] != 3 or frames.stride(3) != 1 or frames.stride(2) != 3):
        raise _l.RxError(f"preview_panel: `frames` must be a uint8 (Z, H, W, 3) tensor with packed pixels on {vol.device}")
    if frames.shape[0] < zk or frames.shape[1] < y0 + h or frames.shape[2] < x0 + w:
        raise _l.RxError(f"preview_panel: a {zk} x {h} x {w} panel at (y0={y0}, x0={x0}) does not fit frames of shape {tuple(frames.shape)}")
    if minmax is not None:
        result_tensor("preview_panel", "minmax", minmax, (3 if c == 3 else 1, zk, 2), torch.float32, vol.device)
    timed_bytes("preview_panel", _preview_bytes(vol, z_step), lambda: _preview_launch(vol, frames, y0, x0, z_step, sigmoid, minmax))
    return frames


def preview_frames(image, targets, preds, sample=0, every=1, sigmoid_tasks=(), out=None):
    """the frames of the validation preview of one sample of a batch: image (B, C, Z, H, W), targets / preds {task: (B, C, Z, H, W)}
    device tensors -> uint8 (Zk, 2H, (1 + T)W, 3) on the device, Zk = ceil(Z / every): the input panel and one target panel per task
    (sorted by name) above a blank tile and the prediction panels (training.visualization.frames_numpy is the statement).  One
    rx_preview_panel launch per panel on the current stream, no synchronisation.  The tensor is zeroed when it is created and the
    blank tile is never written, so `out` -- a tensor an earlier call of the same shapes returned -- is reused as it is."""
    names = sorted(targets)
    vols = [("image", image, False)] + [(f"targets['{n}']", targets[n], False) for n in names]
    for n in names:
        if n not in preds:
            raise _l.RxError(f"preview_frames: no prediction for task '{n}'")
        vols.append((f"preds['{n}']", preds[n], None))
    sample, every = int(sample), int(every)
    if every < 1:
        raise _l.RxError(f"preview_frames: every must be >= 1 (got {every})")
    samples = []
    for label, t, _ in vols:
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise _l.RxError(f"preview_frames: {label} must be a device tensor")
        if t.dim() != 5:
            raise _l.RxError(f"preview_frames: {label}: expected (B, C, Z, H, W), got {tuple(t.shape)} (2-D patches have no slices to page through)")
        if not 0 <= sample < t.shape[0]:
            raise _l.RxError(f"preview_frames: sample {sample} of a batch of {t.shape[0]}")
        samples.append(_preview_vol("preview_frames", t[sample]))
    z, h, w = samples[0].shape[1:]
    for (label, _, _), s in zip(vols, samples):
        if tuple(s.shape[1:]) != (z, h, w) or s.device != samples[0].device:
            raise _l.RxError(f"preview_frames: {label} is {tuple(s.shape[1:])} on {s.device}, the image {(z, h, w)} on {samples[0].device}")
    t_n = len(names)
    out = result_tensor("preview_frames", "out", out, (-(-z // every), 2 * h, (1 + t_n) * w, 3), torch.uint8, samples[0].device, torch.zeros)

    def run():
        for i, s in enumerate(samples):
            row, col = divmod(i, 1 + t_n) if i <= t_n else (1, i - t_n)
            sig = i > t_n and names[i - t_n - 1] in sigmoid_tasks and s.shape[0] == 1
            _preview_launch(s, out, row * h, col * w, every, sig, None)
    timed_bytes("preview_frames", sum(_preview_bytes(s, every) for s in samples), run)
    return out
