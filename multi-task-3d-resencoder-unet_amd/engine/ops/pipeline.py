"""The training input pipeline on the device: the intensity augmentation passes, flips / 90-degree rotations, affine and elastic
resampling, label dilation, box statistics for the patch search, and ingest of raw patches.  The dataloading modules draw the
parameters, pack the tables and hold the numpy statements; the integer codes they share with these wrappers live in core."""
from ctypes import byref, c_void_p

import numpy as np
import torch

from .. import lib as _l
from ..lib import I3, check, load, stream_ptr
from .core import BORDER, INTERP, RULES, SW_DTYPE, _ptr, device_batch, result_tensor, rule_code, timed_bytes


# ---- intensity augmentation (dataloading/augment_device.py draws the parameters and packs the table) ------------------------------
def aug_pointwise(image, out, scratch, host_table, table, pool_words):
    """pass 1 on a contiguous fp32 (B, C, Z, Y, X) batch; `host_table`: the pinned / host uint8 tensor holding the same bytes as the
    device tensor `table`; `scratch` None when no sample has a group-3 member"""
    b, c, z, y, x = image.shape
    check(load().rx_aug_pointwise(_ptr(image), _ptr(out), _ptr(scratch) if scratch is not None else None,
                                  scratch.numel() * scratch.element_size() if scratch is not None else 0, b, c, z, y, x,
                                  c_void_p(host_table.data_ptr()), _ptr(table), pool_words, stream_ptr()), "rx_aug_pointwise")


def aug_filter_zy(scratch, out, host_table, table, pool_words):
    """pass 2: the k x k (Z, Y) correlation or the downscale gather, then the dropout boxes, scratch -> out"""
    b, c, z, y, x = out.shape
    check(load().rx_aug_filter_zy(_ptr(scratch), _ptr(out), b, c, z, y, x, c_void_p(host_table.data_ptr()), _ptr(table), pool_words,
                                  stream_ptr()), "rx_aug_filter_zy")


def augment_batch(image, host_table, table, pool_words, any_group3):
    """both passes -> a new batch (allocated on the current stream)"""
    if not image.is_cuda:
        raise _l.RxError("augment_batch: the image batch must be a device tensor")
    out = torch.empty_like(image)
    scratch = None
    if any_group3:
        b, c, z, y, x = image.shape
        assert load().rx_aug_workspace(b, c, z, y, x) == image.numel() * 4
        scratch = torch.empty_like(image)
    aug_pointwise(image, out, scratch, host_table, table, pool_words)
    if any_group3:
        aug_filter_zy(scratch, out, host_table, table, pool_words)
    return out


def aug_philox_u32(key, n, device):
    """test hook: the raw Philox4x32-10 outputs behind the noise of voxels 0..n-1 -> int64 tensor of the uint32 values"""
    out = torch.empty(n, dtype=torch.int32, device=device)
    check(load().rx_aug_philox_u32(int(key), n, _ptr(out), stream_ptr()), "rx_aug_philox_u32")
    return out.to(torch.int64) & 0xFFFFFFFF


# ---- flips and 90-degree rotations -------------------------------------------------------------------------------------------------
def geom_table(geom_ops):
    """`geom_ops`: one record per sample -- objects with `.row()` (dataloading.geometry_device.GeomOp) or 12 integers
    (src_axis, flip, ch_src, ch_neg) -> the (B, 12) int32 host image of `rx_geom_sample`"""
    rows = [o.row() if hasattr(o, "row") else o for o in geom_ops]
    return np.ascontiguousarray(np.asarray(rows, dtype=np.int32).reshape(len(rows), 12))


def geom_apply(tensor, geom_ops, vector):
    """flips / 90-degree rotations of a float32 (B, C, Z, Y, X) device batch, one record of `geom_ops` per sample -> a new batch
    (allocated on the current stream).  `vector`: the three channels are a vector field and follow the records' component rule."""
    tensor = device_batch("geom_apply", tensor, "the host classes are training/transforms/geometric")
    table = geom_table(geom_ops)
    b, c, z, y, x = tensor.shape
    if table.shape[0] != b:
        raise _l.RxError(f"geom_apply: {table.shape[0]} records for a batch of {b}")
    out = torch.empty_like(tensor)
    check(load().rx_geom_apply(_ptr(tensor), _ptr(out), b, c, z, y, x, table.ctypes.data, 1 if vector else 0, stream_ptr()),
          "rx_geom_apply")
    return out


# ---- rotation / scaling and B-spline deformation -----------------------------------------------------------------------------------
def _modes(fn, interp, border):
    if interp not in INTERP or border not in BORDER:
        raise _l.RxError(f"{fn}: interp {interp!r} (linear, nearest), border {border!r} (constant, clamp)")
    return INTERP[interp], BORDER[border]


def affine_table(affine_ops):
    """`affine_ops`: one record per sample -- objects with `.row()` (dataloading.spatial_device.AffineOp) or 18 numbers (point,
    then vector, row-major), or a (B, 18) array -> the (B, 18) float32 host image of `rx_affine_sample`"""
    if isinstance(affine_ops, np.ndarray):
        rows = affine_ops
    else:
        rows = [o.row() if hasattr(o, "row") else o for o in affine_ops]
    return np.ascontiguousarray(np.asarray(rows, dtype=np.float32).reshape(len(rows), 18))


def affine_apply(tensor, table, interp, border, fill=0.0, vector=False, out=None):
    """rotation / scaling of a float32 (B, C, Z, Y, X) device batch, one record of `table` (`affine_table`, or what it takes) per
    sample -> a new batch on the current stream, or `out` (a distinct contiguous float32 tensor of the same shape).  `interp`:
    "linear" | "nearest"; `border`: "constant" (outside voxels are `fill`) | "clamp"; `vector`: the three channels are a vector
    field and are turned by the records' `vector` matrices.  dataloading.spatial_device.affine_numpy is the statement."""
    src = device_batch("affine_apply", tensor, "the host path is spatial_device.affine_numpy")
    interp, border = _modes("affine_apply", interp, border)
    table = affine_table(table)
    b, c, z, y, x = src.shape
    if table.shape[0] != b:
        raise _l.RxError(f"affine_apply: {table.shape[0]} records for a batch of {b}")
    out = result_tensor("affine_apply", "out", out, src.shape, torch.float32, src.device)
    check(load().rx_affine_apply(_ptr(src), _ptr(out), b, c, z, y, x, table.ctypes.data, interp, border, float(fill),
                                 1 if vector else 0, stream_ptr()), "rx_affine_apply")
    return out


_ELASTIC_TABLES = {}


def elastic_tables(shape, spacing, device=None):
    """the per-axis B-spline tables of a (Z, Y, X) patch at `spacing` = (sz, sy, sx) (dataloading.elastic_device.bspline_tables) on
    the device: ((idx_z, w_z, dw_z), (idx_y, ...), (idx_x, ...)), int32 [n] and float32 [n, 4] tensors.  Cached per (shape, spacing,
    device): a trainer uploads them once."""
    from ...dataloading.elastic_device import bspline_tables      # computation, not a code: the one import from the data pipeline
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    if device.type != "cuda":
        raise _l.RxError(f"elastic_tables: {device} is not a device (the host path is elastic_device.elastic_numpy)")
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    shape, spacing = tuple(int(v) for v in shape), tuple(int(v) for v in spacing)
    if len(shape) != 3 or len(spacing) != 3 or min(shape) < 1 or min(spacing) < 1:
        raise _l.RxError(f"elastic_tables: shape {shape}, spacing {spacing} (three positive extents, three positive spacings)")
    key = (shape, spacing, device)
    if key not in _ELASTIC_TABLES:
        _ELASTIC_TABLES[key] = tuple(tuple(torch.from_numpy(t).to(device) for t in bspline_tables(n, s)) for n, s in zip(shape, spacing))
    return _ELASTIC_TABLES[key]


def elastic_nodes(fields, device=None):
    """`fields`: one `dataloading.elastic_device.ElasticField` per sample, all with one spacing and one lattice -> the
    (B, 3, Gz, Gy, Gx) float32 device tensor of their nodes: staged in pinned host memory and uploaded with ONE non-blocking copy
    on the current stream, no synchronisation.  Nodes that are not finite are refused here (the device cannot refuse them)."""
    fields = list(fields)
    if not fields or any(not hasattr(f, "nodes") or not hasattr(f, "spacing") for f in fields):
        raise _l.RxError("elastic_nodes: expected a non-empty list of ElasticField")
    sp, shp = tuple(fields[0].spacing), tuple(fields[0].nodes.shape)
    for i, f in enumerate(fields):
        if tuple(f.spacing) != sp or tuple(f.nodes.shape) != shp:
            raise _l.RxError(f"elastic_nodes: field {i} has spacing {tuple(f.spacing)} and nodes {tuple(f.nodes.shape)}, field 0 has "
                             f"{sp} and {shp}: one batch, one lattice")
        if not np.isfinite(f.nodes).all():
            raise _l.RxError(f"elastic_nodes: field {i} has nodes that are not finite")
    host = torch.empty((len(fields),) + shp, dtype=torch.float32, pin_memory=True)
    stage = host.numpy()
    for i, f in enumerate(fields):
        stage[i] = f.nodes
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else device
    return host.to(device, non_blocking=True)


def elastic_apply(tensor, nodes, tables, spacing, interp, border, fill=0.0, vector=False, out=None):
    """B-spline deformation of a float32 (B, C, Z, Y, X) device batch: `nodes` (`elastic_nodes`) the (B, 3, Gz, Gy, Gx) float32
    device lattice, `tables` (`elastic_tables`) for (Z, Y, X) at `spacing` = (sz, sy, sx), each >= 8 -> a new batch on the current
    stream, or `out` (a distinct contiguous float32 tensor of the same shape).  `interp`: "linear" | "nearest"; `border`: "constant"
    (outside voxels are `fill`) | "clamp"; `vector`: the three channels are a normal field (Nx, Ny, Nz) and take the covector
    rule.  dataloading.elastic_device.elastic_numpy is the statement.  The fold guard is the config parser's: nodes of any finite
    size are served, and no load leaves a sample."""
    src = device_batch("elastic_apply", tensor, "the host path is elastic_device.elastic_numpy")
    interp, border = _modes("elastic_apply", interp, border)
    b, c, z, y, x = src.shape
    try:
        sp = tuple(int(v) for v in spacing)
    except (TypeError, ValueError):
        sp = ()
    if len(sp) != 3 or min(sp) < 1:
        raise _l.RxError(f"elastic_apply: spacing {spacing!r} (three positive ints)")
    want = (b, 3) + tuple((n - 1) // s + 4 for n, s in zip((z, y, x), sp))
    if (not isinstance(nodes, torch.Tensor) or nodes.device != src.device or nodes.dtype != torch.float32 or tuple(nodes.shape) != want
            or not nodes.is_contiguous()):
        got = (nodes.dtype, tuple(nodes.shape), nodes.device) if isinstance(nodes, torch.Tensor) else type(nodes)
        raise _l.RxError(f"elastic_apply: `nodes` must be a contiguous float32 tensor of shape {want} on {src.device}, got {got}")
    ok = isinstance(tables, (tuple, list)) and len(tables) == 3
    for n, ax in zip((z, y, x), tables if ok else ()):
        ok = ok and isinstance(ax, (tuple, list)) and len(ax) == 3 and all(isinstance(t, torch.Tensor) and t.device == src.device
                                                                            and t.is_contiguous() for t in ax)
        ok = ok and ax[0].dtype == torch.int32 and tuple(ax[0].shape) == (n,) and all(t.dtype == torch.float32 and tuple(t.shape) == (n, 4)
                                                                                      for t in ax[1:])
    if not ok:
        raise _l.RxError(f"elastic_apply: `tables` must be elastic_tables(({z}, {y}, {x}), spacing) on {src.device}")
    out = result_tensor("elastic_apply", "out", out, src.shape, torch.float32, src.device)
    rec = _l.RxElasticTables(*[t.data_ptr() for ax in tables for t in ax])
    timed_bytes("elastic_apply", 2 * src.numel() * 4,
                lambda: check(load().rx_elastic_apply(_ptr(src), _ptr(out), b, c, z, y, x, _ptr(nodes), I3(*sp), byref(rec), interp,
                                                      border, float(fill), 1 if vector else 0, stream_ptr()), "rx_elastic_apply"))
    return out


# ---- label dilation ----------------------------------------------------------------------------------------------------------------
def label_dilate(tensor, radius=5, out=None):
    """binary dilation with the ball of `radius` (1..8) of a float32 (B, C, Z, Y, X) device batch, every (sample, channel) volume
    on its own: 1.0 where a voxel > 0 lies within the radius, else 0.0 (dataloading.dilate_device.dilate_numpy is the statement).
    `out=None`: in place, returns `tensor`; the bit scratch comes from the caching allocator on the current stream."""
    src = device_batch("label_dilate", tensor, "the host path is scipy's binary_dilation in the dataset")
    out = src if out is None else result_tensor("label_dilate", "out", out, src.shape, torch.float32, src.device)
    b, c, z, y, x = src.shape
    nbytes = load().rx_dilate_workspace(b, c, z, y, x)
    scratch = torch.empty(max(nbytes // 8, 1), dtype=torch.int64, device=src.device)
    check(load().rx_label_dilate(_ptr(src), _ptr(out), _ptr(scratch), nbytes, b, c, z, y, x, int(radius), stream_ptr()),
          "rx_label_dilate")
    if out is src and src is not tensor:      # a non-contiguous batch dilated "in place": hand the values back to its own storage
        tensor.copy_(src)
        return tensor
    return out


# ---- box statistics (the patch search) and ingest of raw patches ------------------------------------------------------------------
def box_stats(vol, boxes):
    """per box (z0, y0, x0, dz, dy, dx) of a contiguous (Z, Y, X) device tensor -- uint8, float32, or uint16 (int16 is read as the
    uint16 bits it holds) -- the count of voxels != 0 and the box-local (minz, maxz, miny, maxy, minx, maxx) of the voxels > 0,
    (dz, -1, dy, -1, dx, -1) where there is none (dataloading.patch_search_device.box_stats_numpy is the statement).  Returns
    (count np.uint64 [N], ext np.int32 [N, 6]) after synchronising the current stream."""
    if not isinstance(vol, torch.Tensor) or not vol.is_cuda:
        raise _l.RxError("box_stats: the volume must be a device tensor (the host statement is patch_search_device.box_stats_numpy)")
    if vol.dtype not in SW_DTYPE:      # every raw voxel type
        raise _l.RxError(f"box_stats: dtype {vol.dtype} (uint8, uint16 / int16 or float32)")
    if vol.dim() != 3 or not vol.is_contiguous():
        raise _l.RxError(f"box_stats: expected a contiguous (Z, Y, X) tensor, got {tuple(vol.shape)} with strides {tuple(vol.stride())}")
    if max(vol.shape) >= (1 << 31):
        raise _l.RxError(f"box_stats: an extent of {tuple(vol.shape)} is beyond int32 (only z * y * x may exceed 2^31)")
    table = np.asarray(boxes)
    if table.ndim != 2 or table.shape[1] != 6 or table.shape[0] < 1 or table.dtype.kind not in "iu":
        raise _l.RxError(f"box_stats: boxes must be an (N, 6) integer array with N >= 1, got {table.dtype} {table.shape}")
    if table.min() < -(1 << 31) or table.max() >= (1 << 31):
        raise _l.RxError("box_stats: a box entry is beyond int32")
    table = np.ascontiguousarray(table, dtype=np.int32)      # read by the copy engine until the synchronise below
    n = len(table)
    z, y, x = vol.shape
    with torch.cuda.device(vol.device):
        nbytes = load().rx_box_stats_workspace(n)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=vol.device)
        count = torch.empty(n, dtype=torch.int64, device=vol.device)
        ext = torch.empty((n, 6), dtype=torch.int32, device=vol.device)
        check(load().rx_box_stats(_ptr(vol), SW_DTYPE[vol.dtype], z, y, x, table.ctypes.data, n, _ptr(ws), nbytes, _ptr(count), _ptr(ext),
                                  stream_ptr()), "rx_box_stats")
        torch.cuda.current_stream().synchronize()
        return count.cpu().numpy().view(np.uint64), ext.cpu().numpy()


def ingest(tensor, rule, out=None):
    """raw patches -> the float32 channel-first batch: a uint8, uint16 or float32 device tensor, (B, Z, Y, X) or channels-last
    (B, Z, Y, X, C) with C <= 8, scaled by `rule` (a name of `RULES` or its code; dataloading.ingest_device.ingest_numpy is the
    statement) into a new (B, C, Z, Y, X) float32 tensor on the current stream (C = 1 for a 4-D input), or into `out`.  A
    non-contiguous input is made contiguous first."""
    if not isinstance(tensor, torch.Tensor) or not tensor.is_cuda:
        raise _l.RxError("ingest: the batch must be a device tensor (the host statement is ingest_device.ingest_numpy)")
    if tensor.dtype not in SW_DTYPE or tensor.dtype == torch.int16:      # a store's own types: no uint16 bits in int16 storage here
        raise _l.RxError(f"ingest: dtype {tensor.dtype} (uint8, uint16 or float32)")
    if tensor.dim() not in (4, 5):
        raise _l.RxError(f"ingest: expected (B, Z, Y, X) or channels-last (B, Z, Y, X, C), got {tuple(tensor.shape)}")
    try:
        code = rule_code(rule)
    except ValueError as e:
        raise _l.RxError(str(e)) from None
    src = tensor.contiguous()
    b, z, y, x = src.shape[:4]
    c = src.shape[4] if src.dim() == 5 else 1
    out = result_tensor("ingest", "out", out, (b, c, z, y, x), torch.float32, src.device)
    check(load().rx_ingest(_ptr(src), SW_DTYPE[src.dtype], _ptr(out), b, z, y, x, c, code, stream_ptr()), f"rx_ingest ({RULES[code]})")
    return out
