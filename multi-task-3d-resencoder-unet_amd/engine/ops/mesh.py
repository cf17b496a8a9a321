"""Mesh targets (csrc/rx_meshslice.hip; the numpy statements live in tasks/normals/mesh_targets.py)."""
import torch

from .. import lib as _l
from ..lib import check, load, stream_ptr
from .core import _U16, _ptr, result_tensor

_MESH_MAX_COORD = float(1 << 24)


def _mesh_check(who, vertices, triangles, normals, w, h, z0, nz, window):
    """the refusals the library cannot make (it never reads device data on the host) -> (y0, x0, wh, ww)"""
    _l.require_device()
    if not isinstance(vertices, torch.Tensor) or not isinstance(triangles, torch.Tensor):
        raise _l.RxError(f"{who}: `vertices` and `triangles` must be device tensors")
    dev = vertices.device
    for name, t, dt in (("vertices", vertices, torch.float32), ("triangles", triangles, torch.int32), ("normals", normals, torch.float32)):
        if t is None:
            continue
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.device != dev or t.dtype != dt or t.dim() != 2 or t.shape[1] != 3 \
                or not t.is_contiguous():
            raise _l.RxError(f"{who}: `{name}` must be a contiguous {dt} (n, 3) device tensor")
    if vertices.shape[0] < 1:
        raise _l.RxError(f"{who}: no vertices")
    if normals is not None and normals.shape != vertices.shape:
        raise _l.RxError(f"{who}: `normals` must match `vertices` {tuple(vertices.shape)}")
    if not bool(torch.isfinite(vertices).all()) or (normals is not None and not bool(torch.isfinite(normals).all())):
        raise _l.RxError(f"{who}: vertices and normals must be finite")
    if float(vertices.abs().max()) >= _MESH_MAX_COORD:
        raise _l.RxError(f"{who}: coordinates at or beyond 2^24 are not supported on the device")
    if triangles.shape[0] and (int(triangles.min()) < 0 or int(triangles.max()) >= vertices.shape[0]):
        raise _l.RxError(f"{who}: triangle indices must lie in [0, {vertices.shape[0]})")
    y0, x0, wh, ww = (0, 0, h, w) if window is None else (int(a) for a in window)
    if w < 1 or h < 1 or nz < 1 or y0 < 0 or x0 < 0 or wh < 1 or ww < 1 or y0 + wh > h or x0 + ww > w:
        raise _l.RxError(f"{who}: window {(y0, x0, wh, ww)} / slab of {nz} slices does not fit the {w} x {h} image")
    return y0, x0, wh, ww


def _mesh_out(who, out, name, shape, dtype, device):
    """out[name] or a new tensor; the uint16 results may sit in any 2-byte storage (int16 where torch has no uint16)"""
    return result_tensor(who, f"out[{name!r}]", None if out is None else out.get(name), shape, dtype, device, same_width=True)


def mesh_slice_normals(vertices, triangles, normals, w, h, z0, nz, window=None, exp_factor=1.5, want_viz=False, want_mask=False,
                       keys=None, out=None):
    """slices [z0, z0 + nz) of the meshes' interpolated vertex normals, window (y0, x0, wh, ww) of the w x h image ->
    {"normals": uint16 (nz, wh, ww, 3), "keys": int64 (nz, wh, ww) order keys[, "viz": uint8 (nz, wh, ww, 3)][, "mask": uint8
    (nz, wh, ww)]}, equal to tasks/normals/mesh_targets.py: slice_normals_numpy slice by slice.  `keys`: a reusable int64 buffer of
    that shape (cleared here); `out`: optional preallocated result tensors by name."""
    who = "mesh_slice_normals"
    y0, x0, wh, ww = _mesh_check(who, vertices, triangles, normals, w, h, z0, nz, window)
    if normals is None:
        raise _l.RxError(f"{who}: `normals` is required")
    dev = vertices.device
    keys = _mesh_out(who, {"keys": keys}, "keys", (nz, wh, ww), torch.int64, dev)
    keys.zero_()
    res = {"keys": keys, "normals": _mesh_out(who, out, "normals", (nz, wh, ww, 3), _U16, dev)}
    if want_viz:
        res["viz"] = _mesh_out(who, out, "viz", (nz, wh, ww, 3), torch.uint8, dev)
    if want_mask:
        res["mask"] = _mesh_out(who, out, "mask", (nz, wh, ww), torch.uint8, dev)
    lib, st = load(), stream_ptr()
    geom = (int(w), int(h), int(z0), int(nz), y0, x0, wh, ww)
    check(lib.rx_mesh_slice_keys(0, _ptr(vertices), vertices.shape[0], _ptr(triangles), triangles.shape[0], _ptr(normals), *geom,
                                 float(exp_factor), _ptr(keys), st), "rx_mesh_slice_keys")
    check(lib.rx_mesh_resolve_normals(_ptr(keys), _ptr(vertices), vertices.shape[0], _ptr(triangles), triangles.shape[0], _ptr(normals), *geom,
                                      _ptr(res["normals"]), _ptr(res.get("viz")), _ptr(res.get("mask")), st), "rx_mesh_resolve_normals")
    return res


def mesh_slice_labels(vertices, triangles, tri_labels, w, h, z0, nz, window=None, want_mask=False, keys=None, out=None):
    """slices [z0, z0 + nz) of per-triangle labels (`tri_labels`: int32 device tensor, values in [0, 65535]) ->
    {"labels": uint16 (nz, wh, ww), "keys": int32 (nz, wh, ww)[, "mask": uint8 (nz, wh, ww)]}, equal to
    tasks/normals/mesh_targets.py: slice_labels_numpy slice by slice"""
    who = "mesh_slice_labels"
    y0, x0, wh, ww = _mesh_check(who, vertices, triangles, None, w, h, z0, nz, window)
    dev = vertices.device
    if not isinstance(tri_labels, torch.Tensor) or tri_labels.device != dev or tri_labels.dtype != torch.int32 \
            or tuple(tri_labels.shape) != (triangles.shape[0],) or not tri_labels.is_contiguous():
        raise _l.RxError(f"{who}: `tri_labels` must be a contiguous int32 ({triangles.shape[0]},) device tensor")
    if tri_labels.numel() and (int(tri_labels.min()) < 0 or int(tri_labels.max()) > 65535):
        raise _l.RxError(f"{who}: labels must lie in [0, 65535]")
    keys = _mesh_out(who, {"keys": keys}, "keys", (nz, wh, ww), torch.int32, dev)
    keys.zero_()
    res = {"keys": keys, "labels": _mesh_out(who, out, "labels", (nz, wh, ww), _U16, dev)}
    if want_mask:
        res["mask"] = _mesh_out(who, out, "mask", (nz, wh, ww), torch.uint8, dev)
    lib, st = load(), stream_ptr()
    check(lib.rx_mesh_slice_keys(1, _ptr(vertices), vertices.shape[0], _ptr(triangles), triangles.shape[0], None, int(w), int(h), int(z0),
                                 int(nz), y0, x0, wh, ww, 0.0, _ptr(keys), st), "rx_mesh_slice_keys")
    check(lib.rx_mesh_resolve_labels(_ptr(keys), _ptr(tri_labels), triangles.shape[0], nz * wh * ww, _ptr(res["labels"]),
                                     _ptr(res.get("mask")), st), "rx_mesh_resolve_labels")
    return res
