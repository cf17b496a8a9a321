"""Streaming sliding-window inference (csrc/rx_infer.hip; inference.StreamingInferer is the caller).

A slab is a contiguous (C, ring, Y, X) device tensor whose ring row r holds the volume row z with z % ring == r.  `origins` is a
Python list of (z, y, x) patch origins, z an absolute volume row; `views` a list of `GeomOp.row()` records, one per origin.  The
tables go to the kernels by value: nothing here allocates, copies to the device or synchronises, except `sw_occupancy`'s read."""
from ctypes import c_int32

import numpy as np
import torch

from .. import lib as _l
from ..lib import check, load, stream_ptr
from .core import SW_DTYPE, _ptr

SW_NORM = {"scale": _l.RX_SW_SCALE, "zscore": _l.RX_SW_ZSCORE}
SW_BLEND = {"average": _l.RX_SW_BLEND_AVERAGE, "unit": _l.RX_SW_BLEND_UNIT, "none": _l.RX_SW_BLEND_NONE}
SW_CAST = {"u8": _l.RX_SW_CAST_U8, "u16": _l.RX_SW_CAST_U16}
SW_ACT = {"none": _l.RX_ACT_NONE, "sigmoid": _l.RX_ACT_SIGMOID, "softmax": _l.RX_ACT_SOFTMAX}
_SW_IN = (torch.uint8, torch.int16, torch.float32)      # what an input slab may hold; int16: the uint16 bits


def _sw_table(fn, rows, n, width):
    flat = [v for r in rows for v in r]
    if len(flat) != n * width:
        raise _l.RxError(f"{fn}: expected {n} records of {width} integers, got {len(flat)} integers")
    return (c_int32 * len(flat))(*flat)


def _sw_slab(fn, slab, dtypes=_SW_IN):
    if not isinstance(slab, torch.Tensor) or not slab.is_cuda or slab.dim() != 4 or not slab.is_contiguous() or slab.dtype not in dtypes:
        raise _l.RxError(f"{fn}: a slab is a contiguous (C, ring, Y, X) device tensor of {[str(d) for d in dtypes]}")
    return slab.shape


def sw_gather_workspace(batch, cin, patch):
    """bytes of fp64 scratch that `sw_gather(norm="zscore")` needs for (batch, cin, *patch) patches"""
    return load().rx_sw_gather_workspace(int(batch), int(cin), *(int(p) for p in patch))


def sw_gather(slab, origins, out, norm, workspace, views=None):
    """the patches at `origins` of an input slab (uint8, int16 holding uint16 bits, float32) -> `out` (B, cin, pz, py, px)
    float32, scaled to [0, 1] (`norm` "scale") and then standardised per patch ("zscore"; `workspace`: a float64 tensor of
    `sw_gather_workspace` bytes).  `views` None: rx_sw_gather; a list of B rows: patch b as its view sees it (rx_sw_gather_geom)."""
    fn = "rx_sw_gather" if views is None else "rx_sw_gather_geom"
    cin, ring, y, x = _sw_slab(fn, slab)
    b, pz, py, px = len(origins), out.shape[2], out.shape[3], out.shape[4]
    if out.dtype != torch.float32 or tuple(out.shape[:2]) != (b, cin) or not out.is_contiguous():
        raise _l.RxError(f"{fn}: `out` must be a contiguous float32 ({b}, {cin}, pz, py, px) tensor, got {out.dtype} {tuple(out.shape)}")
    ws_bytes = workspace.numel() * workspace.element_size() if norm == "zscore" else 0
    head = (SW_DTYPE[slab.dtype], _ptr(slab), cin, ring, y, x, b, _sw_table(fn, origins, b, 3))
    tail = (pz, py, px, SW_NORM[norm], _ptr(out), _ptr(workspace), ws_bytes, stream_ptr())
    if views is None:
        check(load().rx_sw_gather(*head, *tail), fn)
    else:
        check(load().rx_sw_gather_geom(*head, _sw_table(fn, views, b, 12), *tail), fn)


def sw_accumulate(logits, valid, origins, act, weights, acc, wsum=None, views=None, vector=False):
    """one task's logits (B, c, pz, py, px) float32 -> activation `act` (an RX_ACT code) -> for the first `valid` patches, in
    order: acc (c, ring, Y, X) += weights * p and, where `wsum` (ring, Y, X) is given, wsum += weights.  `views` None:
    rx_sw_accumulate; a list of B rows: each prediction is first moved by its row -- the inverse of the view it was gathered
    with -- and a `vector` task follows the component and sign rule (rx_sw_accumulate_geom)."""
    fn = "rx_sw_accumulate" if views is None else "rx_sw_accumulate_geom"
    c, ring, y, x = _sw_slab(fn, acc, (torch.float32,))
    b, (pz, py, px) = len(origins), weights.shape
    if logits.dtype != torch.float32 or logits.numel() != b * c * pz * py * px or not logits.is_contiguous():
        raise _l.RxError(f"{fn}: expected contiguous float32 logits of ({b}, {c}, {pz}, {py}, {px}), "
                         f"got {logits.dtype} {tuple(logits.shape)}")
    org = _sw_table(fn, origins, b, 3)
    tail = (_ptr(weights), _ptr(acc), _ptr(wsum) if wsum is not None else None, ring, y, x, stream_ptr())
    if views is None:
        check(load().rx_sw_accumulate(_ptr(logits), b, int(valid), c, pz, py, px, org, int(act), *tail), fn)
    else:
        check(load().rx_sw_accumulate_geom(_ptr(logits), b, int(valid), c, pz, py, px, org, _sw_table(fn, views, b, 12),
                                           1 if vector else 0, int(act), *tail), fn)


def sw_finalize(acc, wsum, z0, rows, blend, cast, blended, final, wsum_out=None, reset_wsum=False):
    """volume rows [z0, z0 + rows) of the ring accumulators -> `blended` (c, rows, Y, X) float32 by the rule `blend` ("average",
    "unit", "none") and `final`, its integer cast ("u8" into uint8, "u16" into int16 storage); `wsum_out`: the weight sum of those
    rows.  The rows of `acc` are zeroed after reading, and with `reset_wsum` (the last task that shares `wsum`) those of `wsum`."""
    c, ring, y, x = _sw_slab("rx_sw_finalize", acc, (torch.float32,))
    check(load().rx_sw_finalize(_ptr(acc), _ptr(wsum), c, ring, y, x, int(z0), int(rows), SW_BLEND[blend], SW_CAST[cast],
                                2 if reset_wsum else 1, _ptr(blended), _ptr(final), _ptr(wsum_out) if wsum_out is not None else None,
                                stream_ptr()), "rx_sw_finalize")


def sw_occupancy(slab, origins, patch, value, counts):
    """per origin, the raw voxels of its patch (all channels) with float32(v) > `value`, counted into the device int64 tensor
    `counts` (at least one element per origin); returns them as np.uint64 [N] -- the one read-back of this family."""
    cin, ring, y, x = _sw_slab("rx_sw_occupancy", slab)
    n = len(origins)
    if counts.dtype != torch.int64 or counts.numel() < n or not counts.is_cuda:
        raise _l.RxError(f"rx_sw_occupancy: `counts` must be a device int64 tensor of at least {n} elements")
    pz, py, px = (int(p) for p in patch)
    check(load().rx_sw_occupancy(SW_DTYPE[slab.dtype], _ptr(slab), cin, ring, y, x, n, _sw_table("rx_sw_occupancy", origins, n, 3),
                                 pz, py, px, float(value), _ptr(counts), stream_ptr()), "rx_sw_occupancy")
    return counts[:n].cpu().numpy().view(np.uint64)
