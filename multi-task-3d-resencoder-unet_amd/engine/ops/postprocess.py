"""Post-processing on the device: connected components of a thresholded uint8 volume, their sizes, and the size filter
(csrc/rx_components.hip; postprocess/components.py holds the numpy statements and the out-of-core driver)."""
import torch

from .. import lib as _l
from ..lib import check, load, stream_ptr
from .core import _ptr, device_batch, result_tensor, timed_bytes

_CONNECTIVITY = (6, 18, 26)


def _volumes(fn, t, what, dtypes, statement):
    """a device (N, C, Z, Y, X) batch of `dtypes`, every volume within the library's limit -> it made contiguous"""
    t = device_batch(fn, t, f"the host statement is postprocess.{statement}", what=what, dtypes=dtypes, rank=5, layout="(N, C, Z, Y, X)")
    z, y, x = t.shape[2:]
    if z * y * x > _l.RX_CC_MAX_VOXELS:
        raise _l.RxError(f"{fn}: {z * y * x} voxels in a volume of {tuple(t.shape)} (at most 2^31 - 2: a label is an index + 1 in int32)")
    return t


def _like(fn, name, t, ref, dtype):
    """`t`: a contiguous `dtype` device tensor of `ref`'s shape on its device"""
    if (not isinstance(t, torch.Tensor) or t.device != ref.device or t.dtype != dtype or tuple(t.shape) != tuple(ref.shape)
            or not t.is_contiguous()):
        raise _l.RxError(f"{fn}: `{name}` must be a contiguous {str(dtype).replace('torch.', '')} tensor of shape {tuple(ref.shape)} on {ref.device}")
    return t


def cc_label(values, level=0, connectivity=26, out=None):
    """the connected components of `values > level` per (sample, channel) volume of a uint8 or bool (N, C, Z, Y, X) device batch (bool:
    level 0) -> int32 (N, C, Z, Y, X): 0 on background, else 1 + the smallest linear index z*Y*X + y*X + x of the voxel's component
    under `connectivity` 6, 18 or 26 (postprocess.label_numpy is the statement).  The labels depend on the mask alone, not on the
    order anything ran in.  Up to five launches on the current stream, no synchronisation, no workspace."""
    v = _volumes("cc_label", values, "values", (torch.uint8, torch.bool), "label_numpy")
    if isinstance(connectivity, bool) or connectivity not in _CONNECTIVITY:
        raise _l.RxError(f"cc_label: connectivity {connectivity!r} (6, 18 or 26)")
    level = 0 if v.dtype == torch.bool else level
    if isinstance(level, bool) or not isinstance(level, int) or not 0 <= level <= 254:
        raise _l.RxError(f"cc_label: level {level!r} (an integer 0 .. 254: the mask is value > level)")
    out = result_tensor("cc_label", "out", out, v.shape, torch.int32, v.device)
    n, c, z, y, x = v.shape
    # the byte once, the label word written once; the seam and root passes are extra time, not bytes
    timed_bytes("cc_label", v.numel() * (1 + 4),
                lambda: check(load().rx_cc_label(_ptr(v), level, n * c, z, y, x, connectivity, _ptr(out), stream_ptr()), "rx_cc_label"))
    return out


def cc_sizes(labels, out=None):
    """the component sizes of an int32 (N, C, Z, Y, X) device batch of `cc_label` labels -> int32 (N, C, Z*Y*X): per volume, at index
    label - 1 (the component's root) its voxel count, 0 everywhere else (postprocess.component_sizes_numpy is the statement).
    Zeroes `out` itself.  On the current stream, no synchronisation."""
    lab = _volumes("cc_sizes", labels, "labels", (torch.int32,), "component_sizes_numpy")
    n, c = lab.shape[:2]
    voxels = lab.numel() // (n * c)
    out = result_tensor("cc_sizes", "out", out, (n, c, voxels), torch.int32, lab.device)
    timed_bytes("cc_sizes", lab.numel() * (4 + 4),
                lambda: check(load().rx_cc_sizes(_ptr(lab), n * c, voxels, _ptr(out), stream_ptr()), "rx_cc_sizes"))
    return out


def cc_filter(values, labels, sizes, min_voxels, out=None):
    """`values` where the voxel's component has at least `min_voxels` voxels, else 0: uint8 or bool (N, C, Z, Y, X) device values, their
    int32 labels and the int32 (N, C, Z*Y*X) table `cc_sizes` returned -> a tensor of `values`' type (postprocess.filter_numpy is the
    statement).  The kernel compares whatever `sizes` holds at label - 1.  `out` may be `values` itself.  On the current stream, no
    synchronisation."""
    v = _volumes("cc_filter", values, "values", (torch.uint8, torch.bool), "filter_numpy")
    lab = _like("cc_filter", "labels", labels, v, torch.int32)
    n, c = v.shape[:2]
    voxels = v.numel() // (n * c)
    if (not isinstance(sizes, torch.Tensor) or sizes.device != v.device or sizes.dtype != torch.int32 or tuple(sizes.shape) != (n, c, voxels)
            or not sizes.is_contiguous()):
        raise _l.RxError(f"cc_filter: `sizes` must be a contiguous int32 tensor of shape {(n, c, voxels)} on {v.device}")
    if isinstance(min_voxels, bool) or not isinstance(min_voxels, int) or not 1 <= min_voxels <= 2**31 - 1:
        raise _l.RxError(f"cc_filter: min_voxels {min_voxels!r} (an integer 1 .. 2^31 - 1)")
    out = result_tensor("cc_filter", "out", out, v.shape, v.dtype, v.device)
    timed_bytes("cc_filter", v.numel() * (1 + 4 + 1),
                lambda: check(load().rx_cc_filter(_ptr(v), _ptr(lab), _ptr(sizes), min_voxels, n * c, voxels, _ptr(out), stream_ptr()),
                              "rx_cc_filter"))
    return out
