"""Post-processing on the device: connected components of a thresholded uint8 volume, their sizes, and the size filter
(csrc/rx_components.hip; postprocess/components.py holds the numpy statements and the out-of-core driver), and the triangle mesh of
a uint8 volume by surface nets (csrc/rx_isosurface.hip; postprocess/isosurface.py).  What happens to that mesh afterwards is in
mesh.py."""
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


def _iso_volume(fn, values, level):
    """a device (Z, Y, X) uint8 volume within the library's limits -> it made contiguous"""
    v = device_batch(fn, values, "the host statement is postprocess.surface_nets_numpy", what="values", dtypes=(torch.uint8,), rank=3,
                     layout="(Z, Y, X)")
    if isinstance(level, bool) or not isinstance(level, int) or not 0 <= level <= 254:
        raise _l.RxError(f"{fn}: level {level!r} (an integer 0 .. 254: inside is value > level; postprocess.surface_nets_numpy)")
    z, y, x = v.shape
    if max(z, y, x) > _l.RX_ISO_MAX_EXTENT:
        raise _l.RxError(f"{fn}: an extent of 2^24 - 2 or more in {tuple(v.shape)}: a position must be an exact float32")
    if (z + 1) * (y + 1) * (x + 1) > _l.RX_ISO_MAX_CELLS:
        raise _l.RxError(f"{fn}: more than 2^31 - 2 cells in a volume of {tuple(v.shape)}")
    return v


def _iso_window(fn, window, z):
    """(k_lo, k_emit, k_hi): the cell planes that exist, from which on they are emitted, and where they end; None: the whole grid"""
    if window is None:
        return 0, 0, z + 1
    k_lo, k_emit, k_hi = (int(k) for k in window)
    if not 0 <= k_lo <= k_emit <= k_hi <= z + 1:
        raise _l.RxError(f"{fn}: window {tuple(window)} (0 <= k_lo <= k_emit <= k_hi <= {z + 1})")
    return k_lo, k_emit, k_hi


def _iso_scan(fn, v, level, k_lo, k_hi):
    """classify + scan -> bits, row_offsets (rows, 2) int64, totals (2,) int64, all on the device"""
    z, y, x = v.shape
    rows, words = (z + 1) * (y + 1), (x + 1 + 63) // 64
    bits = torch.empty((rows, words), dtype=torch.int64, device=v.device)
    counts = torch.empty((rows, 2), dtype=torch.int32, device=v.device)
    offsets = torch.empty((rows, 2), dtype=torch.int64, device=v.device)
    totals = torch.empty(2, dtype=torch.int64, device=v.device)
    timed_bytes("iso_classify", v.numel() + bits.numel() * 8 + counts.numel() * 4,
                lambda: check(load().rx_iso_classify(_ptr(v), level, z, y, x, k_lo, k_hi, _ptr(bits), _ptr(counts), stream_ptr()), "rx_iso_classify"))
    timed_bytes("iso_scan", counts.numel() * 4 + offsets.numel() * 8,
                lambda: check(load().rx_iso_scan(_ptr(counts), rows, _ptr(offsets), _ptr(totals), stream_ptr()), "rx_iso_scan"))
    return bits, offsets, totals


def iso_counts(values, level=127):
    """(number of vertices, number of triangles) of `iso_mesh(values, level)` for a (Z, Y, X) uint8 device volume
    (postprocess.counts_numpy is the statement): classify and scan, then one small device-to-host read."""
    v = _iso_volume("iso_counts", values, level)
    _, _, totals = _iso_scan("iso_counts", v, level, 0, v.shape[0] + 1)
    nv, nq = totals.tolist()
    return int(nv), 2 * int(nq)


def iso_mesh(values, level=127, vertex_base=0, out=None, window=None, z_base=0, return_last_plane=False):
    """the surface `values > level` of a (Z, Y, X) uint8 device volume by surface nets -> (vertices float32 (n, 3) as (x, y, z) in
    voxel coordinates, triangles int64 (m, 3)), bit for bit postprocess.surface_nets_numpy: one vertex per active cell in ascending
    linear cell index, two triangles per crossing lattice edge in (cell, axis) order, `vertex_base` added to every id.  `out`: a
    (vertices, triangles) pair of exactly those shapes to write into.  Classify, scan, one small device-to-host read (the counts size
    the outputs), emit; beyond the outputs 1/8 byte per cell and 24 bytes per cell row are allocated.

    For a slab of a larger volume: `window` = (k_lo, k_emit, k_hi) in the slab's own cell planes -- planes outside [k_lo, k_hi) do not
    exist (their voxels are not in the slab), planes [k_lo, k_emit) are only referenced -- and `z_base` is the slab's first voxel plane,
    added to z.  Ids count from the first vertex of plane k_lo.  `return_last_plane`: also return the number of vertices of plane
    k_hi - 1."""
    v = _iso_volume("iso_mesh", values, level)
    z, y, x = v.shape
    k_lo, k_emit, k_hi = _iso_window("iso_mesh", window, z)
    if isinstance(vertex_base, bool) or not isinstance(vertex_base, int) or not 0 <= vertex_base < 2**62:
        raise _l.RxError(f"iso_mesh: vertex_base {vertex_base!r} (a non-negative integer)")
    if isinstance(z_base, bool) or not isinstance(z_base, int) or not 0 <= z_base <= _l.RX_ISO_MAX_EXTENT - z:
        raise _l.RxError(f"iso_mesh: z_base {z_base!r}: plane z_base + {z} must stay below 2^24 - 2")
    bits, offsets, totals = _iso_scan("iso_mesh", v, level, k_lo, k_hi)
    # the one device-to-host read: the totals, the offsets of the first emitted row and those of plane k_hi - 1's first row
    marks = ([k_emit * (y + 1)] if k_emit <= z else []) + ([(k_hi - 1) * (y + 1)] if k_hi >= 1 else [])
    host = torch.cat([totals] + [offsets[m] for m in marks]).tolist()
    nv_all, nq_all = host[0], host[1]
    v_skip, q_skip = (host[2], host[3]) if k_emit <= z else (nv_all, nq_all)
    last_plane = nv_all - host[-2] if k_hi >= 1 else 0      # planes from k_hi on hold nothing
    nv, nq = nv_all - v_skip, nq_all - q_skip
    if out is None:
        out = (None, None)
    vertices = result_tensor("iso_mesh", "out[0]", out[0], (nv, 3), torch.float32, v.device)
    triangles = result_tensor("iso_mesh", "out[1]", out[1], (2 * nq, 3), torch.int64, v.device)
    if nv or nq:
        timed_bytes("iso_emit", v.numel() + bits.numel() * 8 + offsets.numel() * 8 + vertices.numel() * 4 + triangles.numel() * 8,
                    lambda: check(load().rx_iso_emit(_ptr(v), level, z, y, x, z_base, _ptr(bits), _ptr(offsets), k_emit, v_skip, q_skip,
                                                     vertex_base, nv, nq, _ptr(vertices), _ptr(triangles), stream_ptr()), "rx_iso_emit"))
    return (vertices, triangles, int(last_plane)) if return_last_plane else (vertices, triangles)


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
