"""Post-processing on the device: connected components of a thresholded uint8 volume, their sizes, and the size filter
(csrc/rx_components.hip; postprocess/components.py holds the numpy statements and the out-of-core driver), and the triangle mesh of
a uint8 volume by surface nets (csrc/rx_isosurface.hip; postprocess/isosurface.py), and the refinement of such a mesh: canonical
adjacency, Taubin smoothing, vertex normals (csrc/rx_meshrefine.hip; postprocess/refine.py), its decimation by vertex clustering
(csrc/rx_meshdecimate.hip; postprocess/decimate.py), and its orientation against a sampled vector field: trilinear sampling at the
vertices, the per-triangle cosine and side, the selection of one face (csrc/rx_meshsample.hip; postprocess/orient.py)."""
from ctypes import c_void_p
from typing import NamedTuple

import torch

from .. import lib as _l
from ..lib import check, load, stream_ptr
from .core import _U16, _ptr, device_batch, result_tensor, timed_bytes

_CONNECTIVITY = (6, 18, 26)
_F32_MAX = 3.4028234663852886e38      # a factor or a clamp must be finite as a float32


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


# ---- mesh refinement (csrc/rx_meshrefine.hip; postprocess/refine.py) ----------------------------------------------------------------------------
class MeshAdjacency(NamedTuple):
    """what `mesh_adjacency` returns.  The first three are postprocess.adjacency_numpy's, with the ids as int32; the last two are the
    triangles of the corners at each vertex, ascending (postprocess.refine.corner_faces_numpy), which the normals gather over."""
    offsets: torch.Tensor          # int64 (V + 1,)
    neighbours: torch.Tensor       # int32 (E,)
    boundary: torch.Tensor         # uint8 (V,)
    face_offsets: torch.Tensor     # int64 (V + 1,)
    faces: torch.Tensor            # int32 (3 T,)


def _mesh_triangles(fn, n_vertices, triangles):
    if isinstance(n_vertices, bool) or not isinstance(n_vertices, int) or not 0 <= n_vertices <= _l.RX_MESH_MAX_VERTICES:
        raise _l.RxError(f"{fn}: n_vertices {n_vertices!r} (an integer 0 .. 2^31 - 2: ids are held as int32)")
    t = triangles
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise _l.RxError(f"{fn}: `triangles` must be a device tensor (the host statement is postprocess.adjacency_numpy)")
    if t.dtype != torch.int64 or t.dim() != 2 or t.shape[1] != 3:
        raise _l.RxError(f"{fn}: `triangles` must be an int64 (T, 3) tensor, got {t.dtype} {tuple(t.shape)}")
    if t.shape[0] > _l.RX_MESH_MAX_TRIANGLES:
        raise _l.RxError(f"{fn}: `triangles`: {t.shape[0]} of them (at most (2^31 - 2) / 3: a vertex's corners are counted in int32)")
    if t.shape[0] and n_vertices == 0:
        raise _l.RxError(f"{fn}: `triangles` name vertices of a mesh that has none")
    return t.contiguous()


def _mesh_vertices(fn, vertices):
    v = vertices
    if not isinstance(v, torch.Tensor) or not v.is_cuda:
        raise _l.RxError(f"{fn}: `vertices` must be a device tensor (the host statement is postprocess.refine_numpy)")
    if v.dtype != torch.float32 or v.dim() != 2 or v.shape[1] != 3:
        raise _l.RxError(f"{fn}: `vertices` must be a float32 (V, 3) tensor, got {v.dtype} {tuple(v.shape)}")
    return v.contiguous()


def _mesh_finite(fn, v):
    """one launch and one small device-to-host read: refuses `vertices` that hold a NaN or an infinity"""
    flag = torch.zeros(1, dtype=torch.int32, device=v.device)
    check(load().rx_mesh_check_vertices(_ptr(v), v.shape[0], _ptr(flag), stream_ptr()), "rx_mesh_check_vertices")
    if flag.item():
        raise _l.RxError(f"{fn}: `vertices` hold a NaN or an infinity")


def _mesh_adjacency_of(fn, adjacency, n_vertices, t):
    """`adjacency` (None: built here) checked against the mesh's sizes"""
    if adjacency is None:
        return mesh_adjacency(n_vertices, t)
    a = adjacency
    want = ((n_vertices + 1,), torch.int64), (None, torch.int32), ((n_vertices,), torch.uint8), ((n_vertices + 1,), torch.int64), ((3 * t.shape[0],), torch.int32)
    if not isinstance(a, MeshAdjacency) or any(not isinstance(x, torch.Tensor) or x.device != t.device or x.dtype != d or not x.is_contiguous()
                                               or x.dim() != 1 or (s is not None and tuple(x.shape) != s) for x, (s, d) in zip(a, want)):
        raise _l.RxError(f"{fn}: `adjacency` must be what mesh_adjacency({n_vertices}, triangles) returned for this mesh")
    return a


def mesh_adjacency(n_vertices, triangles):
    """the canonical vertex adjacency of an int64 (T, 3) device tensor of triangles over `n_vertices` vertices -> MeshAdjacency
    (postprocess.adjacency_numpy and corner_faces_numpy are the statements).  Count (integer atomics), scan, fill at a cursor,
    canonicalise per vertex, scan, compact: after the canonicalising pass nothing of the arrival order is left, so two runs give
    the same bytes.  One small device-to-host read (the id check's flag and the number of neighbours, which sizes the result).  No
    launch where `n_vertices` or T is 0."""
    fn = "mesh_adjacency"
    t = _mesh_triangles(fn, n_vertices, triangles)
    V, T, dev = n_vertices, t.shape[0], t.device
    if V == 0 or T == 0:
        z = torch.zeros(V + 1, dtype=torch.int64, device=dev)
        return MeshAdjacency(z, torch.zeros(0, dtype=torch.int32, device=dev), torch.zeros(V, dtype=torch.uint8, device=dev), z.clone(),
                             torch.zeros(0, dtype=torch.int32, device=dev))
    so, st = load(), stream_ptr()
    counts = torch.empty(V, dtype=torch.int32, device=dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    foff = torch.empty(V + 1, dtype=torch.int64, device=dev)
    faces = torch.empty(3 * T, dtype=torch.int32, device=dev)
    raw = torch.empty(6 * T, dtype=torch.int32, device=dev)
    boundary = torch.empty(V, dtype=torch.uint8, device=dev)
    offsets = torch.empty(V + 1, dtype=torch.int64, device=dev)
    timed_bytes("mesh_count", T * 24 + 3 * T * 4, lambda: check(so.rx_mesh_count(_ptr(t), T, V, _ptr(counts), _ptr(flag), st), "rx_mesh_count"))
    timed_bytes("mesh_scan", V * 12, lambda: check(so.rx_mesh_scan(_ptr(counts), V, _ptr(foff), st), "rx_mesh_scan"))
    # `counts` is free again: it serves as the fill cursor, then holds the degrees
    timed_bytes("mesh_fill", T * 24 + 3 * T * (16 + 4 + 12),
                lambda: check(so.rx_mesh_fill(_ptr(t), T, V, _ptr(foff), _ptr(counts), 3 * T, _ptr(faces), _ptr(raw), st), "rx_mesh_fill"))
    timed_bytes("mesh_canonical", 2 * 3 * T * 12 + V * (8 + 4 + 1),
                lambda: check(so.rx_mesh_canonical(V, _ptr(foff), 3 * T, _ptr(faces), _ptr(raw), _ptr(counts), _ptr(boundary), st), "rx_mesh_canonical"))
    timed_bytes("mesh_scan", V * 12, lambda: check(so.rx_mesh_scan(_ptr(counts), V, _ptr(offsets), st), "rx_mesh_scan"))
    bad, E = torch.cat([flag.to(torch.int64), offsets[V:]]).tolist()      # the one device-to-host read
    if bad:
        raise _l.RxError(f"{fn}: `triangles` name a vertex outside 0 .. {V - 1}")
    nbr = torch.empty(E, dtype=torch.int32, device=dev)
    timed_bytes("mesh_compact", V * 24 + E * 8,
                lambda: check(so.rx_mesh_compact(V, _ptr(foff), _ptr(raw), 3 * T, _ptr(offsets), E, _ptr(nbr), st), "rx_mesh_compact"))
    return MeshAdjacency(offsets, nbr, boundary, foff, faces)


def mesh_smooth(vertices, triangles, iterations, lam=0.5, mu=-0.53, clamp=None, pin_boundary=True, adjacency=None):
    """Taubin smoothing of a float32 (V, 3) device tensor of vertices over int64 (T, 3) triangles -> a new float32 (V, 3) tensor, bit
    for bit postprocess.smooth_numpy: every iteration is one pass with factor `lam`, then one with `mu` (None: `lam` passes only);
    `clamp` keeps every component within that distance of the input; `pin_boundary` keeps boundary vertices where they are.  One
    launch per pass over two ping-pong buffers; a vertex gathers its neighbours in list order; no atomics.  `adjacency`: what
    `mesh_adjacency` returned for this mesh (None: built here).  One small device-to-host read for the finiteness check."""
    fn = "mesh_smooth"
    v = _mesh_vertices(fn, vertices)
    t = _mesh_triangles(fn, v.shape[0], triangles)
    if isinstance(iterations, bool) or not isinstance(iterations, int) or iterations < 0:
        raise _l.RxError(f"{fn}: `iterations` {iterations!r} (an integer >= 0)")
    for name, x in (("lam", lam), ("mu", mu)):
        if (x is not None or name == "lam") and (isinstance(x, bool) or not isinstance(x, (int, float))
                                                 or not abs(x) <= _F32_MAX):
            raise _l.RxError(f"{fn}: `{name}` {x!r} (a finite number)")
    if clamp is not None and (isinstance(clamp, bool) or not isinstance(clamp, (int, float)) or not 0 <= clamp <= _F32_MAX):
        raise _l.RxError(f"{fn}: `clamp` {clamp!r} (a finite number >= 0, or None)")
    V = v.shape[0]
    if V == 0:
        return v.clone()
    _mesh_finite(fn, v)
    if t.shape[0] == 0 or iterations == 0:
        return v.clone()
    a = _mesh_adjacency_of(fn, adjacency, V, t)
    factors = [lam] if mu is None else [lam, mu]
    bufs = [torch.empty_like(v), torch.empty_like(v)]
    so, st, E, src = load(), stream_ptr(), a.neighbours.shape[0], v
    origin = _ptr(v) if clamp is not None else c_void_p(0)
    pin = _ptr(a.boundary) if pin_boundary else c_void_p(0)
    for i in range(iterations * len(factors)):
        dst, f = bufs[i % 2], factors[i % len(factors)]
        timed_bytes("mesh_smooth_pass", V * (12 + 12 + 16 + 1) + E * (4 + 12) + (V * 12 if clamp is not None else 0),
                    lambda: check(so.rx_mesh_smooth_pass(_ptr(src), origin, V, _ptr(a.offsets), _ptr(a.neighbours), E, pin, f,
                                                         0.0 if clamp is None else clamp, _ptr(dst), st), "rx_mesh_smooth_pass"))
        src = dst
    return src


def mesh_vertex_normals(vertices, triangles, adjacency=None):
    """area-weighted vertex normals of a float32 (V, 3) / int64 (T, 3) device mesh -> float32 (V, 3), bit for bit
    postprocess.vertex_normals_numpy: the face vectors cross(pb - pa, pc - pa) are stored by one pass, then every vertex sums those of
    its corners over its sorted triangle list and normalises.  No float atomics.  `adjacency` as in `mesh_smooth`."""
    fn = "mesh_vertex_normals"
    v = _mesh_vertices(fn, vertices)
    t = _mesh_triangles(fn, v.shape[0], triangles)
    V, T = v.shape[0], t.shape[0]
    if V == 0 or T == 0:
        return torch.zeros_like(v)
    _mesh_finite(fn, v)
    a = _mesh_adjacency_of(fn, adjacency, V, t)
    so, st = load(), stream_ptr()
    fvec = torch.empty((T, 3), dtype=torch.float32, device=v.device)
    out = torch.empty_like(v)
    timed_bytes("mesh_face_vectors", T * (24 + 36 + 12),
                lambda: check(so.rx_mesh_face_vectors(_ptr(v), V, _ptr(t), T, _ptr(fvec), st), "rx_mesh_face_vectors"))
    timed_bytes("mesh_vertex_normals", V * (16 + 12) + 3 * T * (4 + 12),
                lambda: check(so.rx_mesh_vertex_normals(V, _ptr(a.face_offsets), _ptr(a.faces), a.faces.shape[0], _ptr(fvec), T, _ptr(out), st),
                              "rx_mesh_vertex_normals"))
    return out


# ---- mesh decimation (csrc/rx_meshdecimate.hip; postprocess/decimate.py) ------------------------------------------------------------------------
_REPRESENTATIVES = ("mean", "nearest")


def _table_capacity(n_vertices):
    """the smallest power of two that is at least 2 V + 2 (the library wants one above V, and takes at most 2^31)"""
    return min(1 << (2 * n_vertices + 1).bit_length(), 2**31)


def mesh_decimate(vertices, triangles, cell, representative="mean"):
    """vertex clustering of a float32 (V, 3) / int64 (T, 3) device mesh on a grid of `cell`-sized cubes -> (vertices float32 (V', 3),
    triangles int64 (T', 3), cluster_of int64 (V,)), bit for bit postprocess.decimate_numpy: the vertices of a cube become one
    representative ("mean": the sequential float32 mean of the members in ascending id; "nearest": the member nearest the cube's
    centre, lowest id on ties), a triangle with two corners in one cluster is dropped, and of the triangles with the same unordered
    cluster triple the lowest index stays.  Keys, a hash table claimed by 64-bit compare-and-swap with an integer minimum per slot,
    scans, lists filled at a cursor and heap-sorted in place: no float atomics, and every number is derived from keys and smallest
    member ids, so two runs give the same bytes.  Two small device-to-host reads (the number of clusters; the output sizes).  No
    launch where V is 0; none of the triangle passes where T is 0."""
    fn = "mesh_decimate"
    v = _mesh_vertices(fn, vertices)
    t = _mesh_triangles(fn, v.shape[0], triangles)
    if isinstance(cell, bool) or not isinstance(cell, (int, float)) or not 0 < cell <= _F32_MAX or torch.tensor(float(cell), dtype=torch.float32).item() <= 0:
        raise _l.RxError(f"{fn}: `cell` {cell!r} (a finite float32 > 0)")
    if representative not in _REPRESENTATIVES:
        raise _l.RxError(f"{fn}: `representative` {representative!r} (one of {', '.join(_REPRESENTATIVES)})")
    V, T, dev = v.shape[0], t.shape[0], v.device
    empty = lambda: (torch.zeros((0, 3), dtype=torch.float32, device=dev), torch.zeros((0, 3), dtype=torch.int64, device=dev))      # noqa: E731
    if V == 0:
        return empty() + (torch.zeros(0, dtype=torch.int64, device=dev),)
    _mesh_finite(fn, v)
    so, st = load(), stream_ptr()
    i32 = lambda n: torch.empty(n, dtype=torch.int32, device=dev)      # noqa: E731
    i64 = lambda n: torch.empty(n, dtype=torch.int64, device=dev)      # noqa: E731
    cap = _table_capacity(V)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    keys, table_keys, table_min, slot_of, first, rank, cluster_of = i64(V), i64(cap), i32(cap), i32(V), i32(V), i64(V + 1), i64(V)
    timed_bytes("mesh_cluster_keys", V * (12 + 8), lambda: check(so.rx_mesh_cluster_keys(_ptr(v), V, cell, _ptr(keys), _ptr(flag), st), "rx_mesh_cluster_keys"))
    timed_bytes("mesh_cluster_assign", cap * 12 + V * (8 + 12 + 4 + 4),
                lambda: check(so.rx_mesh_cluster_assign(_ptr(keys), V, cap, _ptr(table_keys), _ptr(table_min), _ptr(slot_of), _ptr(first), _ptr(flag), st),
                              "rx_mesh_cluster_assign"))
    timed_bytes("mesh_scan", V * 12, lambda: check(so.rx_mesh_scan(_ptr(first), V, _ptr(rank), st), "rx_mesh_scan"))
    timed_bytes("mesh_cluster_number", V * (4 + 4 + 8 + 8),
                lambda: check(so.rx_mesh_cluster_number(V, _ptr(slot_of), cap, _ptr(table_min), _ptr(rank), _ptr(cluster_of), st), "rx_mesh_cluster_number"))
    bad, C = torch.cat([flag.to(torch.int64), rank[V:]]).tolist()      # the first device-to-host read
    if bad & 1:
        raise _l.RxError(f"{fn}: `cell` {cell!r} puts a vertex in a grid cell with an index of 2^20 or more; choose a larger cell")
    if bad:
        raise _l.RxError(f"{fn}: the hash table of {cap} slots ran out of probes (flag {bad}): not a state this call can reach")
    del table_keys, table_min, slot_of, first, rank
    counts, reps = i32(C), torch.empty((C, 3), dtype=torch.float32, device=dev)
    if representative == "mean":
        moff, members = i64(C + 1), i32(V)
        timed_bytes("mesh_cluster_count", V * 12, lambda: check(so.rx_mesh_cluster_count(_ptr(cluster_of), V, C, _ptr(counts), st), "rx_mesh_cluster_count"))
        timed_bytes("mesh_scan", C * 12, lambda: check(so.rx_mesh_scan(_ptr(counts), C, _ptr(moff), st), "rx_mesh_scan"))
        # `counts` is free again: it serves as the fill cursor
        timed_bytes("mesh_cluster_fill", V * (8 + 16 + 4 + 4),
                    lambda: check(so.rx_mesh_cluster_fill(_ptr(cluster_of), V, C, _ptr(moff), _ptr(counts), V, _ptr(members), st), "rx_mesh_cluster_fill"))
        timed_bytes("mesh_cluster_mean", C * (16 + 12) + 2 * V * 4 + V * 12,
                    lambda: check(so.rx_mesh_cluster_mean(_ptr(v), V, C, _ptr(moff), _ptr(members), V, _ptr(reps), st), "rx_mesh_cluster_mean"))
        del moff, members
    else:
        best = i64(C)
        timed_bytes("mesh_cluster_nearest", V * (12 + 8 + 8 + 8) + C * (8 + 12 + 12),
                    lambda: check(so.rx_mesh_cluster_nearest(_ptr(v), _ptr(keys), V, cell, _ptr(cluster_of), C, _ptr(best), _ptr(reps), st),
                                  "rx_mesh_cluster_nearest"))
        del best
    del keys
    if T == 0:
        return empty() + (cluster_of,)
    used, toff, uoff, entries, keep, koff = i32(C), i64(C + 1), i64(C + 1), i32(3 * T), i32(T), i64(T + 1)
    timed_bytes("mesh_cluster_remap", T * (24 + 24 + 4 + 12),
                lambda: check(so.rx_mesh_cluster_remap(_ptr(t), T, V, _ptr(cluster_of), C, _ptr(counts), _ptr(used), _ptr(flag), st), "rx_mesh_cluster_remap"))
    timed_bytes("mesh_scan", C * 12, lambda: check(so.rx_mesh_scan(_ptr(counts), C, _ptr(toff), st), "rx_mesh_scan"))
    timed_bytes("mesh_scan", C * 12, lambda: check(so.rx_mesh_scan(_ptr(used), C, _ptr(uoff), st), "rx_mesh_scan"))
    timed_bytes("mesh_cluster_unique", T * (24 + 24 + 16 + 4 + 3 * 12 + 4),
                lambda: check(so.rx_mesh_cluster_unique(_ptr(t), T, V, _ptr(cluster_of), C, _ptr(toff), _ptr(counts), T, _ptr(entries), _ptr(keep), st),
                              "rx_mesh_cluster_unique"))
    timed_bytes("mesh_scan", T * 12, lambda: check(so.rx_mesh_scan(_ptr(keep), T, _ptr(koff), st), "rx_mesh_scan"))
    bad, nv, nt = torch.cat([flag.to(torch.int64), uoff[C:], koff[T:]]).tolist()      # the second read: the sizes of the result
    if bad:
        raise _l.RxError(f"{fn}: `triangles` name a vertex outside 0 .. {V - 1}")
    out_v, out_t = torch.empty((nv, 3), dtype=torch.float32, device=dev), torch.empty((nt, 3), dtype=torch.int64, device=dev)
    if nt:
        timed_bytes("mesh_cluster_emit", T * (4 + 8) + nt * (24 + 24 + 24 + 24) + C * (4 + 8) + nv * 24,
                    lambda: check(so.rx_mesh_cluster_emit(_ptr(t), T, V, _ptr(cluster_of), C, _ptr(keep), _ptr(koff), _ptr(used), _ptr(uoff), _ptr(reps),
                                                          nv, _ptr(out_v), nt, _ptr(out_t), st), "rx_mesh_cluster_emit"))
    return out_v, out_t, cluster_of


# ---- mesh orientation (csrc/rx_meshsample.hip; postprocess/orient.py) ---------------------------------------------------------------------------
_SAMPLE_RULES = {"copy": (_l.RX_MESH_SAMPLE_COPY, (torch.float32,)), "u8": (_l.RX_MESH_SAMPLE_U8, (torch.uint8,)),
                 "u16": (_l.RX_MESH_SAMPLE_U16, (_U16, torch.int16)), "normal_u16": (_l.RX_MESH_SAMPLE_NORMAL_U16, (_U16, torch.int16))}
_SIDES = {"both": 0, "front": 1, "back": -1}


def _plain_int(x):
    return isinstance(x, int) and not isinstance(x, bool)


def mesh_sample(volume, points, rule, z_base=0, z_total=None, unit=False, out=None):
    """a (C, Zs, Y, X) device volume, C in 1 .. 8, sampled trilinearly with clamped borders at float32 (V, 3) device `points` given as
    (x, y, z) in voxel coordinates -> float32 (V, C), bit for bit postprocess.sample_points_numpy.  `rule` decodes a stored value:
    "copy" (a float32 volume), "u8" (uint8, v / 255), "u16" (uint16, v / 65535), "normal_u16" (uint16, (v / 65535) * 2 - 1); a
    uint16 volume may be held as int16, whose bits are read as uint16.  `volume` holds planes [z_base, z_base + Zs) of a volume of
    `z_total` planes (default: z_base + Zs); a point whose two clamped z planes are not both among them is left untouched in `out`
    (a new `out` starts as zeros), so successive slab calls fill one buffer.  `unit` (C = 3): the three values are divided by
    their length, (0, 0, 0) where it is 0 (postprocess.unit_numpy).  One launch, a thread per point, no atomics; one small
    device-to-host read for the finiteness check.  No launch where V is 0."""
    fn = "mesh_sample"
    if rule not in _SAMPLE_RULES:
        raise _l.RxError(f"{fn}: rule {rule!r} (one of {', '.join(_SAMPLE_RULES)})")
    code, dtypes = _SAMPLE_RULES[rule]
    if not isinstance(volume, torch.Tensor) or not volume.is_cuda:
        raise _l.RxError(f"{fn}: `volume` must be a device tensor (the host statement is postprocess.sample_points_numpy)")
    if volume.dtype not in dtypes:
        raise _l.RxError(f"{fn}: rule {rule!r} decodes a {str(dtypes[0]).replace('torch.', '')} volume, got {volume.dtype}")
    if volume.dim() != 4 or volume.numel() == 0:
        raise _l.RxError(f"{fn}: `volume` must be a non-empty (C, Z, Y, X) tensor, got {tuple(volume.shape)}")
    C, Zs, Y, X = volume.shape
    if not 1 <= C <= _l.RX_MESH_SAMPLE_MAX_CHANNELS:
        raise _l.RxError(f"{fn}: `volume` has {C} channels (1 .. {_l.RX_MESH_SAMPLE_MAX_CHANNELS})")
    p = points
    if not isinstance(p, torch.Tensor) or not p.is_cuda:
        raise _l.RxError(f"{fn}: `points` must be a device tensor (the host statement is postprocess.sample_points_numpy)")
    if p.dtype != torch.float32 or p.dim() != 2 or p.shape[1] != 3:
        raise _l.RxError(f"{fn}: `points` must be a float32 (V, 3) tensor, got {p.dtype} {tuple(p.shape)}")
    if p.shape[0] > _l.RX_MESH_MAX_VERTICES:
        raise _l.RxError(f"{fn}: `points`: {p.shape[0]} of them (at most 2^31 - 2)")
    if z_total is None and _plain_int(z_base):
        z_total = z_base + Zs
    if not _plain_int(z_base) or not _plain_int(z_total) or z_base < 0 or z_base + Zs > z_total:
        raise _l.RxError(f"{fn}: a slab of planes {z_base!r} .. {z_base!r} + {Zs} does not lie inside z_total {z_total!r}")
    if max(z_total, Y, X) > _l.RX_MESH_SAMPLE_MAX_EXTENT:
        raise _l.RxError(f"{fn}: an extent above 2^24 - 2 in {(z_total, Y, X)}: an index must be an exact float32")
    if not isinstance(unit, bool) or (unit and C != 3):
        raise _l.RxError(f"{fn}: `unit` {unit!r} with {C} channels (true or false; true needs 3 channels)")
    vol, p = volume.contiguous(), p.contiguous()
    V = p.shape[0]
    out = result_tensor(fn, "out", out, (V, C), torch.float32, p.device, alloc=torch.zeros)
    if V == 0:
        return out
    flag = torch.zeros(1, dtype=torch.int32, device=p.device)
    check(load().rx_mesh_check_vertices(_ptr(p), V, _ptr(flag), stream_ptr()), "rx_mesh_check_vertices")
    if flag.item():
        raise _l.RxError(f"{fn}: `points` hold a NaN or an infinity")
    timed_bytes("mesh_sample", V * (12 + 4 * C + 8 * C * vol.element_size()),
                lambda: check(load().rx_mesh_sample(_ptr(vol), code, C, z_base, Zs, z_total, Y, X, _ptr(p), V, int(unit), _ptr(out), stream_ptr()),
                              "rx_mesh_sample"))
    return out


def mesh_face_cos(vertices, triangles, vectors, min_cos, side):
    """per triangle of a float32 (V, 3) / int64 (T, 3) device mesh the cosine between its face vector and the sum of the float32
    (V, 3) `vectors` at its corners, and its classification -> (cos float32 (T,), side int8 (T,), used int32 (V,)), bit for bit
    postprocess.face_cos_numpy and side_numpy: side is 1 (front) where cos > min_cos, -1 (back) where cos < -min_cos, else 0 (rim;
    a NaN, which a degenerate triangle or a zero vector sum gives, included).  `side`: "front", "back" or "both" -- used[v] = 1 for
    the corners of the triangles of that side ("both": of every triangle), a plain store of a constant.  One launch, a thread per
    triangle, no atomics; one small device-to-host read (the id check's flag).  No launch where T is 0."""
    fn = "mesh_face_cos"
    v = _mesh_vertices(fn, vertices)
    t = _mesh_triangles(fn, v.shape[0], triangles)
    n = vectors
    if not isinstance(n, torch.Tensor) or not n.is_cuda:
        raise _l.RxError(f"{fn}: `vectors` must be a device tensor (the host statement is postprocess.face_cos_numpy)")
    if n.dtype != torch.float32 or tuple(n.shape) != tuple(v.shape):
        raise _l.RxError(f"{fn}: `vectors` must be a float32 {tuple(v.shape)} tensor, got {n.dtype} {tuple(n.shape)}")
    if isinstance(min_cos, bool) or not isinstance(min_cos, (int, float)) or not 0 <= min_cos < 1:
        raise _l.RxError(f"{fn}: `min_cos` {min_cos!r} (a number in [0, 1))")
    if not isinstance(side, str) or side not in _SIDES:
        raise _l.RxError(f"{fn}: `side` {side!r} (one of {', '.join(_SIDES)})")
    V, T, dev = v.shape[0], t.shape[0], v.device
    cos, sd = torch.empty(T, dtype=torch.float32, device=dev), torch.empty(T, dtype=torch.int8, device=dev)
    used = torch.zeros(V, dtype=torch.int32, device=dev)
    if T == 0:
        return cos, sd, used
    _mesh_finite(fn, v)
    keep, flag = torch.empty(T, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    n = n.contiguous()
    timed_bytes("mesh_face_cos", T * (24 + 36 + 36 + 4 + 1 + 4 + 12),
                lambda: check(load().rx_mesh_face_cos(_ptr(v), _ptr(n), V, _ptr(t), T, float(min_cos), _SIDES[side], _ptr(cos), _ptr(sd), _ptr(keep),
                                                      _ptr(used), _ptr(flag), stream_ptr()), "rx_mesh_face_cos"))
    if flag.item():
        raise _l.RxError(f"{fn}: `triangles` name a vertex outside 0 .. {V - 1}")
    return cos, sd, used


def mesh_select(vertices, triangles, keep, attrs=(), used=None):
    """the triangles of a float32 (V, 3) / int64 (T, 3) device mesh where the bool or int32 (T,) device tensor `keep` is not 0, in
    input order, over the vertices some kept triangle names, in ascending id, renumbered to match -> (vertices, triangles, attrs,
    row_of), bit for bit postprocess.select_numpy: `attrs` are float32 (V, 3) per-vertex tensors carried along, `row_of` int64 (V,)
    the output row of every input vertex, -1 for a dropped one.  `used`: what `mesh_face_cos` returned for the same selection
    (None: marked here, one launch).  Scans of the keep and the used flags (rx_mesh_scan), then the emit pass of the decimation
    under the identity map: no atomic chooses a slot, so two runs give the same bytes.  One small device-to-host read (the id
    check's flag and the output sizes).  No launch where V or T is 0."""
    fn = "mesh_select"
    v = _mesh_vertices(fn, vertices)
    t = _mesh_triangles(fn, v.shape[0], triangles)
    V, T, dev = v.shape[0], t.shape[0], v.device
    if not isinstance(keep, torch.Tensor) or not keep.is_cuda or keep.dtype not in (torch.bool, torch.int32) or tuple(keep.shape) != (T,):
        raise _l.RxError(f"{fn}: `keep` must be a bool or int32 device tensor of shape {(T,)}")
    attrs = tuple(attrs)
    for a in attrs:
        if not isinstance(a, torch.Tensor) or a.device != dev or a.dtype != torch.float32 or tuple(a.shape) != (V, 3):
            raise _l.RxError(f"{fn}: every attribute must be a float32 {(V, 3)} tensor on {dev}")
    if used is not None and (not isinstance(used, torch.Tensor) or used.device != dev or used.dtype != torch.int32 or tuple(used.shape) != (V,)
                             or not used.is_contiguous()):
        raise _l.RxError(f"{fn}: `used` must be what mesh_face_cos returned for this mesh: a contiguous int32 {(V,)} tensor on {dev}")
    if V == 0 or T == 0:
        return (torch.zeros((0, 3), dtype=torch.float32, device=dev), torch.zeros((0, 3), dtype=torch.int64, device=dev),
                tuple(torch.zeros((0, 3), dtype=torch.float32, device=dev) for _ in attrs), torch.full((V,), -1, dtype=torch.int64, device=dev))
    so, st = load(), stream_ptr()
    keep = (keep != 0).to(torch.int32).contiguous()
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    if used is None:
        used = torch.empty(V, dtype=torch.int32, device=dev)
        timed_bytes("mesh_select_mark", T * (4 + 24 + 12),
                    lambda: check(so.rx_mesh_select_mark(_ptr(t), T, V, _ptr(keep), _ptr(used), _ptr(flag), st), "rx_mesh_select_mark"))
    koff, uoff = torch.empty(T + 1, dtype=torch.int64, device=dev), torch.empty(V + 1, dtype=torch.int64, device=dev)
    timed_bytes("mesh_scan", T * 12, lambda: check(so.rx_mesh_scan(_ptr(keep), T, _ptr(koff), st), "rx_mesh_scan"))
    timed_bytes("mesh_scan", V * 12, lambda: check(so.rx_mesh_scan(_ptr(used), V, _ptr(uoff), st), "rx_mesh_scan"))
    bad, nv, nt = torch.cat([flag.to(torch.int64), uoff[V:], koff[T:]]).tolist()      # the one device-to-host read
    if bad:
        raise _l.RxError(f"{fn}: `triangles` name a vertex outside 0 .. {V - 1}")
    identity = torch.arange(V, dtype=torch.int64, device=dev)
    out_v, out_t = torch.empty((nv, 3), dtype=torch.float32, device=dev), torch.empty((nt, 3), dtype=torch.int64, device=dev)
    out_a = tuple(torch.empty((nv, 3), dtype=torch.float32, device=dev) for _ in attrs)
    if nt:
        timed_bytes("mesh_cluster_emit", T * (4 + 8) + nt * (24 + 24 + 24 + 24) + V * (4 + 8) + nv * 24,
                    lambda: check(so.rx_mesh_cluster_emit(_ptr(t), T, V, _ptr(identity), V, _ptr(keep), _ptr(koff), _ptr(used), _ptr(uoff), _ptr(v),
                                                          nv, _ptr(out_v), nt, _ptr(out_t), st), "rx_mesh_cluster_emit"))
        for a, o in zip(attrs, out_a):      # the vertex half of the emit pass alone
            a = a.contiguous()
            timed_bytes("mesh_cluster_emit", V * (4 + 8) + nv * 24,
                        lambda: check(so.rx_mesh_cluster_emit(_ptr(t), T, V, _ptr(identity), V, _ptr(keep), _ptr(koff), _ptr(used), _ptr(uoff), _ptr(a),
                                                              nv, _ptr(o), 0, c_void_p(0), st), "rx_mesh_cluster_emit"))
    row_of = torch.where(used != 0, uoff[:V], torch.full_like(uoff[:V], -1))
    return out_v, out_t, out_a, row_of
