"""Triangle meshes on the device.  First the mesh targets of training: slices of a mesh as normal and label volumes
(csrc/rx_meshslice.hip; the numpy statements live in tasks/normals/mesh_targets.py).  Then the post-processing of an extracted mesh,
each stage bit for bit the numpy statements of its module under postprocess/: refinement -- canonical adjacency, Taubin smoothing,
vertex normals (csrc/rx_meshrefine.hip; refine.py); decimation by vertex clustering (csrc/rx_meshdecimate.hip; decimate.py);
orientation against a sampled vector field -- trilinear sampling at the vertices, the per-triangle cosine and side, the selection
of one face (csrc/rx_meshsample.hip; orient.py).  The post-processing operations share one set of argument checks (`_f32x3`,
`_mesh_triangles`, `_mesh_finite`), one device-to-host read (`_sizes`) and one compaction tail (`_compact`)."""
from ctypes import c_void_p
from typing import NamedTuple

import torch

from .. import lib as _l
from ..lib import check, load, stream_ptr
from .core import _U16, _ptr, result_tensor, timed_bytes

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


# ---- post-processing: the shared checks, the one read and the compaction tail -------------------------------------------------------------------
_F32_MAX = 3.4028234663852886e38      # a factor or a clamp must be finite as a float32
_STATEMENT = {"vertices": "refine_numpy", "points": "sample_points_numpy", "vectors": "face_cos_numpy"}


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


def _f32x3(fn, name, t, rows=None, device=None):
    """`t`: a float32 (V, 3) device tensor -- with `rows`, of exactly that many; with `device`, one carried beside the vertices on
    it, and `name` is how the refusal calls it -> it made contiguous"""
    shape = "(V, 3)" if rows is None else (rows, 3)      # as a refusal prints it
    fits = isinstance(t, torch.Tensor) and t.dtype == torch.float32 and (tuple(t.shape) == (rows, 3) if rows is not None
                                                                          else t.dim() == 2 and t.shape[1] == 3)
    if device is not None:
        if not fits or t.device != device:
            raise _l.RxError(f"{fn}: {name} must be a float32 {shape} tensor on {device}")
    elif not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise _l.RxError(f"{fn}: `{name}` must be a device tensor (the host statement is postprocess.{_STATEMENT[name]})")
    elif not fits:
        raise _l.RxError(f"{fn}: `{name}` must be a float32 {shape} tensor, got {t.dtype} {tuple(t.shape)}")
    return t.contiguous()


def _mesh_finite(fn, v, name="vertices"):
    """one launch and one small device-to-host read: refuses positions that hold a NaN or an infinity"""
    flag = torch.zeros(1, dtype=torch.int32, device=v.device)
    check(load().rx_mesh_check_vertices(_ptr(v), v.shape[0], _ptr(flag), stream_ptr()), "rx_mesh_check_vertices")
    if flag.item():
        raise _l.RxError(f"{fn}: `{name}` hold a NaN or an infinity")


def _sizes(fn, flag, *scan_tails, n_vertices=None):
    """the one device-to-host read of a pass: the int32 `flag` and the last word of each scan -> [flag, sizes ...] on the host.
    With `n_vertices` a raised flag is the id check's, and is refused here."""
    host = torch.cat([flag.to(torch.int64), *scan_tails]).tolist() if scan_tails else flag.tolist()
    if n_vertices is not None and host[0]:
        raise _l.RxError(f"{fn}: `triangles` name a vertex outside 0 .. {n_vertices - 1}")
    return host


def _scan(counts, n, offsets):
    timed_bytes("mesh_scan", n * 12, lambda: check(load().rx_mesh_scan(_ptr(counts), n, _ptr(offsets), stream_ptr()), "rx_mesh_scan"))


def _compact(fn, t, V, cluster_of, C, keep, used, flag, reps, attrs=(), uoff=None):
    """the tail of a decimation or a selection: the scan of the int32 (T,) `keep` flags, the scan of the int32 (C,) `used` flags
    (`uoff`: that scan, where it has run already), the read of the two sizes, and the emit pass -- the kept triangles renumbered, the
    rows of `reps` and of every float32 (C, 3) tensor of `attrs` of the used clusters -> (vertices, triangles, attrs, uoff).
    `cluster_of` None: the identity map, made here once the sizes are known."""
    T, dev, so, st = t.shape[0], t.device, load(), stream_ptr()
    koff = torch.empty(T + 1, dtype=torch.int64, device=dev)
    _scan(keep, T, koff)
    if uoff is None:
        uoff = torch.empty(C + 1, dtype=torch.int64, device=dev)
        _scan(used, C, uoff)
    _, nv, nt = _sizes(fn, flag, uoff[C:], koff[T:], n_vertices=V)
    if cluster_of is None:
        cluster_of = torch.arange(C, dtype=torch.int64, device=dev)
    out_v, out_t = torch.empty((nv, 3), dtype=torch.float32, device=dev), torch.empty((nt, 3), dtype=torch.int64, device=dev)
    out_a = tuple(torch.empty((nv, 3), dtype=torch.float32, device=dev) for _ in attrs)
    if nt:
        timed_bytes("mesh_cluster_emit", T * (4 + 8) + nt * (24 + 24 + 24 + 24) + C * (4 + 8) + nv * 24,
                    lambda: check(so.rx_mesh_cluster_emit(_ptr(t), T, V, _ptr(cluster_of), C, _ptr(keep), _ptr(koff), _ptr(used), _ptr(uoff), _ptr(reps),
                                                          nv, _ptr(out_v), nt, _ptr(out_t), st), "rx_mesh_cluster_emit"))
        for a, o in zip(attrs, out_a):      # the vertex half of the emit pass alone
            timed_bytes("mesh_cluster_emit", C * (4 + 8) + nv * 24,
                        lambda: check(so.rx_mesh_cluster_emit(_ptr(t), T, V, _ptr(cluster_of), C, _ptr(keep), _ptr(koff), _ptr(used), _ptr(uoff), _ptr(a),
                                                              nv, _ptr(o), 0, c_void_p(0), st), "rx_mesh_cluster_emit"))
    return out_v, out_t, out_a, uoff


# ---- mesh refinement (csrc/rx_meshrefine.hip; postprocess/refine.py) ----------------------------------------------------------------------------
class MeshAdjacency(NamedTuple):
    """what `mesh_adjacency` returns.  The first three are postprocess.adjacency_numpy's, with the ids as int32; the last two are the
    triangles of the corners at each vertex, ascending (postprocess.refine.corner_faces_numpy), which the normals gather over."""
    offsets: torch.Tensor          # int64 (V + 1,)
    neighbours: torch.Tensor       # int32 (E,)
    boundary: torch.Tensor         # uint8 (V,)
    face_offsets: torch.Tensor     # int64 (V + 1,)
    faces: torch.Tensor            # int32 (3 T,)


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
    _scan(counts, V, foff)
    # `counts` is free again: it serves as the fill cursor, then holds the degrees
    timed_bytes("mesh_fill", T * 24 + 3 * T * (16 + 4 + 12),
                lambda: check(so.rx_mesh_fill(_ptr(t), T, V, _ptr(foff), _ptr(counts), 3 * T, _ptr(faces), _ptr(raw), st), "rx_mesh_fill"))
    timed_bytes("mesh_canonical", 2 * 3 * T * 12 + V * (8 + 4 + 1),
                lambda: check(so.rx_mesh_canonical(V, _ptr(foff), 3 * T, _ptr(faces), _ptr(raw), _ptr(counts), _ptr(boundary), st), "rx_mesh_canonical"))
    _scan(counts, V, offsets)
    _, E = _sizes(fn, flag, offsets[V:], n_vertices=V)      # the one device-to-host read
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
    v = _f32x3(fn, "vertices", vertices)
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
    v = _f32x3(fn, "vertices", vertices)
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
    v = _f32x3(fn, "vertices", vertices)
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
    _scan(first, V, rank)
    timed_bytes("mesh_cluster_number", V * (4 + 4 + 8 + 8),
                lambda: check(so.rx_mesh_cluster_number(V, _ptr(slot_of), cap, _ptr(table_min), _ptr(rank), _ptr(cluster_of), st), "rx_mesh_cluster_number"))
    bad, C = _sizes(fn, flag, rank[V:])      # the first device-to-host read
    if bad & 1:
        raise _l.RxError(f"{fn}: `cell` {cell!r} puts a vertex in a grid cell with an index of 2^20 or more; choose a larger cell")
    if bad:
        raise _l.RxError(f"{fn}: the hash table of {cap} slots ran out of probes (flag {bad}): not a state this call can reach")
    del table_keys, table_min, slot_of, first, rank
    counts, reps = i32(C), torch.empty((C, 3), dtype=torch.float32, device=dev)
    if representative == "mean":
        moff, members = i64(C + 1), i32(V)
        timed_bytes("mesh_cluster_count", V * 12, lambda: check(so.rx_mesh_cluster_count(_ptr(cluster_of), V, C, _ptr(counts), st), "rx_mesh_cluster_count"))
        _scan(counts, C, moff)
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
    used, toff, uoff, entries, keep = i32(C), i64(C + 1), i64(C + 1), i32(3 * T), i32(T)
    timed_bytes("mesh_cluster_remap", T * (24 + 24 + 4 + 12),
                lambda: check(so.rx_mesh_cluster_remap(_ptr(t), T, V, _ptr(cluster_of), C, _ptr(counts), _ptr(used), _ptr(flag), st), "rx_mesh_cluster_remap"))
    _scan(counts, C, toff)
    _scan(used, C, uoff)
    timed_bytes("mesh_cluster_unique", T * (24 + 24 + 16 + 4 + 3 * 12 + 4),
                lambda: check(so.rx_mesh_cluster_unique(_ptr(t), T, V, _ptr(cluster_of), C, _ptr(toff), _ptr(counts), T, _ptr(entries), _ptr(keep), st),
                              "rx_mesh_cluster_unique"))
    out_v, out_t, _, _ = _compact(fn, t, V, cluster_of, C, keep, used, flag, reps, uoff=uoff)      # the second read: the sizes of the result
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
    p = _f32x3(fn, "points", points)
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
    vol, V = volume.contiguous(), p.shape[0]
    out = result_tensor(fn, "out", out, (V, C), torch.float32, p.device, alloc=torch.zeros)
    if V == 0:
        return out
    _mesh_finite(fn, p, "points")
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
    v = _f32x3(fn, "vertices", vertices)
    t = _mesh_triangles(fn, v.shape[0], triangles)
    n = _f32x3(fn, "vectors", vectors, rows=v.shape[0])
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
    timed_bytes("mesh_face_cos", T * (24 + 36 + 36 + 4 + 1 + 4 + 12),
                lambda: check(load().rx_mesh_face_cos(_ptr(v), _ptr(n), V, _ptr(t), T, float(min_cos), _SIDES[side], _ptr(cos), _ptr(sd), _ptr(keep),
                                                      _ptr(used), _ptr(flag), stream_ptr()), "rx_mesh_face_cos"))
    _sizes(fn, flag, n_vertices=V)
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
    v = _f32x3(fn, "vertices", vertices)
    t = _mesh_triangles(fn, v.shape[0], triangles)
    V, T, dev = v.shape[0], t.shape[0], v.device
    if not isinstance(keep, torch.Tensor) or not keep.is_cuda or keep.dtype not in (torch.bool, torch.int32) or tuple(keep.shape) != (T,):
        raise _l.RxError(f"{fn}: `keep` must be a bool or int32 device tensor of shape {(T,)}")
    attrs = tuple(_f32x3(fn, "every attribute", a, rows=V, device=dev) for a in attrs)
    if used is not None and (not isinstance(used, torch.Tensor) or used.device != dev or used.dtype != torch.int32 or tuple(used.shape) != (V,)
                             or not used.is_contiguous()):
        raise _l.RxError(f"{fn}: `used` must be what mesh_face_cos returned for this mesh: a contiguous int32 {(V,)} tensor on {dev}")
    if V == 0 or T == 0:
        return (torch.zeros((0, 3), dtype=torch.float32, device=dev), torch.zeros((0, 3), dtype=torch.int64, device=dev),
                tuple(torch.zeros((0, 3), dtype=torch.float32, device=dev) for _ in attrs), torch.full((V,), -1, dtype=torch.int64, device=dev))
    keep = (keep != 0).to(torch.int32).contiguous()
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    if used is None:
        used = torch.empty(V, dtype=torch.int32, device=dev)
        timed_bytes("mesh_select_mark", T * (4 + 24 + 12),
                    lambda: check(load().rx_mesh_select_mark(_ptr(t), T, V, _ptr(keep), _ptr(used), _ptr(flag), stream_ptr()), "rx_mesh_select_mark"))
    out_v, out_t, out_a, uoff = _compact(fn, t, V, None, V, keep, used, flag, v, attrs)      # the one device-to-host read
    row_of = torch.where(used != 0, uoff[:V], torch.full_like(uoff[:V], -1))
    return out_v, out_t, out_a, row_of
