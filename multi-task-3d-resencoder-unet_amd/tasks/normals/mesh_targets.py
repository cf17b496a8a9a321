"""Mesh targets: slice triangle meshes with every z-plane into the volumes the network trains on.

The reference makes its targets in three scripts (tasks/normals/write_face_normals_final.py, write_mesh_labels.py,
slices_to_zarr.py): per integer z, every triangle that reaches the plane is cut, the cut is drawn as a line, and the slices are
stacked into a `(Z, Y, X, 3)` uint16 normals volume, a `(Z, Y, X)` uint16 label volume or a uint8 sheet mask.  This module is the
host statement of that work, the definition of the order keys the device pass (csrc/rx_meshslice.hip) relies on, and the public
builder that writes the zarr stores `ZarrSegmentationDataset3D` reads.

WHAT IS PINNED.  `slice_normals_numpy` and `slice_labels_numpy` equal, bit for bit, what the reference's `process_slice_points` and
`process_slice_points_label` return when their text runs as plain Python under numpy 2 (tests/golden/mesh_slices.npz, made by
scripts/make_mesh_fixture.py, records the numpy version).  Every operation below names its dtype:

  normals  vertices, normals and z as float32.  An edge gives a point if an end lies on the plane (|z_v - z| <= float32(1e-8): the
           end itself with its UNNORMALISED normal), else if |dz| > float32(1e-8) and t = (z - z_s) / dz (float32) lies in
           [float32(-0.01), float32(1.01)]: p = s + t * (e - s), n = normalise(n_s + t * (n_e - n_s)), all float32.  A point closer
           than float32(1e-10) (squared, float32) to an earlier one is dropped.  Every pair (0,1), (0,2), (1,2) of the 2 or 3 points
           is a segment between the half-even rounded points; a segment with an end outside the image is dropped.
           steps = max(int(2 * sqrt(dx^2 + dy^2)), |dx|, |dy|) + 1 in float64; at step s, t = s / (steps - 1) (float64, 0 for one
           step), (x, y) = (x0 + t * dx, y0 + t * dy) in float64, n = normalise(float32(1 - t) * n0 + float32(t) * n1) in float32,
           where normalise divides by sqrt((n0^2 + n1^2) + n2^2) and passes a zero vector through.  Sample e of E = int(4 * eff + 1),
           eff = exp_factor * 1.2 (float64): u = (e / (E - 1)) * 2 - 1, pixel = half-even round of float32(x) + float32(u * eff) * n_x
           (float32), likewise y; painted, if inside the image, with uint16((n + 1) * 32767.5) (float32, truncated).
           The viz byte is `(rgb * 255) // 65535` in uint16, as numpy 2 computes it: the product wraps, so the byte is 1 where the
           code is 257 and 0 elsewhere.
  labels   float32 vertices, z an int64 (as the reference's main() passes it), so the plane tests run in float64: an end is on the
           plane if |z_v - z| < 1e-8; else dz = z_e - z_s (float32) must have |dz| >= float32(1e-15), t = (z - z_s) / dz in float64
           within [-1e-3, 1 + 1e-3], p = float32(s + t * (e - s)) with e - s in float32 and the rest in float64.  Duplicates at
           squared float32 distance < float32(1e-12).  A segment is a float32 DDA: steps = int(max(|dx|, |dy|)); one rounded point if
           0, else steps + 1 points with x_f += dx / steps accumulated step by step; each pixel is clipped on its own.
           (One expression differs in form: the reference squares the two float32 differences of the duplicate test with `** 2`,
           numpy's powf, which is not always the correctly rounded product; the statement multiplies.  The two can disagree only
           when the squared distance lies within an ulp of 1e-12.)

WHAT IS NOT.  numba compiles the reference's functions with its own type unification, which keeps float64 where numpy 2 keeps
float32 (`(1 - t) * n0`, `(normal + 1) * 32767.5`, `x + t_exp * eff * normal[0]`): a numba run may differ from the fixture in
the last unit of a few pixels, and numba is not available to find out.  `vertex_normals_numpy` stands in for open3d's
`compute_vertex_normals` (area-weighted: the normalised sum of the unnormalised face cross products) and is not compared with
open3d; callers may pass their own normals.  The TIFF slices are not written: the slices go straight into the zarr store.

THE ORDER KEYS.  The reference paints serially, so a pixel keeps its LAST writer.  Writers are ordered by (triangle, pair, step,
sample), hence the last writer is the largest such tuple, and the largest tuple is a maximum, which does not depend on the order
in which the writers arrive.  `key_pack_normals` packs the tuple into 64 bits, `(triangle + 1) << 26 | pair << 24 | step << 4 | e`
(0 = never painted); a label pixel is owned by its largest triangle index, a 32-bit key `triangle + 1`.  `resolve_*_numpy` recompute
a pixel's value from its key alone.  "Paint serially" and "take the maximum key, then resolve" give identical images; the device
pass is the second form with an integer atomic maximum.
"""
import glob as _glob
import json
import os

import numpy as np

F32 = np.float32
KEY_STEP_BITS, KEY_E_BITS, KEY_PAIR_BITS = 20, 4, 2
KEY_TRI_SHIFT = KEY_STEP_BITS + KEY_E_BITS + KEY_PAIR_BITS       # 26
KEY_PAIR_SHIFT = KEY_STEP_BITS + KEY_E_BITS                       # 24
KEY_MAX_STEPS = 1 << KEY_STEP_BITS
KEY_MAX_SAMPLES = 1 << KEY_E_BITS
KEY_MAX_TRIANGLES = (1 << 38) - 2
LABEL_KEY_MAX_TRIANGLES = (1 << 32) - 2
DEVICE_MAX_COORD = float(1 << 24)      # the device pass refuses |x|, |y| or |z| at or above this (int32 pixels, exact float32 z)
_PAIRS = ((0, 1), (0, 2), (1, 2))


class MeshTargetError(ValueError):
    pass


# ---- keys ----------------------------------------------------------------------------------------------------------------------
def key_pack_normals(tri, pair, step, e):
    if not 0 <= tri <= KEY_MAX_TRIANGLES - 1:
        raise MeshTargetError(f"triangle index {tri} does not fit the 38-bit key field (at most {KEY_MAX_TRIANGLES} triangles)")
    if not 0 <= pair < 3:
        raise MeshTargetError(f"pair {pair} out of range")
    if not 0 <= step < KEY_MAX_STEPS:
        raise MeshTargetError(f"a segment of {step + 1} or more steps does not fit the key (fewer than {KEY_MAX_STEPS})")
    if not 0 <= e < KEY_MAX_SAMPLES:
        raise MeshTargetError(f"expansion sample {e} does not fit the key (at most {KEY_MAX_SAMPLES} samples)")
    return ((int(tri) + 1) << KEY_TRI_SHIFT) | (int(pair) << KEY_PAIR_SHIFT) | (int(step) << KEY_E_BITS) | int(e)


def key_unpack_normals(key):
    """-> (triangle, pair, step, e) of a non-zero key"""
    key = int(key)
    if key <= 0:
        raise MeshTargetError("key 0 is the empty pixel")
    return ((key >> KEY_TRI_SHIFT) - 1, (key >> KEY_PAIR_SHIFT) & 3, (key >> KEY_E_BITS) & (KEY_MAX_STEPS - 1), key & (KEY_MAX_SAMPLES - 1))


def key_pack_label(tri):
    if not 0 <= tri <= LABEL_KEY_MAX_TRIANGLES - 1:
        raise MeshTargetError(f"triangle index {tri} does not fit the 32-bit label key (at most {LABEL_KEY_MAX_TRIANGLES} triangles)")
    return int(tri) + 1


def key_unpack_label(key):
    key = int(key)
    if key <= 0:
        raise MeshTargetError("key 0 is the empty pixel")
    return key - 1


def expansion_samples(exp_factor):
    """(eff, E): the float64 effective factor and the number of samples across the line; refuses what cannot be drawn or keyed"""
    eff = float(exp_factor) * 1.2
    if not np.isfinite(eff) or eff < 0:
        raise MeshTargetError(f"exp_factor {exp_factor} must be finite and not negative")
    n = int(4 * eff + 1)
    if n < 2:
        raise MeshTargetError(f"exp_factor {exp_factor} gives {n} expansion sample: the reference divides by samples - 1")
    if n > KEY_MAX_SAMPLES:
        raise MeshTargetError(f"exp_factor {exp_factor} gives {n} expansion samples, the key holds {KEY_MAX_SAMPLES}")
    return eff, n


def check_mesh(vertices, triangles, normals=None, tri_labels=None, label_keys=False):
    """the refusals shared by the statement and the device pass -> (float32 vertices, int64 triangles, ...)"""
    v = np.asarray(vertices)
    t = np.asarray(triangles)
    if v.ndim != 2 or v.shape[1] != 3:
        raise MeshTargetError(f"vertices must be (n, 3), got {v.shape}")
    if t.ndim != 2 or t.shape[1] != 3 or t.dtype.kind not in "iu":
        raise MeshTargetError(f"triangles must be an integer (m, 3) array, got {t.dtype} {t.shape}")
    v = v.astype(F32)
    t = t.astype(np.int64)
    if not np.isfinite(v).all():
        raise MeshTargetError("vertices must be finite")
    if t.size and (t.min() < 0 or t.max() >= len(v)):
        raise MeshTargetError(f"triangle indices must lie in [0, {len(v)})")
    if len(t) > (LABEL_KEY_MAX_TRIANGLES if label_keys else KEY_MAX_TRIANGLES):
        raise MeshTargetError(f"{len(t)} triangles do not fit the order key")
    out = [v, t]
    if normals is not None:
        n = np.asarray(normals)
        if n.shape != v.shape:
            raise MeshTargetError(f"vertex normals must be {v.shape}, got {n.shape}")
        n = n.astype(F32)
        if not np.isfinite(n).all():
            raise MeshTargetError("vertex normals must be finite")
        out.append(n)
    if tri_labels is not None:
        lab = np.asarray(tri_labels)
        if lab.shape != (len(t),) or lab.dtype.kind not in "iu" or (lab.size and (lab.min() < 0 or lab.max() > 65535)):
            raise MeshTargetError(f"tri_labels must be ({len(t)},) integers in [0, 65535]")
        out.append(lab.astype(np.uint16))
    return out


def _window(window, w, h):
    if window is None:
        return 0, 0, h, w
    y0, x0, wh, ww = (int(a) for a in window)
    if y0 < 0 or x0 < 0 or wh < 1 or ww < 1 or y0 + wh > h or x0 + ww > w:
        raise MeshTargetError(f"window (y0, x0, wh, ww) = {(y0, x0, wh, ww)} does not lie inside the {w} x {h} image")
    return y0, x0, wh, ww


def _rint(x):
    """int(round(np.float32)): half to even"""
    return int(np.rint(x))


# ---- normals: the statement ----------------------------------------------------------------------------------------------------
def _normalise(v):
    q = v * v
    s = (q[0] + q[1]) + q[2]
    norm = np.sqrt(s)
    if norm == 0:
        return v
    return v / norm


def _edge_point_normals(s, e, ns, ne, zf):
    if abs(s[2] - zf) <= F32(1e-8):
        return s[:2], ns
    if abs(e[2] - zf) <= F32(1e-8):
        return e[:2], ne
    dz = e[2] - s[2]
    if abs(dz) <= F32(1e-8):
        return None, None
    t = (zf - s[2]) / dz
    if not (F32(-0.01) <= t <= F32(1.01)):
        return None, None
    p = s + t * (e - s)
    n = ns + t * (ne - ns)
    return p[:2], _normalise(n)


def _tri_segments_normals(v, nrm, tri, zf, w, h):
    """the segments triangle `tri` draws in slice zf: [(pair, x0, y0, x1, y1, n_a, n_b)]"""
    a, b, c = tri
    v0, v1, v2 = v[a], v[b], v[c]
    if not (min(v0[2], v1[2], v2[2]) <= zf <= max(v0[2], v1[2], v2[2])):
        return []
    n0, n1, n2 = nrm[a], nrm[b], nrm[c]
    pts, nrs = [], []
    for s, e, ns, ne in ((v0, v1, n0, n1), (v1, v2, n1, n2), (v2, v0, n2, n0)):
        p, n = _edge_point_normals(s, e, ns, ne, zf)
        if p is None:
            continue
        dup = False
        for q in pts:
            d = p - q
            d = d * d
            if d[0] + d[1] < F32(1e-10):
                dup = True
                break
        if not dup:
            pts.append(p)
            nrs.append(n)
    out = []
    if len(pts) >= 2:
        k = 0
        for i in range(len(pts)):
            for j in range(i + 1, len(pts)):
                pair = k
                k += 1
                x0, y0, x1, y1 = _rint(pts[i][0]), _rint(pts[i][1]), _rint(pts[j][0]), _rint(pts[j][1])
                if 0 <= x0 < w and 0 <= y0 < h and 0 <= x1 < w and 0 <= y1 < h:
                    out.append((pair, x0, y0, x1, y1, nrs[i], nrs[j]))
    return out


def _segment_steps(x0, y0, x1, y1):
    dx, dy = x1 - x0, y1 - y0
    dist = np.sqrt(np.float64(dx * dx + dy * dy))
    return max(int(dist * np.float64(2.0)), max(abs(dx), abs(dy))) + 1


def _step_state(x0, y0, x1, y1, na, nb, steps, step):
    """-> (x, y) float64 and the float32 unit normal at `step`"""
    t = np.float64(step) / np.float64(steps - 1) if steps > 1 else np.float64(0.0)
    x = np.float64(x0) + t * np.float64(x1 - x0)
    y = np.float64(y0) + t * np.float64(y1 - y0)
    n = F32(np.float64(1.0) - t) * na + F32(t) * nb
    return x, y, _normalise(n)


def _rgb(n):
    return ((n + F32(1.0)) * F32(32767.5)).astype(np.uint16)


def _viz(rgb):
    return ((rgb * np.uint16(255)) // np.uint16(65535)).astype(np.uint8)


def _normals_events(v, tris, nrm, z, w, h, exp_factor):
    """every paint of slice z in the reference's order: (triangle, pair, step, e, x, y, rgb)"""
    eff, n_exp = expansion_samples(exp_factor)
    zf = F32(z)
    for ti in range(len(tris)):
        for pair, x0, y0, x1, y1, na, nb in _tri_segments_normals(v, nrm, tris[ti], zf, w, h):
            steps = _segment_steps(x0, y0, x1, y1)
            for step in range(steps):
                x, y, n = _step_state(x0, y0, x1, y1, na, nb, steps, step)
                rgb = None
                for e in range(n_exp):
                    u = (np.float64(e) / np.float64(n_exp - 1)) * np.float64(2.0) - np.float64(1.0)
                    off = F32(u * np.float64(eff))
                    ex = _rint(F32(x) + off * n[0])
                    ey = _rint(F32(y) + off * n[1])
                    if 0 <= ex < w and 0 <= ey < h:
                        if rgb is None:
                            rgb = _rgb(n)
                        yield ti, pair, step, e, ex, ey, rgb


def slice_normals_numpy(vertices, triangles, vertex_normals, z, w, h, exp_factor=1.5, return_viz=False):
    """one slice painted serially, as the reference does -> (h, w, 3) uint16 [, (h, w, 3) uint8 viz]"""
    v, t, n = check_mesh(vertices, triangles, vertex_normals)
    img = np.zeros((h, w, 3), np.uint16)
    for _, _, _, _, x, y, rgb in _normals_events(v, t, n, z, w, h, exp_factor):
        img[y, x] = rgb
    return (img, _viz(img)) if return_viz else img


def keys_normals_numpy(vertices, triangles, vertex_normals, z, w, h, exp_factor=1.5, window=None):
    """the largest key per pixel of slice z, window pixels only -> (wh, ww) uint64"""
    v, t, n = check_mesh(vertices, triangles, vertex_normals)
    y0, x0, wh, ww = _window(window, w, h)
    keys = np.zeros((wh, ww), np.uint64)
    for ti, pair, step, e, x, y, _ in _normals_events(v, t, n, z, w, h, exp_factor):
        k = key_pack_normals(ti, pair, step, e)
        if y0 <= y < y0 + wh and x0 <= x < x0 + ww and k > keys[y - y0, x - x0]:
            keys[y - y0, x - x0] = k
    return keys


def resolve_normals_numpy(keys, vertices, triangles, vertex_normals, z, w, h, return_viz=False):
    """the image of a key plane: every value recomputed from (triangle, pair, step) alone"""
    v, t, n = check_mesh(vertices, triangles, vertex_normals)
    keys = np.asarray(keys)
    img = np.zeros(keys.shape + (3,), np.uint16)
    zf = F32(z)
    for y, x in zip(*np.nonzero(keys)):
        ti, pair, step, _ = key_unpack_normals(keys[y, x])
        seg = [s for s in _tri_segments_normals(v, n, t[ti], zf, w, h) if s[0] == pair]
        if len(seg) != 1:
            raise MeshTargetError(f"key {int(keys[y, x]):#x} names a segment triangle {ti} does not draw in slice {z}")
        _, sx0, sy0, sx1, sy1, na, nb = seg[0]
        steps = _segment_steps(sx0, sy0, sx1, sy1)
        img[y, x] = _rgb(_step_state(sx0, sy0, sx1, sy1, na, nb, steps, step)[2])
    return (img, _viz(img)) if return_viz else img


# ---- labels: the statement -----------------------------------------------------------------------------------------------------
def _edge_point_labels(s, e, z):
    zp = np.float64(z)
    if abs(np.float64(s[2]) - zp) < np.float64(1e-8):
        return s[:2]
    if abs(np.float64(e[2]) - zp) < np.float64(1e-8):
        return e[:2]
    dz = e[2] - s[2]
    if abs(dz) < F32(1e-15):
        return None
    t = (zp - np.float64(s[2])) / np.float64(dz)
    if not (np.float64(0.0 - 1e-3) <= t <= np.float64(1.0 + 1e-3)):
        return None
    x = np.float64(s[0]) + t * np.float64(e[0] - s[0])
    y = np.float64(s[1]) + t * np.float64(e[1] - s[1])
    return np.array([x, y], dtype=F32)


def _tri_points_labels(v, tri, z):
    a, b, c = tri
    v0, v1, v2 = v[a], v[b], v[c]
    zp = np.float64(z)
    if not (np.float64(min(v0[2], v1[2], v2[2])) <= zp <= np.float64(max(v0[2], v1[2], v2[2]))):
        return []
    pts = []
    for s, e in ((v0, v1), (v1, v2), (v2, v0)):
        p = _edge_point_labels(s, e, z)
        if p is None:
            continue
        dup = False
        for q in pts:
            dx, dy = p[0] - q[0], p[1] - q[1]
            if dx * dx + dy * dy < F32(1e-12):
                dup = True
                break
        if not dup:
            pts.append(p)
    return pts


def _label_line(p, q):
    """the pixels of one segment, unclipped, in drawing order"""
    x0, y0, x1, y1 = p[0], p[1], q[0], q[1]
    dx, dy = x1 - x0, y1 - y0
    steps = int(max(abs(dx), abs(dy)))
    if steps == 0:
        yield _rint(x0), _rint(y0)
        return
    x_inc, y_inc = dx / F32(steps), dy / F32(steps)
    xf, yf = x0, y0
    for _ in range(steps + 1):
        yield _rint(xf), _rint(yf)
        xf = xf + x_inc
        yf = yf + y_inc


def _labels_events(v, tris, z, w, h):
    """every paint of slice z in the reference's order: (triangle, x, y)"""
    for ti in range(len(tris)):
        pts = _tri_points_labels(v, tris[ti], z)
        for i in range(len(pts)):
            for j in range(i + 1, len(pts)):
                for x, y in _label_line(pts[i], pts[j]):
                    if 0 <= x < w and 0 <= y < h:
                        yield ti, x, y


def slice_labels_numpy(vertices, triangles, tri_labels, z, w, h):
    """one label slice painted serially, as the reference does -> (h, w) uint16.  `z` is an integer (the reference passes np.int64)"""
    v, t, lab = check_mesh(vertices, triangles, tri_labels=tri_labels, label_keys=True)
    z = np.int64(z)
    img = np.zeros((h, w), np.uint16)
    for ti, x, y in _labels_events(v, t, z, w, h):
        img[y, x] = lab[ti]
    return img


def keys_labels_numpy(vertices, triangles, z, w, h, window=None):
    """the largest key (triangle + 1) per pixel of slice z, window pixels only -> (wh, ww) uint32"""
    v, t = check_mesh(vertices, triangles, label_keys=True)
    y0, x0, wh, ww = _window(window, w, h)
    keys = np.zeros((wh, ww), np.uint32)
    for ti, x, y in _labels_events(v, t, np.int64(z), w, h):
        k = key_pack_label(ti)
        if y0 <= y < y0 + wh and x0 <= x < x0 + ww and k > keys[y - y0, x - x0]:
            keys[y - y0, x - x0] = k
    return keys


def resolve_labels_numpy(keys, tri_labels):
    keys = np.asarray(keys).astype(np.int64)
    lab = np.asarray(tri_labels).astype(np.uint16)
    return np.where(keys > 0, lab[np.maximum(keys - 1, 0)] if lab.size else 0, 0).astype(np.uint16)


def binary_mask_numpy(img, channels_last=True):
    """slices_to_zarr --binary: 255 where any channel of a (..., 3) normals image (or, channels_last=False, the label) is non-zero"""
    img = np.asarray(img)
    nz = (img > 0).any(axis=-1) if channels_last else img > 0
    return nz.astype(np.uint8) * np.uint8(255)


# ---- volumes on the host -------------------------------------------------------------------------------------------------------
def normals_volume_numpy(vertices, triangles, vertex_normals, w, h, z0, nz, window=None, exp_factor=1.5):
    """slices z0 .. z0 + nz - 1, cropped to the window -> (nz, wh, ww, 3) uint16"""
    y0, x0, wh, ww = _window(window, w, h)
    out = np.zeros((nz, wh, ww, 3), np.uint16)
    for k in range(nz):
        out[k] = slice_normals_numpy(vertices, triangles, vertex_normals, z0 + k, w, h, exp_factor)[y0:y0 + wh, x0:x0 + ww]
    return out


def labels_volume_numpy(vertices, triangles, tri_labels, w, h, z0, nz, window=None):
    y0, x0, wh, ww = _window(window, w, h)
    out = np.zeros((nz, wh, ww), np.uint16)
    for k in range(nz):
        out[k] = slice_labels_numpy(vertices, triangles, tri_labels, z0 + k, w, h)[y0:y0 + wh, x0:x0 + ww]
    return out


# ---- meshes --------------------------------------------------------------------------------------------------------------------
def read_obj(path):
    """`v` and `f` lines of a Wavefront OBJ -> (float32 (n, 3) vertices, int64 (m, 3) triangles).  Polygons are fanned from their
    first corner; `a`, `a/b`, `a//c` and `a/b/c` corners and negative (relative) indices are accepted; everything else is skipped."""
    verts, tris = [], []
    with open(path) as f:
        for lineno, line in enumerate(f, 1):
            parts = line.split()
            if not parts:
                continue
            if parts[0] == "v":
                if len(parts) < 4:
                    raise MeshTargetError(f"{path}:{lineno}: a vertex needs three coordinates")
                verts.append([float(parts[1]), float(parts[2]), float(parts[3])])
            elif parts[0] == "f":
                idx = []
                for corner in parts[1:]:
                    i = int(corner.split("/")[0])
                    i = i - 1 if i > 0 else len(verts) + i
                    if i < 0 or i >= len(verts) or corner.split("/")[0] == "0":
                        raise MeshTargetError(f"{path}:{lineno}: corner {corner} names no vertex read so far")
                    idx.append(i)
                if len(idx) < 3:
                    raise MeshTargetError(f"{path}:{lineno}: a face needs three corners")
                for k in range(1, len(idx) - 1):
                    tris.append([idx[0], idx[k], idx[k + 1]])
    return np.asarray(verts, F32).reshape(-1, 3), np.asarray(tris, np.int64).reshape(-1, 3)


def vertex_normals_numpy(vertices, triangles):
    """area-weighted vertex normals: per vertex the sum of the unnormalised cross products (v1 - v0) x (v2 - v0) of its faces,
    normalised, float32 (a vertex of no face, or whose sum is zero, gets the zero vector).  This stands in for open3d's
    `compute_vertex_normals`, which is NOT available to compare with: the one function of this module that is not pinned."""
    v, t = check_mesh(vertices, triangles)
    a, b, c = v[t[:, 0]], v[t[:, 1]], v[t[:, 2]]
    face = np.cross(b - a, c - a).astype(F32)
    acc = np.zeros_like(v)
    for k in range(3):
        np.add.at(acc, t[:, k], face)
    norm = np.sqrt((acc * acc).sum(axis=1, dtype=F32))
    out = np.zeros_like(acc)
    np.divide(acc, norm[:, None], out=out, where=norm[:, None] > 0)
    return out


def merge_meshes(meshes):
    """[(vertices, triangles[, normals])] -> vertices, triangles (indices offset), normals, tri_labels (mesh i paints label i + 1)"""
    vs, ts, ns, ls, off = [], [], [], [], 0
    for i, m in enumerate(meshes):
        v, t = check_mesh(m[0], m[1])
        n = np.asarray(m[2], F32) if len(m) > 2 and m[2] is not None else vertex_normals_numpy(v, t)
        if n.shape != v.shape:
            raise MeshTargetError(f"mesh {i}: normals {n.shape} for vertices {v.shape}")
        if i + 1 > 65535:
            raise MeshTargetError("more than 65535 meshes: the label is a uint16")
        vs.append(v), ts.append(t + off), ns.append(n), ls.append(np.full(len(t), i + 1, np.uint16))
        off += len(v)
    if not vs:
        raise MeshTargetError("no meshes")
    return np.vstack(vs), np.vstack(ts), np.vstack(ns), np.concatenate(ls)


# ---- the builder ---------------------------------------------------------------------------------------------------------------
class MeshTargetBuilder:
    """Meshes -> the zarr stores the dataset reads.

    meshes     a list of OBJ paths or of (vertices, triangles[, vertex_normals]) tuples; mesh i paints label i + 1
    shape_zyx  (Z, h, w): Z slices of the full w x h image; volume index k is slice min_z + k
    slab       slices per device pass (the key buffer holds slab * window pixels); the default is one chunk row
    window     (y0, x0, wh, ww): store only this part of every slice (the store is then (Z, wh, ww)); None = the image
    where      "device": csrc/rx_meshslice.hip through engine/ops/mesh.py; "host": the numpy statement

    `normals_volume`, `labels_volume` and `sheet_mask` each write a zarr v2 GROUP at `path` with the array `volume` (chunks
    (128, 128, 128[, 3])) and the attributes slices_to_zarr.py writes.  The sheet mask is `slices_to_zarr --binary` over the normals
    slices: uint8, 255 where any channel is non-zero."""

    CHUNK = 128

    def __init__(self, meshes, shape_zyx, slab=None, window=None, min_z=0, exp_factor=1.5, where="device", compressor=None):
        if where not in ("device", "host"):
            raise MeshTargetError(f"where must be \"device\" or \"host\", got {where!r}")
        loaded = []
        for m in meshes:
            if isinstance(m, (str, os.PathLike)):
                m = read_obj(m)
            loaded.append(tuple(m))
        self.vertices, self.triangles, self.normals, self.tri_labels = merge_meshes(loaded)
        self.Z, self.h, self.w = (int(s) for s in shape_zyx)
        if self.Z < 1 or self.h < 1 or self.w < 1:
            raise MeshTargetError(f"shape_zyx {shape_zyx} must be positive")
        self.window = _window(window, self.w, self.h)
        self.min_z = int(min_z)
        self.slab = self.CHUNK if slab is None else int(slab)
        if self.slab < 1:
            raise MeshTargetError("slab must be positive")
        self.exp_factor = float(exp_factor)
        expansion_samples(self.exp_factor)
        self.where, self.compressor = where, compressor
        self._dev = None

    # one slab of slices [z, z + n) as numpy
    def _device_mesh(self):
        if self._dev is None:
            import torch
            dev = torch.device("cuda")
            self._dev = (torch.from_numpy(self.vertices).to(dev), torch.from_numpy(self.triangles.astype(np.int32)).to(dev),
                         torch.from_numpy(self.normals).to(dev), torch.from_numpy(self.tri_labels.astype(np.int32)).to(dev))
        return self._dev

    def _slab(self, kind, z, n):
        if self.where == "host":
            if kind == "labels":
                return labels_volume_numpy(self.vertices, self.triangles, self.tri_labels, self.w, self.h, z, n, self.window)
            vol = normals_volume_numpy(self.vertices, self.triangles, self.normals, self.w, self.h, z, n, self.window, self.exp_factor)
            return vol if kind == "normals" else binary_mask_numpy(vol)
        from ...engine import ops
        v, t, nrm, lab = self._device_mesh()
        if kind == "labels":
            return ops.mesh_slice_labels(v, t, lab, self.w, self.h, z, n, window=self.window)["labels"].cpu().numpy()
        r = ops.mesh_slice_normals(v, t, nrm, self.w, self.h, z, n, window=self.window, exp_factor=self.exp_factor,
                                   want_mask=kind == "mask")
        return r["normals" if kind == "normals" else "mask"].cpu().numpy()

    def _write(self, path, kind):
        from ...dataloading.zarr_lite import ChunkedWriter
        path = str(path)
        if os.path.exists(path):
            raise FileExistsError(f"{path} already exists")
        _, _, wh, ww = self.window
        c = self.CHUNK
        if kind == "normals":
            shape, chunks, dtype = (self.Z, wh, ww, 3), (c, c, c, 3), np.uint16
        else:
            shape, chunks, dtype = (self.Z, wh, ww), (c, c, c), np.uint16 if kind == "labels" else np.uint8
        os.makedirs(path)
        with open(os.path.join(path, ".zgroup"), "w") as f:
            json.dump({"zarr_format": 2}, f)
        writer = ChunkedWriter(os.path.join(path, "volume"), shape, chunks, dtype, compressor=self.compressor, axis=0)
        painted = 0
        for k0 in range(0, self.Z, c):                      # a chunk row of the store at a time, filled slab by slab
            rows = min(c, self.Z - k0)
            block = np.zeros((rows,) + shape[1:], dtype)
            for s0 in range(0, rows, self.slab):
                n = min(self.slab, rows - s0)
                block[s0:s0 + n] = self._slab(kind, self.min_z + k0 + s0, n)
            painted += int(block.reshape(rows, -1).any(axis=1).sum())
            writer.write_rows(k0, block)
        attrs = {"n_channels": 3 if kind != "labels" else 1, "dimensions": ["z", "y", "x", "c"] if kind == "normals" else ["z", "y", "x"],
                 "min_z": self.min_z, "max_z": self.min_z + self.Z - 1, "processed_files": painted, "total_slices": self.Z,
                 "chunk_size": list(chunks)}
        with open(os.path.join(path, ".zattrs"), "w") as f:
            json.dump(attrs, f)
        return os.path.join(path, "volume")

    def normals_volume(self, path):
        """(Z, wh, ww, 3) uint16 -> the path of the array inside the group"""
        return self._write(path, "normals")

    def labels_volume(self, path):
        """(Z, wh, ww) uint16 instance labels"""
        return self._write(path, "labels")

    def sheet_mask(self, path):
        """(Z, wh, ww) uint8, 255 on the painted normals voxels"""
        return self._write(path, "mask")


def expand_mesh_args(args):
    """OBJ paths and glob patterns -> a sorted list of paths"""
    out = []
    for a in args:
        hits = sorted(_glob.glob(a)) if any(ch in a for ch in "*?[") else [a]
        if not hits:
            raise MeshTargetError(f"{a}: no file matches")
        out.extend(hits)
    return out
