"""The planning side of sliding-window inference: pure functions of shapes, options and numpy arrays (no torch, no device).

Patch positions, the Gaussian importance map, the views of test-time augmentation, the streaming schedule, the Y/X tiles, the
empty-patch rule and the output rule of a task.  `inference.py` holds the two inferers that run what is planned here and
re-exports every public name of this module.
"""
import itertools
from typing import Dict, Sequence

import numpy as np

from .dataloading.geometry_device import AXIS_OF, GeomOp, allowed_rot90_axes, compose, flip_op, rot90_op


def generate_positions(min_val: int, max_val: int, patch_size: int, step: int):
    """start indices of sliding-window patches; the last patch is forced to end at `max_val` (helpers.py:200-216)"""
    if patch_size > max_val - min_val:
        raise ValueError(f"patch ({patch_size}) larger than the volume extent ({max_val - min_val})")
    positions = []
    pos = min_val
    while pos + patch_size <= max_val:
        positions.append(pos)
        pos += step
    last = max_val - patch_size
    if last > positions[-1]:
        positions.append(last)
    return sorted(set(positions))


def all_positions(shape: Sequence[int], patch: Sequence[int], overlap: float):
    """(z, y, x) patch origins, z-major; step = patch * (1 - overlap) per axis, at least 1"""
    axes = []
    for dim, p in zip(shape, patch):
        step = max(1, int(round(p * (1.0 - overlap))))
        axes.append(generate_positions(0, dim, p, step))
    return [(z, y, x) for z in axes[0] for y in axes[1] for x in axes[2]]


def task_output_rule(name, channels):
    """THE rule of the reference's overlap pass and cast (inference.py:166-210, 251-263), by target name and channel count:
    -> (blend, cast, host dtype, is_vector_default).  A target named `normals` is cast `(v+1)/2*65535` -> uint16 and, with 3
    channels, is a unit-vector field: re-normalised `sum / (|sum| + 1e-8)` ("unit"), its components following the sign rule
    of test-time augmentation by default; with another channel count it is left as summed ("none").  Everything else is
    averaged `sum / count` ("average") and cast `v*255` -> uint8."""
    if str(name).lower() == "normals":
        unit = int(channels) == 3
        return ("unit" if unit else "none"), "u16", np.dtype(np.uint16), unit
    return "average", "u8", np.dtype(np.uint8), False


# ---- Gaussian importance map (reference inference/helpers.py:8-91) -------------------------------------------------------------
def _gaussian_kernel1d(sigma: float, radius: int) -> np.ndarray:
    """scipy.ndimage's order-0 kernel: exp(-x^2 / 2 sigma^2) on [-radius, radius], normalised, float64"""
    x = np.arange(-radius, radius + 1)
    phi = np.exp(-0.5 / (sigma * sigma) * x ** 2)
    return phi / phi.sum()


def gaussian_importance_map(patch: Sequence[int], sigma_scale: float = 1.0 / 8, value_scaling_factor: float = 1.0) -> np.ndarray:
    """float32 (pz, py, px) blending weights: `compute_gaussian_3d` (helpers.py:8-68) without scipy.

    The reference filters a unit delta at `dim // 2` with `scipy.ndimage.gaussian_filter(sigma = dim * sigma_scale,
    mode='constant')`.  For a delta that filter is separable and exact to restate: scipy runs one 1-D pass per axis (axis 0 first;
    axes with sigma <= 1e-15 skipped), each pass sums in float64 with the kernel of `_gaussian_kernel1d` (radius
    int(4 sigma + 0.5)) and rounds to the float32 output; along a line with one non-zero value the sum IS that value times one tap.
    So pass k turns the float32 result of pass k-1 into float32(float64(v) * w_k[i]), which is what is computed here.  Then, as the
    reference: divide by the max over the peak value, replace exact zeros by the smallest positive value."""
    patch = tuple(int(d) for d in patch)
    g = np.ones((1,) * len(patch), dtype=np.float32)
    for axis, dim in enumerate(patch):
        sigma = dim * sigma_scale
        line = np.zeros(dim, dtype=np.float64)
        c = dim // 2
        if sigma > 1e-15:
            radius = int(4.0 * float(sigma) + 0.5)
            k = _gaussian_kernel1d(float(sigma), radius)
            lo, hi = max(0, c - radius), min(dim, c + radius + 1)
            line[lo:hi] = k[lo - c + radius:hi - c + radius]
        else:
            line[c] = 1.0
        shape = [1] * len(patch)
        shape[axis] = dim
        g = (g.astype(np.float64) * line.reshape(shape)).astype(np.float32)
    g /= (g.max() / value_scaling_factor)
    g[g == 0] = g[g > 0].min()
    return np.ascontiguousarray(g)


# ---- test-time augmentation: the views of a patch -------------------------------------------------------------------------
TTA_MAX_VIEWS = 48          # the signed permutations of three axes: every flip / 90-degree rotation of a cube


def default_normal_keys(tasks) -> tuple:
    """the tasks whose predictions are surface normals: lower-case name `normals` and 3 channels (`task_output_rule`)"""
    return tuple(n for n, t in (tasks or {}).items() if task_output_rule(n, t.get("channels", 0))[3])


def _tta_axes(owner, v):
    axes = [str(a).lower() for a in (v if not isinstance(v, str) else list(v))] if v is not None else []
    if any(a not in ("z", "y", "x") for a in axes) or len(set(axes)) != len(axes):
        raise ValueError(f"{owner}: {v!r} (a list of distinct axes out of z, y, x)")
    return axes


def tta_views(spec, patch, tasks=None, normal_keys=None) -> tuple:
    """The views of test-time augmentation, a tuple of `GeomOp` (dataloading.geometry_device); pure, no device.

    spec  None / False: off, `(GeomOp(),)`.  "flip": shorthand for {"flip": ["z", "y", "x"]}.
          {"flip": [axes], "rot90": [axes]} (either key may be absent): for every flip combination -- binary counting order over
          the listed axes, bit i = the i-th listed axis, combination 0 the identity -- every rotation chain, the first listed
          rotation axis outermost and k = 0..3 quarter turns per axis (applied in the listed order); a view is
          `compose(flip_combo, rot_chain)`.  Or an explicit sequence of `GeomOp` (Python only).
          Duplicates are dropped (the first occurrence stays), so view 0 of a mapping is the identity; flips over z, y, x give 8
          views, with rotations about z 16, with rotations about all three axes the whole group of 48.
    Refused, with the offending key named: unknown keys, a rotation axis whose plane has unequal patch extents, an explicit op
    that would change the patch shape, a task of `normal_keys` without 3 channels, more than 48 views.  `normal_keys`
    (default: `default_normal_keys(tasks)`) names the tasks un-transformed with the component and sign rule."""
    patch = tuple(int(v) for v in patch)
    if len(patch) != 3:
        raise ValueError(f"tta: needs a 3-D patch, patch_size is {list(patch)}")
    nk = default_normal_keys(tasks) if normal_keys is None else ((normal_keys,) if isinstance(normal_keys, str) else tuple(normal_keys))
    for k in nk:
        if tasks is not None and k not in tasks:
            raise ValueError(f"tta normal_keys: {k!r} is not a task (tasks: {sorted(tasks)})")
        if tasks is not None and int(tasks[k].get("channels", 0)) != 3:
            raise ValueError(f"tta normal_keys: task {k!r} has channels = {tasks[k].get('channels')}, a normals prediction has 3")
    if spec is None or spec is False:
        return (GeomOp(),)
    if isinstance(spec, str):
        if spec.lower() != "flip":
            raise ValueError(f"tta: {spec!r} (\"flip\", a mapping with the keys flip / rot90, or a sequence of GeomOp)")
        spec = {"flip": ["z", "y", "x"]}
    if isinstance(spec, dict):
        unknown = set(spec) - {"flip", "rot90"}
        if unknown:
            raise ValueError(f"tta: unknown key(s) {sorted(str(k) for k in unknown)} (known: flip, rot90)")
        flips, rots = _tta_axes("tta.flip", spec.get("flip")), _tta_axes("tta.rot90", spec.get("rot90"))
        allowed = allowed_rot90_axes(patch)
        wrong = [a for a in rots if a not in allowed]
        if wrong:
            raise ValueError(f"tta.rot90: a rotation about {wrong} turns a plane of unequal extents of the patch {list(patch)} and "
                             f"would change its shape; axes this patch allows: {list(allowed)}")
        views = []
        for m in range(1 << len(flips)):
            f = GeomOp()
            for i, a in enumerate(flips):
                if (m >> i) & 1:
                    f = compose(f, flip_op(AXIS_OF[a]))
            for ks in itertools.product(range(4), repeat=len(rots)):
                r = GeomOp()
                for a, k in zip(rots, ks):
                    if k:
                        r = compose(r, rot90_op(a, k))
                views.append(compose(f, r))
    else:
        try:
            views = list(spec)
        except TypeError:
            raise ValueError(f"tta: {spec!r} (\"flip\", a mapping with the keys flip / rot90, or a sequence of GeomOp)") from None
        if not views or not all(isinstance(v, GeomOp) for v in views):
            raise ValueError("tta: an explicit view list is a non-empty sequence of GeomOp")
        for i, v in enumerate(views):
            if not v.preserves(patch):
                raise ValueError(f"tta: view {i} {v} would change the shape of the patch {list(patch)}; rotation axes this patch "
                                 f"allows: {list(allowed_rot90_axes(patch))}")
    out = tuple(dict.fromkeys(views))
    if len(out) > TTA_MAX_VIEWS:
        raise ValueError(f"tta: {len(out)} distinct views, at most {TTA_MAX_VIEWS}")
    return out


# ---- streaming schedule ------------------------------------------------------------------------------------------------------
def cut_batches(positions, B: int, n_views: int = 1):
    """the (position, view) slots of one z-row, position-major and view-minor, cut into batches of B; the last batch is padded by
    repeating its last slot.  Returns (batches, views) as `stream_schedule` lists them; no positions, no batches."""
    batches, views = [], []
    slots = [(p, v) for p in positions for v in range(int(n_views))]
    for i in range(0, len(slots), B):
        chunk = slots[i:i + B]
        chunk_p, chunk_v = [p for p, _ in chunk], [v for _, v in chunk]
        batches.append((tuple(chunk_p) + (chunk_p[-1],) * (B - len(chunk)), len(chunk)))
        views.append(tuple(chunk_v) + (chunk_v[-1],) * (B - len(chunk)))
    return batches, views


def row_positions(step) -> list:
    """the positions of one step of `stream_schedule`, each once, in the order they run"""
    return list(dict.fromkeys(p for chunk, valid in step["batches"] for p in chunk[:valid]))


def _slab_bytes(patch, plane: int, max_fin: int, B: int, cin: int, in_itemsize: int, acc_channels: int, out_bytes_per_voxel: int):
    """the device bytes of one slab of `plane` = Y * X voxels per row (the formulas of `stream_schedule`)"""
    pz = int(patch[0])
    acc = pz * plane * 4 * (int(acc_channels) + 1)
    inp = int(cin) * pz * plane * int(in_itemsize)
    staging = max_fin * plane * int(out_bytes_per_voxel)
    patch_b = B * int(cin) * int(np.prod(patch)) * 4
    return dict(accumulator_bytes=acc, input_bytes=inp, staging_bytes=staging, patch_bytes=patch_b,
                device_bytes=acc + inp + staging + patch_b)


def stream_schedule(shape: Sequence[int], patch: Sequence[int], overlap: float, batch_size: int, cin: int = 1,
                    in_itemsize: int = 1, acc_channels: int = 1, out_bytes_per_voxel: int = 0, n_views: int = 1,
                    positions=None) -> dict:
    """Positions -> the order of work of `StreamingInferer`, one step per z-origin z_k (all_positions is z-major):

      load      input rows [lo, hi) to bring to the device (hi = z_k + pz; rows already there are not read again)
      batches   [(B positions, valid)] of the patches at z_k; the last is padded by repeating its last patch (one plan shape)
      views     parallel to `batches`: per batch, the B view indices of its slots.  With `n_views` = V > 1 (test-time
                augmentation) the slots of a z-row are its (position, view) pairs, position-major and view-minor, cut into
                batches of B -- so `batches` repeats every position V times -- and the last batch repeats its last slot
      finalize  rows [lo, hi) no later patch touches (hi = z_{k+1}, the volume end at the last step): blended, cast, copied out
      write     output rows [lo, hi) whose chunk rows (chunk = patch) are now complete

    Device arrays are rings of `ring` = pz rows (the rows [z_k, z_k + pz) are the only ones live at step k: rows below z_k were
    finalized at step k-1), so the reported bytes do not depend on Z:
      accumulator_bytes  fp32 sums of every channel plus the weight sum
      input_bytes        the input ring (and `staging_bytes` covers the largest finalize block: blended + final + weight sum)
      patch_bytes        the fp32 (B, Cin, pz, py, px) batch the network reads
    """
    Z, Y, X = (int(s) for s in shape)
    pz = int(patch[0])
    V = int(n_views)
    if V < 1:
        raise ValueError(f"n_views must be at least 1, got {n_views!r}")
    # `positions` (a tile of `tile_schedule`): the origins to run instead of all_positions, z-major, inside `shape` (the tile's box)
    pos = all_positions((Z, Y, X), patch, overlap) if positions is None else list(positions)
    B = max(1, min(int(batch_size), len(pos)))      # not a function of V: the device bytes are those of the run without views
    rows: Dict[int, list] = {}
    for p in pos:
        rows.setdefault(p[0], []).append(p)
    zs = sorted(rows)
    steps, loaded, fin, written = [], 0, 0, 0
    for k, zk in enumerate(zs):
        batches, views = cut_batches(rows[zk], B, V)
        load = (max(loaded, zk), zk + pz)
        loaded = zk + pz
        f_hi = zs[k + 1] if k + 1 < len(zs) else Z
        w_hi = Z if f_hi == Z else (f_hi // pz) * pz
        steps.append(dict(z=zk, load=load, batches=batches, views=views, finalize=(fin, f_hi),
                          write=(written, max(written, w_hi))))
        fin, written = f_hi, max(written, w_hi)
    max_fin = max(s["finalize"][1] - s["finalize"][0] for s in steps)
    return dict(positions=pos, batch=B, ring=pz, steps=steps, max_finalize_rows=max_fin,
                **_slab_bytes(patch, Y * X, max_fin, B, cin, in_itemsize, acc_channels, out_bytes_per_voxel))


# ---- Y/X tiles -----------------------------------------------------------------------------------------------------------------
class TileList(list):
    """the tiles of `tile_schedule`, with the totals `positions` (of the whole volume), `positions_run` (summed over the tiles) and
    `recompute` = positions_run / positions"""
    positions = 0
    positions_run = 0
    recompute = 1.0


def _axis_positions(dim: int, p: int, overlap: float):
    return generate_positions(0, int(dim), int(p), max(1, int(round(p * (1.0 - overlap)))))


def check_tile(tile, patch):
    """`tile` of StreamingInferer: None, "auto" or (ty, tx), each a positive multiple of the patch's (py, px)"""
    if tile is None:
        return None
    if isinstance(tile, str):
        if tile.lower() != "auto":
            raise ValueError(f"tile: {tile!r} (None, \"auto\" or (ty, tx))")
        return "auto"
    try:
        t = tuple(tile)
    except TypeError:
        raise ValueError(f"tile: {tile!r} (None, \"auto\" or (ty, tx))") from None
    ok = len(t) == 2 and all(isinstance(v, (int, np.integer)) and not isinstance(v, bool) for v in t)
    if not ok or any(v < 1 or v % p for v, p in zip(t, patch[1:])):
        raise ValueError(f"tile: {tile!r}; the owned extents (ty, tx) must be positive multiples of the patch's (py, px) = "
                         f"{tuple(patch[1:])}, because the output chunks equal the patch")
    return (int(t[0]), int(t[1]))


def tile_schedule(shape: Sequence[int], patch: Sequence[int], overlap: float, tile) -> TileList:
    """The Y/X tiles of `StreamingInferer(tile=(ty, tx))`; pure, no device.  The position grid stays `all_positions`'.  The (Y, X)
    plane is cut into owned boxes [i ty, min((i+1) ty, Y)) x [j tx, min((j+1) tx, X)), i-major; a tile is
      own  (y0, y1, x0, x1)  the box it writes
      ys   the y origins whose patch [y, y + py) meets the owned rows, ascending;  xs the same in x
      box  (y0, y1, x0, x1)  the hull of those patches: what is read and held on the device
    and it runs the positions z x ys x xs for every z origin.  Patches that reach into a neighbour's owned box are run by both
    tiles: `recompute` says how many times a position is run on average."""
    Z, Y, X = (int(s) for s in shape)
    pz, py, px = (int(p) for p in patch)
    ty, tx = check_tile(tile, patch)
    ay, ax = _axis_positions(Y, py, overlap), _axis_positions(X, px, overlap)
    nz = len(_axis_positions(Z, pz, overlap))
    out = TileList()
    for y0 in range(0, Y, ty):
        y1 = min(y0 + ty, Y)
        ys = [y for y in ay if y < y1 and y + py > y0]
        for x0 in range(0, X, tx):
            x1 = min(x0 + tx, X)
            xs = [x for x in ax if x < x1 and x + px > x0]
            out.append(dict(own=(y0, y1, x0, x1), box=(ys[0], ys[-1] + py, xs[0], xs[-1] + px), ys=ys, xs=xs))
    out.positions = nz * len(ay) * len(ax)
    out.positions_run = nz * sum(len(t["ys"]) * len(t["xs"]) for t in out)
    out.recompute = out.positions_run / out.positions
    return out


def _max_finalize_rows(Z: int, pz: int, overlap: float) -> int:
    zs = _axis_positions(Z, pz, overlap)
    return max(b - a for a, b in zip([0] + zs[1:], zs[1:] + [Z]))


def tiled_bytes(shape, patch, overlap, batch_size, tile, cin=1, in_itemsize=1, acc_channels=1, out_bytes_per_voxel=0) -> dict:
    """the byte counts of `stream_schedule`, each the maximum over the tiles of `tile_schedule` (a tile's slab is its box), with
    `batch` (one plan shape for every tile), `tiles`, `tile`, `positions`, `positions_run` and `recompute`"""
    tiles = tile_schedule(shape, patch, overlap, tile)
    nz = len(_axis_positions(shape[0], patch[0], overlap))
    B = max(1, min(int(batch_size), min(nz * len(t["ys"]) * len(t["xs"]) for t in tiles)))
    max_fin = _max_finalize_rows(int(shape[0]), int(patch[0]), overlap)
    per = [_slab_bytes(patch, (t["box"][1] - t["box"][0]) * (t["box"][3] - t["box"][2]), max_fin, B, cin, in_itemsize, acc_channels,
                       out_bytes_per_voxel) for t in tiles]
    out = {k: max(p[k] for p in per) for k in per[0]}
    out.update(batch=B, ring=int(patch[0]), max_finalize_rows=max_fin, tiles=len(tiles), tile=check_tile(tile, patch),
               positions=tiles.positions, positions_run=tiles.positions_run, recompute=tiles.recompute)
    return out


def choose_tile(shape, patch, overlap, batch_size, max_device_bytes, plan_bytes=0, cin=1, in_itemsize=1, acc_channels=1,
                out_bytes_per_voxel=0):
    """`tile="auto"`: None when the untiled slab plus the plan fits `max_device_bytes`; otherwise full width (tx = X rounded up to a
    multiple of px) with the largest ty that fits; if not even ty = py fits at full width, ty = py with the largest tx (a multiple
    of px) that fits; if (py, px) does not fit, MemoryError with the bytes it needs.  `plan_bytes`: the bytes of the network plan,
    a number or a function of the batch size.  Deterministic: a function of its arguments only."""
    Z, Y, X = (int(s) for s in shape)
    pz, py, px = (int(p) for p in patch)
    plan = plan_bytes if callable(plan_bytes) else (lambda B: int(plan_bytes))
    nz = len(_axis_positions(Z, pz, overlap))
    B0 = max(1, min(int(batch_size), nz * len(_axis_positions(Y, py, overlap)) * len(_axis_positions(X, px, overlap))))
    whole = _slab_bytes(patch, Y * X, _max_finalize_rows(Z, pz, overlap), B0, cin, in_itemsize, acc_channels, out_bytes_per_voxel)
    if whole["device_bytes"] + plan(B0) <= max_device_bytes:
        return None

    def need(t):
        b = tiled_bytes(shape, patch, overlap, batch_size, t, cin, in_itemsize, acc_channels, out_bytes_per_voxel)
        return b["device_bytes"] + plan(b["batch"])

    full_y, full_x = -(-Y // py) * py, -(-X // px) * px
    for ty in range(full_y, 0, -py):
        if need((ty, full_x)) <= max_device_bytes:
            return (ty, full_x)
    for tx in range(full_x - px, 0, -px):
        if need((py, tx)) <= max_device_bytes:
            return (py, tx)
    raise MemoryError(f"streaming inference needs {need((py, px))} bytes on the device for the smallest tile (one chunk, "
                      f"{py} x {px} owned voxels per row, plan included); the budget is {int(max_device_bytes)} bytes")


# ---- empty-patch skipping ------------------------------------------------------------------------------------------------------
def check_skip_empty(spec):
    """`skip_empty` of StreamingInferer: None / False -> None (off); True -> {"value": 0, "min_fraction": 0.0}; a mapping with
    those keys (either may be absent)"""
    if spec is None or spec is False:
        return None
    if spec is True:
        return {"value": 0.0, "min_fraction": 0.0}
    if not isinstance(spec, dict):
        raise ValueError(f"skip_empty: {spec!r} (None, a bool or a mapping with the keys value / min_fraction)")
    unknown = set(spec) - {"value", "min_fraction"}
    if unknown:
        raise ValueError(f"skip_empty: unknown key(s) {sorted(str(k) for k in unknown)} (known: value, min_fraction)")
    try:
        value, frac = float(spec.get("value", 0)), float(spec.get("min_fraction", 0.0))
    except (TypeError, ValueError):
        raise ValueError(f"skip_empty: value and min_fraction are numbers, got {spec!r}") from None
    if value != value:
        raise ValueError("skip_empty.value: NaN compares false with everything")
    if not 0.0 <= frac < 1.0:
        raise ValueError(f"skip_empty.min_fraction: {frac!r} is not in [0, 1)")
    return {"value": value, "min_fraction": frac}


def occupancy_numpy(vol, positions, patch, value) -> np.ndarray:
    """The statement of `rx_sw_occupancy`: uint64 count per position p of the raw voxels v of the patch at p, over all channels
    of a (C, Z, Y, X) or (Z, Y, X) volume, with float32(v) > float32(value) -- numpy's `>`, so a NaN never counts."""
    vol = np.asarray(vol)
    if vol.ndim == 3:
        vol = vol[None]
    pz, py, px = (int(p) for p in patch)
    thr = np.float32(value)
    return np.array([np.count_nonzero(vol[:, z:z + pz, y:y + py, x:x + px].astype(np.float32) > thr) for z, y, x in positions],
                    dtype=np.uint64)


def keep_mask(counts, n: int, min_fraction: float) -> np.ndarray:
    """a patch of n voxels is run iff count > min_fraction * n"""
    return np.asarray(counts).astype(np.float64) > float(min_fraction) * float(n)
