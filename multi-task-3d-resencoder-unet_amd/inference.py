"""Sliding-window inference with overlap blending, on the device.

Reference: inference.py:115-157 (patch loop: activation, `sum += pred`, `count += 1` per patch), :166-210 (overlap
processing: targets named "normals" with 3 channels are re-normalised `sum / (|sum| + 1e-8)`, everything else is averaged
`sum / count`, both only where count > 0), :251-263 (cast: normals `(v+1)/2*65535` -> uint16, others `v*255` -> uint8, clipped),
patch positions helpers.py:200-216.  The reference streams every patch through zarr chunks on the host (read-modify-write
per patch) and is broken at HEAD against its own ConfigManager; here the volume, the sum and the count
accumulators live in HBM for the whole run and only the finished arrays come back.

The forward passes are the HIP engine's inference plans with the module in eval mode (inference.py:112; stochastic depth off),
asked for raw logits (`NetworkFromConfig.forward_logits`) -- the activation is applied HERE exactly as
inference.py:121-133 does it from the target's `activation` key, never twice, so a CPU tensor is an error as everywhere
else in this package.  Accumulation / blending are a handful of torch slice ops on device tensors: plumbing, not kernels.
"""
import ctypes
import json
import os
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch


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


class SlidingWindowInferer:
    """`SlidingWindowInferer(model, targets, patch_size, batch_size, overlap)(volume)` -> dict of arrays.

    model    : NetworkFromConfig (HIP engine); run in eval mode (restored afterwards).
    targets  : mapping name -> {"channels": c, "activation": "sigmoid" | "softmax" | "none"}  (inference.py:121-133);
               defaults to the model's own task table.
    volume   : (C, Z, Y, X) or (Z, Y, X) float array / tensor, host or device.
    returns  : {name: float32 (c, Z, Y, X) blended prediction, name + "_final": uint8 / uint16 cast (reference dtype rule)}
    """

    def __init__(self, model, targets: Optional[dict] = None, patch_size: Optional[Sequence[int]] = None, batch_size: int = 2,
                 overlap: float = 0.5, compute_dtype: Optional[torch.dtype] = torch.bfloat16, device="cuda"):
        self.model = model
        self.targets = dict(targets if targets is not None else model.tasks)
        self.patch = tuple(patch_size if patch_size is not None else model.patch_size)
        if len(self.patch) != 3:
            raise ValueError("sliding-window inference is implemented for 3-D patches")
        self.batch_size = int(batch_size)
        self.overlap = float(overlap)
        self.compute_dtype = compute_dtype
        self.device = torch.device(device)

    @staticmethod
    def _activate(logits, kind):
        kind = (kind or "none").lower()
        if kind == "sigmoid":
            return torch.sigmoid(logits)
        if kind == "softmax":
            return torch.softmax(logits, dim=1)
        return logits

    @torch.no_grad()
    def accumulate(self, volume) -> Tuple[Dict[str, torch.Tensor], torch.Tensor]:
        """the patch loop (inference.py:115-157): returns ({name: sum (c,Z,Y,X)}, count (Z,Y,X)) on the device"""
        vol = torch.as_tensor(volume)
        if vol.dim() == 3:
            vol = vol.unsqueeze(0)
        vol = vol.to(self.device, torch.float32)
        _, Z, Y, X = vol.shape
        pz, py, px = self.patch
        pos = all_positions((Z, Y, X), self.patch, self.overlap)
        sums = {n: torch.zeros((int(t["channels"]), Z, Y, X), dtype=torch.float32, device=self.device) for n, t in self.targets.items()}
        count = torch.zeros((Z, Y, X), dtype=torch.float32, device=self.device)
        was_training = self.model.training
        self.model.eval()           # inference.py:112 (DropPath off); logits come from `forward_logits`, the activation is
                                    # applied below, once (inference.py:121-133)
        prev_dtype = getattr(self.model, "compute_dtype", None)
        if self.compute_dtype is not None:
            self.model.compute_dtype = self.compute_dtype
        try:
            for i in range(0, len(pos), self.batch_size):
                chunk = pos[i:i + self.batch_size]
                while len(chunk) < self.batch_size and i > 0:      # keep ONE plan shape: pad the last batch with a repeat
                    chunk = chunk + [chunk[-1]]
                patches = torch.stack([vol[:, z:z + pz, y:y + py, x:x + px] for z, y, x in chunk]).contiguous()
                raw = self.model.forward_logits(patches)
                valid = min(self.batch_size, len(pos) - i)
                for name, t in self.targets.items():
                    pred = self._activate(raw[name].float(), t.get("activation", "none"))
                    for b in range(valid):
                        z, y, x = chunk[b]
                        sums[name][:, z:z + pz, y:y + py, x:x + px] += pred[b]
                for b in range(valid):
                    z, y, x = chunk[b]
                    count[z:z + pz, y:y + py, x:x + px] += 1.0
        finally:
            self.model.compute_dtype = prev_dtype
            self.model.train(was_training)
        return sums, count

    @staticmethod
    def blend(name: str, sum_t: torch.Tensor, count: torch.Tensor) -> torch.Tensor:
        """overlap processing (inference.py:166-210)"""
        mask = count > 0
        out = sum_t.clone()
        if name.lower() == "normals":
            if sum_t.shape[0] == 3:
                mag = torch.sqrt((sum_t * sum_t).sum(0)) + 1e-8
                out = torch.where(mask, sum_t / mag, sum_t)
            return out
        return torch.where(mask, sum_t / count.clamp(min=1.0), sum_t)

    @staticmethod
    def cast_final(name: str, blended: torch.Tensor) -> torch.Tensor:
        """float32 -> uint16 (normals, [-1,1] -> [0,65535]) or uint8 ([0,1] -> [0,255]), truncating like astype (inference.py:251-263)"""
        if name.lower() == "normals":
            v = ((blended + 1.0) / 2.0 * 65535.0).clamp(0, 65535)
            return v.to(torch.int32).to(torch.uint16) if hasattr(torch, "uint16") else v.to(torch.int32)
        return (blended * 255.0).clamp(0, 255).to(torch.uint8)

    @torch.no_grad()
    def __call__(self, volume) -> Dict[str, np.ndarray]:
        sums, count = self.accumulate(volume)
        out = {}
        for name, s in sums.items():
            b = self.blend(name, s, count)
            out[name] = b.cpu().numpy()
            f = self.cast_final(name, b)
            out[name + "_final"] = f.cpu().numpy() if f.dtype != torch.int32 else f.cpu().numpy().astype(np.uint16)
        return out

    # ---- output side (inference.py:66-113, 214-263): a zarr v2 group `predictions.zarr` -------------------------------------
    def write_store(self, volume, output_path: str, compressor: Optional[str] = "zlib") -> str:
        """run the inference and write `<output_path>/predictions.zarr` with the reference's array set: `<target>_sum` (float32; AFTER
        the overlap pass it holds the blended prediction, as upstream leaves it), `<target>_count` (float32) and `<target>_final`
        (uint8 / uint16).  Single-channel targets are stored (Z, Y, X), others (c, Z, Y, X); chunks = the patch size (inference.py:
        76-90).  Refuses to overwrite an existing store (inference.py:67-72).  The reference compresses with Blosc/zstd (numcodecs,
        absent here): chunks are written with zlib or raw through `dataloading.zarr_lite` -- any zarr v2 reader opens them."""
        from .dataloading import zarr_lite
        store = os.path.join(output_path, "predictions.zarr")
        if os.path.isdir(store):
            raise FileExistsError(f"Zarr store '{store}' already exists. Aborting to prevent overwrite.")
        sums, count = self.accumulate(volume)
        os.makedirs(store)
        with open(os.path.join(store, ".zgroup"), "w") as f:
            json.dump({"zarr_format": 2}, f)
        pz, py, px = self.patch
        cnt = count.cpu().numpy()
        for name, s_t in sums.items():
            blended = self.blend(name, s_t, count)
            final = self.cast_final(name, blended)
            final_np = final.cpu().numpy() if final.dtype != torch.int32 else final.cpu().numpy().astype(np.uint16)
            b_np = blended.cpu().numpy()
            c = b_np.shape[0]
            if c == 1:
                b_np, final_np, chunks = b_np[0], final_np[0], (pz, py, px)
            else:
                chunks = (c, pz, py, px)
            zarr_lite.write_array(os.path.join(store, f"{name}_sum"), b_np, chunks, compressor=compressor)
            zarr_lite.write_array(os.path.join(store, f"{name}_count"), cnt, (pz, py, px), compressor=compressor)
            zarr_lite.write_array(os.path.join(store, f"{name}_final"), final_np, chunks, compressor=compressor)
        return store


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


_WEIGHT_CACHE: Dict[tuple, torch.Tensor] = {}


def _device_weights(kind: str, patch: Tuple[int, int, int], device) -> torch.Tensor:
    """the patch-shaped weight table on the device, uploaded once per (kind, patch, device)"""
    key = (kind, tuple(patch), str(device))
    w = _WEIGHT_CACHE.get(key)
    if w is None:
        host = gaussian_importance_map(patch) if kind == "gaussian" else np.ones(patch, dtype=np.float32)
        w = torch.from_numpy(host).to(device)
        _WEIGHT_CACHE[key] = w
    return w


# ---- test-time augmentation: the views of a patch -------------------------------------------------------------------------
TTA_MAX_VIEWS = 48          # the signed permutations of three axes: every flip / 90-degree rotation of a cube


def default_normal_keys(tasks) -> tuple:
    """the tasks whose predictions are surface normals: lower-case name `normals` and 3 channels (the rule of `_task_modes`)"""
    return tuple(n for n, t in (tasks or {}).items() if str(n).lower() == "normals" and int(t.get("channels", 0)) == 3)


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
    import itertools
    from .dataloading.geometry_device import AXIS_OF, GeomOp, allowed_rot90_axes, compose, flip_op, rot90_op
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


# ---- streaming schedule (pure: testable without a device) ------------------------------------------------------------------
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


# ---- Y/X tiles (pure) ----------------------------------------------------------------------------------------------------------
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


# ---- empty-patch skipping (pure) -----------------------------------------------------------------------------------------------
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


_IN_CODES = {np.dtype(np.uint8): 0, np.dtype(np.uint16): 1, np.dtype(np.float32): 2}     # RX_SW_U8 / U16 / F32
_ACT_CODES = {"none": 0, "sigmoid": 1, "softmax": 2}                                        # rx_head_act


def _open_source(source):
    if isinstance(source, (str, os.PathLike)):
        from .dataloading import zarr_lite
        source = zarr_lite.open(str(source))
    if len(source.shape) not in (3, 4):
        raise ValueError(f"source must be (Z, Y, X) or (C, Z, Y, X), got shape {tuple(source.shape)}")
    dt = np.dtype(source.dtype)
    if dt not in _IN_CODES:
        raise ValueError(f"source dtype {dt}: streaming inference reads uint8, uint16 or float32")
    return source


class StreamingInferer:
    """Out-of-core sliding-window inference: `StreamingInferer(model, ...).run(source, output_path)` -> `<output_path>/predictions.zarr`.

    The volume is read slab by slab (rows [z_k, z_k + pz) of each z-origin, see `stream_schedule`) and the output is written chunk
    row by chunk row; device memory is O(pz * Y * X), independent of Z.  The work around the network forward is HIP
    (csrc/rx_infer.hip): gather + normalisation of the patches, activation + weighted accumulation, finalize + integer cast.

    model / targets / patch_size / batch_size / overlap / compute_dtype: as `SlidingWindowInferer`.
    blend          "uniform" (the reference's rule, default): every patch weighs 1, so `<t>_count` is the patch count and the
                   result is `SlidingWindowInferer`'s; "gaussian": patches weighted by `gaussian_importance_map(patch)`, `<t>_count`
                   then holds the Gaussian weight SUM and the average is sum(w p) / sum(w).
    normalization  "scale" (default): uint8 / 255, uint16 / 65535, float32 as is (the training feeder, dataset.py:179-184);
                   "zscore": then (x - mean) / max(std, 1e-10) per patch over all voxels and channels (population std), the
                   reference inference dataset's pytorch3dunet `Standardize(channelwise=False)` -- that package is not available
                   here, so this parity is UNPINNED; the statistics are summed in fp64 in a fixed order.
    max_device_bytes  refuse (before any launch) a volume whose slab, plan included, does not fit (MemoryError), unless `tile`
                   says how to cut it.
    tile           None (default): one slab of the whole (Y, X) plane, the run without this argument.  (ty, tx): the plane is cut
                   into owned boxes of ty x tx voxels (positive multiples of the patch's py, px: output chunks equal the patch) and
                   the whole z loop runs tile after tile on the hull of the patches that meet the owned box, with box-local
                   origins; only the owned box is written.  The position grid is unchanged, and the patches that cover an owned
                   voxel arrive in the same relative order as in the whole run, so the fp32 sums are the same sums; patches that
                   reach into a neighbour are run again there (`last_schedule["recompute"]`, see `tile_schedule`).  Device memory
                   is that of the largest box: pz * Yb * Xb * (4 (channels + 1) + cin * itemsize) + finalize staging.  "auto":
                   chosen by `choose_tile` from max_device_bytes (required then); untiled where that fits.
    skip_empty     None / False (default): off.  True or {"value": v, "min_fraction": f}: a position p is run iff
                   count(p) > f * cin * pz * py * px, count(p) the raw input voxels of its patch above v (`occupancy_numpy`; on
                   the device `rx_sw_occupancy`, one launch and one small read per z-row).  A skipped position adds nothing to the
                   sums or the weight sum, with all its views; the kept (position, view) slots of a z-row are cut into batches of B
                   as the schedule cuts them, and a z-row with nothing kept runs no forward.  Voxels no kept patch covers stay 0
                   with weight 0 -- in `<t>_final` too, where the host writes the fill value instead of the cast of 0 -- and
                   all-zero chunks are not stored.  The decision depends on the data at p only.
    tta            test-time augmentation: None / False (default: off, the run is the one without this argument, bit for bit),
                   "flip", {"flip": [axes], "rot90": [axes]} or a sequence of `GeomOp` -- see `tta_views`.  For every patch
                   position p (all_positions order) and every view v with op g_v (view order; position-major, view-minor):
                       x = apply_op(g_v, scaled_patch(p))            image channels: moved, never the vector rule
                       P = act(forward_logits(x))                    the activation on the view-frame logits
                       q = apply_op(g_v.inverse(), P, is_normal = task in normal_keys)
                       sum[p-box] += w * q;  wsum[p-box] += w        w indexed by the destination voxel (the volume frame: the
                                                                     Gaussian map is not mirror-symmetric for even extents)
                   Finalize, blend and cast are unchanged, so `<t>_count` holds V x the patch count (uniform) or V x the Gaussian
                   weight sum.  With zscore the statistics are taken on the transformed patch -- the same multiset of values.
                   Device memory is the same with and without views.  Both ends are HIP (rx_sw_gather_geom,
                   rx_sw_accumulate_geom): no extra pass and no extra buffer per view or task.
    normal_keys    the tasks whose 3 channels are a vector field (components x, y, z) and follow the component and sign rule when
                   a view is undone; default: the tasks named `normals` with 3 channels.
    source         a zarr path, a `zarr_lite` array, or any numpy-sliceable (Z, Y, X) / (C, Z, Y, X) array (e.g. a memmap) of
                   uint8 / uint16 / float32.
    The output store has `write_store`'s array set, dtypes, shapes and chunking (= patch), zlib or raw chunks.  Host work
    overlaps the device: the next slab is read on a worker thread; D2H results are assembled and compressed on a pool of at most
    16 threads.  `last_timing` after a run: read_s, write_wait_s, total_s, patches (positions of the volume), views (V), forwards
    (network forward calls really made: batches of B (position, view) slots), tiles, positions_run (summed over the tiles) and
    skipped (positions of those that `skip_empty` dropped).
    """

    def __init__(self, model, targets: Optional[dict] = None, patch_size: Optional[Sequence[int]] = None, batch_size: int = 2,
                 overlap: float = 0.5, compute_dtype: Optional[torch.dtype] = torch.bfloat16, blend: str = "uniform",
                 normalization: str = "scale", max_device_bytes: Optional[int] = None, device="cuda", io_threads: int = 16,
                 tta=None, normal_keys=None, tile=None, skip_empty=None):
        self.model = model
        self.targets = dict(targets if targets is not None else model.tasks)
        self.patch = tuple(int(p) for p in (patch_size if patch_size is not None else model.patch_size))
        if len(self.patch) != 3:
            raise ValueError("sliding-window inference is implemented for 3-D patches")
        self.batch_size = int(batch_size)
        if not 1 <= self.batch_size <= 32:
            raise ValueError("batch_size must be 1..32")
        self.overlap = float(overlap)
        self.compute_dtype = compute_dtype
        self.blend = str(blend).lower()
        if self.blend not in ("uniform", "gaussian"):
            raise ValueError(f"blend must be 'uniform' or 'gaussian', got {blend!r}")
        self.normalization = str(normalization).lower()
        if self.normalization not in ("scale", "zscore"):
            raise ValueError(f"normalization must be 'scale' or 'zscore', got {normalization!r}")
        self.max_device_bytes = max_device_bytes
        self.device = torch.device(device)
        self.io_threads = max(1, min(16, int(io_threads)))
        # test-time augmentation: everything that can be refused is refused here, before any device work
        self.views = tta_views(tta, self.patch, self.targets, normal_keys)
        self.normal_keys = default_normal_keys(self.targets) if normal_keys is None else \
            ((normal_keys,) if isinstance(normal_keys, str) else tuple(normal_keys))
        self.tta = not (tta is None or tta is False)
        self.tile = check_tile(tile, self.patch)
        if self.tile == "auto" and self.max_device_bytes is None:
            raise ValueError("tile: \"auto\" chooses the tile from max_device_bytes, which is not set")
        self.skip_empty = check_skip_empty(skip_empty)
        self.last_schedule = None
        self.last_timing = None

    def _task_modes(self, name, t):
        from .engine import lib as L
        c = int(t["channels"])
        if name.lower() == "normals":
            return c, (L.RX_SW_BLEND_UNIT if c == 3 else L.RX_SW_BLEND_NONE), L.RX_SW_CAST_U16, np.uint16
        return c, L.RX_SW_BLEND_AVERAGE, L.RX_SW_CAST_U8, np.uint8

    def _byte_args(self, cin, in_itemsize):
        sc = sum(int(t["channels"]) for t in self.targets.values())
        out_b = 4 + sum(int(t["channels"]) * (4 + (2 if n.lower() == "normals" else 1)) for n, t in self.targets.items())
        return cin, in_itemsize, sc, out_b

    def schedule(self, shape, cin: int = 1, in_itemsize: int = 1, tile=None, plan_bytes=0) -> dict:
        """the schedule of a run over `shape`.  Untiled: `stream_schedule`'s dict plus tile = None, tiles = 1, recompute = 1.0.
        With a tile (`tile`, default the inferer's own; "auto" is resolved by `choose_tile` with `plan_bytes`): the byte counts are
        the maximum over the tiles (`tiled_bytes`), `tile_list` holds the tiles of `tile_schedule`, each with its own
        `stream_schedule` under "schedule" (box-local origins), and `steps` are those of the first tile."""
        args = self._byte_args(cin, in_itemsize)
        tile = self.tile if tile is None else (None if tile is False else check_tile(tile, self.patch))      # False: untiled
        if tile == "auto":
            tile = choose_tile(shape, self.patch, self.overlap, self.batch_size, self.max_device_bytes, plan_bytes, *args)
        if tile is None:
            s = stream_schedule(shape, self.patch, self.overlap, self.batch_size, *args, len(self.views))
            s.update(tile=None, tiles=1, recompute=1.0)
            return s
        s = tiled_bytes(shape, self.patch, self.overlap, self.batch_size, tile, *args)
        tiles = tile_schedule(shape, self.patch, self.overlap, tile)
        s.update(tile_list=list(tiles), steps=self.tile_stream_schedule(tiles[0], shape[0], s["batch"], cin, in_itemsize)["steps"],
                 positions=all_positions(shape, self.patch, self.overlap))
        return s

    def tile_stream_schedule(self, t, Z, B, cin: int = 1, in_itemsize: int = 1) -> dict:
        """`stream_schedule` of one tile of `tile_schedule`: its box as the slab, its positions with box-local origins"""
        by0, by1, bx0, bx1 = t["box"]
        local = [(z, y - by0, x - bx0) for z in _axis_positions(Z, self.patch[0], self.overlap) for y in t["ys"] for x in t["xs"]]
        return stream_schedule((int(Z), by1 - by0, bx1 - bx0), self.patch, self.overlap, B, *self._byte_args(cin, in_itemsize),
                               len(self.views), positions=local)

    @torch.no_grad()
    def run(self, source, output_path: str, compressor: Optional[str] = "zlib") -> str:
        import threading
        import time
        from concurrent.futures import ThreadPoolExecutor
        from .dataloading import zarr_lite
        from .engine import lib as L
        store = os.path.join(output_path, "predictions.zarr")
        if os.path.isdir(store):
            raise FileExistsError(f"Zarr store '{store}' already exists. Aborting to prevent overwrite.")
        src = _open_source(source)
        four = len(src.shape) == 4
        cin = int(src.shape[0]) if four else 1
        Z, Y, X = (int(s) for s in src.shape[-3:])
        in_dt = np.dtype(src.dtype)
        pz, py, px = self.patch
        shape = (Z, Y, X)
        L.require_device()
        dev = self.device

        # the plan for (B, Cin, patch) -- allocation only -- then the budget check, before any launch
        was_training = self.model.training
        prev_dtype = getattr(self.model, "compute_dtype", None)
        self.model.eval()
        if self.compute_dtype is not None:
            self.model.compute_dtype = self.compute_dtype
        try:
            def plan_of(b):
                return self.model.plan_for(torch.Size((b, cin, pz, py, px)), self.model._resolve_dtype(), dev, False)

            tile = self.tile
            if tile == "auto":      # None where the untiled slab fits: today's path
                tile = choose_tile(shape, self.patch, self.overlap, self.batch_size, self.max_device_bytes,
                                   lambda b: int(plan_of(b).bytes_alloc), *self._byte_args(cin, in_dt.itemsize))
            sched = self.schedule(shape, cin, in_dt.itemsize, tile=tile if tile is not None else False)
            self.last_schedule = sched
            plan = plan_of(sched["batch"])
            if self.max_device_bytes is not None:
                need = sched["device_bytes"] + int(plan.bytes_alloc)
                if need > self.max_device_bytes:
                    what = f"one slab of {pz} x {Y} x {X}" if tile is None else f"the largest box of the tiles {tile} of {Y} x {X}"
                    hint = "pass tile=(ty, tx) or tile=\"auto\" to run it in Y/X tiles" if tile is None else "a smaller tile is needed"
                    raise MemoryError(f"streaming inference needs {need / 2**30:.3f} GiB on the device for {what} "
                                      f"(plan {plan.bytes_alloc / 2**30:.3f} GiB included), the budget is "
                                      f"{self.max_device_bytes / 2**30:.3f} GiB; {hint}")
            return self._run(src, four, cin, shape, in_dt, sched, plan, store, compressor, zarr_lite, L,
                             ThreadPoolExecutor, threading, time)
        finally:
            self.model.compute_dtype = prev_dtype
            self.model.train(was_training)

    def _run(self, src, four, cin, shape, in_dt, sched, plan, store, compressor, zarr_lite, L, ThreadPoolExecutor, threading, time):
        Z, Y, X = shape
        pz, py, px = self.patch
        B, R = sched["batch"], sched["ring"]
        V = len(self.views)
        dev = self.device
        lib = L.load()
        t_start = time.perf_counter()
        tiled = sched["tile"] is not None
        # a run is a sequence of tiles, each the whole z loop on its box; untiled, the one tile is the plane and writes whole rows
        tiles = sched["tile_list"] if tiled else [dict(own=(0, Y, 0, X), box=(0, Y, 0, X), schedule=sched)]
        cap = max((t["box"][1] - t["box"][0]) * (t["box"][3] - t["box"][2]) for t in tiles)      # voxels per row of the largest box

        # device state, sized by the largest box and viewed per tile: input ring, accumulators (one wsum shared by every task),
        # finalize staging, the batch, weights
        tdt = {np.dtype(np.uint8): torch.uint8, np.dtype(np.uint16): torch.int16, np.dtype(np.float32): torch.float32}[in_dt]
        ring_flat = torch.empty((cin * R * cap,), dtype=tdt, device=dev)
        tasks = []
        for name, t in self.targets.items():
            c, blend, cast, fdt = self._task_modes(name, t)
            act = _ACT_CODES.get(str(t.get("activation", "none") or "none").lower(), 0)
            tasks.append(dict(name=name, c=c, blend=blend, cast=cast, fdt=fdt, act=act,
                              sum=torch.zeros((c * R * cap,), dtype=torch.float32, device=dev)))
        wsum = torch.zeros((R * cap,), dtype=torch.float32, device=dev)
        # finalize blocks of n <= F rows are written as contiguous (c, n, Y, X) arrays: flat buffers, viewed per block
        F = sched["max_finalize_rows"]
        for tk in tasks:
            tk["tdt"] = torch.uint8 if tk["fdt"] == np.uint8 else torch.int16
            tk["blended"] = torch.empty((tk["c"] * F * cap,), dtype=torch.float32, device=dev)
            tk["final"] = torch.empty((tk["c"] * F * cap,), dtype=tk["tdt"], device=dev)
        wsum_out = torch.empty((F * cap,), dtype=torch.float32, device=dev)
        xb = torch.empty((B, cin, pz, py, px), dtype=torch.float32, device=dev)
        weights = _device_weights(self.blend, self.patch, dev)
        ws_b = lib.rx_sw_gather_workspace(B, cin, pz, py, px) if self.normalization == "zscore" else 0
        ws = torch.empty((max(1, ws_b // 8),), dtype=torch.float64, device=dev)
        norm = L.RX_SW_ZSCORE if self.normalization == "zscore" else L.RX_SW_SCALE
        in_code = _IN_CODES[in_dt]
        O3 = ctypes.c_int32 * (3 * B)
        G12 = ctypes.c_int32 * (12 * B)                       # B records of rx_geom_sample
        fwd_rows = [v.row() for v in self.views]              # the view, applied to the patch
        inv_rows = [v.inverse().row() for v in self.views]    # its inverse, applied to the prediction
        for tk in tasks:
            tk["vector"] = 1 if tk["name"] in self.normal_keys else 0
        skip = self.skip_empty
        occ = None                                            # uint64 counts of rx_sw_occupancy, one per position of a z-row
        n_vox = cin * pz * py * px

        # output store
        os.makedirs(store)
        with open(os.path.join(store, ".zgroup"), "w") as f:
            json.dump({"zarr_format": 2}, f)
        writers = {}
        for tk in tasks:
            c, n = tk["c"], tk["name"]
            shp, ch = ((Z, Y, X), (pz, py, px)) if c == 1 else ((c, Z, Y, X), (c, pz, py, px))
            writers[n] = (zarr_lite.ChunkedWriter(os.path.join(store, f"{n}_sum"), shp, ch, np.float32, compressor),
                          zarr_lite.ChunkedWriter(os.path.join(store, f"{n}_count"), (Z, Y, X), (pz, py, px), np.float32, compressor),
                          zarr_lite.ChunkedWriter(os.path.join(store, f"{n}_final"), shp, ch, tk["fdt"], compressor))

        # host staging: two pinned input buffers and two pinned output sets, each guarded by an event
        # (flat as well: every asynchronous copy below is contiguous on both sides)
        in_pin = [torch.empty((cin * pz * cap,), dtype=tdt).pin_memory() for _ in range(2)]
        in_ev = [None, None]
        out_pin = [dict(w=torch.empty((F * cap,), dtype=torch.float32).pin_memory(),
                        **{tk["name"]: (torch.empty((tk["c"] * F * cap,), dtype=torch.float32).pin_memory(),
                                        torch.empty((tk["c"] * F * cap,), dtype=tk["tdt"]).pin_memory()) for tk in tasks})
                   for _ in range(2)]
        out_busy = [None, None]
        pend_rows = pz + F      # rows finalized but not yet written (at most one chunk row plus one finalize block)
        timing = dict(read_s=0.0, write_wait_s=0.0)
        lock = threading.Lock()

        chunks = getattr(src, "chunks", None)
        cy = int(chunks[-2]) if chunks is not None and len(chunks) == len(src.shape) else Y

        def contexts():
            """per tile: its schedule, its box and owned box, and the host rows of the OWNED box that wait to be written"""
            for ti, t in enumerate(tiles):
                ts = t.get("schedule") or self.tile_stream_schedule(t, Z, B, cin, in_dt.itemsize)
                (by0, by1, bx0, bx1), (oy0, oy1, ox0, ox1) = t["box"], t["own"]
                oyn, oxn = oy1 - oy0, ox1 - ox0
                yield dict(index=ti, steps=ts["steps"], box=t["box"], Yb=by1 - by0, Xb=bx1 - bx0, own=t["own"],
                           crop=(oy0 - by0, oy1 - by0, ox0 - bx0, ox1 - bx0), base=0,      # base: volume row of pend[..., 0, :, :]
                           pend={tk["name"]: (np.zeros((tk["c"], pend_rows, oyn, oxn), np.float32),
                                              np.zeros((tk["c"], pend_rows, oyn, oxn), tk["fdt"])) for tk in tasks},
                           pend_w=np.zeros((pend_rows, oyn, oxn), np.float32))

        def items():
            for ctx in contexts():
                for k, st in enumerate(ctx["steps"]):
                    yield ctx, k, st

        def read_piece(a, lo, hi, y0, y1, by0, bx0, bx1):
            a[:, :, y0 - by0:y1 - by0] = src[:, lo:hi, y0:y1, bx0:bx1] if four else src[lo:hi, y0:y1, bx0:bx1][None]

        def read_rows(box, lo, hi):
            """rows [lo, hi) of every channel of the box, read as columns of whole chunks on the I/O pool (zlib releases the GIL)"""
            t0 = time.perf_counter()
            by0, by1, bx0, bx1 = box
            a = np.empty((cin, hi - lo, by1 - by0, bx1 - bx0), in_dt)
            cuts = [by0] + list(range((by0 // cy + 1) * cy, by1, cy)) + [by1]
            for f in [pool.submit(read_piece, a, lo, hi, y0, y1, by0, bx0, bx1) for y0, y1 in zip(cuts, cuts[1:])]:
                f.result()
            if a.dtype == np.uint16:
                a = a.view(np.int16)
            with lock:
                timing["read_s"] += time.perf_counter() - t0
            return a

        pool = ThreadPoolExecutor(max_workers=self.io_threads)
        reader = ThreadPoolExecutor(max_workers=1)
        drainer = ThreadPoolExecutor(max_workers=1)
        chunk_futs = []

        def drain(ctx, slot, ev, f_lo, n, w_lo, w_hi):
            """host side of one finalize block: wait for its D2H, park the rows of the owned box, hand complete chunk rows to the pool"""
            ev.synchronize()
            o = out_pin[slot]
            Yb, Xb = ctx["Yb"], ctx["Xb"]
            c0, c1, d0, d1 = ctx["crop"]
            pend, pend_w = ctx["pend"], ctx["pend_w"]
            off = f_lo - ctx["base"]
            pend_w[off:off + n] = o["w"][:n * Yb * Xb].view(n, Yb, Xb).numpy()[:, c0:c1, d0:d1]
            for tk in tasks:
                b, f = o[tk["name"]]
                m4 = (tk["c"], n, Yb, Xb)
                pend[tk["name"]][0][:, off:off + n] = b[:tk["c"] * n * Yb * Xb].view(m4).numpy()[:, :, c0:c1, d0:d1]
                fv = f[:tk["c"] * n * Yb * Xb].view(m4).numpy()[:, :, c0:c1, d0:d1]
                pend[tk["name"]][1][:, off:off + n] = fv.view(np.uint16) if tk["fdt"] == np.uint16 else fv
            if skip is not None:      # a voxel no kept patch covers holds the store's fill value in `_final` too, not the cast of 0
                dead = pend_w[off:off + n] == 0
                if dead.any():
                    for tk in tasks:
                        pend[tk["name"]][1][:, off:off + n][:, dead] = 0
            if w_hi > w_lo:
                m = w_hi - w_lo
                assert w_lo == ctx["base"]
                oy0, ox0 = ctx["own"][0], ctx["own"][2]

                def put(w, blk):
                    chunk_futs.extend(w.write_block(w_lo, oy0, ox0, blk, pool) if tiled else w.write_rows(w_lo, blk, pool))

                wblk = pend_w[:m].copy()
                for tk in tasks:
                    s_w, c_w, f_w = writers[tk["name"]]
                    bb, ff = pend[tk["name"]][0][:, :m].copy(), pend[tk["name"]][1][:, :m].copy()
                    if tk["c"] == 1:
                        bb, ff = bb[0], ff[0]
                    put(s_w, bb)
                    put(c_w, wblk)
                    put(f_w, ff)
                keep = off + n - m
                pend_w[:keep] = pend_w[m:m + keep].copy()
                for tk in tasks:
                    for arr in pend[tk["name"]]:
                        arr[:, :keep] = arr[:, m:m + keep].copy()
                ctx["base"] = w_hi

        it = items()
        cur = next(it)
        nxt = reader.submit(read_rows, cur[0]["box"], *cur[2]["load"])
        drains = []
        n_fwd = n_run = n_skipped = 0
        g = -1                                                 # steps so far, over all tiles: the staging slots alternate with it
        stream = torch.cuda.current_stream(dev)
        sp = L.stream_ptr()
        try:
            while cur is not None:
                ctx, k, st = cur
                g += 1
                Yb, Xb = ctx["Yb"], ctx["Xb"]
                if k == 0:                                     # this tile's views of the device state
                    ring_in = ring_flat[:cin * R * Yb * Xb].view(cin, R, Yb, Xb)
                    if ctx["index"] > 0:                       # every row was reset by its finalize; the layout changes with the box
                        wsum.zero_()
                        for tk in tasks:
                            tk["sum"].zero_()
                lo, hi = st["load"]
                host = nxt.result()
                cur = next(it, None)
                if cur is not None:
                    nxt = reader.submit(read_rows, cur[0]["box"], *cur[2]["load"])
                if hi > lo:
                    slot = g % 2
                    if in_ev[slot] is not None:
                        in_ev[slot].synchronize()
                    pin = in_pin[slot][:cin * (hi - lo) * Yb * Xb].view(cin, hi - lo, Yb, Xb)
                    pin.copy_(torch.from_numpy(host))
                    z = lo
                    while z < hi:                          # ring rows wrap: at most two contiguous pieces per channel
                        r0 = z % R
                        seg = min(hi - z, R - r0)
                        for ci in range(cin):
                            ring_in[ci, r0:r0 + seg].copy_(pin[ci, z - lo:z - lo + seg], non_blocking=True)
                        z += seg
                    ev = torch.cuda.Event()
                    ev.record(stream)
                    in_ev[slot] = ev
                batches, views = st["batches"], st["views"]
                row = row_positions(st)
                n_run += len(row)
                if skip is not None:      # one count per position of the row, one small read, then the batches are cut again
                    if occ is None or occ.numel() < len(row):
                        occ = torch.empty((len(row),), dtype=torch.int64, device=dev)
                    org = (ctypes.c_int32 * (3 * len(row)))(*[v for p in row for v in p])
                    L.check(lib.rx_sw_occupancy(in_code, ring_in.data_ptr(), cin, R, Yb, Xb, len(row), org, pz, py, px,
                                                ctypes.c_float(skip["value"]), occ.data_ptr(), sp), "rx_sw_occupancy")
                    keep = keep_mask(occ[:len(row)].cpu().numpy().view(np.uint64), n_vox, skip["min_fraction"])
                    kept = [p for p, kp in zip(row, keep) if kp]
                    n_skipped += len(row) - len(kept)
                    batches, views = cut_batches(kept, B, V)
                for (chunk, valid), vidx in zip(batches, views):
                    org = O3(*[v for p in chunk for v in p])
                    if self.tta:      # the patch as its view sees it; the prediction is moved back by the view's inverse below
                        fwd = G12(*[v for j in vidx for v in fwd_rows[j]])
                        inv = G12(*[v for j in vidx for v in inv_rows[j]])
                        L.check(lib.rx_sw_gather_geom(in_code, ring_in.data_ptr(), cin, R, Yb, Xb, B, org, fwd, pz, py, px, norm,
                                                      xb.data_ptr(), ws.data_ptr(), ws_b, sp), "rx_sw_gather_geom")
                    else:
                        L.check(lib.rx_sw_gather(in_code, ring_in.data_ptr(), cin, R, Yb, Xb, B, org, pz, py, px, norm, xb.data_ptr(),
                                                 ws.data_ptr(), ws_b, sp), "rx_sw_gather")
                    outs = plan.run_forward(xb, apply_act=False)     # the plan's own head buffers, read before the next forward
                    n_fwd += 1
                    for i, tk in enumerate(tasks):
                        ws_p = wsum.data_ptr() if i == 0 else None
                        if self.tta:
                            L.check(lib.rx_sw_accumulate_geom(outs[tk["name"]].data_ptr(), B, valid, tk["c"], pz, py, px, org, inv,
                                                              tk["vector"], tk["act"], weights.data_ptr(), tk["sum"].data_ptr(), ws_p,
                                                              R, Yb, Xb, sp), "rx_sw_accumulate_geom")
                        else:
                            L.check(lib.rx_sw_accumulate(outs[tk["name"]].data_ptr(), B, valid, tk["c"], pz, py, px, org, tk["act"],
                                                         weights.data_ptr(), tk["sum"].data_ptr(), ws_p, R, Yb, Xb, sp),
                                    "rx_sw_accumulate")
                f_lo, f_hi = st["finalize"]
                n = f_hi - f_lo
                if n > 0:
                    slot = g % 2
                    if out_busy[slot] is not None:                     # its previous block has been parked on the host
                        t0 = time.perf_counter()
                        out_busy[slot].result()
                        timing["write_wait_s"] += time.perf_counter() - t0
                    o = out_pin[slot]
                    for i, tk in enumerate(tasks):
                        L.check(lib.rx_sw_finalize(tk["sum"].data_ptr(), wsum.data_ptr(), tk["c"], R, Yb, Xb, f_lo, n, tk["blend"],
                                                   tk["cast"], 2 if i == len(tasks) - 1 else 1, tk["blended"].data_ptr(),
                                                   tk["final"].data_ptr(), wsum_out.data_ptr() if i == 0 else None, sp),
                                "rx_sw_finalize")
                        b, f = o[tk["name"]]
                        m = tk["c"] * n * Yb * Xb
                        b[:m].copy_(tk["blended"][:m], non_blocking=True)
                        f[:m].copy_(tk["final"][:m], non_blocking=True)
                    o["w"][:n * Yb * Xb].copy_(wsum_out[:n * Yb * Xb], non_blocking=True)
                    ev = torch.cuda.Event()
                    ev.record(stream)
                    w_lo, w_hi = st["write"]
                    out_busy[slot] = drainer.submit(drain, ctx, slot, ev, f_lo, n, w_lo, w_hi)
                    drains.append(out_busy[slot])
            for d in drains:
                d.result()
            t0 = time.perf_counter()
            for fu in chunk_futs:
                fu.result()
            timing["write_wait_s"] += time.perf_counter() - t0
        finally:
            reader.shutdown(wait=True)
            drainer.shutdown(wait=True)
            pool.shutdown(wait=True)
        timing.update(total_s=time.perf_counter() - t_start, forwards=n_fwd, patches=len(sched["positions"]), views=V,
                      tiles=len(tiles), positions_run=n_run, skipped=n_skipped)
        self.last_timing = timing
        return store


# ---- command line: `python -m mt3d_amd.inference --config_path X` ---------------------------------------------------------------
def load_model(mgr, device="cuda"):
    """NetworkFromConfig(mgr) with the weights of `inference_config.checkpoint_path`, loaded as the trainer resumes
    (checkpoint["model"], `_orig_mod.` prefixes of a compiled model stripped, train.py:251-252)"""
    from .builders.build_network_from_config import NetworkFromConfig
    model = NetworkFromConfig(mgr).to(device)
    if not mgr.infer_checkpoint_path:
        raise ValueError("inference_config.checkpoint_path is required")
    ck = torch.load(mgr.infer_checkpoint_path, map_location=device, weights_only=True)
    sd = ck["model"] if isinstance(ck, dict) and "model" in ck else ck
    model.load_state_dict({(k[len("_orig_mod."):] if k.startswith("_orig_mod.") else k): v for k, v in sd.items()})
    return model


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(description="Streaming sliding-window inference of the multi-task 3-D ResEnc U-Net (HIP engine).")
    ap.add_argument("--config_path", type=str, required=True)
    ap.add_argument("--input_path", type=str, default=None, help="overrides inference_config.input_path")
    ap.add_argument("--output_path", type=str, default=None, help="overrides inference_config.output_path")
    ap.add_argument("--compressor", choices=["zlib", "none"], default="zlib")
    ap.add_argument("--write_layers", action="store_true", help="(reference option: per-slice image layers; needs cv2)")
    ap.add_argument("--verbose", action="store_true")
    a = ap.parse_args(argv)
    if a.write_layers:
        raise SystemExit("--write_layers writes image slices with cv2 (OpenCV), which is not available in this environment; "
                         "the zarr store is the only output")
    from .configuration.config_manager import ConfigManager
    mgr = ConfigManager(a.config_path, verbose=a.verbose)
    src = a.input_path or mgr.infer_input_path
    if not src:
        raise SystemExit("no input: set inference_config.input_path or pass --input_path")
    gb = mgr.infer_max_device_gb
    runner = StreamingInferer(load_model(mgr), mgr.infer_targets, mgr.infer_patch_size, mgr.infer_batch_size, mgr.infer_overlap,
                              blend=mgr.infer_blend, normalization=mgr.infer_normalization,
                              max_device_bytes=None if gb is None else int(gb * 2**30), tta=mgr.infer_tta,
                              normal_keys=mgr.infer_tta_normal_keys, tile=mgr.infer_tile, skip_empty=mgr.infer_skip_empty)
    store = runner.run(src, a.output_path or mgr.infer_output_path, compressor=None if a.compressor == "none" else "zlib")
    print(store, flush=True)
    return store


if __name__ == "__main__":
    main()
