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

Layout: `inference_schedule.py` holds everything that plans a run without torch (positions, Gaussian map, views, schedules,
tiles, the empty-patch rule, `task_output_rule`) and is re-exported here.  This file holds `SlidingWindowInferer`, the parts of a
streaming run -- `StreamTask`, `SlabReader` and `RowSink` (host only, numpy), `_DeviceState`, `_StreamRun` (the step loop) --
`StreamingInferer`, and the command line.  The `rx_sw_*` kernels are reached through `engine.ops.sw_*`.
"""
import contextlib
import json
import os
import time
from concurrent.futures import ThreadPoolExecutor
from dataclasses import dataclass
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from .dataloading import zarr_lite
from .engine import lib as L
from .engine import ops
from .inference_schedule import (TTA_MAX_VIEWS, TileList, all_positions, check_skip_empty, check_tile, choose_tile,  # noqa: F401
                                 cut_batches, default_normal_keys, gaussian_importance_map, generate_positions, keep_mask,
                                 occupancy_numpy, row_positions, stream_schedule, task_output_rule, tile_schedule, tiled_bytes,
                                 tta_views, _axis_positions)


@contextlib.contextmanager
def inference_mode(model, compute_dtype):
    """the model in eval mode (inference.py:112: DropPath off) and, unless None, computing in `compute_dtype`; both restored"""
    was_training = model.training
    prev_dtype = getattr(model, "compute_dtype", None)
    model.eval()
    if compute_dtype is not None:
        model.compute_dtype = compute_dtype
    try:
        yield
    finally:
        model.compute_dtype = prev_dtype
        model.train(was_training)


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
        # logits come from `forward_logits`, the activation is applied below, once (inference.py:121-133)
        with inference_mode(self.model, self.compute_dtype):
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
        return sums, count

    @staticmethod
    def blend(name: str, sum_t: torch.Tensor, count: torch.Tensor) -> torch.Tensor:
        """overlap processing (inference.py:166-210)"""
        mask = count > 0
        rule = task_output_rule(name, sum_t.shape[0])[0]
        if rule == "unit":
            mag = torch.sqrt((sum_t * sum_t).sum(0)) + 1e-8
            return torch.where(mask, sum_t / mag, sum_t)
        if rule == "none":
            return sum_t.clone()
        return torch.where(mask, sum_t / count.clamp(min=1.0), sum_t)

    @staticmethod
    def cast_final(name: str, blended: torch.Tensor) -> torch.Tensor:
        """float32 -> uint16 (normals, [-1,1] -> [0,65535]) or uint8 ([0,1] -> [0,255]), truncating like astype (inference.py:251-263)"""
        if task_output_rule(name, blended.shape[0])[1] == "u16":
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


# ---- the parts of a streaming run ---------------------------------------------------------------------------------------------
# source dtype -> the dtype of its device ring (torch has no uint16 arithmetic: the ring holds the bits as int16)
_IN_TORCH = {np.dtype(np.uint8): torch.uint8, np.dtype(np.uint16): torch.int16, np.dtype(np.float32): torch.float32}


def _open_source(source):
    if isinstance(source, (str, os.PathLike)):
        source = zarr_lite.open(str(source))
    if len(source.shape) not in (3, 4):
        raise ValueError(f"source must be (Z, Y, X) or (C, Z, Y, X), got shape {tuple(source.shape)}")
    dt = np.dtype(source.dtype)
    if dt not in _IN_TORCH:
        raise ValueError(f"source dtype {dt}: streaming inference reads uint8, uint16 or float32")
    return source


@dataclass
class StreamTask:
    """one target of a streaming run: its output rule (`task_output_rule`), its activation and, once `alloc` has run, its
    device buffers -- all flat, sized by the largest box and viewed per tile and per finalize block"""
    name: str
    c: int
    blend: str                  # "average" | "unit" | "none"
    cast: str                   # "u8" | "u16"
    fdt: np.dtype               # host dtype of `<name>_final`
    act: int                    # RX_ACT code applied to the logits
    vector: bool                # a 3-channel vector field: follows the component and sign rule when a view is undone
    sum: Optional[torch.Tensor] = None          # fp32 (c * ring * cap)
    blended: Optional[torch.Tensor] = None      # fp32 (c * F * cap), F = the largest finalize block
    final: Optional[torch.Tensor] = None        # uint8 / int16 (c * F * cap)

    @classmethod
    def of(cls, name, target, normal_keys=()):
        c = int(target["channels"])
        blend, cast, fdt, _ = task_output_rule(name, c)
        act = ops.SW_ACT.get(str(target.get("activation", "none") or "none").lower(), L.RX_ACT_NONE)
        return cls(name, c, blend, cast, fdt, act, name in normal_keys)

    @property
    def tdt(self):
        return torch.uint8 if self.fdt == np.uint8 else torch.int16

    def alloc(self, ring, fin_rows, cap, device):
        self.sum = torch.zeros((self.c * ring * cap,), dtype=torch.float32, device=device)
        self.blended = torch.empty((self.c * fin_rows * cap,), dtype=torch.float32, device=device)
        self.final = torch.empty((self.c * fin_rows * cap,), dtype=self.tdt, device=device)


class SlabReader:
    """Reads the rows of a box of the source, host only: `read(box, lo, hi)` -> (cin, hi - lo, Yb, Xb) of the source dtype, uint16
    as the int16 holding its bits (what the device ring stores).  The box is read as columns of whole source chunks on the I/O
    `pool` (zlib releases the GIL); `prefetch` runs `read` on the reader's own thread, one step ahead of the device.  `read_s`
    sums the time spent in `read`."""

    def __init__(self, src, pool):
        self.src, self.pool = src, pool
        self.four = len(src.shape) == 4
        self.cin = int(src.shape[0]) if self.four else 1
        chunks = getattr(src, "chunks", None)
        self.cy = int(chunks[-2]) if chunks is not None and len(chunks) == len(src.shape) else int(src.shape[-2])
        self.read_s = 0.0
        self._thread = ThreadPoolExecutor(max_workers=1)

    def _piece(self, a, lo, hi, y0, y1, by0, bx0, bx1):
        src = self.src
        a[:, :, y0 - by0:y1 - by0] = src[:, lo:hi, y0:y1, bx0:bx1] if self.four else src[lo:hi, y0:y1, bx0:bx1][None]

    def read(self, box, lo, hi):
        t0 = time.perf_counter()
        by0, by1, bx0, bx1 = box
        a = np.empty((self.cin, hi - lo, by1 - by0, bx1 - bx0), np.dtype(self.src.dtype))
        cuts = [by0] + list(range((by0 // self.cy + 1) * self.cy, by1, self.cy)) + [by1]
        for f in [self.pool.submit(self._piece, a, lo, hi, y0, y1, by0, bx0, bx1) for y0, y1 in zip(cuts, cuts[1:])]:
            f.result()
        if a.dtype == np.uint16:
            a = a.view(np.int16)
        self.read_s += time.perf_counter() - t0
        return a

    def prefetch(self, box, lo, hi):
        return self._thread.submit(self.read, box, lo, hi)

    def close(self):
        self._thread.shutdown(wait=True)


def open_store(store, tasks, shape, patch, compressor):
    """create the output group and, per task, the writers of `<t>_sum`, `<t>_count` and `<t>_final` (`write_store`'s array set:
    single-channel targets are (Z, Y, X), others (c, Z, Y, X); chunks = the patch)"""
    Z, Y, X = shape
    pz, py, px = patch
    os.makedirs(store)
    with open(os.path.join(store, ".zgroup"), "w") as f:
        json.dump({"zarr_format": 2}, f)
    writers = {}
    for tk in tasks:
        c, n = tk.c, tk.name
        shp, ch = ((Z, Y, X), (pz, py, px)) if c == 1 else ((c, Z, Y, X), (c, pz, py, px))
        writers[n] = (zarr_lite.ChunkedWriter(os.path.join(store, f"{n}_sum"), shp, ch, np.float32, compressor),
                      zarr_lite.ChunkedWriter(os.path.join(store, f"{n}_count"), (Z, Y, X), (pz, py, px), np.float32, compressor),
                      zarr_lite.ChunkedWriter(os.path.join(store, f"{n}_final"), shp, ch, tk.fdt, compressor))
    return writers


class RowSink:
    """The host side of one tile's output, numpy only.  `put` takes a finalize block of the tile's BOX, crops it to the OWNED box
    and parks it; when the schedule says a range of chunk rows is complete (`write`), those rows go to the writers of
    `open_store` -- whole rows of the volume (`write_rows`) or, `tiled`, the owned box of them (`write_block`).
    `pend_rows`: rows that can wait at once (one chunk row plus one finalize block).  `fill_dead` (empty-patch skipping): a voxel
    with weight 0 -- no kept patch covers it -- holds the store's fill value 0 in `<t>_final` too, not the cast of 0."""

    def __init__(self, writers, tasks, own, box, pend_rows, tiled=False, fill_dead=False, pool=None):
        self.writers, self.tasks, self.tiled, self.fill_dead, self.pool = writers, tasks, tiled, fill_dead, pool
        (by0, _, bx0, _), (oy0, oy1, ox0, ox1) = box, own
        self.own = own
        self.crop = (oy0 - by0, oy1 - by0, ox0 - bx0, ox1 - bx0)
        self.base = 0      # volume row of pend[..., 0, :, :]
        oyn, oxn = oy1 - oy0, ox1 - ox0
        self.pend = {tk.name: (np.zeros((tk.c, pend_rows, oyn, oxn), np.float32), np.zeros((tk.c, pend_rows, oyn, oxn), tk.fdt))
                     for tk in tasks}
        self.pend_w = np.zeros((pend_rows, oyn, oxn), np.float32)

    def put(self, f_lo, blocks, weights, write):
        """rows [f_lo, f_lo + n) of the box: `blocks[name]` = (blended (c, n, Yb, Xb) float32, final (c, n, Yb, Xb) of the task's
        host dtype), `weights` (n, Yb, Xb) float32; `write` = (lo, hi), the output rows to hand to the writers now (lo == hi:
        none).  Returns the futures of the chunk writes ([] without a pool)."""
        c0, c1, d0, d1 = self.crop
        n = weights.shape[0]
        off = f_lo - self.base
        self.pend_w[off:off + n] = weights[:, c0:c1, d0:d1]
        for tk in self.tasks:
            b, f = blocks[tk.name]
            self.pend[tk.name][0][:, off:off + n] = b[:, :, c0:c1, d0:d1]
            self.pend[tk.name][1][:, off:off + n] = f[:, :, c0:c1, d0:d1]
        if self.fill_dead:
            dead = self.pend_w[off:off + n] == 0
            if dead.any():
                for tk in self.tasks:
                    self.pend[tk.name][1][:, off:off + n][:, dead] = 0
        w_lo, w_hi = write
        return self._write(w_lo, w_hi, off + n) if w_hi > w_lo else []

    def _write(self, w_lo, w_hi, parked):
        """hand the first w_hi - w_lo parked rows to the writers and move the rest to the front"""
        m = w_hi - w_lo
        assert w_lo == self.base
        oy0, ox0 = self.own[0], self.own[2]
        futs = []

        def emit(w, blk):
            futs.extend(w.write_block(w_lo, oy0, ox0, blk, self.pool) if self.tiled else w.write_rows(w_lo, blk, self.pool))

        wblk = self.pend_w[:m].copy()
        for tk in self.tasks:
            s_w, c_w, f_w = self.writers[tk.name]
            bb, ff = self.pend[tk.name][0][:, :m].copy(), self.pend[tk.name][1][:, :m].copy()
            if tk.c == 1:
                bb, ff = bb[0], ff[0]
            emit(s_w, bb)
            emit(c_w, wblk)
            emit(f_w, ff)
        keep = parked - m
        self.pend_w[:keep] = self.pend_w[m:m + keep].copy()
        for tk in self.tasks:
            for arr in self.pend[tk.name]:
                arr[:, :keep] = arr[:, m:m + keep].copy()
        self.base = w_hi
        return futs


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

    def _byte_args(self, cin, in_itemsize):
        sc = sum(int(t["channels"]) for t in self.targets.values())
        out_b = 4 + sum(int(t["channels"]) * (4 + task_output_rule(n, t["channels"])[2].itemsize) for n, t in self.targets.items())
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

    def _plan(self, batch, cin):
        """the network plan for (batch, cin, patch): allocation only, no launch"""
        return self.model.plan_for(torch.Size((batch, cin) + self.patch), self.model._resolve_dtype(), self.device, False)

    def _check_budget(self, sched, plan, shape):
        """refuse, before any launch, a run whose largest slab plus the plan does not fit `max_device_bytes`"""
        need = sched["device_bytes"] + int(plan.bytes_alloc)
        if self.max_device_bytes is None or need <= self.max_device_bytes:
            return
        tile, (_, Y, X) = sched["tile"], shape
        what = f"one slab of {self.patch[0]} x {Y} x {X}" if tile is None else f"the largest box of the tiles {tile} of {Y} x {X}"
        hint = "pass tile=(ty, tx) or tile=\"auto\" to run it in Y/X tiles" if tile is None else "a smaller tile is needed"
        raise MemoryError(f"streaming inference needs {need / 2**30:.3f} GiB on the device for {what} "
                          f"(plan {plan.bytes_alloc / 2**30:.3f} GiB included), the budget is "
                          f"{self.max_device_bytes / 2**30:.3f} GiB; {hint}")

    @torch.no_grad()
    def run(self, source, output_path: str, compressor: Optional[str] = "zlib") -> str:
        store = os.path.join(output_path, "predictions.zarr")
        if os.path.isdir(store):
            raise FileExistsError(f"Zarr store '{store}' already exists. Aborting to prevent overwrite.")
        src = _open_source(source)
        cin = int(src.shape[0]) if len(src.shape) == 4 else 1
        shape = tuple(int(s) for s in src.shape[-3:])
        L.require_device()
        # the plan for (B, Cin, patch) -- allocation only -- then the budget check, before any launch
        with inference_mode(self.model, self.compute_dtype):
            sched = self.schedule(shape, cin, np.dtype(src.dtype).itemsize, plan_bytes=lambda b: int(self._plan(b, cin).bytes_alloc))
            self.last_schedule = sched
            plan = self._plan(sched["batch"], cin)
            self._check_budget(sched, plan, shape)
            self.last_timing = _StreamRun(self, src, cin, shape, sched, plan, store, compressor).execute()
        return store


class _DeviceState:
    """The device memory of a streaming run, sized by the largest box (`cap` voxels per row) and viewed per tile: the input ring,
    the accumulators (one weight sum shared by every task), the finalize staging, the batch the network reads, the weight table
    and the zscore workspace."""

    def __init__(self, inferer, tasks, sched, cin, in_dt, cap):
        dev, (pz, py, px) = inferer.device, inferer.patch
        B, R, F = sched["batch"], sched["ring"], sched["max_finalize_rows"]
        self.cin, self.R, self.tasks = cin, R, tasks
        self.ring_flat = torch.empty((cin * R * cap,), dtype=_IN_TORCH[in_dt], device=dev)
        for tk in tasks:
            tk.alloc(R, F, cap, dev)
        self.wsum = torch.zeros((R * cap,), dtype=torch.float32, device=dev)
        # finalize blocks of n <= F rows are written as contiguous (c, n, Y, X) arrays: flat buffers, viewed per block
        self.wsum_out = torch.empty((F * cap,), dtype=torch.float32, device=dev)
        self.xb = torch.empty((B, cin, pz, py, px), dtype=torch.float32, device=dev)
        self.weights = _device_weights(inferer.blend, inferer.patch, dev)
        ws_b = ops.sw_gather_workspace(B, cin, inferer.patch) if inferer.normalization == "zscore" else 0
        self.ws = torch.empty((max(1, ws_b // 8),), dtype=torch.float64, device=dev)

    def views(self, Yb, Xb):
        """(input ring (cin, R, Yb, Xb), weight sum (R, Yb, Xb), [sum (c, R, Yb, Xb) per task]) for a tile whose box is Yb x Xb"""
        R, n = self.R, self.R * Yb * Xb
        return (self.ring_flat[:self.cin * n].view(self.cin, R, Yb, Xb), self.wsum[:n].view(R, Yb, Xb),
                [tk.sum[:tk.c * n].view(tk.c, R, Yb, Xb) for tk in self.tasks])

    def zero(self):
        """between tiles: every row was reset by its finalize, but the layout changes with the box"""
        self.wsum.zero_()
        for tk in self.tasks:
            tk.sum.zero_()


@dataclass
class _TileRun:
    """a tile while it runs: its steps (`stream_schedule`, box-local origins), the box held on the device, and its row sink"""
    index: int
    steps: list
    box: tuple
    sink: RowSink

    @property
    def plane(self):
        return self.box[1] - self.box[0], self.box[3] - self.box[2]


class _StreamRun:
    """One run of `StreamingInferer.run`, after the schedule, the plan and the budget check: device state, pinned staging, the
    store and the step loop.  A run is a sequence of tiles, each the whole z loop on its box; untiled, the one tile is the plane
    and writes whole rows.  Per step: upload its rows, pick the row's positions, run the batches, finalize."""

    def __init__(self, inferer, src, cin, shape, sched, plan, store, compressor):
        self.t_start = time.perf_counter()
        self.inf, self.src, self.cin, self.shape, self.sched, self.plan = inferer, src, cin, shape, sched, plan
        self.in_dt = np.dtype(src.dtype)
        _, Y, X = shape
        self.tiled = sched["tile"] is not None
        self.tiles = sched["tile_list"] if self.tiled else [dict(own=(0, Y, 0, X), box=(0, Y, 0, X), schedule=sched)]
        cap = max((t["box"][1] - t["box"][0]) * (t["box"][3] - t["box"][2]) for t in self.tiles)     # voxels per row, largest box
        self.tasks = [StreamTask.of(n, t, inferer.normal_keys) for n, t in inferer.targets.items()]
        self.dev = _DeviceState(inferer, self.tasks, sched, cin, self.in_dt, cap)
        self.fwd_rows = [v.row() for v in inferer.views]              # the view, applied to the patch
        self.inv_rows = [v.inverse().row() for v in inferer.views]    # its inverse, applied to the prediction
        self.occ = None                                               # counts of sw_occupancy, one per position of a z-row
        self.writers = open_store(store, self.tasks, shape, inferer.patch, compressor)
        self._alloc_staging(cap)
        self.timing = dict(read_s=0.0, write_wait_s=0.0)
        self.n_fwd = self.n_run = self.n_skipped = 0
        self.drains, self.chunk_futs = [], []
        self.stream = torch.cuda.current_stream(inferer.device)

    def _alloc_staging(self, cap):
        """host staging: two pinned input buffers and two pinned output sets, each guarded by an event (flat, like the device
        buffers: every asynchronous copy is contiguous on both sides)"""
        pz, F = self.inf.patch[0], self.sched["max_finalize_rows"]
        self.in_pin = [torch.empty((self.cin * pz * cap,), dtype=_IN_TORCH[self.in_dt]).pin_memory() for _ in range(2)]
        self.in_ev = [None, None]
        self.out_pin = [dict(w=torch.empty((F * cap,), dtype=torch.float32).pin_memory(),
                             **{tk.name: (torch.empty((tk.c * F * cap,), dtype=torch.float32).pin_memory(),
                                          torch.empty((tk.c * F * cap,), dtype=tk.tdt).pin_memory()) for tk in self.tasks})
                        for _ in range(2)]
        self.out_busy = [None, None]

    def _items(self):
        """(tile, k, step) over all tiles; a tile's sink, with its parked rows, exists from its first step"""
        inf, Z = self.inf, self.shape[0]
        pend_rows = inf.patch[0] + self.sched["max_finalize_rows"]      # at most one chunk row plus one finalize block wait
        for ti, t in enumerate(self.tiles):
            ts = t.get("schedule") or inf.tile_stream_schedule(t, Z, self.sched["batch"], self.cin, self.in_dt.itemsize)
            sink = RowSink(self.writers, self.tasks, t["own"], t["box"], pend_rows, self.tiled, inf.skip_empty is not None, self.pool)
            tile = _TileRun(ti, ts["steps"], t["box"], sink)
            for k, st in enumerate(tile.steps):
                yield tile, k, st

    def execute(self):
        """the whole run; returns `last_timing`"""
        self.pool = ThreadPoolExecutor(max_workers=self.inf.io_threads)
        self.reader = SlabReader(self.src, self.pool)
        self.drainer = ThreadPoolExecutor(max_workers=1)
        try:
            self._loop()
            for d in self.drains:
                d.result()
            t0 = time.perf_counter()
            for fu in self.chunk_futs:
                fu.result()
            self.timing["write_wait_s"] += time.perf_counter() - t0
        finally:
            self.reader.close()
            self.drainer.shutdown(wait=True)
            self.pool.shutdown(wait=True)
        self.timing.update(read_s=self.reader.read_s, total_s=time.perf_counter() - self.t_start, forwards=self.n_fwd,
                           patches=len(self.sched["positions"]), views=len(self.inf.views), tiles=len(self.tiles),
                           positions_run=self.n_run, skipped=self.n_skipped)
        return self.timing

    def _loop(self):
        it = self._items()
        cur = next(it)
        nxt = self.reader.prefetch(cur[0].box, *cur[2]["load"])
        g = -1                                                 # steps so far, over all tiles: the staging slots alternate with it
        while cur is not None:
            tile, k, st = cur
            g += 1
            if k == 0:                                         # this tile's views of the device state
                self.ring, self.wsum, self.sums = self.dev.views(*tile.plane)
                if tile.index > 0:
                    self.dev.zero()
            host = nxt.result()
            cur = next(it, None)
            if cur is not None:
                nxt = self.reader.prefetch(cur[0].box, *cur[2]["load"])
            self._upload(host, st["load"], g % 2)
            for (chunk, valid), vidx in zip(*self._row_batches(st)):
                self._forward(chunk, valid, vidx)
            self._finalize(tile, st, g % 2)

    def _upload(self, host, load, slot):
        """rows [lo, hi) of the box: host -> pinned slot -> the ring rows they live in"""
        lo, hi = load
        if hi <= lo:
            return
        if self.in_ev[slot] is not None:
            self.in_ev[slot].synchronize()
        cin, R, Yb, Xb = self.ring.shape
        pin = self.in_pin[slot][:cin * (hi - lo) * Yb * Xb].view(cin, hi - lo, Yb, Xb)
        pin.copy_(torch.from_numpy(host))
        z = lo
        while z < hi:                          # ring rows wrap: at most two contiguous pieces per channel
            r0 = z % R
            seg = min(hi - z, R - r0)
            for ci in range(cin):
                self.ring[ci, r0:r0 + seg].copy_(pin[ci, z - lo:z - lo + seg], non_blocking=True)
            z += seg
        ev = torch.cuda.Event()
        ev.record(self.stream)
        self.in_ev[slot] = ev

    def _row_batches(self, st):
        """(batches, views) of the step: the schedule's, or with skipping those of the positions kept -- one count per position
        of the row, one small read, then the batches are cut again"""
        row = row_positions(st)
        self.n_run += len(row)
        skip = self.inf.skip_empty
        if skip is None:
            return st["batches"], st["views"]
        if self.occ is None or self.occ.numel() < len(row):
            self.occ = torch.empty((len(row),), dtype=torch.int64, device=self.inf.device)
        counts = ops.sw_occupancy(self.ring, row, self.inf.patch, skip["value"], self.occ)
        keep = keep_mask(counts, self.cin * int(np.prod(self.inf.patch)), skip["min_fraction"])
        kept = [p for p, kp in zip(row, keep) if kp]
        self.n_skipped += len(row) - len(kept)
        return cut_batches(kept, self.sched["batch"], len(self.inf.views))

    def _forward(self, chunk, valid, vidx):
        """one batch: gather (as its views see the patches), the network, activation + weighted accumulation per task (moved back
        by the views' inverses); the plan's own head buffers are read before the next forward"""
        d, tta = self.dev, self.inf.tta
        ops.sw_gather(self.ring, chunk, d.xb, self.inf.normalization, d.ws, [self.fwd_rows[j] for j in vidx] if tta else None)
        outs = self.plan.run_forward(d.xb, apply_act=False)
        self.n_fwd += 1
        inv = [self.inv_rows[j] for j in vidx] if tta else None
        for i, (tk, acc) in enumerate(zip(self.tasks, self.sums)):
            ops.sw_accumulate(outs[tk.name], valid, chunk, tk.act, d.weights, acc, self.wsum if i == 0 else None, inv, tk.vector)

    def _finalize(self, tile, st, slot):
        """blend and cast the rows no later patch touches, start their D2H into the pinned slot, hand the rest to the drainer"""
        f_lo, f_hi = st["finalize"]
        n = f_hi - f_lo
        if n <= 0:
            return
        if self.out_busy[slot] is not None:                     # its previous block has been parked on the host
            t0 = time.perf_counter()
            self.out_busy[slot].result()
            self.timing["write_wait_s"] += time.perf_counter() - t0
        d, o = self.dev, self.out_pin[slot]
        Yb, Xb = tile.plane
        for i, (tk, acc) in enumerate(zip(self.tasks, self.sums)):
            ops.sw_finalize(acc, self.wsum, f_lo, n, tk.blend, tk.cast, tk.blended, tk.final, d.wsum_out if i == 0 else None,
                            reset_wsum=i == len(self.tasks) - 1)
            b, f = o[tk.name]
            m = tk.c * n * Yb * Xb
            b[:m].copy_(tk.blended[:m], non_blocking=True)
            f[:m].copy_(tk.final[:m], non_blocking=True)
        o["w"][:n * Yb * Xb].copy_(d.wsum_out[:n * Yb * Xb], non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(self.stream)
        self.out_busy[slot] = self.drainer.submit(self._drain, tile, slot, ev, f_lo, n, st["write"])
        self.drains.append(self.out_busy[slot])

    def _drain(self, tile, slot, ev, f_lo, n, write):
        """host side of one finalize block (on the drainer thread): wait for its D2H, hand numpy views of the pinned slot to the sink"""
        ev.synchronize()
        o = self.out_pin[slot]
        Yb, Xb = tile.plane
        blocks = {}
        for tk in self.tasks:
            b, f = (t[:tk.c * n * Yb * Xb].view(tk.c, n, Yb, Xb).numpy() for t in o[tk.name])
            blocks[tk.name] = (b, f.view(np.uint16) if tk.fdt == np.uint16 else f)
        self.chunk_futs.extend(tile.sink.put(f_lo, blocks, o["w"][:n * Yb * Xb].view(n, Yb, Xb).numpy(), write))


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


def _mesh_chain():
    """the mesh stages after the mesher, in the order they run: (config key, (block, max_device_bytes) -> driver, (block, store) ->
    what `run` takes beside the mesh file)"""
    from .postprocess import MeshDecimator, MeshOrienter, MeshRefiner
    return (("refine", lambda c, b: MeshRefiner(c["iterations"], c["lam"], c["mu"], c["clamp"], c["pin_boundary"], c["normals"], max_device_bytes=b),
             lambda c, store: ()),
            ("decimate", lambda c, b: MeshDecimator(c["cell"], c["representative"], c["normals"], max_device_bytes=b), lambda c, store: ()),
            ("orient", lambda c, b: MeshOrienter(c["side"], c["min_cos"], c["normals"], max_device_bytes=b),
             lambda c, store: (store, f"{c['normals_task']}_final")))


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
    pp = (mgr.infer_postprocess or {}).get("components")
    if pp:
        from .postprocess import ComponentFilter
        gb = pp["max_device_gb"]
        for task in pp["tasks"]:
            print(task, ComponentFilter(pp["level"], pp["connectivity"], pp["min_voxels"], pp["write_labels"],
                                        None if gb is None else int(gb * 2**30)).run(store, task), flush=True)
    mesh = (mgr.infer_postprocess or {}).get("mesh")
    if mesh:      # after the filter: `source: filtered` reads what it has just written
        from .postprocess import SurfaceMesher
        gb = mesh["max_device_gb"]
        for task in mesh["tasks"]:
            print(task, SurfaceMesher(mesh["level"], mesh["format"], None if gb is None else int(gb * 2**30)).run(store, task, mesh["source"]),
                  flush=True)
    newest = {task: os.path.join(store, f"{task}_{mesh['source']}.{mesh['format']}") for task in mesh["tasks"]} if mesh else {}
    for key, make, more in _mesh_chain():      # every stage reads the newest mesh file of its task: the stage's before it, else the mesher's
        c = (mgr.infer_postprocess or {}).get(key)
        if not c:
            continue
        gb = c["max_device_gb"]
        for task in c["tasks"]:
            stage = make(c, None if gb is None else int(gb * 2**30))
            print(task, stage.run(newest[task], *more(c, store)), flush=True)
            newest[task] = f"{os.path.splitext(newest[task])[0]}_{stage.suffix}.{mesh['format']}"
    return store


if __name__ == "__main__":
    main()
