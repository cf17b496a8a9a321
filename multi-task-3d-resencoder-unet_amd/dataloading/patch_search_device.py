"""The valid-patch search -- the reference's `helpers._find_valid_patches` (+ `_check_patch_chunk`, `find_label_bounding_box`), here
`dataset.find_valid_patches` -- with its voxel work on the device (csrc/rx_patchsearch.hip: rx_box_stats).

What the search asks of a candidate patch is two numbers: `np.count_nonzero(patch)` and the bounding box of
`np.argwhere(patch > 0)`.  `box_stats_numpy` states both for a list of boxes in plain numpy (the oracle of the GPU tests):

    count[i] = voxels != 0 of box i;   ext[i] = (minz, maxz, miny, maxy, minx, maxx) of its voxels > 0, box-local,
    (dz, -1, dy, -1, dx, -1) when there is none (the reference's empty record, as `find_label_bounding_box` returns it).

`find_valid_patches_device` takes those integers from the device and applies the three tests on the host with the Python
expressions of `find_valid_patches`, over the same `range`s: the decisions are the same, never rounded differently, and the list
that comes back is that function's list, order included.  The label bounding box is the same kernel on one box per slab.

`parse_patch_search` reads `dataset_config.patch_search` ({where: host | device, max_device_gb: > 0}; absent: {where: host}, the
host search)."""
import time

import numpy as np

from . import stages

BUDGET_FRACTION = 0.5      # max_device_bytes=None: this share of the device's free bytes
MAX_BOXES_PER_CALL = 1 << 20
DTYPES = (np.dtype(np.uint8), np.dtype(np.uint16), np.dtype(np.float32))

last_timing = {}           # what the last find_valid_patches_device call did and where its time went (see its docstring)


def box_stats_numpy(arr, boxes):
    """what rx_box_stats computes, in numpy: `arr` (Z, Y, X), `boxes` (N, 6) rows (z0, y0, x0, dz, dy, dx) inside it ->
    (count uint64 [N], ext int32 [N, 6])"""
    arr = np.asarray(arr)
    boxes = np.asarray(boxes)
    if arr.ndim != 3 or boxes.ndim != 2 or boxes.shape[1] != 6:
        raise ValueError(f"box_stats_numpy: expected a (Z, Y, X) array and (N, 6) boxes, got {arr.shape} and {boxes.shape}")
    count = np.zeros(len(boxes), np.uint64)
    ext = np.zeros((len(boxes), 6), np.int32)
    for i, (z0, y0, x0, dz, dy, dx) in enumerate(boxes.tolist()):
        if min(dz, dy, dx) <= 0 or min(z0, y0, x0) < 0 or z0 + dz > arr.shape[0] or y0 + dy > arr.shape[1] or x0 + dx > arr.shape[2]:
            raise ValueError(f"box_stats_numpy: box {i} {(z0, y0, x0, dz, dy, dx)} is empty or leaves the {arr.shape} array")
        patch = arr[z0:z0 + dz, y0:y0 + dy, x0:x0 + dx]
        count[i] = np.count_nonzero(patch)
        with np.errstate(invalid="ignore"):
            nz = np.argwhere(patch > 0)
        if nz.size == 0:
            ext[i] = (dz, -1, dy, -1, dx, -1)
        else:
            lo, hi = nz.min(axis=0), nz.max(axis=0)
            ext[i] = (lo[0], hi[0], lo[1], hi[1], lo[2], hi[2])
    return count, ext


def candidate_starts(bbox, patch_size):
    """the start positions `find_valid_patches` visits, per axis: its `range`s (half-patch steps, at least 1)"""
    return [list(range(bbox[2 * d], bbox[2 * d + 1] - patch_size[d] + 2, max(patch_size[d] // 2, 1))) for d in range(3)]


def decide(count, ext, patch_vol, bbox_threshold, label_threshold):
    """the three tests of `find_valid_patches` on one candidate's integers: "empty", "bbox", "label" (the rule that rejects it)
    or None (kept).  Same expressions, same order."""
    if ext[1] < 0:
        return "empty"
    ez, ey, ex = ext[1] - ext[0] + 1, ext[3] - ext[2] + 1, ext[5] - ext[4] + 1
    if float(ez * ey * ex) / patch_vol < bbox_threshold:
        return "bbox"
    if count / patch_vol < label_threshold:
        return "label"
    return None


def parse_patch_search(dataset_config):
    """`dataset_config.patch_search` -> {"where": "host" | "device", "max_device_bytes": None | int}.  An absent block is
    {where: host}.  Unknown keys, a `where` that is neither host nor device and a `max_device_gb` that is not a positive number
    raise with the key named."""
    d = stages.block(dataset_config, "patch_search", ("where", "max_device_gb"), "host", {})
    gb = d.get("max_device_gb", None)
    if gb is not None:
        if isinstance(gb, bool) or not isinstance(gb, (int, float, np.integer, np.floating)) or not float(gb) > 0 or not np.isfinite(gb):
            raise ValueError(f"dataset_config.patch_search.max_device_gb: {gb!r} (a positive number of GiB)")
        gb = int(float(gb) * (1 << 30))
    return {"where": d["where"], "max_device_bytes": gb}


def _pieces(arr, z0, z1, y0, y1):
    """[(za, zb, ya, yb)]: rows [z0, z1) x columns [y0, y1) cut at the store's chunk boundaries in z and y (one piece per chunk
    row and column; every chunk is then decompressed by exactly one piece)"""
    chunks = getattr(arr, "chunks", None)
    if chunks is None or len(chunks) != 3:
        return [(z0, z1, y0, y1)]
    cz, cy = max(int(chunks[0]), 1), max(int(chunks[1]), 1)
    zs = [z0] + list(range((z0 // cz + 1) * cz, z1, cz)) + [z1]
    ys = [y0] + list(range((y0 // cy + 1) * cy, y1, cy)) + [y1]
    return [(za, zb, ya, yb) for za, zb in zip(zs[:-1], zs[1:]) for ya, yb in zip(ys[:-1], ys[1:])]


def _read_region(arr, pool, region, timing):
    """the (z0, z1, y0, y1, x0, x1) region of `arr` as one contiguous host array, its chunk-aligned pieces read on the pool (zlib
    releases the GIL), as `StreamingInferer` reads its slabs"""
    z0, z1, y0, y1, x0, x1 = region
    t0 = time.perf_counter()
    out = np.empty((z1 - z0, y1 - y0, x1 - x0), arr.dtype)

    def piece(za, zb, ya, yb):
        out[za - z0:zb - z0, ya - y0:yb - y0] = arr[za:zb, ya:yb, x0:x1]

    for f in [pool.submit(piece, *p) for p in _pieces(arr, z0, z1, y0, y1)]:
        f.result()
    timing["read_s"] += time.perf_counter() - t0
    timing["bytes_read"] += out.nbytes
    return out


def _upload(host, device, timing):
    import torch
    t0 = time.perf_counter()
    if host.dtype == np.uint16:
        host = host.view(np.int16)      # the bits are what the kernel reads; torch moves int16 on every build
    t = torch.from_numpy(host).to(device)
    torch.cuda.synchronize(t.device)
    timing["upload_s"] += time.perf_counter() - t0
    return t


def _stats(vol, boxes, timing):
    from ..engine import ops as E
    t0 = time.perf_counter()
    counts, exts = [], []
    for i in range(0, len(boxes), MAX_BOXES_PER_CALL):
        c, e = E.box_stats(vol, boxes[i:i + MAX_BOXES_PER_CALL])
        counts.append(c), exts.append(e)
        timing["launches"] += 1
    timing["kernel_s"] += time.perf_counter() - t0
    return np.concatenate(counts), np.concatenate(exts)


def find_valid_patches_device(arr, patch_size, bbox_threshold=0.97, label_threshold=0.10, max_device_bytes=None, device="cuda",
                              io_threads=16):
    """`dataset.find_valid_patches(arr, patch_size, bbox_threshold, label_threshold)` with the voxel work on the device: the same
    list, contents and order (z outermost, x innermost).

    `arr`: 3-D, numpy-sliceable with `.shape` / `.dtype` (a numpy array, a `zarr_lite` array), uint8, uint16 or float32; anything
    else raises ValueError.  Without a gfx950 device: RxError, no fallback.

    `max_device_bytes` is what the label may occupy on the device; None takes BUDGET_FRACTION = 0.5 of the free bytes
    `torch.cuda.mem_get_info()` reports.  A label within the budget is uploaded once and both passes run on the resident copy.
    A larger one is streamed: pass A uploads z-slabs (whole chunk rows of the store where the budget allows), one box per slab,
    and merges the slabs' boxes into the label bounding box; pass B takes groups of consecutive candidate z-rows, uploads of each
    only the part of the bounding box its rows touch, and makes one launch per group (neighbouring groups share patch - step
    rows, which are read twice).  The next slab or group is read while the device works on the current one.  A budget below
    one patch-deep slab, patch_size[0] * Y * X voxels of the ARRAY's y / x extent -- which bounds the bounding box's, and is known
    before anything is read -- raises ValueError before any read or launch.

    `last_timing` (module attribute) afterwards: mode ("resident" / "streamed"), slabs_a, groups_b, launches, candidates,
    bytes_read, read_s (waiting for the store), upload_s, kernel_s (launches up to their synchronise and the copy back), host_s
    (the three tests), total_s."""
    from concurrent.futures import ThreadPoolExecutor

    import torch

    from ..engine import lib as L
    shape = tuple(int(s) for s in getattr(arr, "shape", ()))
    if len(shape) != 3 or min(shape) <= 0:
        raise ValueError(f"find_valid_patches_device: expected a non-empty 3-D (Z, Y, X) label, got shape {shape}")
    dtype = np.dtype(arr.dtype)
    if dtype not in DTYPES:
        raise ValueError(f"find_valid_patches_device: label dtype {dtype} (uint8, uint16 or float32)")
    patch = tuple(int(p) for p in patch_size)
    if len(patch) != 3 or min(patch) <= 0:
        raise ValueError(f"find_valid_patches_device: patch_size {patch_size!r} (three positive integers)")
    if isinstance(io_threads, bool) or not isinstance(io_threads, (int, np.integer)) or io_threads < 1:
        raise ValueError(f"find_valid_patches_device: io_threads {io_threads!r} (a positive integer)")
    L.require_device()
    device = torch.device(device)
    if device.type != "cuda":
        raise L.RxError(f"find_valid_patches_device: device {device} (the kernels run only on a HIP device)")
    D, H, W = shape
    pZ, pY, pX = patch
    patch_vol = pZ * pY * pX
    with torch.cuda.device(device):
        if max_device_bytes is None:
            budget = int(torch.cuda.mem_get_info()[0] * BUDGET_FRACTION)
        else:
            budget = int(max_device_bytes)
        item = dtype.itemsize
        resident = D * H * W * item <= budget
        if not resident and budget < pZ * H * W * item:
            raise ValueError(f"find_valid_patches_device: max_device_bytes {budget} is below one patch-deep slab "
                             f"({pZ} x {H} x {W} x {item} bytes = {pZ * H * W * item})")
        timing = dict(mode="resident" if resident else "streamed", slabs_a=0, groups_b=0, launches=0, candidates=0, bytes_read=0,
                      read_s=0.0, upload_s=0.0, kernel_s=0.0, host_s=0.0, total_s=0.0)
        t_start = time.perf_counter()
        pool = ThreadPoolExecutor(max_workers=int(io_threads))
        reader = ThreadPoolExecutor(max_workers=1)
        try:
            found = _search(arr, shape, patch, patch_vol, bbox_threshold, label_threshold, budget, resident, item, device, pool,
                            reader, timing)
        finally:
            reader.shutdown(wait=True)
            pool.shutdown(wait=True)
        timing["total_s"] = time.perf_counter() - t_start
    last_timing.clear()
    last_timing.update(timing)
    return found


def _prefetched(reader, arr, pool, regions, timing):
    """the regions as host arrays, in order, each read on the reader thread while the caller works on the one before"""
    io = dict(read_s=0.0, bytes_read=0)      # the reader thread's clock; the caller is charged only what it waits
    nxt = reader.submit(_read_region, arr, pool, regions[0], io) if regions else None
    for i in range(len(regions)):
        t0 = time.perf_counter()
        host = nxt.result()
        timing["read_s"] += time.perf_counter() - t0
        timing["bytes_read"] += host.nbytes
        nxt = reader.submit(_read_region, arr, pool, regions[i + 1], io) if i + 1 < len(regions) else None
        yield host


def _search(arr, shape, patch, patch_vol, bbox_threshold, label_threshold, budget, resident, item, device, pool, reader, timing):
    D, H, W = shape
    pZ, pY, pX = patch
    chunks = getattr(arr, "chunks", None)
    cz = max(int(chunks[0]), 1) if chunks is not None and len(chunks) == 3 else 1
    vol = None
    # ---- pass A: the label bounding box -----------------------------------------------------------------------------------
    if resident:
        vol = _upload(_read_region(arr, pool, (0, D, 0, H, 0, W), timing), device, timing)
        _, e = _stats(vol, np.array([[0, 0, 0, D, H, W]], np.int32), timing)
        bbox = tuple(int(v) for v in e[0])
        timing["slabs_a"] = 1
    else:
        depth = min(budget // (H * W * item), D)
        if depth >= cz:
            depth = depth // cz * cz
        lo, hi = [D, H, W], [-1, -1, -1]
        starts = list(range(0, D, depth))
        regions = [(z0, min(z0 + depth, D), 0, H, 0, W) for z0 in starts]
        for z0, host in zip(starts, _prefetched(reader, arr, pool, regions, timing)):
            slab = _upload(host, device, timing)
            _, e = _stats(slab, np.array([[0, 0, 0, host.shape[0], H, W]], np.int32), timing)
            del slab
            timing["slabs_a"] += 1
            e = [int(v) for v in e[0]]
            if e[1] >= 0:
                off = (z0, 0, 0)
                for d in range(3):
                    lo[d], hi[d] = min(lo[d], e[2 * d] + off[d]), max(hi[d], e[2 * d + 1] + off[d])
        bbox = (lo[0], hi[0], lo[1], hi[1], lo[2], hi[2])
    # ---- pass B: the candidates ---------------------------------------------------------------------------------------------
    zs, ys, xs = candidate_starts(bbox, patch)
    out = []
    if not zs or not ys or not xs:
        return out
    timing["candidates"] = len(zs) * len(ys) * len(xs)
    yx = np.array([(y, x) for y in ys for x in xs], np.int32)

    def boxes_of(z_rows, origin):
        b = np.empty((len(z_rows), len(yx), 6), np.int32)
        b[:, :, 0] = np.asarray(z_rows, np.int32)[:, None] - origin[0]
        b[:, :, 1:3] = yx[None] - np.array(origin[1:], np.int32)
        b[:, :, 3:] = patch
        return b.reshape(-1, 6)

    def tests(z_rows, count, ext):
        t0 = time.perf_counter()
        count, ext = count.tolist(), ext.tolist()
        i = 0
        for z in z_rows:
            for y in ys:
                for x in xs:
                    if decide(count[i], ext[i], patch_vol, bbox_threshold, label_threshold) is None:
                        out.append({"volume_idx": 0, "start_pos": [int(z), int(y), int(x)]})
                    i += 1
        timing["host_s"] += time.perf_counter() - t0

    if resident:
        # whole z-rows per call: the launch's outputs stay bounded whatever the candidate count
        per = max(MAX_BOXES_PER_CALL // len(yx), 1)
        for i in range(0, len(zs), per):
            c, e = _stats(vol, boxes_of(zs[i:i + per], (0, 0, 0)), timing)
            tests(zs[i:i + per], c, e)
            timing["groups_b"] += 1
        return out
    by, bx = bbox[3] - bbox[2] + 1, bbox[5] - bbox[4] + 1
    sz = max(pZ // 2, 1)
    g = (budget // (by * bx * item) - pZ) // sz + 1      # candidate z-rows per group; >= 1: by * bx <= H * W and the check above
    groups = [zs[i:i + g] for i in range(0, len(zs), g)]
    regions = [(zr[0], zr[-1] + pZ, bbox[2], bbox[3] + 1, bbox[4], bbox[5] + 1) for zr in groups]
    for zr, host in zip(groups, _prefetched(reader, arr, pool, regions, timing)):
        part = _upload(host, device, timing)
        c, e = _stats(part, boxes_of(zr, (zr[0], bbox[2], bbox[4])), timing)
        del part
        tests(zr, c, e)
        timing["groups_b"] += 1
    return out
