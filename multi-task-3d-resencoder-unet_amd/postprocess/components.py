"""Connected-component filtering of a prediction: the numpy statements of csrc/rx_components.hip, the host half of the out-of-core
run, the config block and the driver.

The label of a foreground voxel is 1 + the smallest linear index z*Y*X + y*X + x over its component.  That canonical label is a
property of the mask alone, so every layer -- the statements here, the kernels, a slab labelled twice -- produces the same integers
and everything downstream compares with array_equal.  The statements use numpy only (no scipy, no torch)."""
import json
import os
import shutil

import numpy as np

CONNECTIVITIES = (6, 18, 26)
INT32_MAX = 2**31 - 1
BYTES_PER_VOXEL = 9      # on the device: the values (1), the labels (4), the sizes (4) of one slab, allocated once per run and reused
SCRATCH_ELEMENTS = 1 << 20      # table compaction, scatter and gather work on this many elements at a time: <= 32 MiB of transients
KEY = "inference_config.postprocess.components"


def _max_steps(connectivity):
    if isinstance(connectivity, bool) or connectivity not in CONNECTIVITIES:
        raise ValueError(f"connectivity {connectivity!r} (6, 18 or 26)")
    return {6: 1, 18: 2, 26: 3}[connectivity]


def _union_pairs(n, a, b):
    """the forest of `n` nodes after joining a[i] with b[i] for every i: parent int64[n], every node pointing at the SMALLEST node
    of its component.  Rounds of "hook the larger root under the smaller, then point everybody at their root": every tree that
    still has an edge to another one either hooks or is hooked onto, so the number of such trees at least halves per round --
    O(log n) rounds of whole-array numpy, whatever the diameter of the graph."""
    parent = np.arange(n, dtype=np.int64)
    a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
    while a.size:
        pa, pb = parent[a], parent[b]
        live = pa != pb
        if not live.any():
            break
        a, b, pa, pb = a[live], b[live], pa[live], pb[live]
        np.minimum.at(parent, np.maximum(pa, pb), np.minimum(pa, pb))
        while True:
            pp = parent[parent]
            if np.array_equal(pp, parent):
                break
            parent = pp
    return parent


def label_numpy(mask, connectivity):
    """(Z, Y, X) bool mask -> int32 (Z, Y, X): 0 on background, else 1 + the smallest linear index of the voxel's component under
    `connectivity` 6, 18 or 26.  Union-find over x-runs: a row's runs are found by one diff, the runs of neighbouring rows that touch
    by two searches in the sorted run table, and the run graph is collapsed by `_union_pairs`."""
    steps = _max_steps(connectivity)
    mask = np.asarray(mask)
    if mask.ndim != 3 or mask.dtype != np.bool_:
        raise ValueError(f"label_numpy: expected a (Z, Y, X) bool mask, got {mask.dtype} {mask.shape}")
    Z, Y, X = mask.shape
    if mask.size > INT32_MAX - 1:
        raise ValueError(f"label_numpy: {mask.size} voxels (at most 2^31 - 2: a label is an index + 1 in int32)")
    labels = np.zeros(mask.shape, np.int32)
    if not mask.size:
        return labels
    rows = mask.reshape(Z * Y, X)
    edge = np.diff(np.pad(rows, ((0, 0), (1, 1))).astype(np.int8), axis=1)      # (rows, X + 1): +1 at a run's start, -1 past its end
    row, x0 = np.nonzero(edge == 1)      # sorted by (row, x0): run k's first voxel has the k-th smallest linear index of all runs
    x1 = np.nonzero(edge == -1)[1]
    if not row.size:
        return labels
    W = X + 2      # a key = row * W + x separates the rows even for x = -1 and x = X + 1
    start_key, end_key = row * W + x0, row * W + x1
    z, y = row // Y, row % Y
    pa, pb = [], []
    for dz, dy in ((0, -1), (-1, -1), (-1, 0), (-1, 1)):
        n = (dz != 0) + (dy != 0)
        if n > steps:
            continue
        reach = 1 if n + 1 <= steps else 0      # how far along x a neighbour in that row may be
        ok = np.nonzero((z + dz >= 0) & (y + dy >= 0) & (y + dy < Y))[0]
        other = (row[ok] + dz * Y + dy) * W
        lo = np.searchsorted(end_key, other + x0[ok] - reach, side="right")      # the first run there that ends past x0 - reach
        hi = np.searchsorted(start_key, other + x1[ok] + reach, side="left")     # the first one that starts at x1 + reach or later
        cnt = np.maximum(hi - lo, 0)
        pa.append(np.repeat(ok, cnt))
        pb.append(np.repeat(lo, cnt) + (np.arange(cnt.sum()) - np.repeat(np.cumsum(cnt) - cnt, cnt)))
    parent = _union_pairs(row.size, np.concatenate(pa), np.concatenate(pb))
    run_label = (row[parent] * X + x0[parent] + 1).astype(np.int32)
    labels.reshape(-1)[mask.reshape(-1)] = np.repeat(run_label, x1 - x0)
    return labels


def label_values_numpy(values, level, connectivity):
    """`label_numpy(values > level, connectivity)`: the form `ComponentFilter(labeler=...)` takes"""
    return label_numpy(np.asarray(values) > level, connectivity)


def component_sizes_numpy(labels):
    """int32 (Z, Y, X) labels -> int32 (Z*Y*X,): at index root = label - 1 the voxel count of that component, 0 everywhere else"""
    labels = np.asarray(labels)
    fg = labels.reshape(-1)
    return np.bincount(fg[fg > 0].astype(np.int64) - 1, minlength=labels.size).astype(np.int32)


def filter_numpy(values, level, connectivity, min_voxels):
    """uint8 (Z, Y, X) values -> (filtered uint8, labels int32): the mask is `values > level`; `filtered` is `values` where the voxel's
    component has at least `min_voxels` voxels, else 0"""
    values = np.asarray(values)
    if values.dtype != np.uint8 or values.ndim != 3:
        raise ValueError(f"filter_numpy: expected (Z, Y, X) uint8 values, got {values.dtype} {values.shape}")
    labels = label_numpy(values > level, connectivity)
    sizes = component_sizes_numpy(labels)
    keep = (labels > 0) & (sizes[np.maximum(labels, 1) - 1] >= min_voxels)
    return np.where(keep, values, np.uint8(0)), labels


def merge_slabs(tables, seams, connectivity, starts):
    """The host half of the out-of-core run: slabs labelled on their own -> the components of the whole volume.

    tables[k] = (roots int32[K_k] ascending, sizes int32[K_k]) of slab k, which begins at row starts[k]; seams[k] = (the bottom label
    plane of slab k, the top label plane of slab k + 1), both int32 (Y, X) with slab-local labels.  The global id of a local root is
    the int64 starts[k] * Y * X + root: its linear index in the whole volume.  Across a seam the 1, 5 or 9 in-plane offsets that
    `connectivity` allows one z-step apart are joined, always the larger id under the smaller, so a global root is its component's
    smallest linear index.  Returns, per slab, (global root int64[K_k], global size int64[K_k]) of each local root."""
    steps = _max_steps(connectivity)
    if len(seams) != max(len(tables) - 1, 0) or len(starts) != len(tables):
        raise ValueError(f"merge_slabs: {len(tables)} slabs need {max(len(tables) - 1, 0)} seams and {len(tables)} starts")
    roots = [np.asarray(t[0], np.int64) for t in tables]
    base = np.concatenate([[0], np.cumsum([r.size for r in roots])])      # slab k's roots are nodes base[k] .. base[k + 1]
    pa, pb = [], []
    for k, (bottom, top) in enumerate(seams):
        bottom, top = np.asarray(bottom), np.asarray(top)
        Y, X = bottom.shape
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                if 1 + (dy != 0) + (dx != 0) > steps:
                    continue
                b = bottom[max(-dy, 0):Y - max(dy, 0), max(-dx, 0):X - max(dx, 0)]      # (y, x) of the slab above the seam ...
                t = top[max(dy, 0):Y - max(-dy, 0), max(dx, 0):X - max(-dx, 0)]         # ... and (y + dy, x + dx) below it
                both = (b > 0) & (t > 0)
                if not both.any():
                    continue
                pair = np.unique(np.stack([b[both], t[both]], 1), axis=0).astype(np.int64)
                pa.append(base[k] + np.searchsorted(roots[k], pair[:, 0] - 1))
                pb.append(base[k + 1] + np.searchsorted(roots[k + 1], pair[:, 1] - 1))
    n = int(base[-1])
    parent = _union_pairs(n, np.concatenate(pa) if pa else [], np.concatenate(pb) if pb else [])
    if seams:
        plane = int(np.asarray(seams[0][0]).size)
    else:
        plane = 0      # one slab: its ids are its roots
    gid = np.concatenate([r + int(s) * plane for r, s in zip(roots, starts)]) if n else np.zeros(0, np.int64)
    total = np.zeros(n, np.int64)
    np.add.at(total, parent, np.concatenate([np.asarray(t[1], np.int64) for t in tables]) if n else np.zeros(0, np.int64))
    return [(gid[parent[base[k]:base[k + 1]]], total[parent[base[k]:base[k + 1]]]) for k in range(len(tables))]


# ---- the config block ----------------------------------------------------------------------------------------------------------------------
_DEFAULTS = dict(level=127, connectivity=26, write_labels=False, max_device_gb=None)


def _int(key, v, lo, hi):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= int(v) <= hi:
        raise ValueError(f"{KEY}.{key}: {v!r} (an integer {lo} .. {hi})")
    return int(v)


def _check_options(level, connectivity, min_voxels):
    """the three numbers every entry point takes, refused by key"""
    level = _int("level", level, 0, 254)
    if isinstance(connectivity, bool) or connectivity not in CONNECTIVITIES:
        raise ValueError(f"{KEY}.connectivity: {connectivity!r} (6, 18 or 26)")
    return level, int(connectivity), _int("min_voxels", min_voxels, 1, INT32_MAX)


def parse_config(block, targets, patch_size=None):
    """`inference_config.postprocess` -> None when absent, else {"components": {tasks, level, connectivity, min_voxels, write_labels,
    max_device_gb}} and / or {"mesh": {tasks, source, level, format, max_device_gb}} (isosurface.parse_mesh_config) and / or
    {"refine": {...}} (refine.parse_refine_config) and / or {"decimate": {...}} (decimate.parse_decimate_config) and / or
    {"orient": {...}} (orient.parse_orient_config), whichever the block holds.  Unknown keys and bad values raise ValueError naming the key; `targets` is {task: {"channels": c, ...}}."""
    if block is None:
        return None
    if not isinstance(block, dict):
        raise ValueError(f"inference_config.postprocess: expected a mapping, got {block!r}")
    for k in block:
        if k not in ("components", "mesh", "refine", "decimate", "orient"):
            raise ValueError(f"inference_config.postprocess.{k}: unknown key (components, mesh, refine, decimate), or orient")
    out = _parse_components(block["components"], targets, patch_size) if "components" in block else {}
    if "mesh" in block:
        from .isosurface import parse_mesh_config
        out["mesh"] = parse_mesh_config(block["mesh"], targets, patch_size, out["components"]["tasks"] if "components" in out else None)
    if "refine" in block:      # a sibling of `mesh`, whose parsed dict stays as it is
        from .refine import parse_refine_config
        out["refine"] = parse_refine_config(block["refine"], out["mesh"]["tasks"] if "mesh" in out else None)
    if "decimate" in block:      # another sibling: it reads the refiner's file where there is one, else the mesher's
        from .decimate import parse_decimate_config
        out["decimate"] = parse_decimate_config(block["decimate"], out["mesh"]["tasks"] if "mesh" in out else None)
    if "orient" in block:      # the last sibling: it reads the newest mesh file of the chain and the store of the normals task
        from .orient import parse_orient_config
        out["orient"] = parse_orient_config(block["orient"], out["mesh"]["tasks"] if "mesh" in out else None, targets)
    return out or None


def _parse_components(c, targets, patch_size):
    """the `components` block -> {"components": {...}}"""
    if not isinstance(c, dict):
        raise ValueError(f"{KEY}: expected a mapping, got {c!r}")
    known = ("tasks", "min_voxels") + tuple(_DEFAULTS)
    for k in c:
        if k not in known:
            raise ValueError(f"{KEY}.{k}: unknown key ({', '.join(known)})")
    if patch_size is not None and len(tuple(patch_size)) != 3:
        raise ValueError(f"{KEY}: a {len(tuple(patch_size))}-D patch_size {tuple(patch_size)}: components are labelled in (Z, Y, X) volumes only")
    tasks = c.get("tasks")
    if isinstance(tasks, str):
        tasks = [tasks]
    if not isinstance(tasks, (list, tuple)) or not tasks:
        raise ValueError(f"{KEY}.tasks: {tasks!r} (a list of task names)")
    for t in tasks:
        if t not in targets:
            raise ValueError(f"{KEY}.tasks: unknown task {t!r} (one of {', '.join(targets)})")
        if int(targets[t].get("channels", 1)) != 1:
            raise ValueError(f"{KEY}.tasks: task {t!r} has {targets[t].get('channels')} channels (single-channel tasks only)")
    if "min_voxels" not in c:
        raise ValueError(f"{KEY}.min_voxels: required")
    level, connectivity, min_voxels = _check_options(c.get("level", _DEFAULTS["level"]), c.get("connectivity", _DEFAULTS["connectivity"]),
                                                    c["min_voxels"])
    wl = c.get("write_labels", False)
    if not isinstance(wl, bool):
        raise ValueError(f"{KEY}.write_labels: {wl!r} (true or false)")
    gb = c.get("max_device_gb")
    if gb is not None and (isinstance(gb, bool) or not isinstance(gb, (int, float)) or not gb > 0):
        raise ValueError(f"{KEY}.max_device_gb: {gb!r} (a positive number)")
    return {"components": dict(tasks=tuple(tasks), level=level, connectivity=connectivity, min_voxels=min_voxels, write_labels=wl,
                               max_device_gb=None if gb is None else float(gb))}


# ---- the driver ----------------------------------------------------------------------------------------------------------------------------
class _Rows:
    """takes blocks of consecutive rows of any depth and hands whole chunk rows on to a `ChunkedWriter`"""

    def __init__(self, writer):
        self.w, self.z0, self.held = writer, 0, []

    def put(self, block, last):
        self.held.append(block)
        n = sum(b.shape[0] for b in self.held)
        take = n if last else n - n % self.w.chunks[0]
        if take:
            rows = np.concatenate(self.held) if len(self.held) > 1 else self.held[0]
            self.w.write_rows(self.z0, np.ascontiguousarray(rows[:take]))
            self.z0 += take
            self.held = [rows[take:]] if take < n else []


class _HostSlab:
    """one slab through `labeler`: numpy all the way"""

    def __init__(self, labeler, level, connectivity, min_voxels):
        self.labeler, self.level, self.connectivity, self.min_voxels = labeler, level, connectivity, min_voxels

    def load(self, values):
        self.v = values
        self.labels = np.asarray(self.labeler(values, self.level, self.connectivity), np.int32)
        self.sizes = component_sizes_numpy(self.labels)

    def seam_planes(self):
        return self.labels[0].copy(), self.labels[-1].copy()

    def table(self):
        roots = np.nonzero(self.sizes)[0]
        return roots.astype(np.int32), self.sizes[roots]

    def set_sizes(self, roots, sizes):
        self.sizes[roots] = sizes

    def filtered(self):
        keep = (self.labels > 0) & (self.sizes[np.maximum(self.labels, 1) - 1] >= self.min_voxels)
        return np.where(keep, self.v, np.uint8(0))

    def compact_labels(self, roots, ids):
        table = np.zeros(self.sizes.size, np.uint32)
        table[roots] = ids
        return np.where(self.labels > 0, table[np.maximum(self.labels, 1) - 1], np.uint32(0)).astype(np.uint32)


class _DeviceSlab:
    """one slab on the device.  The three buffers -- values, labels, sizes: 9 bytes per voxel of the deepest slab -- are allocated
    once and every slab of both passes is loaded into them; the table compaction, the scatter of global sizes and the gather of
    compact ids walk them SCRATCH_ELEMENTS at a time, so what they allocate on the side does not grow with the volume."""

    def __init__(self, depth, Y, X, level, connectivity, min_voxels):
        import torch
        self.level, self.connectivity, self.min_voxels, self.plane = level, connectivity, min_voxels, (Y, X)
        n = depth * Y * X
        self.vbuf = torch.empty(n, dtype=torch.uint8, device="cuda")
        self.lbuf = torch.empty(n, dtype=torch.int32, device="cuda")
        self.sbuf = torch.empty(n, dtype=torch.int32, device="cuda")

    def load(self, values):
        import torch
        from ..engine import ops
        n = values.size
        shape = (1, 1, values.shape[0]) + self.plane
        self.v, self.labels, self.sizes = self.vbuf[:n].view(shape), self.lbuf[:n].view(shape), self.sbuf[:n].view(1, 1, n)
        self.v.copy_(torch.from_numpy(np.ascontiguousarray(values)).view(shape))
        ops.cc_label(self.v, self.level, self.connectivity, out=self.labels)
        ops.cc_sizes(self.labels, out=self.sizes)

    def seam_planes(self):
        return self.labels[0, 0, 0].cpu().numpy(), self.labels[0, 0, -1].cpu().numpy()

    def table(self):
        import torch
        s = self.sizes.view(-1)
        roots, sizes = [], []
        for a in range(0, s.numel(), SCRATCH_ELEMENTS):      # compaction with torch.nonzero is plumbing, kept to a fixed working set
            part = s[a:a + SCRATCH_ELEMENTS]
            idx = torch.nonzero(part).view(-1)
            roots.append((idx + a).to(torch.int32).cpu().numpy())
            sizes.append(part[idx].cpu().numpy())
        return np.concatenate(roots), np.concatenate(sizes)

    def _scatter(self, roots, values):
        import torch
        s = self.sizes.view(-1)
        for a in range(0, roots.size, SCRATCH_ELEMENTS):
            r = torch.from_numpy(roots[a:a + SCRATCH_ELEMENTS].astype(np.int64)).cuda()
            s[r] = torch.from_numpy(np.ascontiguousarray(values[a:a + SCRATCH_ELEMENTS], np.int32)).cuda()

    def set_sizes(self, roots, sizes):
        self._scatter(roots, sizes)

    def filtered(self):
        from ..engine import ops
        return ops.cc_filter(self.v, self.labels, self.sizes, self.min_voxels, out=self.v)[0, 0].cpu().numpy()

    def compact_labels(self, roots, ids):
        """after `filtered`: the sizes buffer becomes the id table, and the labels are replaced by their ids in place, a piece at a time"""
        self.sizes.zero_()
        self._scatter(roots, ids.astype(np.int64))
        s, lab = self.sizes.view(-1), self.labels.view(-1)
        for a in range(0, lab.numel(), SCRATCH_ELEMENTS):
            part = lab[a:a + SCRATCH_ELEMENTS]
            fg = part > 0
            part.copy_(s[(part - 1).clamp_(min=0).long()] * fg)
        return self.labels[0, 0].cpu().numpy().astype(np.uint32)


class ComponentFilter:
    """Removes the small connected components of `<store>/<task>_final` (a single-channel (Z, Y, X) uint8 array): writes
    `<task>_filtered` -- `_final` where `_final > level` lies in a component of at least `min_voxels` voxels, 0 elsewhere -- and, with
    `write_labels`, `<task>_labels`: uint32, the kept components numbered 1 .. K in ascending order of their smallest linear index.
    Both are written under a temporary name and renamed when the run has succeeded; a failed run leaves nothing behind.

    The volume is labelled in slabs of `slab` rows (full planes).  Device memory is 9 bytes per voxel of a slab -- three buffers
    allocated once and reused by every slab, with or without `write_labels` -- plus at most 32 MiB of scratch that does not grow with
    the volume and that the budget does not count.  `slab` defaults to the whole volume if that fits `max_device_bytes` (default:
    half of the free device memory), else to the largest depth that does.
    One slab: label, sizes, filter, write.  Several: pass 1 labels every slab and keeps its seam planes and its (roots, sizes) table;
    `merge_slabs` joins them on the host; pass 2 labels every slab again -- the labels are canonical, so they are the same -- and
    filters it against the global sizes.  `labeler`: None runs the HIP kernels; a callable (values uint8, level, connectivity) ->
    labels replaces them (sizes by bincount), which is how the whole two-pass path runs on the host with `label_numpy`.
    `last_slab` is the depth the last run used."""

    def __init__(self, level=127, connectivity=26, min_voxels=1, write_labels=False, max_device_bytes=None, slab=None, labeler=None):
        self.level, self.connectivity, self.min_voxels = _check_options(level, connectivity, min_voxels)
        self.write_labels = bool(write_labels)
        if max_device_bytes is not None and int(max_device_bytes) < 1:
            raise ValueError(f"{KEY}.max_device_gb: {max_device_bytes} bytes")
        if slab is not None and (isinstance(slab, bool) or int(slab) < 1):
            raise ValueError(f"ComponentFilter: slab {slab!r} (a positive number of rows)")
        self.max_device_bytes = None if max_device_bytes is None else int(max_device_bytes)
        self.slab = None if slab is None else int(slab)
        self.labeler = labeler
        self.last_slab = None

    # -- slab depth ----------------------------------------------------------------------------------------------------------------
    def slab_depth(self, shape):
        Z, Y, X = shape
        most = (INT32_MAX - 1) // (Y * X)      # rows of a slab whose labels (index + 1) still fit int32
        if most < min(2, Z):
            raise ValueError(f"ComponentFilter: two slices of a {Y} x {X} plane are more than 2^31 - 2 voxels, the most a slab can hold")
        if self.slab is not None:
            if min(self.slab, Z) > most:
                raise ValueError(f"ComponentFilter: slab {self.slab}: {min(self.slab, Z)} rows of a {Y} x {X} plane are more than "
                                 f"2^31 - 2 voxels (at most {most} rows)")
            return min(self.slab, Z)
        budget = self.max_device_bytes
        if budget is None:
            if self.labeler is not None:
                return min(Z, most)
            import torch
            budget = torch.cuda.mem_get_info()[0] // 2
        depth = min(Z, budget // (BYTES_PER_VOXEL * Y * X), most)
        if depth < min(2, Z):
            raise MemoryError(f"ComponentFilter: two slices of a {Y} x {X} plane need {2 * BYTES_PER_VOXEL * Y * X} bytes on the device "
                              f"({BYTES_PER_VOXEL} per voxel), the budget is {budget}")
        return int(depth)

    # -- the run ---------------------------------------------------------------------------------------------------------------------
    def run(self, store, task):
        from ..dataloading import zarr_lite
        src_path = os.path.join(str(store), f"{task}_final")
        try:
            src = zarr_lite.open(src_path)
        except zarr_lite.ZarrLiteError as e:
            raise ValueError(f"ComponentFilter: task {task!r}: {e}") from None
        if src.ndim != 3 or src.dtype != np.uint8:
            raise ValueError(f"ComponentFilter: task {task!r}: {src_path} is {src.dtype} {src.shape}; a single-channel (Z, Y, X) uint8 "
                             f"array is required")
        depth = self.slab_depth(src.shape)
        self.last_slab = depth
        names = [f"{task}_filtered"] + ([f"{task}_labels"] if self.write_labels else [])
        final = [os.path.join(str(store), n) for n in names]
        for p in final:
            if os.path.exists(p):
                raise FileExistsError(f"{p} already exists")
        partial = [p + ".partial" for p in final]
        try:
            for p in partial:
                shutil.rmtree(p, ignore_errors=True)      # what a killed run left
            summary = self._run(src, depth, partial)
            with open(os.path.join(partial[0], ".zattrs"), "w") as fh:
                json.dump(summary, fh)
            for a, b in zip(partial, final):
                os.rename(a, b)
        except BaseException:
            for p in partial:
                shutil.rmtree(p, ignore_errors=True)
            raise
        return summary

    def _run(self, src, depth, paths):
        from ..dataloading import zarr_lite
        Z, Y, X = src.shape
        # the source's convention: its chunks and dimension separator; compressed like it (the writer has zlib only, so a gzip source
        # gives zlib chunks) or not at all
        how = dict(compressor=None if src.compressor is None else "zlib", dimension_separator=src.dimension_separator)
        out = _Rows(zarr_lite.ChunkedWriter(paths[0], src.shape, src.chunks, np.uint8, **how))
        lab = _Rows(zarr_lite.ChunkedWriter(paths[1], src.shape, src.chunks, np.uint32, **how)) if self.write_labels else None
        starts = list(range(0, Z, depth))
        slab = _HostSlab(self.labeler, self.level, self.connectivity, self.min_voxels) if self.labeler is not None else \
            _DeviceSlab(depth, Y, X, self.level, self.connectivity, self.min_voxels)

        if len(starts) == 1:
            slab.load(src[...])
            tables = [slab.table()]
            groots, gsizes = [tables[0][0].astype(np.int64)], [tables[0][1].astype(np.int64)]
        else:
            tables, seams, prev_bottom = [], [], None
            for z0 in starts:      # pass 1
                slab.load(src[z0:z0 + depth])
                top, bottom = slab.seam_planes()
                if prev_bottom is not None:
                    seams.append((prev_bottom, top))
                prev_bottom = bottom
                tables.append(slab.table())
            merged = merge_slabs(tables, seams, self.connectivity, starts)
            groots, gsizes = [m[0] for m in merged], [m[1] for m in merged]

        all_roots, all_sizes = np.concatenate(groots), np.concatenate(gsizes)
        comp_roots, where = np.unique(all_roots, return_index=True)      # ascending global root
        comp_sizes = all_sizes[where]
        kept = comp_sizes >= self.min_voxels
        kept_roots = comp_roots[kept]
        summary = dict(level=self.level, connectivity=self.connectivity, min_voxels=self.min_voxels, components=int(comp_roots.size),
                       kept=int(kept.sum()), voxels=int(comp_sizes.sum()), kept_voxels=int(comp_sizes[kept].sum()),
                       largest=[int(s) for s in np.sort(comp_sizes)[::-1][:10]])

        def compact(k):      # the compact id (1 .. K, 0 = dropped) of every local root of slab k
            return np.where(np.isin(groots[k], kept_roots), np.searchsorted(kept_roots, groots[k]) + 1, 0).astype(np.uint32)

        for k, z0 in enumerate(starts):
            last = k == len(starts) - 1
            if len(starts) > 1:      # pass 2; one slab is still loaded and its own sizes are the global ones
                slab.load(src[z0:z0 + depth])
                slab.set_sizes(tables[k][0], np.minimum(gsizes[k], INT32_MAX).astype(np.int32))
            out.put(slab.filtered(), last)
            if lab is not None:
                lab.put(slab.compact_labels(tables[k][0], compact(k)), last)
        return summary
