"""Minimal zarr **v2** array reader / writer (the `zarr` package is not in this image).

Covers what the reference's patch feeder needs from `zarr.open(path, mode='r')[z0:z1, y0:y1, x0:x1]`
(dataloading/dataset.py:103-137, helpers.py:71-128): a directory store with a `.zarray` JSON (shape, chunks, dtype,
order, fill_value, compressor, dimension_separator), chunk files `i.j.k` (or `i/j/k`), partial edge chunks stored at
full chunk size, missing chunks = fill value.  Compressors: none, `zlib`, `gzip` (Python's zlib); `blosc` and any filter
raise -- the codecs live in `numcodecs`, which is absent too.  Basic indexing only (ints and unit-step slices).
Format knowledge comes from the public zarr v2 spec; nothing here could be cross-checked against the real package."""
import builtins
import gzip
import json
import os
import zlib

import numpy as np


class ZarrLiteError(RuntimeError):
    pass


class Array:
    def __init__(self, path):
        self.path = str(path)
        meta_file = os.path.join(self.path, ".zarray")
        if not os.path.exists(meta_file):
            if os.path.exists(os.path.join(self.path, ".zgroup")):
                raise ZarrLiteError(f"{path} is a zarr GROUP; open one of its arrays (e.g. {path}/0)")
            raise ZarrLiteError(f"{path}: no .zarray (zarr v2 directory stores only)")
        with builtins.open(meta_file) as f:
            m = json.load(f)
        if m.get("zarr_format") != 2:
            raise ZarrLiteError(f"{path}: zarr_format {m.get('zarr_format')} (only v2)")
        if m.get("filters"):
            raise ZarrLiteError(f"{path}: filters {m['filters']} need numcodecs")
        comp = m.get("compressor")
        self._codec = None if comp is None else comp.get("id")
        if self._codec not in (None, "zlib", "gzip"):
            raise ZarrLiteError(f"{path}: compressor '{self._codec}' needs numcodecs (supported: none, zlib, gzip)")
        self.shape = tuple(m["shape"])
        self.chunks = tuple(m["chunks"])
        self.dtype = np.dtype(m["dtype"])
        self.order = m.get("order", "C")
        fv = m.get("fill_value")
        self.fill_value = 0 if fv is None else fv
        self._sep = m.get("dimension_separator", ".")
        self.compressor, self.dimension_separator = self._codec, self._sep      # what a writer of a sibling array needs to match
        self.ndim = len(self.shape)
        self.store = self           # `arr.store.close()` of the reference's loop is a no-op here

    def close(self):
        pass

    @property
    def size(self):
        return int(np.prod(self.shape))

    def _chunk(self, idx):
        name = self._sep.join(str(i) for i in idx)
        fn = os.path.join(self.path, *name.split("/")) if self._sep == "/" else os.path.join(self.path, name)
        if not os.path.exists(fn):
            return None
        with builtins.open(fn, "rb") as f:
            raw = f.read()
        if self._codec == "zlib":
            raw = zlib.decompress(raw)
        elif self._codec == "gzip":
            raw = gzip.decompress(raw)
        a = np.frombuffer(raw, dtype=self.dtype)
        if a.size != int(np.prod(self.chunks)):
            raise ZarrLiteError(f"{fn}: {a.size} elements, expected a full chunk of {self.chunks}")
        return a.reshape(self.chunks, order=self.order)

    def __getitem__(self, key):
        if not isinstance(key, tuple):
            key = (key,)
        if any(k is Ellipsis for k in key):
            i = key.index(Ellipsis)
            key = key[:i] + (slice(None),) * (self.ndim - len(key) + 1) + key[i + 1:]
        key = key + (slice(None),) * (self.ndim - len(key))
        lo, hi, squeeze = [], [], []
        for d, k in enumerate(key):
            if isinstance(k, (int, np.integer)):
                k = int(k) + (self.shape[d] if k < 0 else 0)
                if not 0 <= k < self.shape[d]:
                    raise IndexError(f"index {k} out of range for axis {d}")
                lo.append(k), hi.append(k + 1), squeeze.append(d)
            elif isinstance(k, slice):
                a, b, st = k.indices(self.shape[d])
                if st != 1:
                    raise ZarrLiteError("only unit-step slices")
                lo.append(a), hi.append(max(a, b))
            else:
                raise ZarrLiteError(f"unsupported index {k!r}")
        out = np.empty([h - l for l, h in zip(lo, hi)], dtype=self.dtype)
        if out.size:
            first = [l // c for l, c in zip(lo, self.chunks)]
            last = [(h - 1) // c for h, c in zip(hi, self.chunks)]
            for idx in np.ndindex(*[b - a + 1 for a, b in zip(first, last)]):
                cidx = tuple(a + i for a, i in zip(first, idx))
                src, dst = [], []
                for d, ci in enumerate(cidx):
                    c0 = ci * self.chunks[d]
                    a, b = max(lo[d], c0), min(hi[d], c0 + self.chunks[d])
                    src.append(slice(a - c0, b - c0)), dst.append(slice(a - lo[d], b - lo[d]))
                ch = self._chunk(cidx)
                out[tuple(dst)] = self.fill_value if ch is None else ch[tuple(src)]
        return out.reshape([s for d, s in enumerate(out.shape) if d not in squeeze]) if squeeze else out


def open(path, mode="r"):   # noqa: A001  (mirrors zarr.open)
    if mode != "r":
        raise ZarrLiteError("read-only (use write_array to create a store)")
    return Array(path)


def _write_meta(path, shape, chunks, dtype, compressor, fill_value, dimension_separator):
    meta = dict(zarr_format=2, shape=list(shape), chunks=list(chunks), dtype=np.dtype(dtype).str, order="C",
                fill_value=fill_value, filters=None, dimension_separator=dimension_separator,
                compressor=None if compressor is None else {"id": "zlib", "level": 1})
    with builtins.open(os.path.join(path, ".zarray"), "w") as f:
        json.dump(meta, f)


def _store_chunk(path, idx, sub, chunks, fill_value, compressor, dimension_separator):
    """one chunk: `sub` (the part inside the array) padded to the full chunk size; all-fill chunks are skipped like zarr does"""
    block = np.full(chunks, fill_value, dtype=sub.dtype)
    block[tuple(slice(0, n) for n in sub.shape)] = sub
    if not (block != fill_value).any():
        return
    raw = block.tobytes(order="C")
    if compressor == "zlib":
        raw = zlib.compress(raw, 1)
    name = dimension_separator.join(str(i) for i in idx)
    fn = os.path.join(path, *name.split("/")) if dimension_separator == "/" else os.path.join(path, name)
    os.makedirs(os.path.dirname(fn), exist_ok=True)
    with builtins.open(fn, "wb") as f:
        f.write(raw)


def write_array(path, data, chunks, compressor=None, fill_value=0, dimension_separator="."):
    """write `data` as a zarr v2 directory store (compressor None or 'zlib'); all-fill chunks are skipped like zarr does"""
    data = np.asarray(data)
    chunks = tuple(int(c) for c in chunks)
    if compressor not in (None, "zlib"):
        raise ZarrLiteError("write_array: compressor None or 'zlib'")
    os.makedirs(path, exist_ok=True)
    _write_meta(path, data.shape, chunks, data.dtype, compressor, fill_value, dimension_separator)
    grid = [(s + c - 1) // c for s, c in zip(data.shape, chunks)]
    for idx in np.ndindex(*grid):
        sl = tuple(slice(i * c, min((i + 1) * c, s)) for i, c, s in zip(idx, chunks, data.shape))
        _store_chunk(path, idx, data[sl], chunks, fill_value, compressor, dimension_separator)
    return Array(path)


class ChunkedWriter:
    """A zarr v2 array filled one block of Z rows at a time, for outputs that never exist whole on the host.

    Z is the third axis from the end ((Z, Y, X) or (C, Z, Y, X)).  `write_rows(z0, block)` takes rows [z0, z0 + n): z0 on a chunk
    boundary and n a whole number of chunk rows, or the rows up to the end of the array (the partial edge chunks are stored at full
    chunk size, as `write_array` does).  Every chunk is an independent file, so the chunk writes of one call may run on a thread
    pool (`pool.submit`; zlib releases the GIL): the call then returns the futures.  Refuses an existing path.
    `axis` names the Z axis where it is not the third from the end: 0 for a channels-last (Z, Y, X, C) array."""

    def __init__(self, path, shape, chunks, dtype, compressor=None, fill_value=0, dimension_separator=".", axis=None):
        self.path = str(path)
        self.shape = tuple(int(s) for s in shape)
        self.chunks = tuple(int(c) for c in chunks)
        self.dtype = np.dtype(dtype)
        if compressor not in (None, "zlib"):
            raise ZarrLiteError("ChunkedWriter: compressor None or 'zlib'")
        if dimension_separator not in (".", "/"):
            raise ZarrLiteError("ChunkedWriter: dimension_separator '.' or '/'")
        if len(self.shape) < 3 or len(self.chunks) != len(self.shape):
            raise ZarrLiteError(f"ChunkedWriter: shape {self.shape} / chunks {self.chunks}: need (..., Z, Y, X) and one chunk per axis")
        if os.path.exists(self.path):
            raise FileExistsError(f"{self.path} already exists")
        self.compressor, self.fill_value, self.sep = compressor, fill_value, dimension_separator
        self.axis = len(self.shape) - 3 if axis is None else int(axis)
        if not 0 <= self.axis < len(self.shape):
            raise ZarrLiteError(f"ChunkedWriter: axis {axis} of a {len(self.shape)}-dimensional array")
        os.makedirs(self.path)
        _write_meta(self.path, self.shape, self.chunks, self.dtype, compressor, fill_value, dimension_separator)

    def write_rows(self, z0, block, pool=None):
        block = np.asarray(block)
        if block.dtype != self.dtype:
            raise ZarrLiteError(f"write_rows: dtype {block.dtype}, array is {self.dtype}")
        a, cz, Z = self.axis, self.chunks[self.axis], self.shape[self.axis]
        n = block.shape[a]
        want = self.shape[:a] + (n,) + self.shape[a + 1:]
        if block.shape != want:
            raise ZarrLiteError(f"write_rows: block {block.shape}, expected {want}")
        if z0 % cz or n < 1 or z0 + n > Z or (n % cz and z0 + n != Z):
            raise ZarrLiteError(f"write_rows: rows [{z0}, {z0 + n}) are not whole chunk rows of {cz} (Z = {Z})")
        grid = [(s + c - 1) // c for s, c in zip(block.shape, self.chunks)]
        futures = []
        for idx in np.ndindex(*grid):
            sl = tuple(slice(i * c, min((i + 1) * c, s)) for i, c, s in zip(idx, self.chunks, block.shape))
            gidx = idx[:a] + (idx[a] + z0 // cz,) + idx[a + 1:]
            args = (self.path, gidx, block[sl], self.chunks, self.fill_value, self.compressor, self.sep)
            if pool is None:
                _store_chunk(*args)
            else:
                futures.append(pool.submit(_store_chunk, *args))
        return futures

    def write_block(self, z0, y0, x0, block, pool=None):
        """`write_rows` for a box of the (Z, Y, X) axes: `block` covers [z0, z0 + n) x [y0, y0 + h) x [x0, x0 + w) and every leading
        axis whole.  Each offset lies on a chunk boundary and each extent is a whole number of chunks or reaches the end of the
        array (partial edge chunks are stored at full chunk size and all-fill chunks skipped, as `write_rows` does).  Blocks that
        share no chunk may be written in any order."""
        block = np.asarray(block)
        if block.dtype != self.dtype:
            raise ZarrLiteError(f"write_block: dtype {block.dtype}, array is {self.dtype}")
        nd = len(self.shape)
        if self.axis != nd - 3:
            raise ZarrLiteError("write_block: needs a (..., Z, Y, X) array")
        lead = nd - 3
        if block.ndim != nd or block.shape[:lead] != self.shape[:lead]:
            raise ZarrLiteError(f"write_block: block {block.shape}, expected {self.shape[:lead]} + (n, h, w)")
        off = (0,) * lead + (int(z0), int(y0), int(x0))
        for d in range(lead, nd):
            o, n, c, s = off[d], block.shape[d], self.chunks[d], self.shape[d]
            if o < 0 or o % c or n < 1 or o + n > s or (n % c and o + n != s):
                raise ZarrLiteError(f"write_block: [{o}, {o + n}) on axis {d} is not whole chunks of {c} (extent {s})")
        grid = [(s + c - 1) // c for s, c in zip(block.shape, self.chunks)]
        futures = []
        for idx in np.ndindex(*grid):
            sl = tuple(slice(i * c, min((i + 1) * c, s)) for i, c, s in zip(idx, self.chunks, block.shape))
            gidx = tuple(i + o // c for i, o, c in zip(idx, off, self.chunks))
            args = (self.path, gidx, block[sl], self.chunks, self.fill_value, self.compressor, self.sep)
            if pool is None:
                _store_chunk(*args)
            else:
                futures.append(pool.submit(_store_chunk, *args))
        return futures
