"""Streaming inference, the host parts that need no device: the row sink (crop to the owned box, dead-voxel fill, parking,
chunk-row hand-off to the zarr writers) and the slab reader (chunk-column cuts, the int16 view of uint16), fed with numpy."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import mt3d_amd  # noqa: F401
from mt3d_amd import inference as inf
from mt3d_amd.dataloading import zarr_lite

PATCH, OVERLAP, SHAPE = (16, 16, 16), 0.5, (40, 32, 24)      # Z = 40 is no multiple of the step 8 or of the chunk 16
TARGETS = {"normals": {"channels": 3, "activation": "none"}, "ink": {"channels": 1, "activation": "sigmoid"}}


def _tasks():
    tasks = [inf.StreamTask.of(n, t, inf.default_normal_keys(TARGETS)) for n, t in TARGETS.items()]
    assert [(t.name, t.c, t.fdt, t.blend, t.vector) for t in tasks] == [("normals", 3, np.uint16, "unit", True),
                                                                        ("ink", 1, np.uint8, "average", False)]
    return tasks


def _truth(seed, dead=False):
    """what the device would hand over for the whole volume: blended, final (never 0, so a fill shows) and the weight sum"""
    rng = np.random.default_rng(seed)
    Z, Y, X = SHAPE
    full = {t.name: (rng.standard_normal((t.c, Z, Y, X)).astype(np.float32),
                     rng.integers(1, np.iinfo(t.fdt).max, (t.c, Z, Y, X), endpoint=True).astype(t.fdt)) for t in _tasks()}
    w = rng.uniform(0.5, 4.0, SHAPE).astype(np.float32)
    if dead:
        w[rng.random(SHAPE) < 0.3] = 0.0
        w[16:32, :16, :16] = 0.0      # a whole chunk of dead voxels
    return full, w


def _feed(sink, steps, box, full, w, rng=None):
    """the finalize blocks of `steps` for the box; with `rng`, everything outside the sink's owned box is random"""
    by0, by1, bx0, bx1 = box
    c0, c1, d0, d1 = sink.crop
    for st in steps:
        lo, hi = st["finalize"]
        if hi <= lo:
            continue
        blocks = {n: [a[:, lo:hi, by0:by1, bx0:bx1].copy() for a in pair] for n, pair in full.items()}
        wb = w[lo:hi, by0:by1, bx0:bx1].copy()
        if rng is not None:
            for arr in [a for pair in blocks.values() for a in pair] + [wb[None]]:
                own = arr[:, :, c0:c1, d0:d1].copy()
                arr[...] = rng.integers(1, 200, arr.shape).astype(arr.dtype)
                arr[:, :, c0:c1, d0:d1] = own
        assert sink.put(lo, blocks, wb, st["write"]) == []      # no pool: written before it returns


def _check_store(store, full, w, final=None):
    for t in _tasks():
        b, f = full[t.name]
        f = f if final is None else final[t.name]
        got_b, got_c, got_f = (zarr_lite.open(os.path.join(store, f"{t.name}_{k}")) for k in ("sum", "count", "final"))
        want_shape = SHAPE if t.c == 1 else (t.c,) + SHAPE      # single-channel arrays are stored (Z, Y, X)
        assert got_b.shape == got_f.shape == want_shape and got_c.shape == SHAPE
        assert got_b.chunks == got_f.chunks == (PATCH if t.c == 1 else (t.c,) + PATCH) and got_c.chunks == PATCH
        assert (got_b.dtype, got_c.dtype, got_f.dtype) == (np.float32, np.float32, t.fdt)
        assert np.array_equal(got_b[...], b[0] if t.c == 1 else b)
        assert np.array_equal(got_c[...], w)
        assert np.array_equal(got_f[...], f[0] if t.c == 1 else f)


def _untiled(tmp_path, name, full, w, fill_dead):
    tasks = _tasks()
    sched = inf.stream_schedule(SHAPE, PATCH, OVERLAP, 2)
    assert [s["finalize"] for s in sched["steps"]] == [(0, 8), (8, 16), (16, 24), (24, 40)]
    assert [s["write"] for s in sched["steps"]] == [(0, 0), (0, 16), (16, 16), (16, 40)]
    store = str(tmp_path / name)
    writers = inf.open_store(store, tasks, SHAPE, PATCH, None)
    box = (0, SHAPE[1], 0, SHAPE[2])
    sink = inf.RowSink(writers, tasks, box, box, PATCH[0] + sched["max_finalize_rows"], fill_dead=fill_dead)
    _feed(sink, sched["steps"], box, full, w)
    return store


def test_row_sink_untiled_store_equals_what_was_fed(tmp_path):
    full, w = _truth(0)
    _check_store(_untiled(tmp_path, "u", full, w, False), full, w)


def test_row_sink_tiled_writes_the_owned_boxes_only(tmp_path):
    full, w = _truth(1)
    tasks = _tasks()
    runner = inf.StreamingInferer(None, TARGETS, PATCH, batch_size=2, overlap=OVERLAP, tile=(16, 16))
    sched = runner.schedule(SHAPE)
    tiles = inf.tile_schedule(SHAPE, PATCH, OVERLAP, (16, 16))
    assert len(tiles) == 4 and any(t["box"] != t["own"] for t in tiles)
    store = str(tmp_path / "t")
    writers = inf.open_store(store, tasks, SHAPE, PATCH, None)
    rng = np.random.default_rng(2)
    for t in tiles:                                   # one sink per tile, tile after tile as the run does
        steps = runner.tile_stream_schedule(t, SHAPE[0], sched["batch"])["steps"]
        sink = inf.RowSink(writers, tasks, t["own"], t["box"], PATCH[0] + sched["max_finalize_rows"], tiled=True)
        _feed(sink, steps, t["box"], full, w, rng)
    _check_store(store, full, w)


@pytest.mark.parametrize("fill_dead", [True, False])
def test_row_sink_dead_voxels_hold_the_fill_value_only_when_skipping(tmp_path, fill_dead):
    full, w = _truth(3, dead=True)
    assert (w == 0).sum() > 1000 and all((f[:, w == 0] != 0).all() for _, f in full.values())
    final = {n: f.copy() for n, (_, f) in full.items()}
    if fill_dead:
        for f in final.values():
            f[:, w == 0] = 0
    store = _untiled(tmp_path, "d", full, w, fill_dead)
    _check_store(store, full, w, final)               # `_sum` keeps what was fed in both cases
    got = zarr_lite.open(os.path.join(store, "normals_final"))[...]
    assert ((got[:, w == 0] == 0).all()) == fill_dead


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.float32])
@pytest.mark.parametrize("four", [False, True])
def test_slab_reader_equals_the_plain_slice(tmp_path, dtype, four):
    rng = np.random.default_rng(4)
    shape = ((2,) if four else ()) + (20, 48, 40)
    data = (rng.integers(0, 65536, shape) % (256 if dtype == np.uint8 else 65536)).astype(dtype)
    if dtype == np.uint16:
        data[..., 5, 9, 5] = 40000                    # above int16: the bit pattern must survive
    path = str(tmp_path / "src")
    zarr_lite.write_array(path, data, ((2,) if four else ()) + (8, 16, 16), compressor="zlib")
    src = zarr_lite.open(path)
    box, lo, hi = (8, 40, 4, 36), 3, 17               # by0 = 8 is inside the first Y-chunk of 16; by1 = 40 inside the third
    want = data[..., lo:hi, 8:40, 4:36] if four else data[lo:hi, 8:40, 4:36][None]
    pool = ThreadPoolExecutor(max_workers=4)
    reader = inf.SlabReader(src, pool)
    try:
        assert reader.cy == 16 and reader.cin == (2 if four else 1)
        got = reader.read(box, lo, hi)
        ahead = reader.prefetch(box, lo, hi).result()
    finally:
        reader.close()
        pool.shutdown(wait=True)
    assert got.shape == want.shape == (reader.cin, 14, 32, 32)
    if dtype == np.uint16:
        assert got.dtype == np.int16 and (got < 0).any()
        assert np.array_equal(got.view(np.uint16), want)
    else:
        assert got.dtype == dtype and np.array_equal(got, want)
    assert np.array_equal(ahead, got) and reader.read_s > 0
    plain = inf.SlabReader(data, None)                # a numpy source has no chunks: one piece, the whole Y extent
    assert plain.cy == 48
    plain.close()
