"""Y/X tiles and empty-patch skipping of streaming inference, CPU side: the pure tile schedule (partition, positions, hull, the
one-tile case), an integer-valued simulation of the tiled accumulation against the whole-volume one, the three outcomes of
`tile="auto"`, `ChunkedWriter.write_block` against `write_array`, the numpy statement of the occupancy count, the re-cut of the
batches of a z-row, and the refusals of the new arguments and config keys."""
import ctypes
import os
import re

import numpy as np
import pytest

import mt3d_amd  # noqa: F401
from mt3d_amd import inference as inf
from mt3d_amd.dataloading import zarr_lite

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TARGETS = {"sheet": {"channels": 1, "activation": "sigmoid"}, "normals": {"channels": 3, "activation": "none"}}

# extents 16..70 (every residue of the steps below, Y == py apart), with irregular forced last positions among them
EXTENTS = [16, 17, 18, 23, 24, 29, 36, 41, 52, 63, 70]
PATCHES = [(8, 8, 8), (8, 8, 12)]
OVERLAPS = [0.0, 0.25, 0.5, 0.75]


def _tiles_for(Y, X, py, px):
    """from one chunk to beyond the plane"""
    fy, fx = -(-Y // py) * py, -(-X // px) * px
    return [(py, px), (2 * py, px), (py, 3 * px), (3 * py, 2 * px), (fy, fx), (fy + 5 * py, fx + 2 * px)]


def _check_tiles(shape, patch, overlap, tile):
    Z, Y, X = shape
    pz, py, px = patch
    ts = inf.tile_schedule(shape, patch, overlap, tile)
    pos = inf.all_positions(shape, patch, overlap)
    plane = sorted({(y, x) for _, y, x in pos})
    nz = len({z for z, _, _ in pos})
    cover = np.zeros((Y, X), np.int32)
    run = 0
    for t in ts:
        y0, y1, x0, x1 = t["own"]
        cover[y0:y1, x0:x1] += 1
        assert y0 % py == 0 and x0 % px == 0 and (y1 % py == 0 or y1 == Y) and (x1 % px == 0 or x1 == X)      # chunk-aligned
        assert y1 - y0 <= tile[0] and x1 - x0 <= tile[1] and y1 > y0 and x1 > x0
        want = [(y, x) for y, x in plane if y < y1 and y + py > y0 and x < x1 and x + px > x0]                # meets the owned box
        assert [(y, x) for y in t["ys"] for x in t["xs"]] == want
        assert t["box"] == (min(y for y, _ in want), max(y for y, _ in want) + py,
                            min(x for _, x in want), max(x for _, x in want) + px)                            # the hull
        assert t["box"][0] <= y0 and t["box"][1] >= y1 and t["box"][2] <= x0 and t["box"][3] >= x1
        run += nz * len(want)
    assert (cover == 1).all()                                                                                  # a partition
    assert ts.positions == len(pos) and ts.positions_run == run and ts.recompute == run / len(pos) >= 1.0
    return ts


@pytest.mark.parametrize("patch", PATCHES)
@pytest.mark.parametrize("overlap", OVERLAPS)
def test_tile_schedule_properties(patch, overlap):
    n = 0
    for i, Y in enumerate(EXTENTS):
        X = EXTENTS[(3 * i + 5) % len(EXTENTS)]
        for tile in _tiles_for(Y, X, patch[1], patch[2]):
            ts = _check_tiles((20, Y, X), patch, overlap, tile)
            n += len(ts)
    # Y == py, and a tile that is one chunk wide next to it
    for X in (12, 30, 70):
        _check_tiles((8, 8, X), patch, overlap, (8, patch[2]))
        _check_tiles((8, 8, X), patch, overlap, (16, 2 * patch[2]))
    assert n > 100


def test_irregular_last_position_widens_a_hull():
    """Y = 36, py = 16, step 8: origins 0, 8, 16, 20; the owned rows [16, 32) meet 8, 16 and the forced 20"""
    ts = inf.tile_schedule((40, 36, 44), (16, 16, 16), 0.5, (16, 16))
    by_own = {t["own"]: t for t in ts}
    t = by_own[(16, 32, 16, 32)]
    assert t["ys"] == [8, 16, 20] and t["xs"] == [8, 16, 24, 28] and t["box"] == (8, 36, 8, 44)
    assert by_own[(32, 36, 32, 44)]["ys"] == [20] and by_own[(32, 36, 32, 44)]["xs"] == [24, 28]
    assert len(ts) == 9 and ts.positions == 4 * 4 * 5


@pytest.mark.parametrize("shape,patch,overlap", [((40, 36, 44), (16, 16, 16), 0.5), ((20, 29, 52), (8, 8, 12), 0.25),
                                                  ((17, 8, 41), (8, 8, 8), 0.75)])
def test_a_tile_as_large_as_the_plane_is_the_untiled_schedule(shape, patch, overlap):
    r = inf.StreamingInferer(None, TARGETS, patch, batch_size=3, overlap=overlap, tta="flip")
    whole = r.schedule(shape, cin=2, in_itemsize=2)
    assert whole["tile"] is None and whole["tiles"] == 1 and whole["recompute"] == 1.0
    for tile in [(-(-shape[1] // patch[1]) * patch[1], -(-shape[2] // patch[2]) * patch[2]), (10 * patch[1], 20 * patch[2])]:
        s = inf.StreamingInferer(None, TARGETS, patch, batch_size=3, overlap=overlap, tta="flip", tile=tile).schedule(shape, 2, 2)
        assert s["tiles"] == 1 and s["recompute"] == 1.0 and s["tile"] == tile
        t = s["tile_list"][0]
        assert t["own"] == t["box"] == (0, shape[1], 0, shape[2])
        assert s["steps"] == whole["steps"] and s["positions"] == whole["positions"]
        for k in ("batch", "ring", "max_finalize_rows", "accumulator_bytes", "input_bytes", "staging_bytes", "patch_bytes",
                  "device_bytes"):
            assert s[k] == whole[k], k


def _pred(p, patch):
    """a small integer function of the position and the voxel"""
    z, y, x = p
    lz, ly, lx = np.meshgrid(*[np.arange(n) for n in patch], indexing="ij")
    return (((z + 2 * y + 3 * x) + lz * 5 + ly * 3 + lx) % 7 - 3).astype(np.float32)


@pytest.mark.parametrize("shape,patch,overlap,tile", [((20, 36, 41), (8, 8, 8), 0.5, (8, 16)), ((17, 29, 52), (8, 8, 12), 0.25, (16, 12)),
                                                      ((24, 18, 23), (8, 8, 8), 0.75, (8, 8)), ((9, 8, 70), (8, 8, 12), 0.0, (8, 24))])
def test_tiled_accumulation_equals_the_whole_volume(shape, patch, overlap, tile):
    Z, Y, X = shape
    rng = np.random.default_rng(5)
    w = (rng.integers(1, 9, size=patch) / 8).astype(np.float32)                  # dyadic: every sum is exact
    r0 = inf.StreamingInferer(None, TARGETS, patch, batch_size=3, overlap=overlap)
    r = inf.StreamingInferer(None, TARGETS, patch, batch_size=3, overlap=overlap, tile=tile)
    s_ref, c_ref = np.zeros(shape, np.float32), np.zeros(shape, np.float32)
    for st in r0.schedule(shape)["steps"]:
        for chunk, valid in st["batches"]:
            for z, y, x in chunk[:valid]:
                s_ref[z:z + patch[0], y:y + patch[1], x:x + patch[2]] += w * _pred((z, y, x), patch)
                c_ref[z:z + patch[0], y:y + patch[1], x:x + patch[2]] += w
    sched = r.schedule(shape)
    s_out, c_out = np.full(shape, np.nan, np.float32), np.full(shape, np.nan, np.float32)
    ran = 0
    for t in sched["tile_list"]:
        by0, by1, bx0, bx1 = t["box"]
        ts = r.tile_stream_schedule(t, Z, sched["batch"])
        s, c = np.zeros((Z, by1 - by0, bx1 - bx0), np.float32), np.zeros((Z, by1 - by0, bx1 - bx0), np.float32)
        for st in ts["steps"]:
            for chunk, valid in st["batches"]:
                assert len(chunk) == sched["batch"]
                for z, y, x in chunk[:valid]:                                      # box-local origins, inside the box
                    assert 0 <= y <= by1 - by0 - patch[1] and 0 <= x <= bx1 - bx0 - patch[2]
                    s[z:z + patch[0], y:y + patch[1], x:x + patch[2]] += w * _pred((z, y + by0, x + bx0), patch)
                    c[z:z + patch[0], y:y + patch[1], x:x + patch[2]] += w
                    ran += 1
        y0, y1, x0, x1 = t["own"]
        assert np.isnan(s_out[:, y0:y1, x0:x1]).all()
        s_out[:, y0:y1, x0:x1] = s[:, y0 - by0:y1 - by0, x0 - bx0:x1 - bx0]
        c_out[:, y0:y1, x0:x1] = c[:, y0 - by0:y1 - by0, x0 - bx0:x1 - bx0]
    assert np.array_equal(s_out, s_ref) and np.array_equal(c_out, c_ref)
    assert ran == sched["positions_run"] and sched["recompute"] == ran / len(sched["positions"])


def test_tiled_byte_counts_are_the_maximum_over_the_tiles():
    """the fixed cases of the device test: with 16^3 patches at overlap 0.5 and tile (16, 16), the forced last x origin 28 of
    X = 44 makes one hull 28 x 36 voxels; on the regular grid of 68 x 84 the largest hull is 32 x 32, and no larger plane adds to it"""
    r = inf.StreamingInferer(None, TARGETS, (16, 16, 16), batch_size=2, overlap=0.5, tile=(16, 16))
    per_voxel_row = 16 * (4 * 5 + 1) + 16 * (4 + 1 * 5 + 3 * 6)      # accumulators + input ring, staging of 16 finalize rows
    a, b, c = (r.schedule(s) for s in ((40, 36, 44), (40, 68, 84), (40, 132, 260)))
    assert a["device_bytes"] == 28 * 36 * per_voxel_row + a["patch_bytes"]
    assert b["device_bytes"] == 32 * 32 * per_voxel_row + b["patch_bytes"] == c["device_bytes"]
    assert a["tiles"] == 9 and b["tiles"] == 30
    whole = inf.StreamingInferer(None, TARGETS, (16, 16, 16), batch_size=2, overlap=0.5).schedule((40, 68, 84))
    assert whole["device_bytes"] == 68 * 84 * per_voxel_row + whole["patch_bytes"]


def test_auto_tile_three_outcomes():
    shape, patch, ov, bs = (40, 68, 84), (16, 16, 16), 0.5, 2
    args = dict(cin=1, in_itemsize=1, acc_channels=4, out_bytes_per_voxel=27)
    plan = 12345
    whole = inf.stream_schedule(shape, patch, ov, bs, 1, 1, 4, 27)["device_bytes"] + plan

    def need(t):
        return inf.tiled_bytes(shape, patch, ov, bs, t, **args)["device_bytes"] + plan

    assert inf.choose_tile(shape, patch, ov, bs, whole, plan, **args) is None                       # fits untiled
    for budget in (whole - 1, need((32, 96)), need((32, 96)) - 1, need((16, 96))):                  # full width, the largest ty
        t = inf.choose_tile(shape, patch, ov, bs, budget, lambda b: plan, **args)
        assert t[1] == 96 and t[0] % 16 == 0 and 16 <= t[0] < 80 and need(t) <= budget
        assert all(need((ty, 96)) > budget for ty in range(t[0] + 16, 81, 16))
    assert inf.choose_tile(shape, patch, ov, bs, need((16, 96)), plan, **args) == (16, 96)
    assert need((80, 96)) == whole and inf.choose_tile(shape, patch, ov, bs, whole - 1, plan, **args)[0] >= 32
    budget = need((16, 96)) - 1                                                                      # not even ty = py at full width
    t = inf.choose_tile(shape, patch, ov, bs, budget, plan, **args)
    assert t[0] == 16 and t[1] < 96 and t[1] % 16 == 0 and need(t) <= budget
    assert all(need((16, tx)) > budget for tx in range(t[1] + 16, 97, 16))
    assert inf.choose_tile(shape, patch, ov, bs, need((16, 16)), plan, **args) == (16, 16)
    with pytest.raises(MemoryError, match=str(need((16, 16)))):                                      # below one chunk
        inf.choose_tile(shape, patch, ov, bs, need((16, 16)) - 1, plan, **args)
    # the inferer: "auto" needs the budget, and its schedule carries the chosen tile
    with pytest.raises(ValueError, match="tile"):
        inf.StreamingInferer(None, TARGETS, patch, tile="auto")
    r = inf.StreamingInferer(None, TARGETS, patch, batch_size=bs, overlap=ov, tile="auto", max_device_bytes=whole - 1)
    s = r.schedule(shape, plan_bytes=plan)
    assert s["tile"] == inf.choose_tile(shape, patch, ov, bs, whole - 1, plan, **args) and s["tiles"] == -(-68 // s["tile"][0]) > 1
    assert s["device_bytes"] + plan <= whole - 1
    r = inf.StreamingInferer(None, TARGETS, patch, batch_size=bs, overlap=ov, tile="auto", max_device_bytes=whole)
    assert r.schedule(shape, plan_bytes=plan)["tile"] is None


def _files(path):
    out = {}
    for d, _, names in os.walk(path):
        for n in names:
            with open(os.path.join(d, n), "rb") as f:
                out[os.path.relpath(os.path.join(d, n), path)] = f.read()
    return out


@pytest.mark.parametrize("comp", [None, "zlib"])
def test_write_block_in_shuffled_tile_order_equals_write_array(tmp_path, comp):
    rng = np.random.default_rng(9)
    Z, Y, X = 21, 29, 30
    vol3 = rng.integers(1, 255, size=(Z, Y, X), dtype=np.uint8)
    vol3[8:16, 8:16, 12:24] = 0                                  # an all-zero chunk: no file
    vol4 = rng.normal(size=(3, Z, Y, X)).astype(np.float32)
    vol4[:, 0:8, 24:29, 24:30] = 0                               # ... and an all-zero partial edge chunk
    ch = (8, 8, 12)
    zarr_lite.write_array(str(tmp_path / "ref3"), vol3, ch, compressor=comp)
    zarr_lite.write_array(str(tmp_path / "ref4"), vol4, (3,) + ch, compressor=comp)
    w3 = zarr_lite.ChunkedWriter(tmp_path / "a3", (Z, Y, X), ch, np.uint8, comp)
    w4 = zarr_lite.ChunkedWriter(tmp_path / "a4", (3, Z, Y, X), (3,) + ch, np.float32, comp)
    blocks = [(z0, y0, x0) for y0 in range(0, Y, 16) for x0 in range(0, X, 12) for z0 in range(0, Z, 8)]
    order = rng.permutation(len(blocks))
    for i in order:
        z0, y0, x0 = blocks[i]
        sl = np.s_[z0:min(z0 + 8, Z), y0:min(y0 + 16, Y), x0:min(x0 + 12, X)]
        assert w3.write_block(z0, y0, x0, vol3[sl]) == []
        w4.write_block(z0, y0, x0, vol4[(slice(None),) + sl])
    f3, f4 = _files(str(tmp_path / "a3")), _files(str(tmp_path / "a4"))
    assert f3 == _files(str(tmp_path / "ref3")) and f4 == _files(str(tmp_path / "ref4"))
    assert "1.1.1" not in f3 and "0.0.3.2" not in f4 and "2.3.2" in f3 and "0.2.3.2" in f4
    assert np.array_equal(zarr_lite.open(str(tmp_path / "a3"))[...], vol3)
    # on a pool, and the refusals
    from concurrent.futures import ThreadPoolExecutor
    w5 = zarr_lite.ChunkedWriter(tmp_path / "a5", (Z, Y, X), ch, np.uint8, comp)
    with ThreadPoolExecutor(4) as pool:
        for f in [f for z0, y0, x0 in blocks for f in w5.write_block(z0, y0, x0, vol3[z0:z0 + 8, y0:y0 + 16, x0:x0 + 12], pool)]:
            f.result()
    assert _files(str(tmp_path / "a5")) == f3
    for bad in [(0, 4, 0, vol3[0:8, 4:12, 0:12]), (0, 0, 0, vol3[0:8, 0:10, 0:12]), (0, 0, 6, vol3[0:8, 0:8, 6:18]),
                (16, 24, 24, vol3[16:20, 24:29, 24:30]), (0, 0, 0, vol3[0:8, 0:8, 0:12].astype(np.uint16)), (0, 0, 0, vol4[:2, 0:8, 0:8, 0:12])]:
        with pytest.raises(zarr_lite.ZarrLiteError):
            (w4 if bad[3].ndim == 4 else w5).write_block(*bad)


def test_occupancy_numpy_hand_built():
    vol = np.zeros((2, 6, 6, 8), np.uint8)
    vol[0, 1, 1, 1] = 1
    vol[1, 2, 3, 4] = 200
    vol[1, 5, 5, 7] = 255
    pos = [(0, 0, 0), (2, 2, 4), (0, 2, 0), (2, 0, 0)]
    assert inf.occupancy_numpy(vol, pos, (4, 4, 4), 0).tolist() == [1, 2, 0, 0]
    assert inf.occupancy_numpy(vol, pos, (4, 4, 4), 1).tolist() == [0, 2, 0, 0]
    assert inf.occupancy_numpy(vol, pos, (4, 4, 4), 200).tolist() == [0, 1, 0, 0]
    assert inf.occupancy_numpy(vol, pos, (4, 4, 4), 255).tolist() == [0, 0, 0, 0]
    assert inf.occupancy_numpy(vol[0], [(0, 0, 0)], (6, 6, 8), 0).dtype == np.uint64
    f = np.zeros((4, 4, 4), np.float32)
    f[0, 0, :4] = [np.nan, -0.0, -3.0, 1e-30]
    assert inf.occupancy_numpy(f, [(0, 0, 0)], (4, 4, 4), 0).tolist() == [1]                       # NaN, -0.0, negatives never count
    assert inf.occupancy_numpy(f, [(0, 0, 0)], (4, 4, 4), -1).tolist() == [62]
    # run iff count > min_fraction * n
    assert inf.keep_mask(np.array([0, 1, 16, 17], np.uint64), 64, 0.0).tolist() == [False, True, True, True]
    assert inf.keep_mask(np.array([0, 1, 16, 17], np.uint64), 64, 0.25).tolist() == [False, False, False, True]


def test_batches_are_cut_again_from_the_kept_slots():
    row = [(8, 0, 0), (8, 0, 4), (8, 4, 0), (8, 4, 4), (8, 8, 0)]
    s = inf.stream_schedule((16, 16, 8), (8, 8, 4), 0.5, 2, n_views=1)
    assert inf.row_positions(s["steps"][2]) == [(8, y, x) for y in (0, 4, 8) for x in (0, 2, 4)]
    assert inf.cut_batches(inf.row_positions(s["steps"][2]), 2, 1) == (s["steps"][2]["batches"], s["steps"][2]["views"])   # the schedule's own rule
    kept = [row[0], row[3], row[4]]
    b, v = inf.cut_batches(kept, 2, 1)
    assert b == [((row[0], row[3]), 2), ((row[4], row[4]), 1)] and v == [(0, 0), (0, 0)]
    b, v = inf.cut_batches(kept[:2], 4, 3)                     # views stay with their position; the last batch repeats its last slot
    assert b == [((row[0],) * 3 + (row[3],), 4), ((row[3],) * 4, 2)] and v == [(0, 1, 2, 0), (1, 2, 2, 2)]
    assert inf.cut_batches([], 2, 3) == ([], [])              # nothing kept: no forward
    s3 = inf.stream_schedule((16, 16, 8), (8, 8, 4), 0.5, 4, n_views=3)
    for st in s3["steps"]:
        assert inf.cut_batches(inf.row_positions(st), s3["batch"], 3) == (st["batches"], st["views"])


def test_argument_refusals_name_the_key():
    mk = lambda **k: inf.StreamingInferer(None, TARGETS, (16, 16, 12), **k)      # noqa: E731
    for bad in [(16, 16), (8, 12), (0, 12), (16, -12), (16,), (16, 12, 12), "full", 16, (16.0, 12), (True, 12)]:
        with pytest.raises(ValueError, match="tile"):
            mk(tile=bad)
    assert mk(tile=(32, 12)).tile == (32, 12) and mk(tile=[16, 36]).tile == (16, 36) and mk().tile is None
    assert mk(tile="AUTO", max_device_bytes=1).tile == "auto"
    assert mk().skip_empty is None and mk(skip_empty=False).skip_empty is None
    assert mk(skip_empty=True).skip_empty == {"value": 0.0, "min_fraction": 0.0}
    assert mk(skip_empty={"value": 3, "min_fraction": 0.5}).skip_empty == {"value": 3.0, "min_fraction": 0.5}
    assert mk(skip_empty={"min_fraction": 0.125}).skip_empty == {"value": 0.0, "min_fraction": 0.125}
    with pytest.raises(ValueError, match="threshold"):
        mk(skip_empty={"threshold": 1})
    for f in (1.0, -0.1, 2, float("nan")):
        with pytest.raises(ValueError, match="min_fraction"):
            mk(skip_empty={"min_fraction": f})
    with pytest.raises(ValueError, match="skip_empty"):
        mk(skip_empty="yes")
    with pytest.raises(ValueError, match="tile"):
        inf.tile_schedule((16, 16, 16), (8, 8, 8), 0.5, (8, 12))


def _cfg(tmp_path, ic):
    import yaml
    cfg = {"tr_setup": {}, "tr_config": {"patch_size": [16, 16, 16]}, "model_config": {},
           "dataset_config": {"targets": {"sheet": {"channels": 1, "activation": "sigmoid"}}}, "inference_config": ic}
    p = tmp_path / "cfg.yaml"
    p.write_text(yaml.safe_dump(cfg))
    return str(p)


def test_config_keys(tmp_path):
    from mt3d_amd.configuration.config_manager import ConfigManager
    m = ConfigManager(_cfg(tmp_path, {}), verbose=False)
    assert m.infer_tile is None and m.infer_skip_empty is None
    m = ConfigManager(_cfg(tmp_path, {"tile": [32, 16], "skip_empty": True}), verbose=False)
    assert m.infer_tile == (32, 16) and m.infer_skip_empty == {"value": 0.0, "min_fraction": 0.0}
    m = ConfigManager(_cfg(tmp_path, {"tile": "auto", "max_device_gb": 2, "skip_empty": {"value": 10, "min_fraction": 0.01}}), verbose=False)
    assert m.infer_tile == "auto" and m.infer_skip_empty == {"value": 10.0, "min_fraction": 0.01}
    for ic, key in [({"tile": [24, 16]}, r"inference_config\.tile"), ({"tile": "auto"}, r"inference_config\.tile"),
                    ({"tile": "wide"}, r"inference_config\.tile"), ({"skip_empty": {"fraction": 0.5}}, r"inference_config\.skip_empty.*fraction"),
                    ({"skip_empty": {"min_fraction": 1.5}}, r"inference_config\.skip_empty\.min_fraction")]:
        with pytest.raises(ValueError, match=key):
            ConfigManager(_cfg(tmp_path, ic), verbose=False)


def test_occupancy_entry_point_is_declared_bound_and_exported():
    from mt3d_amd.engine import lib
    with open(os.path.join(ROOT, "include", "rxunet.h")) as f:
        hdr = f.read()
    so = ctypes.CDLL(lib.LIB_PATH)
    assert re.search(r"\brx_sw_occupancy\s*\(", hdr) and hasattr(so, "rx_sw_occupancy") and "rx_sw_occupancy" in lib.exported_symbols()
    fn = lib.load().rx_sw_occupancy
    fake = ctypes.c_void_p(0x10000)
    org = (ctypes.c_int32 * 6)(0, 0, 0, 0, 9, 0)
    # refused on the host, before any device call: an origin that leaves the slab, rows that do not fit the ring, bad pointers
    assert fn(0, fake, 1, 8, 16, 16, 2, org, 8, 8, 8, 0.0, fake, None) != 0
    assert b"leaves the slab" in lib.load().rx_last_error()
    assert fn(0, fake, 1, 8, 16, 16, 2, (ctypes.c_int32 * 6)(0, 0, 0, 1, 0, 0), 8, 8, 8, 0.0, fake, None) != 0
    assert b"ring" in lib.load().rx_last_error()
    assert fn(0, fake, 1, 4, 16, 16, 1, org, 8, 8, 8, 0.0, fake, None) != 0
    assert fn(3, fake, 1, 8, 16, 16, 1, org, 8, 8, 8, 0.0, fake, None) != 0
    assert fn(1, ctypes.c_void_p(0x10001), 1, 8, 16, 16, 1, org, 8, 8, 8, 0.0, fake, None) != 0
    assert fn(0, fake, 1, 8, 16, 16, 1, org, 8, 8, 8, 0.0, ctypes.c_void_p(0x10004), None) != 0
    assert fn(0, fake, 1, 8, 16, 16, 1, None, 8, 8, 8, 0.0, fake, None) != 0
    assert fn(0, fake, 1, 8, 16, 16, 0, None, 8, 8, 8, 0.0, fake, None) == 0          # no positions: nothing to do
