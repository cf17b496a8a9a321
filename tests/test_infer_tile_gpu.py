"""Y/X tiles and empty-patch skipping of streaming inference on the device: `rx_sw_occupancy` against `occupancy_numpy` (exact),
tiled runs against the untiled run (bit for bit at batch 1), `tile="auto"`, device memory against the plane, and skipped runs
against a torch statement of the kept patches."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import resenc_oracle as oracle      # noqa: E402

pytestmark = pytest.mark.gpu

TASKS = {"sheet": {"channels": 1, "activation": "sigmoid"}, "normals": {"channels": 3, "activation": "none"}}
PATCH = (16, 16, 16)
SHAPE = (40, 52, 44)


def _lib():
    import mt3d_amd  # noqa: F401
    from mt3d_amd.engine import lib as L
    L.require_device()
    return L, L.load()


def _org(patches):
    return (ctypes.c_int32 * (3 * len(patches)))(*[v for p in patches for v in p])


def _ring(vol, R):
    """(C, Z, Y, X) volume -> its (C, R, Y, X) ring holding row z at z % R (all rows, last writer wins)"""
    ring = np.zeros((vol.shape[0], R) + vol.shape[2:], vol.dtype)
    for z in range(vol.shape[1]):
        ring[:, z % R] = vol[:, z]
    return ring


# ---- rx_sw_occupancy ----------------------------------------------------------------------------------------------------------
def _occ_volume(dt, shape, rng):
    if dt == np.float32:
        vol = (rng.normal(size=shape) * 2).astype(np.float32)
        vol[rng.random(shape) < 0.3] = 0.0
        vol[rng.random(shape) < 0.05] = np.nan
        vol[rng.random(shape) < 0.05] = -0.0
        vol[0, shape[1] // 2, 0, :3] = [np.inf, np.finfo(np.float32).max, -np.inf]
    else:
        top = np.iinfo(dt).max
        vol = rng.integers(0, top + 1, size=shape).astype(dt)
        vol[rng.random(shape) < 0.4] = 0
        vol[0, shape[1] // 2, 0, :4] = top                                              # the top of the range: never above the type's maximum
    return vol


@pytest.mark.parametrize("dt", [np.uint8, np.uint16, np.float32])
@pytest.mark.parametrize("px", [12, 10])
def test_occupancy_kernel_is_exact(dt, px):
    import mt3d_amd.inference as inf
    L, lib = _lib()
    rng = np.random.default_rng(4)
    cin, Z, Y, X, R, pz, py = 2, 20, 24, 28, 12, 8, 8
    vol = _occ_volume(dt, (cin, Z, Y, X), rng)
    vol[:, :, 16:24, X - px:] = 0                                           # an empty patch among them (-0.0 / NaN would do too)
    ring = _ring(vol[:, :7 + R], R)                                         # rows [7, 19) wrap around R = 12
    code = {np.uint8: L.RX_SW_U8, np.uint16: L.RX_SW_U16, np.float32: L.RX_SW_F32}[dt]
    dev = torch.from_numpy(ring.view(np.int16) if dt == np.uint16 else ring).cuda()
    patches = [(7, 0, 0), (9, 16, X - px), (11, 5, 3), (10, Y - py, 0), (7, 3, X - px - 1)]   # both slab edges, interior, odd x
    n = len(patches)
    mid, top = (1.0, float(np.finfo(np.float32).max)) if dt == np.float32 else (float(np.iinfo(dt).max // 2), float(np.iinfo(dt).max))
    counts = torch.full((n + 1,), -7, dtype=torch.int64, device="cuda")
    for value in (0.0, mid, top, -1.0):
        L.check(lib.rx_sw_occupancy(code, dev.data_ptr(), cin, R, Y, X, n, _org(patches), pz, py, px, value, counts.data_ptr(),
                                    L.stream_ptr()), "occupancy")
        got = counts.cpu().numpy()
        want = inf.occupancy_numpy(vol, patches, (pz, py, px), value)
        assert np.array_equal(got[:n].view(np.uint64), want), (dt, px, value)
        assert got[n] == -7                                                 # nothing past n_pos is written
    assert inf.occupancy_numpy(vol, patches, (pz, py, px), 0.0)[1] == 0 and inf.occupancy_numpy(vol, patches, (pz, py, px), top).max() == \
        (1 if dt == np.float32 else 0)
    # a position that leaves the slab, or rows that do not fit the ring: refused, nothing launched (the counts are not even zeroed)
    counts.fill_(-7)
    for bad in ([(7, 0, 0), (7, Y - py + 1, 0)], [(7, 0, X - px + 1)], [(7, 0, 0), (12, 0, 0)], [(-1, 0, 0)]):
        assert lib.rx_sw_occupancy(code, dev.data_ptr(), cin, R, Y, X, len(bad), _org(bad), pz, py, px, 0.0, counts.data_ptr(),
                                   L.stream_ptr()) != 0
    assert lib.rx_sw_occupancy(code, dev.data_ptr(), cin, R, Y, X, 1, _org([(7, 0, 0)]), R + 1, py, px, 0.0, counts.data_ptr(),
                               L.stream_ptr()) != 0
    torch.cuda.synchronize()
    assert (counts.cpu().numpy() == -7).all()


def test_occupancy_of_more_positions_than_one_launch_holds():
    """323 positions: two launches behind one call (the origins travel by value, 256 per launch), patches of one chunk each"""
    import mt3d_amd.inference as inf
    L, lib = _lib()
    rng = np.random.default_rng(6)
    Y, X, R, patch = 24, 28, 8, (8, 8, 10)
    vol = _occ_volume(np.uint8, (1, 8, Y, X), rng)
    vol[:, :, :12, :14] = 0
    patches = [(0, y, x) for y in range(Y - 8 + 1) for x in range(X - 10 + 1)]
    assert len(patches) == 323
    dev = torch.from_numpy(vol).cuda()
    counts = torch.empty((len(patches),), dtype=torch.int64, device="cuda")
    L.check(lib.rx_sw_occupancy(L.RX_SW_U8, dev.data_ptr(), 1, R, Y, X, len(patches), _org(patches), *patch, 0.0, counts.data_ptr(),
                                L.stream_ptr()), "occupancy")
    want = inf.occupancy_numpy(vol, patches, patch, 0)
    assert np.array_equal(counts.cpu().numpy().view(np.uint64), want) and want.min() == 0 and want.max() > 300


# ---- end to end ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _net():
    import mt3d_amd  # noqa: F401
    from mt3d_amd.builders.build_network_from_config import NetworkFromConfig
    mgr = oracle.make_mgr(PATCH, TASKS, 1, 2, True, {})
    torch.manual_seed(3)
    return NetworkFromConfig(mgr).cuda()


@functools.lru_cache(maxsize=None)
def _volume(kind="full", shape=SHAPE):
    vol = np.random.default_rng(11).integers(0, 256, size=shape).astype(np.uint8)
    if kind == "holes":                       # whole z-rows of patches and whole columns drop out
        vol[:, :, 24:] = 0
        vol[16:40] = 0
    vol.setflags(write=False)
    return vol


def _read(path):
    from mt3d_amd.dataloading import zarr_lite
    return {n + suf: zarr_lite.open(os.path.join(path, n + suf))[...] for n in TASKS for suf in ("_sum", "_count", "_final")}


_RUNS = {}


def _run(tmp_path_factory, kind="full", shape=SHAPE, **k):
    """one streaming run per distinct argument set, shared by the tests: (arrays, last_timing, last_schedule, store path)"""
    import mt3d_amd.inference as inf
    key = (kind, shape, tuple(sorted((a, repr(b)) for a, b in k.items())))
    if key not in _RUNS:
        k.setdefault("batch_size", 1)
        r = inf.StreamingInferer(_net(), TASKS, PATCH, overlap=0.5, compute_dtype=torch.float32, **k)
        store = r.run(_volume(kind, shape), str(tmp_path_factory.mktemp("run")), compressor=None)
        _RUNS[key] = (_read(store), r.last_timing, r.last_schedule, store)
    return _RUNS[key]


def _same(a, b):
    for k in a:
        assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), k


@pytest.mark.parametrize("mode", ["uniform", "gaussian", "tta"])
def test_tiled_equals_untiled_at_batch_one(tmp_path_factory, mode):
    import mt3d_amd.inference as inf
    L, _ = _lib()
    k = {"uniform": {}, "gaussian": {"blend": "gaussian"}, "tta": {"tta": {"flip": ["x"]}}}[mode]
    whole, t0, s0, _ = _run(tmp_path_factory, **k)
    views = 2 if mode == "tta" else 1
    assert t0["tiles"] == 1 and s0["tile"] is None and t0["forwards"] == views * len(s0["positions"]) and t0["skipped"] == 0
    for tile in ((16, 16), (32, 16)):
        got, t, s, _ = _run(tmp_path_factory, tile=tile, **k)
        _same(whole, got)
        ts = inf.tile_schedule(SHAPE, PATCH, 0.5, tile)
        assert t["tiles"] == len(ts) == s["tiles"] > 1 and s["recompute"] == ts.recompute > 1.0
        assert t["forwards"] == views * ts.positions_run == views * t["positions_run"] and t["patches"] == len(s0["positions"])
        assert s["device_bytes"] < s0["device_bytes"]


def test_tiled_at_batch_two_within_the_bounds_of_the_streaming_test(tmp_path_factory):
    """batches are composed differently per tile, so a logit may differ in its last bit (tests/test_infer_stream_gpu.py (a)): the
    averages agree to 1e-6, the unit normals s / |s| to 1e-6 + 2e-6 / |s|, the casts to +-1; the counts are exact"""
    import mt3d_amd.inference as inf
    L, _ = _lib()
    whole = _run(tmp_path_factory, batch_size=2)[0]
    got, t, s, _ = _run(tmp_path_factory, batch_size=2, tile=(16, 16))
    assert s["batch"] == 2 and t["forwards"] < t["positions_run"]
    swi = inf.SlidingWindowInferer(_net(), TASKS, PATCH, batch_size=2, overlap=0.5, compute_dtype=torch.float32)
    sums, _ = swi.accumulate(_volume().astype(np.float32) / np.float32(255.0))
    mag = torch.sqrt((sums["normals"] ** 2).sum(0)).cpu().numpy()
    for n in TASKS:
        bound = 1e-6 if n != "normals" else 1e-6 + 2e-6 / np.maximum(mag, 1e-30)
        d = np.abs(got[n + "_sum"] - whole[n + "_sum"])
        print(n, "max |tiled - untiled|", d.max(), "final", np.abs(got[n + "_final"].astype(np.int64) - whole[n + "_final"].astype(np.int64)).max())
        assert (d <= bound).all(), (n, d.max())
        assert np.abs(got[n + "_final"].astype(np.int64) - whole[n + "_final"].astype(np.int64)).max() <= 1, n
        assert np.array_equal(got[n + "_count"], whole[n + "_count"])


def test_auto_tile(tmp_path_factory, tmp_path):
    import mt3d_amd.inference as inf
    L, _ = _lib()
    whole, _, s0, _ = _run(tmp_path_factory)
    need = s0["device_bytes"] + _net().plan_for(torch.Size((1, 1) + PATCH), torch.float32, torch.device("cuda"), False).bytes_alloc
    got, t, s, _ = _run(tmp_path_factory, tile="auto", max_device_bytes=need - 1)
    assert t["tiles"] > 1 and s["tile"] is not None and s["tile"][1] == 48 and s["device_bytes"] < s0["device_bytes"]
    _same(whole, got)
    fits, t1, s1, _ = _run(tmp_path_factory, tile="auto", max_device_bytes=need)      # fits: the untiled path
    assert t1["tiles"] == 1 and s1["tile"] is None
    _same(whole, fits)
    r = inf.StreamingInferer(_net(), TASKS, PATCH, batch_size=1, overlap=0.5, compute_dtype=torch.float32, max_device_bytes=need - 1)
    with pytest.raises(MemoryError, match="tile"):
        r.run(_volume(), str(tmp_path / "refused"))
    assert not os.path.exists(tmp_path / "refused" / "predictions.zarr")


def test_device_memory_does_not_grow_with_the_plane(tmp_path):
    """Measured as test_device_memory_does_not_grow_with_z measures it.  The peak may grow by no more than one tile's input ring
    and staging.  `device_bytes` is the maximum over the tiles' hulls: on the regular grid of (40, 68, 84) the largest hull is
    32 x 32 and no larger plane adds to it (checked against a plane four times as large); on (40, 36, 44) the forced last x origin
    28 stretches one hull to 28 x 36 = 1008 voxels per row, 16 fewer, so the two are not equal and the small plane needs no more."""
    import mt3d_amd.inference as inf
    L, _ = _lib()
    net = _net()

    def peak(shape, name):
        r = inf.StreamingInferer(net, TASKS, PATCH, batch_size=2, overlap=0.5, compute_dtype=torch.float32, tile=(16, 16))
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        r.run(_volume("full", shape), str(tmp_path / name), compressor=None)
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - base, r.last_schedule

    peak((40, 36, 44), "warm")              # builds the plan and its lazy buffers
    p1, s1 = peak((40, 36, 44), "small")
    p2, s2 = peak((40, 68, 84), "wide")
    print("peaks", p1, p2, "device_bytes", s1["device_bytes"], s2["device_bytes"])
    assert p2 - p1 <= s1["input_bytes"] + s1["staging_bytes"], (p1, p2)
    r = inf.StreamingInferer(None, TASKS, PATCH, batch_size=2, overlap=0.5, tile=(16, 16))
    assert s2["device_bytes"] == r.schedule((40, 132, 164))["device_bytes"] == r.schedule((40, 132, 324))["device_bytes"]
    assert s1["device_bytes"] <= s2["device_bytes"] and s2["device_bytes"] - s1["device_bytes"] == 16 * 16 * (4 * 5 + 1 + 27)
    untiled = inf.StreamingInferer(None, TASKS, PATCH, batch_size=2, overlap=0.5).schedule((40, 68, 84))
    assert s2["device_bytes"] * 5 < untiled["device_bytes"]


def _skip_statement(vol):
    """forward_logits per kept position, activation, sum += w * p in position order, then blend and cast_final; voxels that no kept
    patch covers hold 0 in every array (the fill value of the store), `_final` included"""
    import mt3d_amd.inference as inf
    net = _net()
    pos = inf.all_positions(vol.shape, PATCH, 0.5)
    occ = inf.occupancy_numpy(vol, pos, PATCH, 0)
    kept = [p for p, c in zip(pos, occ) if c > 0]
    v = torch.from_numpy(vol.astype(np.float32) / np.float32(255.0)).cuda()[None]
    sums = {n: torch.zeros((t["channels"],) + vol.shape, dtype=torch.float32, device="cuda") for n, t in TASKS.items()}
    count = torch.zeros(vol.shape, dtype=torch.float32, device="cuda")
    was, prev = net.training, getattr(net, "compute_dtype", None)
    net.eval()
    net.compute_dtype = torch.float32
    try:
        with torch.no_grad():
            for z, y, x in kept:
                raw = net.forward_logits(v[:, z:z + 16, y:y + 16, x:x + 16][None].contiguous())
                for n, t in TASKS.items():
                    p = inf.SlidingWindowInferer._activate(raw[n].float(), t["activation"])
                    sums[n][:, z:z + 16, y:y + 16, x:x + 16] += p[0]
                count[z:z + 16, y:y + 16, x:x + 16] += 1.0
    finally:
        net.compute_dtype = prev
        net.train(was)
    out = {"count": count.cpu().numpy(), "mag": torch.sqrt((sums["normals"] ** 2).sum(0)).cpu().numpy()}
    for n in TASKS:
        b = inf.SlidingWindowInferer.blend(n, sums[n], count)
        f = inf.SlidingWindowInferer.cast_final(n, b).cpu().numpy().astype(np.uint16 if n == "normals" else np.uint8)
        f[:, out["count"] == 0] = 0
        out[n] = b.cpu().numpy()
        out[n + "_final"] = f
    return out, len(pos) - len(kept)


def test_skip_empty_against_the_torch_statement(tmp_path_factory):
    L, _ = _lib()
    vol = _volume("holes")
    want, n_skipped = _skip_statement(vol)
    got, t, s, store = _run(tmp_path_factory, "holes", skip_empty=True)
    assert n_skipped == 120 - 36 and t["skipped"] == n_skipped and t["forwards"] == 36 and t["patches"] == 120
    for n in TASKS:
        one = TASKS[n]["channels"] == 1
        wb, wf = (want[n][0], want[n + "_final"][0]) if one else (want[n], want[n + "_final"])
        bound = 1e-6 if n != "normals" else 1e-6 + 2e-6 / np.maximum(want["mag"], 1e-30)
        d = np.abs(got[n + "_sum"] - wb)
        print(n, "max |stream - statement|", d.max())
        assert (d <= bound).all(), (n, d.max())
        assert np.abs(got[n + "_final"].astype(np.int64) - wf.astype(np.int64)).max() <= 1, n
        assert np.array_equal(got[n + "_count"], want["count"])
        assert not got[n + "_final"][..., want["count"] == 0].any() and not got[n + "_sum"][..., want["count"] == 0].any()
    # a fully empty chunk leaves no file under any array; every other chunk of the count arrays is there
    empty = 0
    for cz in range(3):
        for cy in range(4):
            for cx in range(3):
                covered = want["count"][cz * 16:cz * 16 + 16, cy * 16:cy * 16 + 16, cx * 16:cx * 16 + 16].any()
                empty += not covered
                for n in TASKS:
                    lead = "" if TASKS[n]["channels"] == 1 else "0."
                    for suf in ("_sum", "_final"):
                        assert os.path.exists(os.path.join(store, n + suf, f"{lead}{cz}.{cy}.{cx}")) == bool(covered), (n, suf, cz, cy, cx)
                    assert os.path.exists(os.path.join(store, n + "_count", f"{cz}.{cy}.{cx}")) == bool(covered)
    assert empty == 36 - 2 * 4 * 2
    # with tiles the decision is the same, position by position, and so is the store
    tiled, tt, _, _ = _run(tmp_path_factory, "holes", skip_empty=True, tile=(16, 16))
    _same(got, tiled)
    assert tt["tiles"] == 12 and tt["forwards"] == tt["positions_run"] - tt["skipped"] > 36 and tt["skipped"] > t["skipped"]
    # a threshold of its own: nothing is above 255
    none, tn, _, _ = _run(tmp_path_factory, "holes", skip_empty={"value": 255, "min_fraction": 0.0})
    assert tn["forwards"] == 0 and tn["skipped"] == 120 and not any(a.any() for a in none.values())


def test_skip_empty_changes_nothing_where_no_patch_is_empty(tmp_path_factory):
    L, _ = _lib()
    whole = _run(tmp_path_factory)[0]
    got, t, _, _ = _run(tmp_path_factory, skip_empty=True)
    assert t["skipped"] == 0 and t["forwards"] == 120
    _same(whole, got)
    whole2 = _run(tmp_path_factory, batch_size=2)[0]
    got2, t2, _, _ = _run(tmp_path_factory, batch_size=2, skip_empty={"value": 0, "min_fraction": 0.5})
    assert t2["skipped"] == 0 and t2["forwards"] == 60
    _same(whole2, got2)
