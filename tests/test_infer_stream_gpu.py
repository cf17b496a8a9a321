"""Streaming sliding-window inference on the device: the three HIP kernels of csrc/rx_infer.hip against numpy, and the whole
`StreamingInferer` against `SlidingWindowInferer` (uniform), against a numpy weighted-blend oracle driven by the CPU oracle network
(Gaussian), for determinism and for device memory that does not grow with Z."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import resenc_oracle as oracle      # noqa: E402

import infer_ref as IR              # noqa: E402

pytestmark = pytest.mark.gpu


def _lib():
    import mt3d_amd  # noqa: F401
    from mt3d_amd.engine import lib as L
    L.require_device()
    return L, L.load()


def _org(patches):
    return (ctypes.c_int32 * (3 * len(patches)))(*[v for p in patches for v in p])


def _ring(vol, R):
    """(C, Z, Y, X) volume -> its (C, R, Y, X) ring holding rows [z0, z0 + R) at row % R (all rows, last writer wins)"""
    C, Z, Y, X = vol.shape
    ring = np.zeros((C, R, Y, X), vol.dtype)
    for z in range(Z):
        ring[:, z % R] = vol[:, z]
    return ring


@pytest.mark.parametrize("dt", [np.uint8, np.uint16, np.float32])
@pytest.mark.parametrize("px", [12, 10])
def test_gather_scale_and_zscore(dt, px):
    L, lib = _lib()
    rng = np.random.default_rng(1)
    cin, Z, Y, X, R, pz, py = 2, 20, 24, 28, 12, 8, 8
    if dt == np.float32:
        vol = rng.normal(size=(cin, Z, Y, X)).astype(np.float32) * 3 + 1
    else:
        vol = rng.integers(0, np.iinfo(dt).max + 1, size=(cin, Z, Y, X)).astype(dt)
        vol[0, 9, 0, :4] = np.iinfo(dt).max                                # the top of the range
    slab_z = 7                                                              # rows [7, 19) of the ring wrap around R = 12
    ring = _ring(vol[:, :slab_z + R], R)
    code = {np.uint8: L.RX_SW_U8, np.uint16: L.RX_SW_U16, np.float32: L.RX_SW_F32}[dt]
    dev = torch.from_numpy(ring.view(np.int16) if dt == np.uint16 else ring).cuda()
    patches = [(7, 0, 0), (9, 16, X - px), (11, 5, 3)]                      # slab edges and an interior patch
    B = len(patches)
    out = torch.empty((B, cin, pz, py, px), dtype=torch.float32, device="cuda")
    ws_b = lib.rx_sw_gather_workspace(B, cin, pz, py, px)
    ws = torch.empty((ws_b // 8 + 1,), dtype=torch.float64, device="cuda")
    div = {np.uint8: np.float32(255.0), np.uint16: np.float32(65535.0), np.float32: None}[dt]
    want = []
    for z, y, x in patches:
        p = vol[:, z:z + pz, y:y + py, x:x + px].astype(np.float32)
        want.append(p / div if div is not None else p)
    want = np.stack(want)
    L.check(lib.rx_sw_gather(code, dev.data_ptr(), cin, R, Y, X, B, _org(patches), pz, py, px, L.RX_SW_SCALE, out.data_ptr(),
                             None, 0, L.stream_ptr()), "gather")
    assert np.array_equal(out.cpu().numpy(), want)                          # bit-exact: numpy's float32 division
    L.check(lib.rx_sw_gather(code, dev.data_ptr(), cin, R, Y, X, B, _org(patches), pz, py, px, L.RX_SW_ZSCORE, out.data_ptr(),
                             ws.data_ptr(), ws_b, L.stream_ptr()), "gather zscore")
    IR.check_zscore(out.cpu().numpy(), want, f"zscore {dt.__name__} px {px}")      # per element: 3u |z| + u |mean| / std
    bad = _org([(7, Y - py + 1, 0)])                                        # leaves the slab: refused, nothing launched
    assert lib.rx_sw_gather(code, dev.data_ptr(), cin, R, Y, X, 1, bad, pz, py, px, 0, out.data_ptr(), None, 0, L.stream_ptr()) != 0


def _acc_oracle(sum0, wsum0, logits, patches, valid, w, act, R):
    s, ws = sum0.copy(), wsum0.copy()
    pz, py, px = w.shape
    for b in range(valid):
        z, y, x = patches[b]
        lg = logits[b].astype(np.float32)
        if act == 1:
            p = (np.float32(1) / (np.float32(1) + np.exp(-lg))).astype(np.float32)
        elif act == 2:
            e = np.exp(lg - lg.max(0, keepdims=True))
            p = (e / e.sum(0, keepdims=True)).astype(np.float32)
        else:
            p = lg
        rows = [(z + i) % R for i in range(pz)]
        s[:, rows, y:y + py, x:x + px] += w[None] * p
        ws[rows, y:y + py, x:x + px] += w
    return s, ws


@pytest.mark.parametrize("X", [24, 22])
@pytest.mark.parametrize("act", [0, 1, 2])
@pytest.mark.parametrize("weights", ["uniform", "gauss"])
def test_accumulate_overlapping_patches(X, act, weights):
    L, lib = _lib()
    import mt3d_amd.inference as inf
    rng = np.random.default_rng(2 + act)
    c, R, Y, pz = 3, 16, 20, 8
    patch = (pz, 8, 8)
    patches = [(12, 0, 0), (12, 4, 3), (12, 12, X - 8), (12, 4, 3), (12, 0, 1)]   # overlaps, a repeat, both edges, ring wrap
    B, valid = 5, 4                                                            # the last (a padding repeat) must not count
    logits = rng.integers(-4, 5, size=(B, c, *patch)).astype(np.float32)
    sum0 = rng.integers(-3, 4, size=(c, R, Y, X)).astype(np.float32)
    wsum0 = rng.integers(0, 3, size=(R, Y, X)).astype(np.float32)
    if weights == "uniform":
        w = np.ones(patch, np.float32)
    elif act == 0:
        w = (rng.integers(1, 9, size=patch) / 8).astype(np.float32)            # dyadic: the sums stay exact
    else:
        w = inf.gaussian_importance_map(patch)
    s_d, w_d, l_d, wt_d = (torch.from_numpy(a).cuda() for a in (sum0, wsum0, logits, w))
    L.check(lib.rx_sw_accumulate(l_d.data_ptr(), B, valid, c, *patch, _org(patches), act, wt_d.data_ptr(), s_d.data_ptr(),
                                 w_d.data_ptr(), R, Y, X, L.stream_ptr()), "accumulate")
    s_ref, w_ref = _acc_oracle(sum0, wsum0, logits, patches, valid, w, act, R)
    if act == 0:
        assert np.array_equal(s_d.cpu().numpy(), s_ref) and np.array_equal(w_d.cpu().numpy(), w_ref)
    elif weights == "uniform":
        assert np.array_equal(w_d.cpu().numpy(), w_ref)
    ref = IR.accumulate_ref(sum0, wsum0, logits, patches, valid, w, act, R)                # fp64, per-element bounds
    IR.check_accumulate(s_d.cpu().numpy(), w_d.cpu().numpy(), ref, sum0, wsum0, f"accumulate act {act} {weights}", exact=act == 0)
    # wsum == NULL: the sums only
    s2 = torch.from_numpy(sum0).cuda()
    L.check(lib.rx_sw_accumulate(l_d.data_ptr(), B, valid, c, *patch, _org(patches), act, wt_d.data_ptr(), s2.data_ptr(), None,
                                 R, Y, X, L.stream_ptr()), "accumulate")
    assert np.array_equal(s2.cpu().numpy(), s_d.cpu().numpy())
    # a batch whose rows do not fit the ring is refused
    assert lib.rx_sw_accumulate(l_d.data_ptr(), 2, 2, c, *patch, _org([(0, 0, 0), (9, 0, 0)]), act, wt_d.data_ptr(), s2.data_ptr(),
                                None, R, Y, X, L.stream_ptr()) != 0


@pytest.mark.parametrize("mode", [(0, 0, 1), (1, 1, 3), (2, 1, 2), (0, 0, 2)])
@pytest.mark.parametrize("X", [20, 18])
def test_finalize_and_cast(mode, X):
    L, lib = _lib()
    blend, cast, c = mode
    rng = np.random.default_rng(3)
    R, Y, z0, n = 16, 11, 14, 5                                               # rows 14..18 wrap around the ring; the plane is 220
    assert (Y * X) % 4 == (0 if X == 20 else 2)                               # voxels (whole quads) or 198 (a tail of 2: the scalar form)
    wsum = rng.integers(0, 4, size=(R, Y, X)).astype(np.float32)
    wsum[wsum == 3] = 0.375
    s = (rng.normal(size=(c, R, Y, X)) * 1.5).astype(np.float32) * np.maximum(wsum, 1)
    # values at the clip bounds: exactly 0 and 1 (u8) / -1 and 1 (u16) after blending, and beyond them
    edge = np.array([0.0, 1.0, -1.0, 2.0, -0.5, 1.0 / 255, 254.999 / 255, 255.0 / 255], np.float32)
    s[:, 15, 0, :edge.size] = edge
    wsum[15, 0, :edge.size] = 1.0
    s_d, w_d = torch.from_numpy(s).cuda(), torch.from_numpy(wsum).cuda()
    bl = torch.empty((c, n, Y, X), dtype=torch.float32, device="cuda")
    fi = torch.empty((c, n, Y, X), dtype=torch.uint8 if cast == 0 else torch.int16, device="cuda")
    wo = torch.empty((n, Y, X), dtype=torch.float32, device="cuda")
    L.check(lib.rx_sw_finalize(s_d.data_ptr(), w_d.data_ptr(), c, R, Y, X, z0, n, blend, cast, 2, bl.data_ptr(), fi.data_ptr(),
                               wo.data_ptr(), L.stream_ptr()), "finalize")
    rows = [(z0 + i) % R for i in range(n)]
    b_ref, f_ref = IR.finalize_ref(s, wsum, R, z0, n, blend, cast, 2)[:2]
    assert np.array_equal(bl.cpu().numpy(), b_ref)
    got_f = fi.cpu().numpy().view(np.uint16) if cast == 1 else fi.cpu().numpy()
    assert np.array_equal(got_f, f_ref)
    assert np.array_equal(wo.cpu().numpy(), wsum[rows])
    s_after, w_after = s_d.cpu().numpy(), w_d.cpu().numpy()
    assert not s_after[:, rows].any() and not w_after[rows].any()            # reset for the rows that follow
    other = [r for r in range(R) if r not in rows]
    assert np.array_equal(s_after[:, other], s[:, other]) and np.array_equal(w_after[other], wsum[other])


# ---- end to end ---------------------------------------------------------------------------------------------------------------
TASKS = {"sheet": {"channels": 1, "activation": "sigmoid"}, "normals": {"channels": 3, "activation": "none"}}


def _nets():
    import mt3d_amd  # noqa: F401
    from mt3d_amd.builders.build_network_from_config import NetworkFromConfig
    mgr = oracle.make_mgr((16, 16, 16), TASKS, 1, 2, True, {})
    torch.manual_seed(3)
    ref_net = oracle.NetworkFromConfig(mgr).eval()
    torch.manual_seed(3)
    return NetworkFromConfig(mgr).cuda(), ref_net


def _store(path):
    from mt3d_amd.dataloading import zarr_lite
    out = {}
    for n in TASKS:
        for suf in ("_sum", "_count", "_final"):
            out[n + suf] = zarr_lite.open(os.path.join(path, n + suf))[...]
    return out


def _volume(tmp_path, Z=40):
    from mt3d_amd.dataloading import zarr_lite
    rng = np.random.default_rng(11)
    vol = rng.integers(0, 256, size=(Z, 36, 44)).astype(np.uint8)
    return vol, zarr_lite.write_array(str(tmp_path / f"vol{Z}.zarr"), vol, (16, 16, 16), compressor="zlib")


def test_streaming_end_to_end(tmp_path):
    L, _ = _lib()
    import mt3d_amd.inference as inf
    net, ref_net = _nets()
    vol, arr = _volume(tmp_path)

    def streamer(**k):
        return inf.StreamingInferer(net, TASKS, (16, 16, 16), batch_size=2, overlap=0.5, compute_dtype=torch.float32, **k)

    # (a) uniform + scale == SlidingWindowInferer on the scaled volume.  The two group patches into batches differently (per z-row
    # here), so a logit may differ in its last bit: the averages agree to 1e-6, the unit normals s / |s| to 1e-6 + 2e-6 / |s| --
    # where the summed raw normals nearly cancel, their direction is not determined by fp32 logits.
    s1 = _store(streamer().run(str(arr.path), str(tmp_path / "a")))
    swi = inf.SlidingWindowInferer(net, TASKS, (16, 16, 16), batch_size=2, overlap=0.5, compute_dtype=torch.float32)
    scaled = vol.astype(np.float32) / np.float32(255.0)
    want = swi(scaled)
    sums, _ = swi.accumulate(scaled)
    mag = torch.sqrt((sums["normals"] ** 2).sum(0)).cpu().numpy()
    cnt = np.zeros(vol.shape, np.float32)
    for z, y, x in inf.all_positions(vol.shape, (16, 16, 16), 0.5):
        cnt[z:z + 16, y:y + 16, x:x + 16] += 1
    for n in TASKS:
        one = TASKS[n]["channels"] == 1
        b, wb = s1[n + "_sum"], (want[n][0] if one else want[n])
        assert b.shape == wb.shape, n
        bound = 1e-6 if n != "normals" else 1e-6 + 2e-6 / np.maximum(mag, 1e-30)
        assert (np.abs(b - wb) <= bound).all(), (n, np.abs(b - wb).max())
        f = want[n + "_final"][0] if one else want[n + "_final"]
        assert np.abs(s1[n + "_final"].astype(np.int64) - f.astype(np.int64)).max() <= 1, n
        assert np.array_equal(s1[n + "_count"], cnt)
    assert s1["sheet_final"].dtype == np.uint8 and s1["normals_final"].dtype == np.uint16

    # (b) bit-identical across runs, for a budget of exactly one slab and for none; a smaller budget is refused up front
    r = streamer(max_device_bytes=None)
    s2 = _store(r.run(vol, str(tmp_path / "b")))                             # a numpy source this time
    steps = len(r.last_schedule["steps"])
    need = r.last_schedule["device_bytes"] + net.plan_for(torch.Size((2, 1, 16, 16, 16)), torch.float32, torch.device("cuda"),
                                                           False).bytes_alloc
    s3 = _store(streamer(max_device_bytes=need).run(str(arr.path), str(tmp_path / "c")))
    assert steps >= 3
    for k in s1:
        assert np.array_equal(s1[k], s2[k]) and np.array_equal(s1[k], s3[k]), k
    with pytest.raises(MemoryError):
        streamer(max_device_bytes=need - 1).run(vol, str(tmp_path / "d"))
    assert not os.path.exists(tmp_path / "d" / "predictions.zarr")

    # (c) Gaussian blending against a numpy weighted-blend oracle fed by the CPU oracle network (fp32)
    g = _store(streamer(blend="gaussian").run(str(arr.path), str(tmp_path / "g")))
    w = inf.gaussian_importance_map((16, 16, 16))
    v = (vol.astype(np.float32) / np.float32(255.0))[None]
    sums = {n: np.zeros((t["channels"],) + vol.shape, np.float32) for n, t in TASKS.items()}
    wsum = np.zeros(vol.shape, np.float32)
    pos = inf.all_positions(vol.shape, (16, 16, 16), 0.5)
    for i in range(0, len(pos), 8):
        chunk = pos[i:i + 8]
        x = torch.from_numpy(np.stack([v[:, z:z + 16, y:y + 16, xx:xx + 16] for z, y, xx in chunk]))
        with torch.no_grad():
            ref_net.train()
            out = {k: o.numpy() for k, o in ref_net(x).items()}
        for b, (z, y, xx) in enumerate(chunk):
            sl = np.s_[z:z + 16, y:y + 16, xx:xx + 16]
            sums["sheet"][(slice(None),) + sl] += w * (1.0 / (1.0 + np.exp(-out["sheet"][b])))
            sums["normals"][(slice(None),) + sl] += w * out["normals"][b]
            wsum[sl] += w
    assert np.abs(g["sheet_count"] - wsum).max() <= 1e-5
    sheet = sums["sheet"][0] / wsum
    assert np.abs(g["sheet_sum"] - sheet).max() < 2e-4
    nrm = sums["normals"] / (np.sqrt((sums["normals"] ** 2).sum(0)) + 1e-8)
    assert np.abs(g["normals_sum"] - nrm).max() < 2e-4


def test_device_memory_does_not_grow_with_z(tmp_path):
    L, _ = _lib()
    import mt3d_amd.inference as inf
    net, _ = _nets()
    vol, _ = _volume(tmp_path, 40)
    deep = np.concatenate([vol] * 4, axis=0)

    def peak(v, name):
        r = inf.StreamingInferer(net, TASKS, (16, 16, 16), batch_size=2, overlap=0.5, compute_dtype=torch.float32)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        r.run(v, str(tmp_path / name))
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - base, r.last_schedule

    peak(vol, "warm")                       # builds the plan and its lazy buffers
    p1, s1 = peak(vol, "small")
    p4, s4 = peak(deep, "deep")
    assert s4["device_bytes"] == s1["device_bytes"]
    assert p4 - p1 <= s1["input_bytes"] + s1["staging_bytes"], (p1, p4)
