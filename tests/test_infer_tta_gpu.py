"""Test-time augmentation of streaming inference on the device: `rx_sw_gather_geom` and `rx_sw_accumulate_geom` against numpy
(`apply_op_numpy` is the statement of the transform), and `StreamingInferer(tta=...)` against the numpy statement of the semantics
driven by the CPU oracle network, for bit-identity of the path without views and for determinism."""
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

FULL = {"flip": ["z", "y", "x"], "rot90": ["z", "y", "x"]}


def _lib():
    import mt3d_amd  # noqa: F401
    from mt3d_amd.engine import lib as L
    L.require_device()
    return L, L.load()


def _geo():
    import mt3d_amd  # noqa: F401
    from mt3d_amd.dataloading import geometry_device as G
    return G


def _org(patches):
    return (ctypes.c_int32 * (3 * len(patches)))(*[v for p in patches for v in p])


def _rows(ops):
    return (ctypes.c_int32 * (12 * len(ops)))(*[v for o in ops for v in o.row()])


def _ring(vol, R):
    C, Z, Y, X = vol.shape
    ring = np.zeros((C, R, Y, X), vol.dtype)
    for z in range(Z):
        ring[:, z % R] = vol[:, z]
    return ring


# ---- rx_sw_gather_geom --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [np.uint8, np.uint16, np.float32])
@pytest.mark.parametrize("patch,spec", [((8, 8, 8), FULL), ((8, 8, 12), "flip"), ((8, 8, 10), "flip")])
def test_gather_geom_against_numpy(dt, patch, spec):
    L, lib = _lib()
    G = _geo()
    import mt3d_amd.inference as inf
    rng = np.random.default_rng(1)
    pz, py, px = patch
    cin, Z, Y, X, R = 2, 20, 24, 28, 12
    if dt == np.float32:
        vol = rng.normal(size=(cin, Z, Y, X)).astype(np.float32) * 3 + 1
    else:
        vol = rng.integers(0, np.iinfo(dt).max + 1, size=(cin, Z, Y, X)).astype(dt)
        vol[0, 9, 0, :4] = np.iinfo(dt).max
    slab_z = 7                                                              # rows [7, 19) of the ring wrap around R = 12
    ring = _ring(vol[:, :slab_z + R], R)
    code = {np.uint8: L.RX_SW_U8, np.uint16: L.RX_SW_U16, np.float32: L.RX_SW_F32}[dt]
    dev = torch.from_numpy(ring.view(np.int16) if dt == np.uint16 else ring).cuda()
    div = {np.uint8: np.float32(255.0), np.uint16: np.float32(65535.0), np.float32: None}[dt]
    places = [(7, 0, 0), (9, Y - py, X - px), (11, 5, 3), (slab_z + R - pz, 16, 1)]      # slab edges, ring wrap, the interior
    views = inf.tta_views(spec, patch)
    assert len(views) == (48 if spec is FULL else 8)
    B = 12 if spec is FULL else 8                                           # 48 views over four calls; the 8 flips in one
    ws_b = lib.rx_sw_gather_workspace(B, cin, pz, py, px)
    ws = torch.empty((ws_b // 8 + 1,), dtype=torch.float64, device="cuda")

    def scaled(z, y, x):
        p = vol[:, z:z + pz, y:y + py, x:x + px].astype(np.float32)
        return p / div if div is not None else p

    for call, i0 in enumerate(range(0, len(views), B)):
        ops = list(views[i0:i0 + B])                                        # mixed ops within one batch
        patches = [places[(call + j) % len(places)] for j in range(B)]
        want = np.stack([G.apply_op_numpy(op, scaled(*p)) for op, p in zip(ops, patches)])
        out = torch.full((B, cin, pz, py, px), -7.0, dtype=torch.float32, device="cuda")
        L.check(lib.rx_sw_gather_geom(code, dev.data_ptr(), cin, R, Y, X, B, _org(patches), _rows(ops), pz, py, px, L.RX_SW_SCALE,
                                      out.data_ptr(), None, 0, L.stream_ptr()), "gather_geom")
        assert np.array_equal(out.cpu().numpy(), want), (call, dt)          # bit-exact: a gather and numpy's float32 division
        L.check(lib.rx_sw_gather_geom(code, dev.data_ptr(), cin, R, Y, X, B, _org(patches), _rows(ops), pz, py, px, L.RX_SW_ZSCORE,
                                      out.data_ptr(), ws.data_ptr(), ws_b, L.stream_ptr()), "gather_geom zscore")
        IR.check_zscore(out.cpu().numpy(), want, f"zscore {dt.__name__} call {call}")      # per element: 3u |z| + u |mean| / std
    # identity records: rx_sw_gather, bit for bit (scale and zscore)
    patches = places[:3]
    ident = [G.GeomOp()] * 3
    for norm in (L.RX_SW_SCALE, L.RX_SW_ZSCORE):
        a = torch.empty((3, cin, pz, py, px), dtype=torch.float32, device="cuda")
        b = torch.empty_like(a)
        L.check(lib.rx_sw_gather(code, dev.data_ptr(), cin, R, Y, X, 3, _org(patches), pz, py, px, norm, a.data_ptr(), ws.data_ptr(),
                                 ws_b, L.stream_ptr()), "gather")
        L.check(lib.rx_sw_gather_geom(code, dev.data_ptr(), cin, R, Y, X, 3, _org(patches), _rows(ident), pz, py, px, norm,
                                      b.data_ptr(), ws.data_ptr(), ws_b, L.stream_ptr()), "gather_geom")
        assert np.array_equal(a.cpu().numpy().view(np.uint32), b.cpu().numpy().view(np.uint32))


def test_gather_geom_refusals_launch_nothing():
    L, lib = _lib()
    G = _geo()
    cin, R, Y, X, pz, py, px = 1, 8, 16, 20, 8, 8, 12
    dev = torch.zeros((cin, R, Y, X), dtype=torch.uint8, device="cuda")
    out = torch.full((2, cin, pz, py, px), -7.0, dtype=torch.float32, device="cuda")
    ok = [G.GeomOp(), G.flip_op(2)]

    def call(org, rows, batch=2, in_code=0, norm=0):
        return lib.rx_sw_gather_geom(in_code, dev.data_ptr(), cin, R, Y, X, batch, org, rows, pz, py, px, norm, out.data_ptr(), None, 0,
                                     L.stream_ptr())
    here = _org([(0, 0, 0), (0, 8, 8)])
    bad_rows = [
        (ctypes.c_int32 * 24)(*(list(ok[0].row()) + [0, 0, 2, 0, 0, 0, 0, 1, 2, 0, 0, 0])),      # src_axis is no permutation
        (ctypes.c_int32 * 24)(*(list(ok[0].row()) + [0, 1, 2, 0, 0, 0, 0, 1, 1, 0, 0, 0])),      # ch_src is no permutation
        _rows([ok[0], G.rot90_op("z", 1)]),                                                        # 8 x 12 plane: changes the shape
    ]
    for rows in bad_rows:
        assert call(here, rows) != 0
    assert call(here, None) != 0                                            # no records
    assert call(_org([(0, 0, 0), (0, Y - py + 1, 0)]), _rows(ok)) != 0      # leaves the slab, as rx_sw_gather refuses
    assert call(here, _rows(ok), in_code=7) != 0 and call(here, _rows(ok), norm=5) != 0
    assert call(here, _rows(ok), norm=1) != 0                               # zscore without its workspace
    assert call(here, _rows(ok * 17), batch=34) != 0
    torch.cuda.synchronize()
    assert (out == -7.0).all().item()                                       # nothing was launched
    assert call(here, _rows(ok)) == 0
    assert (out.cpu().numpy() == 0).all()


# ---- rx_sw_accumulate_geom ----------------------------------------------------------------------------------------------------
def _acc_oracle(sum0, wsum0, logits, patches, valid, w, act, R, ops, vector, G):
    """the accumulate statement of test_infer_stream_gpu with the prediction moved by the slot's record before it is added"""
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
        p = G.apply_op_numpy(ops[b], p, is_normal=bool(vector))
        rows = [(z + i) % R for i in range(pz)]
        s[:, rows, y:y + py, x:x + px] += w[None] * p
        ws[rows, y:y + py, x:x + px] += w
    return s, ws


@pytest.mark.parametrize("X", [24, 22])
@pytest.mark.parametrize("act", [0, 1, 2])
@pytest.mark.parametrize("vector", [0, 1])
@pytest.mark.parametrize("weights", ["uniform", "gauss"])
@pytest.mark.parametrize("pick", [0, 1, 2])
def test_accumulate_geom_overlapping_patches(X, act, vector, weights, pick):
    L, lib = _lib()
    G = _geo()
    import mt3d_amd.inference as inf
    rng = np.random.default_rng(2 + act)
    c, R, Y, pz = 3, 16, 20, 8
    patch = (pz, 8, 8)
    patches = [(12, 0, 0), (12, 4, 3), (12, 12, X - 8), (12, 4, 3), (12, 0, 1)]   # overlaps, a repeat (with another view), edges, wrap
    B, valid = 5, 4
    views = inf.tta_views(FULL, patch)
    idx = [[5, 17, 30, 41, 9], [0, 7, 12, 23, 47], [36, 3, 44, 2, 29]][pick]     # flips, x-moving turns and the identity, mixed
    ops = [views[i].inverse() for i in idx]                                      # the records undo a view
    assert ops[1] != ops[3]
    logits = rng.integers(-4, 5, size=(B, c, *patch)).astype(np.float32)
    logits[0, :, 0, 0, :4] = 0.0                                                 # exact zeros: a negated one is -0.0
    sum0 = rng.integers(-3, 4, size=(c, R, Y, X)).astype(np.float32)
    wsum0 = rng.integers(0, 3, size=(R, Y, X)).astype(np.float32)
    if weights == "uniform":
        w = np.ones(patch, np.float32)
    elif act == 0:
        w = (rng.integers(1, 9, size=patch) / 8).astype(np.float32)            # dyadic: the sums stay exact
    else:
        w = inf.gaussian_importance_map(patch)
    s_d, w_d, l_d, wt_d = (torch.from_numpy(a).cuda() for a in (sum0, wsum0, logits, w))
    L.check(lib.rx_sw_accumulate_geom(l_d.data_ptr(), B, valid, c, *patch, _org(patches), _rows(ops), vector, act, wt_d.data_ptr(),
                                      s_d.data_ptr(), w_d.data_ptr(), R, Y, X, L.stream_ptr()), "accumulate_geom")
    s_ref, w_ref = _acc_oracle(sum0, wsum0, logits, patches, valid, w, act, R, ops, vector, G)
    if act == 0:
        assert np.array_equal(s_d.cpu().numpy(), s_ref) and np.array_equal(w_d.cpu().numpy(), w_ref)
    elif weights == "uniform":
        assert np.array_equal(w_d.cpu().numpy(), w_ref)
    ref = IR.accumulate_ref(sum0, wsum0, logits, patches, valid, w, act, R, [op.row() for op in ops], vector)      # fp64, per-element bounds
    IR.check_accumulate(s_d.cpu().numpy(), w_d.cpu().numpy(), ref, sum0, wsum0, f"accumulate_geom act {act} {weights}", exact=act == 0)
    # wsum == NULL: the sums only
    s2 = torch.from_numpy(sum0).cuda()
    L.check(lib.rx_sw_accumulate_geom(l_d.data_ptr(), B, valid, c, *patch, _org(patches), _rows(ops), vector, act, wt_d.data_ptr(),
                                      s2.data_ptr(), None, R, Y, X, L.stream_ptr()), "accumulate_geom")
    assert np.array_equal(s2.cpu().numpy().view(np.uint32), s_d.cpu().numpy().view(np.uint32))
    # identity records: rx_sw_accumulate, bit for bit
    ident = [G.GeomOp()] * B
    a_s, a_w, b_s, b_w = (torch.from_numpy(a).cuda() for a in (sum0, wsum0, sum0, wsum0))
    L.check(lib.rx_sw_accumulate(l_d.data_ptr(), B, valid, c, *patch, _org(patches), act, wt_d.data_ptr(), a_s.data_ptr(),
                                 a_w.data_ptr(), R, Y, X, L.stream_ptr()), "accumulate")
    L.check(lib.rx_sw_accumulate_geom(l_d.data_ptr(), B, valid, c, *patch, _org(patches), _rows(ident), vector, act, wt_d.data_ptr(),
                                      b_s.data_ptr(), b_w.data_ptr(), R, Y, X, L.stream_ptr()), "accumulate_geom")
    assert np.array_equal(a_s.cpu().numpy().view(np.uint32), b_s.cpu().numpy().view(np.uint32))
    assert np.array_equal(a_w.cpu().numpy().view(np.uint32), b_w.cpu().numpy().view(np.uint32))
    # refused before any launch: a batch that does not fit the ring, a vector task without 3 channels, a shape-changing record
    before = s2.cpu().numpy().copy()
    two = _org([(0, 0, 0), (9, 0, 0)])
    assert lib.rx_sw_accumulate_geom(l_d.data_ptr(), 2, 2, c, *patch, two, _rows(ops[:2]), vector, act, wt_d.data_ptr(), s2.data_ptr(),
                                     None, R, Y, X, L.stream_ptr()) != 0
    assert lib.rx_sw_accumulate_geom(l_d.data_ptr(), 2, 2, 2, *patch, _org(patches[:2]), _rows(ops[:2]), 1, act, wt_d.data_ptr(),
                                     s2.data_ptr(), None, R, Y, X, L.stream_ptr()) != 0
    assert lib.rx_sw_accumulate_geom(l_d.data_ptr(), 2, 2, c, 8, 8, 4, _org(patches[:2]), _rows([G.rot90_op("z", 1)] * 2), vector, act,
                                     wt_d.data_ptr(), s2.data_ptr(), None, R, Y, X, L.stream_ptr()) != 0
    assert lib.rx_sw_accumulate_geom(l_d.data_ptr(), 2, 2, c, *patch, _org(patches[:2]), None, vector, act, wt_d.data_ptr(),
                                     s2.data_ptr(), None, R, Y, X, L.stream_ptr()) != 0
    torch.cuda.synchronize()
    assert np.array_equal(s2.cpu().numpy().view(np.uint32), before.view(np.uint32))


def test_refusals_name_the_entry_point_called_and_every_record_is_checked():
    """the plain and the record forms share one host path each: a refusal still starts with the name of the entry point that was
    called, and rx_sw_accumulate_geom still refuses a bad record in a slot at or beyond `valid`"""
    L, lib = _lib()
    G = _geo()
    cin, R, Y, X, pz, py, px = 1, 8, 16, 20, 8, 8, 12
    sp = L.stream_ptr()
    slab = torch.zeros((cin, R, Y, X), dtype=torch.uint8, device="cuda")
    out = torch.full((2, cin, pz, py, px), -7.0, dtype=torch.float32, device="cuda")
    logits = torch.ones((2, 1, pz, py, px), dtype=torch.float32, device="cuda")
    w = torch.ones((pz, py, px), dtype=torch.float32, device="cuda")
    acc = torch.full((1, R, Y, X), -7.0, dtype=torch.float32, device="cuda")
    wsum = torch.full((R, Y, X), -7.0, dtype=torch.float32, device="cuda")
    ok = _rows([G.GeomOp(), G.flip_op(2)])
    here, away = _org([(0, 0, 0), (0, 8, 8)]), _org([(0, 0, 0), (0, Y - py + 1, 0)])      # the second origin leaves the slab in y

    def accumulate_geom(org, rows, valid=2):
        return lib.rx_sw_accumulate_geom(logits.data_ptr(), 2, valid, 1, pz, py, px, org, rows, 0, 0, w.data_ptr(), acc.data_ptr(),
                                         wsum.data_ptr(), R, Y, X, sp)
    calls = {
        "rx_sw_gather": lambda: lib.rx_sw_gather(0, slab.data_ptr(), cin, R, Y, X, 2, away, pz, py, px, 0, out.data_ptr(), None, 0, sp),
        "rx_sw_gather_geom": lambda: lib.rx_sw_gather_geom(0, slab.data_ptr(), cin, R, Y, X, 2, away, ok, pz, py, px, 0, out.data_ptr(),
                                                           None, 0, sp),
        "rx_sw_accumulate": lambda: lib.rx_sw_accumulate(logits.data_ptr(), 2, 2, 1, pz, py, px, away, 0, w.data_ptr(), acc.data_ptr(),
                                                         wsum.data_ptr(), R, Y, X, sp),
        "rx_sw_accumulate_geom": lambda: accumulate_geom(away, ok),
    }
    for name, call in calls.items():
        assert call() != 0, name
        assert lib.rx_last_error().decode().startswith(name + ": patch 1 at "), (name, lib.rx_last_error())
    bad = (ctypes.c_int32 * 24)(*(list(G.GeomOp().row()) + [0, 0, 2, 0, 0, 0, 0, 1, 2, 0, 0, 0]))      # slot 1: src_axis is no permutation
    for valid in (1, 0):                                                    # slot 1 is at `valid`, then beyond it
        assert accumulate_geom(here, bad, valid) != 0, valid
        assert lib.rx_last_error().decode().startswith("rx_sw_accumulate_geom: slot 1: src_axis (0, 0, 2) "), lib.rx_last_error()
    torch.cuda.synchronize()
    assert (out == -7.0).all().item() and (acc == -7.0).all().item() and (wsum == -7.0).all().item()      # nothing was launched
    assert accumulate_geom(here, ok, 1) == 0
    torch.cuda.synchronize()
    assert (acc[0, :pz, :py, :px] == -6.0).all().item() and (acc == -7.0).sum().item() == R * Y * X - pz * py * px


# ---- end to end -----------------------------------------------------------------------------------------------------------------
TASKS ={"sheet": {"channels": 1, "activation": "sigmoid"}, "normals": {"channels": 3, "activation": "none"}}
PATCH = (16, 16, 16)


def _nets():
    import mt3d_amd  # noqa: F401
    from mt3d_amd.builders.build_network_from_config import NetworkFromConfig
    mgr = oracle.make_mgr(PATCH, TASKS, 1, 2, True, {})
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


def _volume():
    rng = np.random.default_rng(11)
    return rng.integers(0, 256, size=(40, 36, 44)).astype(np.uint8)


def _oracle_predictions(ref_net, vol, views, G, inf):
    """{(position, view): {task: activated prediction, moved back to the patch frame}} from the CPU oracle network, driven as case
    (c) of test_streaming_end_to_end drives it"""
    v = (vol.astype(np.float32) / np.float32(255.0))[None]
    slots = [(p, g) for p in inf.all_positions(vol.shape, PATCH, 0.5) for g in views]
    preds = {}
    for i in range(0, len(slots), 16):
        chunk = slots[i:i + 16]
        x = torch.from_numpy(np.stack([G.apply_op_numpy(g, v[:, z:z + 16, y:y + 16, xx:xx + 16]) for (z, y, xx), g in chunk]))
        with torch.no_grad():
            ref_net.train()
            out = {k: o.numpy() for k, o in ref_net(x).items()}
        for b, (p, g) in enumerate(chunk):
            inv = g.inverse()
            sheet = (1.0 / (1.0 + np.exp(-out["sheet"][b]))).astype(np.float32)
            preds[(p, g)] = {"sheet": G.apply_op_numpy(inv, sheet), "normals": G.apply_op_numpy(inv, out["normals"][b], is_normal=True)}
    return preds


def _blend_oracle(preds, vol_shape, views, w, inf):
    """the numpy statement of the semantics: position-major, view-minor, the weight indexed by the destination voxel"""
    sums = {n: np.zeros((t["channels"],) + vol_shape, np.float32) for n, t in TASKS.items()}
    wsum, terms = np.zeros(vol_shape, np.float32), np.zeros(vol_shape, np.float32)
    for z, y, x in inf.all_positions(vol_shape, PATCH, 0.5):
        sl = np.s_[z:z + 16, y:y + 16, x:x + 16]
        for g in views:
            q = preds[((z, y, x), g)]
            for n in TASKS:
                sums[n][(slice(None),) + sl] += w * q[n]
            wsum[sl] += w
            terms[sl] += 1
    return sums, wsum, terms


def test_streaming_tta_end_to_end(tmp_path):
    L, _ = _lib()
    G = _geo()
    import mt3d_amd.inference as inf
    net, ref_net = _nets()
    vol = _volume()
    all_views = inf.tta_views(FULL, PATCH, TASKS)
    preds = _oracle_predictions(ref_net, vol, all_views, G, inf)       # the 8 flips are among the 48
    cnt = np.zeros(vol.shape, np.float32)
    for z, y, x in inf.all_positions(vol.shape, PATCH, 0.5):
        cnt[z:z + 16, y:y + 16, x:x + 16] += 1
    for tag, spec in (("flip", "flip"), ("full", FULL)):
        views = inf.tta_views(spec, PATCH, TASKS)
        V = len(views)
        assert V == (8 if tag == "flip" else 48) and set(views) <= set(all_views)
        for blend in ("uniform", "gaussian"):
            r = inf.StreamingInferer(net, TASKS, PATCH, batch_size=2, overlap=0.5, compute_dtype=torch.float32, blend=blend, tta=spec)
            g = _store(r.run(vol, str(tmp_path / f"{tag}_{blend}")))
            assert r.last_timing["views"] == V and r.last_timing["patches"] == 80
            assert r.last_timing["forwards"] == sum(len(st["batches"]) for st in r.last_schedule["steps"])
            w = inf.gaussian_importance_map(PATCH) if blend == "gaussian" else np.ones(PATCH, np.float32)
            sums, wsum, terms = _blend_oracle(preds, vol.shape, views, w, inf)
            assert np.array_equal(terms, V * cnt)
            for n in TASKS:
                if blend == "uniform":
                    assert np.array_equal(g[n + "_count"], V * cnt), (tag, n)
                else:
                    assert np.abs(g[n + "_count"] - wsum).max() <= 1e-5 * V, (tag, n)
            sheet = sums["sheet"][0] / wsum
            err = np.abs(g["sheet_sum"] - sheet).max()
            print(f"tta {tag} {blend}: sheet max |err| {err:.3e}")
            assert err < 2e-4, (tag, blend)
            # unit normals: where the summed views nearly cancel (a mirrored view negates a component) the direction s / |s| is not
            # determined by fp32 logits -- each of the N terms on a voxel carries the project's fp32 logit parity (5e-7), x 2 for
            # the normalisation and x 4 for the order of summation
            s = sums["normals"]
            mag = np.sqrt((s * s).sum(0))
            nrm = s / (mag + 1e-8)
            e = np.abs(g["normals_sum"] - nrm).max(0)
            bound = 2e-4 + 4e-6 * terms / np.maximum(mag, 1e-30)
            print(f"tta {tag} {blend}: normals max |err| {e.max():.3e}, max err / bound {(e / bound).max():.3f}, min |s| {mag.min():.3e}")
            assert (e <= bound).all(), (tag, blend, float((e / bound).max()))
            assert g["sheet_final"].dtype == np.uint8 and g["normals_final"].dtype == np.uint16


def test_tta_off_is_bit_identical_and_tta_is_deterministic(tmp_path):
    L, _ = _lib()
    G = _geo()
    import mt3d_amd.inference as inf
    net, _ = _nets()
    vol = _volume()

    def run(name, **k):
        r = inf.StreamingInferer(net, TASKS, PATCH, batch_size=2, overlap=0.5, compute_dtype=torch.float32, blend="gaussian", **k)
        return _store(r.run(vol, str(tmp_path / name))), r

    base, r0 = run("base")
    for name, k in (("none", dict(tta=None)), ("false", dict(tta=False)), ("ident", dict(tta=[G.GeomOp()]))):
        got, r = run(name, **k)
        assert r.last_schedule["device_bytes"] == r0.last_schedule["device_bytes"]
        for key in base:
            assert np.array_equal(base[key].view(np.uint8), got[key].view(np.uint8)), (name, key)
    spec = {"flip": ["z", "x"], "rot90": ["z"]}
    a, ra = run("tta_a", tta=spec)
    b, rb = run("tta_b", tta=spec)
    assert ra.last_schedule["device_bytes"] == r0.last_schedule["device_bytes"] and ra.last_timing["views"] == 16
    for key in a:
        assert np.array_equal(a[key].view(np.uint8), b[key].view(np.uint8)), key
    assert not np.array_equal(a["sheet_sum"], base["sheet_sum"])              # the views reached the network
