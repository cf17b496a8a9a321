"""The streaming-inference kernels (csrc/rx_infer.hip) through the C ABI, case table by case table, against the fp64 references and
per-element bounds of tests/infer_ref.py: every dispatch path (vector and scalar forms, both zscore caps, plain and record
forms), the edges of the contract (reset 0 / 1 / 2, valid 0 / 1, 32 slots, misaligned views, saturated activations) and the
refusals that must launch nothing.  Each test prints the largest err / bound it saw (`RATIO ...`, visible with -s)."""
import ctypes

import numpy as np
import pytest
import torch

import infer_ref as IR

pytestmark = pytest.mark.gpu

GATHER = {c["name"]: c for c in IR.gather_cases()}
ACC = {c["name"]: c for c in IR.accumulate_cases()}
FIN = {c["name"]: c for c in IR.finalize_cases()}
RX_EWORKSPACE = -4


def _lib():
    import mt3d_amd  # noqa: F401
    from mt3d_amd.engine import lib as L
    L.require_device()
    return L, L.load()


def _org(patches):
    return (ctypes.c_int32 * (3 * len(patches)))(*[int(v) for p in patches for v in p])


def _rows(rows):
    return (ctypes.c_int32 * (12 * len(rows)))(*[int(v) for r in rows for v in r])


def _dev(a, offset=0):
    """a numpy array on the device; offset: elements by which its base is moved off the allocation's (16-byte aligned) start"""
    a = np.ascontiguousarray(a)
    t = torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a)
    if not offset:
        return t.cuda()
    buf = torch.zeros((a.size + 8,), dtype=t.dtype, device="cuda")
    view = buf[offset:offset + a.size].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 != 0 or a.itemsize * offset % 16 == 0
    return view


def _host(t, dt=None):
    a = t.cpu().numpy()
    return a.view(np.uint16) if dt == np.uint16 else a


def _code(L, dt):
    return {"u8": L.RX_SW_U8, "u16": L.RX_SW_U16, "f32": L.RX_SW_F32}[dt]


# ---- gather -------------------------------------------------------------------------------------------------------------------
def _gather(L, lib, code, slab, case, norm, geom, B=None, origins=None, ws_short=0, out=None):
    pz, py, px = case["patch"]
    origins = case["origins"] if origins is None else origins
    B = len(origins) if B is None else B
    cin, (_, Y, X), Rr = case["cin"], case["zyx"], case["R"]
    if out is None:
        out = torch.full((len(origins), cin, pz, py, px), -7.0, dtype=torch.float32, device="cuda")
    ws_b = lib.rx_sw_gather_workspace(B, cin, pz, py, px)
    ws = torch.zeros((ws_b // 8 + 1,), dtype=torch.float64, device="cuda")
    args = (pz, py, px, norm, out.data_ptr(), ws.data_ptr() if norm else None, (ws_b - ws_short) if norm else 0, L.stream_ptr())
    if geom:
        rc = lib.rx_sw_gather_geom(code, slab.data_ptr(), cin, Rr, Y, X, B, _org(origins), _rows([IR.IDENT] * max(B, 1)), *args)
    else:
        rc = lib.rx_sw_gather(code, slab.data_ptr(), cin, Rr, Y, X, B, _org(origins), *args)
    return rc, out


@pytest.mark.parametrize("name", list(GATHER))
def test_gather_case(name):
    L, lib = _lib()
    case = GATHER[name]
    vol = IR.gather_volume(case)
    slab = _dev(IR.ring_of(vol, case["R"], case["z_lo"]))
    code = _code(L, case["dt"])
    scaled = IR.gather_scale_ref(vol, case["origins"], case["patch"])
    got = {}
    for norm in (L.RX_SW_SCALE, L.RX_SW_ZSCORE):
        for geom in (False, True):
            rc, out = _gather(L, lib, code, slab, case, norm, geom)
            L.check(rc, f"gather {name}")
            got[norm, geom] = _host(out)
        assert np.array_equal(IR.bits(got[norm, False]), IR.bits(got[norm, True])), (name, norm)      # identity records: bit for bit
    assert np.array_equal(IR.bits(got[L.RX_SW_SCALE, False]), IR.bits(scaled)), name
    if case["kind"] == "random" and case["dt"] != "f32":
        assert got[L.RX_SW_SCALE, False][0, 0, 0, 0, 0] == 1.0                                     # 255 / 255, 65535 / 65535
    ratio = IR.check_zscore(got[L.RX_SW_ZSCORE, False], scaled, name)
    print(f"RATIO gather-zscore {name} {ratio:.4f}")


def test_gather_fp32_bits_pass_through_scale():
    """NaN, +-inf, -0.0 and subnormals under SCALE: the bits of the input, plain and with identity records"""
    L, lib = _lib()
    case = dict(cin=1, zyx=(10, 6, 9), R=8, z_lo=2, patch=(3, 4, 5), origins=[(2, 0, 0), (7, 2, 4), (6, 1, 3)])
    vol = np.resize(IR.F32_SPECIALS, (1, 10, 6, 9)).astype(np.float32)
    vol.view(np.uint32)[0, 3, 1, 1] = 0x7fc01234                                                 # a NaN with a payload
    slab = _dev(IR.ring_of(vol, 8, 2))
    want = IR.gather_scale_ref(vol, case["origins"], case["patch"])
    assert np.isnan(want).any() and (want == 0).any() and (np.abs(want[np.isfinite(want) & (want != 0)]) < 2.0 ** -126).any()
    for geom in (False, True):
        rc, out = _gather(L, lib, L.RX_SW_F32, slab, case, L.RX_SW_SCALE, geom)
        L.check(rc, "gather specials")
        assert np.array_equal(IR.bits(_host(out)), IR.bits(want)), geom


def test_gather_refusals_write_nothing():
    L, lib = _lib()
    case = GATHER["batch32-u8"]
    vol = IR.gather_volume(case)
    slab = _dev(IR.ring_of(vol, case["R"], case["z_lo"]))
    org33 = case["origins"] + [case["origins"][0]]
    out = torch.full((33, 1) + case["patch"], -7.0, dtype=torch.float32, device="cuda")
    for geom in (False, True):
        rc, _ = _gather(L, lib, L.RX_SW_U8, slab, case, L.RX_SW_SCALE, geom, origins=org33, out=out)
        assert rc == -1, rc                                                                        # 33 slots: RX_EINVAL
        rc, _ = _gather(L, lib, L.RX_SW_U8, slab, case, L.RX_SW_ZSCORE, geom, ws_short=1, out=out)
        assert rc == RX_EWORKSPACE, rc                                                             # one byte short
    torch.cuda.synchronize()
    assert (out == -7.0).all().item()
    rc, _ = _gather(L, lib, L.RX_SW_U8, slab, case, L.RX_SW_ZSCORE, False, out=out)              # 32 slots with the exact size: accepted
    L.check(rc, "gather 32")
    assert (out[:32] != -7.0).all().item() and (out[32] == -7.0).all().item()


# ---- accumulate ---------------------------------------------------------------------------------------------------------------
def _gauss(patch):
    import mt3d_amd.inference as inf
    return inf.gaussian_importance_map(patch)


def _accumulate(L, lib, case, logits, w, s_d, w_d, geom, rows=None, valid=None):
    B = len(case["origins"])
    valid = case["valid"] if valid is None else valid
    a = (logits.data_ptr(), B, valid, case["c"], *case["patch"], _org(case["origins"]))
    b = (case["act"], w.data_ptr(), s_d.data_ptr(), w_d.data_ptr() if w_d is not None else None, case["R"], case["Y"], case["X"],
         L.stream_ptr())
    if geom:
        rows = [IR.IDENT] * B if rows is None else rows
        return lib.rx_sw_accumulate_geom(*a, _rows(rows), case["vector"], *b)
    return lib.rx_sw_accumulate(*a, *b)


@pytest.mark.parametrize("name", list(ACC))
def test_accumulate_case(name):
    L, lib = _lib()
    case = ACC[name]
    sum0, wsum0, logits, w = IR.accumulate_data(case, _gauss)
    ref = IR.accumulate_ref(sum0, wsum0, logits, case["origins"], case["valid"], w, case["act"], case["R"], case["rows"], case["vector"])
    l_d, wt_d = _dev(logits), _dev(w)
    runs = {}
    for geom in ((True,) if case["rows"] is not None else (False, True)):
        s_d, w_d = _dev(sum0), _dev(wsum0)
        L.check(_accumulate(L, lib, case, l_d, wt_d, s_d, w_d, geom, case["rows"]), f"accumulate {name}")
        runs[geom] = (_host(s_d), _host(w_d))
    first = runs[min(runs)]
    ratios = IR.check_accumulate(first[0], first[1], ref, sum0, wsum0, name, exact=case["act"] == 0)
    print(f"RATIO accumulate {name} sum {ratios[0]:.4f} wsum {ratios[1]:.4f}")
    if len(runs) == 2:                                                                             # identity records: bit for bit
        assert np.array_equal(IR.bits(runs[False][0]), IR.bits(runs[True][0])) and np.array_equal(IR.bits(runs[False][1]), IR.bits(runs[True][1]))
    # wsum == NULL: the same sums, bit for bit
    s2 = _dev(sum0)
    L.check(_accumulate(L, lib, case, l_d, wt_d, s2, None, case["rows"] is not None, case["rows"]), f"accumulate {name} without wsum")
    assert np.array_equal(IR.bits(_host(s2)), IR.bits(first[0]))
    if case["valid"] == 0:
        assert np.array_equal(IR.bits(first[0]), IR.bits(sum0)) and np.array_equal(IR.bits(first[1]), IR.bits(wsum0))
    if name.startswith("softmax-c1"):
        assert (first[0][:, ref["K"] > 0] == 1.0).all()                                            # expf(0) / expf(0)


@pytest.mark.parametrize("which", ["sum", "wsum"])
@pytest.mark.parametrize("name", ["span-c3-sigmoid-gauss-X24", "geom566-v1-softmax-X24"])
def test_accumulate_misaligned_view_matches_the_aligned_run(name, which):
    """X % 4 == 0 with one accumulator one float off a 16-byte boundary: the scalar form, bit-equal to the vector form"""
    L, lib = _lib()
    case = ACC[name]
    sum0, wsum0, logits, w = IR.accumulate_data(case, _gauss)
    l_d, wt_d = _dev(logits), _dev(w)
    geom = case["rows"] is not None
    s_a, w_a = _dev(sum0), _dev(wsum0)
    L.check(_accumulate(L, lib, case, l_d, wt_d, s_a, w_a, geom, case["rows"]), name)
    s_m, w_m = _dev(sum0, 1 if which == "sum" else 0), _dev(wsum0, 1 if which == "wsum" else 0)
    assert (s_m if which == "sum" else w_m).data_ptr() % 16 == 4
    L.check(_accumulate(L, lib, case, l_d, wt_d, s_m, w_m, geom, case["rows"]), name)
    assert np.array_equal(IR.bits(_host(s_a)), IR.bits(_host(s_m))) and np.array_equal(IR.bits(_host(w_a)), IR.bits(_host(w_m)))
    ref = IR.accumulate_ref(sum0, wsum0, logits, case["origins"], case["valid"], w, case["act"], case["R"], case["rows"], case["vector"])
    IR.check_accumulate(_host(s_m), _host(w_m), ref, sum0, wsum0, name)


def _table_run(X, name):
    L, lib = _lib()
    case = ACC[f"{name}-X{X}"]
    sum0, wsum0, logits, w = IR.accumulate_data(case)
    s_d, w_d = _dev(sum0), _dev(wsum0)
    L.check(_accumulate(L, lib, case, _dev(logits), _dev(w), s_d, w_d, False), case["name"])
    got = _host(s_d)
    pz, py, px = case["patch"]
    p = np.stack([np.stack([got[:, (z + i) % case["R"], y:y + py, x:x + px] for i in range(pz)], 1) for z, y, x in case["origins"]])
    return logits, p                                        # K = 1, weight 1 onto zeros: the accumulator holds p itself


@pytest.mark.parametrize("X", [24, 22])
def test_sigmoid_table_saturates_exactly(X):
    logits, p = _table_run(X, "sigmoid-table")
    assert not np.isnan(p).any()
    for x, want in ((88, 1.0), (100, 1.0), (np.inf, 1.0), (-100, 0.0), (-np.inf, 0.0)):
        assert (p[logits == x] == want).all(), (x, p[logits == x][:3])
    ref = IR.act_ref(logits[0], 1)
    err = np.abs(p[0].astype(np.float64) - ref) / IR.ulp32(ref)
    print(f"RATIO sigmoid-table X{X}: largest error {err.max():.3f} ulps of p at logit {logits[0].ravel()[np.argmax(err)]}, allowed {IR.SIGMOID_ULPS}")
    assert err.max() <= IR.SIGMOID_ULPS


@pytest.mark.parametrize("X", [24, 22])
def test_softmax_table_against_the_measured_allowance(X):
    """the measurement behind infer_ref.MEASURED_SOFTMAX_ULPS, repeated on every run: the device's p against the fp64 softmax in
    ulps of p over SOFTMAX_TABLE, within twice the recorded value; and the exact demands of the table"""
    logits, p = _table_run(X, "softmax-table")
    assert not np.isnan(p).any()
    n = int(np.prod(p.shape[2:]))
    rows_l, rows_p = logits[0].reshape(3, n).T, p[0].reshape(3, n).T
    t = IR.SOFTMAX_TABLE
    assert np.array_equal(rows_l[:len(t)], t)
    assert (rows_p[5] == np.float32(1) / np.float32(3)).all()                                     # all equal at 1000: 1 / c
    assert rows_p[6, 0] == 0 and rows_p[7, 1] == 0 and rows_p[8, 2] == 0                          # a channel at -inf: 0
    ulps = np.stack([IR.softmax_ulps(p[b], logits[b]) for b in range(p.shape[0])])
    worst = np.unravel_index(np.argmax(ulps[0].reshape(3, n).T[:len(t)]), (len(t), 3))
    print(f"RATIO softmax-table X{X}: largest error {ulps.max():.3f} ulps of p, row {t[worst[0]].tolist()} channel {worst[1]}, "
          f"recorded {IR.MEASURED_SOFTMAX_ULPS}, allowed {IR.SOFTMAX_ULPS}")
    assert ulps.max() <= IR.SOFTMAX_ULPS


# ---- finalize -----------------------------------------------------------------------------------------------------------------
def _finalize(L, lib, case, c, blend, cast, s_d, w_d, wsum_out=True, off=None, reset=None, rows=None):
    """-> (rc, blended, final, wsum_out) device tensors; off: the name of the one output to place off its alignment"""
    Rr, Y, X = case["R"], case["Y"], case["X"]
    rows = case["rows"] if rows is None else rows
    n = max(rows, 1)
    fdt = np.uint16 if cast == 1 else np.uint8
    bl = _dev(np.full((c, n, Y, X), -7.0, np.float32), 1 if off == "blended" else 0)
    fi = _dev(np.full((c, n, Y, X), 9, fdt), 1 if off == "final_out" else 0)
    wo = _dev(np.full((n, Y, X), -7.0, np.float32), 1 if off == "wsum_out" else 0) if wsum_out else None
    rc = lib.rx_sw_finalize(s_d.data_ptr(), w_d.data_ptr(), c, Rr, Y, X, case["z0"], rows, blend, cast,
                            case["reset"] if reset is None else reset, bl.data_ptr(), fi.data_ptr(), wo.data_ptr() if wsum_out else None,
                            L.stream_ptr())
    return rc, bl, fi, wo


def _fin_got(case, cast, s_d, w_d, bl, fi, wo):
    n = case["rows"]
    fdt = np.uint16 if cast == 1 else None
    return (_host(bl)[:, :n], _host(fi, fdt)[:, :n], _host(wo)[:n] if wo is not None else None, _host(s_d), _host(w_d))


@pytest.mark.parametrize("name", list(FIN))
def test_finalize_case(name):
    """every valid (blend, cast, c) on one geometry and reset: the five arrays exactly -- blended, final, the weight rows, and both
    accumulators after the call (which rows are cleared, every other row bit-identical); then the same without wsum_out"""
    L, lib = _lib()
    case = FIN[name]
    for blend, cast, c in IR.FIN_MODES:
        s, ws = IR.finalize_data(case, blend, cast, c)
        want = IR.finalize_ref(s, ws, case["R"], case["z0"], case["rows"], blend, cast, case["reset"])
        for with_wo in (True, False):
            s_d, w_d = _dev(s), _dev(ws)
            rc, bl, fi, wo = _finalize(L, lib, case, c, blend, cast, s_d, w_d, wsum_out=with_wo)
            L.check(rc, f"finalize {name}")
            IR.check_finalize(_fin_got(case, cast, s_d, w_d, bl, fi, wo), want, f"{name} {(blend, cast, c)} wsum_out={with_wo}")
            if case["rows"] == 0:
                assert (bl == -7.0).all().item() and (fi == 9).all().item()


@pytest.mark.parametrize("off", ["sum", "wsum", "blended", "wsum_out", "final_out"])
@pytest.mark.parametrize("mode", [(0, 0, 2), (1, 1, 3)])
def test_finalize_misaligned_pointer_matches_the_aligned_run(off, mode):
    """a 240-voxel plane with one pointer at a time off its alignment: the scalar form, bit-equal to the vector form"""
    L, lib = _lib()
    blend, cast, c = mode
    case = FIN["plane12x20-reset2"]
    s, ws = IR.finalize_data(case, blend, cast, c)
    want = IR.finalize_ref(s, ws, case["R"], case["z0"], case["rows"], blend, cast, case["reset"])
    s_d, w_d = _dev(s, 1 if off == "sum" else 0), _dev(ws, 1 if off == "wsum" else 0)
    rc, bl, fi, wo = _finalize(L, lib, case, c, blend, cast, s_d, w_d, off=off)
    L.check(rc, f"finalize {off}")
    IR.check_finalize(_fin_got(case, cast, s_d, w_d, bl, fi, wo), want, f"misaligned {off} {mode}")


def test_finalize_refusals_launch_nothing():
    L, lib = _lib()
    case = FIN["plane9x7-reset2"]
    s, ws = IR.finalize_data(case, 0, 0, 2)
    s_d, w_d = _dev(s), _dev(ws)
    outs = []
    bad = [dict(c=2, blend=1), dict(c=4, blend=1), dict(rows=case["R"] + 1), dict(reset=3), dict(blend=3), dict(cast=2), dict(reset=-1),
           dict(blend=-1)]
    for k in bad:
        rc, bl, fi, wo = _finalize(L, lib, case, k.get("c", 2), k.get("blend", 0), k.get("cast", 0), s_d, w_d, reset=k.get("reset"),
                                   rows=k.get("rows"))
        assert rc != 0, k
        outs += [bl, fi, wo]
    torch.cuda.synchronize()
    for t in outs:
        assert (t == (9 if t.dtype != torch.float32 else -7.0)).all().item()
    assert np.array_equal(IR.bits(_host(s_d)), IR.bits(s)) and np.array_equal(IR.bits(_host(w_d)), IR.bits(ws))


# ---- occupancy ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["u8", "u16", "f32"])
@pytest.mark.parametrize("px", [1, 2, 3, 5])
def test_occupancy_short_runs_and_an_unaligned_base(dt, px):
    """runs shorter than one 16-byte window, on a slab aligned to its element and, separately, on one that is not 16-byte aligned"""
    import mt3d_amd.inference as inf
    L, lib = _lib()
    rng = np.random.default_rng(40 + px)
    cin, Z, Y, X, Rr, pz, py = 2, 12, 7, 11, 8, 3, 4
    if dt == "f32":
        vol = rng.normal(size=(cin, Z, Y, X)).astype(np.float32)
        vol[0, 5, 1, :3] = [np.nan, np.inf, -0.0]
    else:
        vol = rng.integers(0, 4, size=(cin, Z, Y, X)).astype(IR.NP_DT[dt]) * (np.iinfo(IR.NP_DT[dt]).max // 3)
    ring = IR.ring_of(vol, Rr, 4)
    patches = [(4, 0, 0), (9, Y - py, X - px), (6, 2, 3), (5, 1, 6), (7, 3, X - px)]
    n = len(patches)
    for offset in (0, 1, 3):
        slab = _dev(ring, offset)
        assert slab.data_ptr() % ring.itemsize == 0 and (offset == 0 or slab.data_ptr() % 16 != 0)
        counts = torch.full((n + 1,), -7, dtype=torch.int64, device="cuda")
        for value in (0.0, 0.5, float(vol[np.isfinite(vol.astype(np.float64))].max()) / 2, -1.0):
            L.check(lib.rx_sw_occupancy(_code(L, dt), slab.data_ptr(), cin, Rr, Y, X, n, _org(patches), pz, py, px, value,
                                        counts.data_ptr(), L.stream_ptr()), "occupancy")
            got = counts.cpu().numpy()
            assert np.array_equal(got[:n].view(np.uint64), inf.occupancy_numpy(vol, patches, (pz, py, px), value)), (dt, px, offset, value)
            assert got[n] == -7
