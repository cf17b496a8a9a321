"""GPU (-m gpu): every row of the dispatch ledger (tests/conv_dispatch_cases.py) that does not point at an existing test, in each of
its dtypes.  One case is one ledger shape in one dtype, run through every entry point of its family:

  * the kernel rx_last_conv_kernel() reports equals the row's, in fp32 too;
  * the integer pass of test_ops_gpu.py (every element bit-exact, outputs poisoned between guard channels) runs on the same kernels;
  * a random-float pass is held per element to an fp64 torch reference.  Nothing in the bound is tuned: products of 16-bit operands
    are exact in fp32 and an fp32 sum of K terms in ANY order -- split-K and slab reduces included -- is within gamma(K-1) sum|x w|
    of the exact one (gamma(K) in fp32 mode, where the products round too); the bias, and the old value of `dx +=`, are one more
    term each; then one rounding into the storage type.  dw is an fp32 output of K = batch * voxels terms.
  * the rows of the statistics entry points keep what test_conv3d_fwd_stats / test_conv3d_bwd_data_instats assert.

  * every output of the random pass is hashed and compared with tests/data/conv_dispatch.json, recorded before the dispatch moved
    into the planners of csrc/rx_gather_plan.h and csrc/rx_wgrad_plan.h (conv_dispatch_record.py): the same launches, no new work.

The input is read through a channel slice of a wider buffer (ld = c + 32, c0 = 32) in every case, and dy of the transposed conv through
the second half of a concat (ld = 2 co, c0 = co), so an addressing error cannot hide behind a dense tensor.  The two 16-bit types share one
reference: their data is representable in both (8 significant bits within the fp16 range)."""
import math

import pytest
import torch
import torch.nn.functional as F

import conv_dispatch_cases as L
import conv_dispatch_record as REC
from exact_ops import poisoned
from norm_bounds import check_stats
from op_bounds import check, check_m12
from test_ops_gpu import _EXACT, exact_conv_pass, exact_conv_ref, exact_convT_pass, last_kernel, nan_act, to_act

pytestmark = pytest.mark.gpu

CASES = [(key, dt) for key, s in L.SHAPES.items() for dt in s.dtypes]
DW5 = ("co", "ci", "kz", "ky", "kx")


@pytest.fixture(scope="module")
def ops():
    import mt3d_amd  # noqa: F401
    from mt3d_amd.engine import lib, ops as _ops
    lib.require_device()
    return _ops


def rnd(shape, half, seed, scale=1.0):
    """seeded normal data held in fp64: representable in bf16 AND fp16 (`half`), or in fp32"""
    t = torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale
    return (t.to(torch.bfloat16).to(torch.float16) if half else t).double()


def operands(s, half):
    """x, w and the bias of a shape"""
    T = s.kind == "convT"
    x = rnd((s.n, s.ci, *s.dims), half, 1)
    w = rnd((s.ci, s.co, *s.s) if T else (s.co, s.ci, *s.k), half, 2, (s.ci * (1 if T else math.prod(s.k))) ** -0.5)
    return x, w, rnd((s.co,), False, 3).float().double()


_REF = {}


def reference(key, half):
    """operands, fp64 results and the sums of magnitudes sum|a b| of every output of one ledger shape; the last shape only is kept"""
    if (key, half) in _REF:
        return _REF[(key, half)]
    for k_ in [k_ for k_ in _REF if k_[0] != key]:
        del _REF[k_]
    s = L.SHAPES[key]
    T = s.kind == "convT"
    taps = math.prod(s.s if T else s.k)
    x, w, b = operands(s, half)
    if T:
        conv = lambda a, c: F.conv_transpose3d(a, c, stride=s.s)                                          # noqa: E731
    else:
        conv = lambda a, c: F.conv3d(a, c, stride=s.s, padding=[(kk - 1) // 2 for kk in s.k])             # noqa: E731
    xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    y = conv(xr, wr)
    gy = rnd(tuple(y.shape), half, 4, 0.25)
    base = rnd(tuple(x.shape), half, 5, 0.25)
    y.backward(gy)
    xa, wa = x.abs().requires_grad_(True), w.abs().requires_grad_(True)
    ya = conv(xa, wa)
    ya.backward(gy.abs())
    odims = tuple(y.shape[2:])
    r = dict(x=x, w=w, b=b, gy=gy, base=base, y=y.detach() + b.view(1, -1, 1, 1, 1), dx=xr.grad, dw=wr.grad,
             a_y=ya.detach() + b.abs().view(1, -1, 1, 1, 1), a_dx=xa.grad, a_dw=wa.grad, odims=odims,
             # terms per output element: forward (with the bias), data gradient, weight gradient
             K=(s.ci * (1 if T else taps) + 1, s.co * taps, s.n * math.prod(s.dims if T else odims)))
    _REF[(key, half)] = r
    return r


def expected(key, dtn):
    rows = L.rows_for(key, dtn)
    assert rows, (key, dtn)
    return {r.entry: r for r in rows}


def run_entries(ops, s, dtype, r, case):
    """every entry point of the family of `s` on the operands r (x, w, b, gy, base, odims): the kernel each call names, the handles
    of what it read and wrote; each name and output goes through REC.note as `case`"""
    seen, h = {}, {}
    bias = r["b"].float().cuda()

    def ran(entry, out):
        seen[entry] = last_kernel(ops)
        REC.note(case, entry, seen[entry], out)

    if s.kind == "convT":
        co = s.co
        xa = to_act(ops, r["x"], dtype, ld=s.ci + 32, c0=32)        # x through a channel slice, dy through the SECOND half of a concat
        w_fwd, w_bwd = ops.pack_convT_weight(r["w"].float().cuda(), dtype)
        cat = ops.Act(torch.full((s.n, *r["odims"], 2 * co), 3.0, dtype=dtype, device="cuda"))
        cat.t[..., :co] = float("nan")
        ops.convT3d_fwd(xa, w_fwd, bias, cat.slice(0, co), s.s)
        ran(L.TFWD, cat.t)
        gya = to_act(ops, r["gy"], dtype, ld=2 * co, c0=co)
        dx = nan_act(s.n, s.dims, s.ci, dtype)
        ops.convT3d_bwd_data(gya, w_bwd, dx, s.s)
        ran(L.TDX, dx.t)
        dxa = to_act(ops, r["base"], dtype)
        ops.convT3d_bwd_data(gya, w_bwd, dxa, s.s, True)
        ran(L.TDXA, dxa.t)
        dw = poisoned(r["w"].shape)
        ops.convT3d_bwd_weight(xa, gya, dw, s.s)
        ran(L.TDW, dw)
        h.update(cat=cat)
    else:
        xa = to_act(ops, r["x"], dtype, ld=s.ci + 32, c0=32)
        w_fwd, w_bwd = ops.pack_conv_weight(r["w"].float().cuda(), dtype)
        y = nan_act(s.n, r["odims"], s.co, dtype)
        ops.conv3d_fwd(xa, w_fwd, bias, y, s.k, s.s)
        ran(L.FWD, y.t)
        gya = to_act(ops, r["gy"], dtype)
        dx = nan_act(s.n, s.dims, s.ci, dtype)
        ops.conv3d_bwd_data(gya, w_bwd, dx, s.k, s.s, accumulate=False)
        ran(L.DX, dx.t)
        dxa = to_act(ops, r["base"], dtype)
        ops.conv3d_bwd_data(gya, w_bwd, dxa, s.k, s.s, accumulate=True)
        ran(L.DXA, dxa.t)
        dw = poisoned(r["w"].shape)
        ops.conv3d_bwd_weight(xa, gya, dw, s.k, s.s)
        ran(L.DW, dw)
        h.update(y=y, w_fwd=w_fwd)
    h.update(xa=xa, gya=gya, w_bwd=w_bwd, dx=dx, dxa=dxa, dw=dw, bias=bias)
    return seen, h


@pytest.mark.parametrize("key,dtn", CASES, ids=[f"{k}-{d}" for k, d in CASES])
def test_ledger_row(ops, key, dtn):
    s = L.SHAPES[key]
    dtype = getattr(torch, dtn)
    rows = expected(key, dtn)
    r = reference(key, dtype != torch.float32)
    Kf, Kd, Kw = r["K"]
    seen, h = run_entries(ops, s, dtype, r, f"{key}-{dtn}")
    dx, dxa = h["dx"], h["dxa"]
    if s.kind == "convT":
        co = s.co
        check(h["cat"].slice(0, co).to_ncdhw(), r["y"], r["a_y"], Kf, dtype, f"up ({seen[L.TFWD]})")
        assert torch.all(h["cat"].slice(co, co).tensor() == 3.0)
        check(dx.to_ncdhw(), r["dx"], r["a_dx"], Kd, dtype, f"dx ({seen[L.TDX]})")
        check(dxa.to_ncdhw(), r["base"] + r["dx"], r["a_dx"] + r["base"].abs(), Kd + 1, dtype, f"dx += ({seen[L.TDXA]})")
        check(h["dw"], r["dw"], r["a_dw"], Kw, dtype, f"dw ({seen[L.TDW]})", names=("ci", "co", "kz", "ky", "kx"))
        ex = exact_convT_pass(ops, dtype, exact_conv_ref(("dispatch", key), s.ci, s.co, s.dims, None, s.s, s.n, transposed=True), s.s)
        assert ex["fwd"] == seen[L.TFWD] and ex["wgrad"] == seen[L.TDW], (seen, ex)
    else:
        check(h["y"].to_ncdhw(), r["y"], r["a_y"], Kf, dtype, f"y ({seen[L.FWD]})")
        check(dx.to_ncdhw(), r["dx"], r["a_dx"], Kd, dtype, f"dx ({seen[L.DX]})")
        check(dxa.to_ncdhw(), r["base"] + r["dx"], r["a_dx"] + r["base"].abs(), Kd + 1, dtype, f"dx += ({seen[L.DXA]})")
        check(h["dw"], r["dw"], r["a_dw"], Kw, dtype, f"dw ({seen[L.DW]})", names=DW5)
        if L.STATS in rows:
            stats_rows(ops, s, dtype, rows, h["xa"], h["w_fwd"], h["bias"], h["y"])
        for e, acc, plain in ((L.BS, False, dx), (L.BSA, True, dxa)):
            if e in rows:
                instats_rows(ops, s, dtype, rows[e], r, h["gya"], h["w_bwd"], acc, plain)
        ex = exact_conv_pass(ops, dtype, exact_conv_ref(("dispatch", key), s.ci, s.co, s.dims, s.k, s.s, s.n), s.k, s.s, 32)
        assert {L.FWD: ex["fwd"], L.DX: ex["dgrad"], L.DXA: ex["dgrad+"], L.DW: ex["wgrad"]} == seen, (seen, ex)     # same kernels
    for e, row in rows.items():
        if e in seen:
            assert seen[e] == row.kernel, (key, dtn, e, seen[e], row.kernel, row.why)
    if dtn == s.dtypes[-1]:
        _EXACT.pop(("dispatch", key), None)


def stats_rows(ops, s, dtype, rows, xa, w_fwd, bias, y):
    """conv3d_fwd_stats: y bit-identical to conv3d_fwd, (mean, rstd) within the fp32 bound of the fp64 statistics of y as stored"""
    y2, st = nan_act(s.n, s.dims, s.co, dtype), poisoned((s.n, s.co, 2))
    ops.conv3d_fwd_stats(xa, w_fwd, bias, y2, s.k, s.s, st)
    name = last_kernel(ops)
    torch.cuda.synchronize()
    assert name == rows[L.STATS].kernel, (name, rows[L.STATS])
    assert torch.equal(y.t, y2.t)
    check_stats(st, y2, what=f"stats ({name})")
    st2 = poisoned((s.n, s.co, 2))
    ops.instnorm_stats(y, st2)
    assert torch.allclose(st, st2, rtol=2e-5, atol=2e-6), (st - st2).abs().max()


def instats_rows(ops, s, dtype, row, r, gya, w_bwd, acc, plain):
    """conv3d_bwd_data_instats: dx bit-identical to conv3d_bwd_data; the value returned is the row's take_bs; fused: m12 within its
    per-(n, c) bound of the fp64 sums over the stored dx; not fused: m12 untouched, as include/rxunet.h documents"""
    n, c, dims, slope = s.n, s.ci, s.dims, 0.01
    yv = to_act(ops, rnd((n, c, *dims), dtype != torch.float32, 6) + 0.3, dtype)
    stats = poisoned((n, c, 2))
    ops.instnorm_stats(yv, stats)
    dx2 = to_act(ops, r["base"], dtype)
    m12 = torch.full((n, c, 2), -3.0, device="cuda")
    fused = ops.conv3d_bwd_data_instats(gya, w_bwd, dx2, s.k, s.s, acc, yv, stats, slope, m12)
    name = last_kernel(ops)
    torch.cuda.synchronize()
    assert name == row.kernel, (name, row)
    assert fused == (row.sub != "not fused"), (fused, row)
    assert torch.equal(plain.t, dx2.t)
    if not fused:
        assert (m12 == -3.0).all(), "m12 written by a call that returned fused = 0"
        return
    mean = stats[..., 0].double().cpu().view(n, c, 1, 1, 1)
    rstd = stats[..., 1].double().cpu().view(n, c, 1, 1, 1)
    xh = (yv.to_ncdhw().double().cpu() - mean) * rstd
    check_m12(m12, dx2.to_ncdhw().double().cpu(), xh, slope, dtype, f"m12 ({name})")
