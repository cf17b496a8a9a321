"""CPU: what entitles tests/test_se_gpu.py to the bounds of tests/se_ref.py.
  1. the staged reference, chained in fp64 on its own upstream values, is the published operation (oracle.SqueezeExcite /
     oracle.DropPath under autograd) to 1e-11;
  2. a float32 restatement of the kernels' arithmetic (sequential chunked line sums, fp32 matvecs, fp64 only where the kernels use
     it) stays inside every stage's bound on the whole case matrix in the three storage types, with the exempt share of `out`
     under the 0.1 % cap;
  3. every stage's bound rejects a wrong formula applied to that emulation."""
import types

import pytest
import torch
import torch.nn as nn

import resenc_oracle as oracle
import se_ref
from se_cases import CROSS, DTYPES, MATRIX, OPTIONS, Case, Opts, case_id, make_inputs


# ---- 1. the reference is the published operation -----------------------------------------------------------------------------
def oracle_block(inp, mask, eps=1e-5):
    """a = where(mask, pre, slope * pre), pre = SE(DropPath(IN(y))) + res with the oracle's modules, and its autograd gradients"""
    y = inp["y"].clone().requires_grad_(True)
    res = inp["res"].clone().requires_grad_(True)
    xh = torch.nn.functional.instance_norm(y, eps=eps)
    if inp["scale"] is not None:
        dp = oracle.DropPath(0.2).train()
        dp.forced_scale = inp["scale"]
        xh = dp(xh)
    mod = None
    if inp["se"] is not None:
        w1, b1, w2, b2 = inp["se"]
        rd, c = w1.shape
        n, _, z, yy, x = xh.shape
        # the published forward pools dims 2 and 3: of a 5-D tensor (z, y), keeping x; a 2-D net's 4-D tensor has (y, x) there
        conv = nn.Conv3d if inp["keep_x"] else nn.Conv2d
        mod = oracle.SqueezeExcite(c, types.SimpleNamespace(conv=conv)).double()
        mod.fc1 = conv(c, rd, kernel_size=1, bias=True).double()
        mod.fc2 = conv(rd, c, kernel_size=1, bias=True).double()
        tail = (1,) * (3 if inp["keep_x"] else 2)
        with torch.no_grad():
            mod.fc1.weight.copy_(w1.view(rd, c, *tail)), mod.fc1.bias.copy_(b1)
            mod.fc2.weight.copy_(w2.view(c, rd, *tail)), mod.fc2.bias.copy_(b2)
        xh = mod(xh) if inp["keep_x"] else mod(xh.reshape(n, c, z * yy, x)).reshape(n, c, z, yy, x)
    pre = xh + res
    a = torch.where(mask, pre, inp["slope"] * pre)
    a.backward(inp["g"])
    out = {"a": a.detach(), "dy": y.grad, "dres": res.grad}
    if mod is not None:
        out.update(dw1=mod.fc1.weight.grad.view(rd, c), db1=mod.fc1.bias.grad, dw2=mod.fc2.weight.grad.view(c, rd),
                   db2=mod.fc2.bias.grad)
    return out


CHAIN = [(Case(32, 8, (3, 4, 5), k, None), sc) for k in (1, 0) for sc in (False, True)] + \
        [(Case(32, 8, (1, 6, 5), 0, None), True), (Case(32, 0, (3, 4, 5), 1, None, n=3), True)]         # a 2-D net's form; DropPath only


@pytest.mark.parametrize("case,with_scale", CHAIN, ids=[case_id(c) + ("-scale" if s else "") for c, s in CHAIN])
def test_chain_is_the_published_operation(case, with_scale):
    inp = make_inputs(case, torch.float32, Opts(0.01, True, "overwrite", with_scale))
    mask = torch.rand(inp["y"].shape, generator=torch.Generator().manual_seed(3)) > 0.5     # any mask: both sides take it as given
    want = oracle_block(inp, mask)
    got = se_ref.chain(inp["y"], inp["res"], inp["g"], inp["se"], inp["scale"], case.keep_x, inp["slope"], mask)
    assert set(got) == set(want)
    for k in want:
        err = (got[k] - want[k]).abs().max().item()
        # relative to the tensor, with a floor: with keep_x = 0 pooled is the mean of an InstanceNorm output, analytically 0, and
        # dw1 = sum dh * pooled is fp64 rounding noise (1e-17) on both sides
        assert err <= 1e-11 * max(want[k].abs().max().item(), 1e-3), (k, err)
    if with_scale and case.rd:                 # the dropped sample's rows contribute nothing to dw1
        keep = inp["scale"] != 0
        sub = dict(inp, y=inp["y"][keep], res=inp["res"][keep], g=inp["g"][keep], scale=inp["scale"][keep])
        alone = se_ref.chain(sub["y"], sub["res"], sub["g"], sub["se"], sub["scale"], case.keep_x, inp["slope"], mask[keep])
        assert (got["dw1"] - alone["dw1"]).abs().max().item() <= 1e-11 * max(alone["dw1"].abs().max().item(), 1e-3)


# ---- 2. an fp32 emulation of the kernels -------------------------------------------------------------------------------------
F = torch.float32


def _plan(rows):
    want = min(max(rows // 8, 1), 128)
    rpc = (rows + want - 1) // want
    return rpc, (rows + rpc - 1) // rpc


def _line_sums(t, keep_x, c, one_column=False):
    """t: (n, c, z, y, x) float32 -> (n, L, c): per-chunk sequential sums over the rows, then the gather of se_gather_line (KL strided
    partial sums for C < 256), every add in float32 and in the kernels' order"""
    n, _, z, yy, x = t.shape
    rows = z * yy
    rpc, chunks = _plan(rows)
    tr = t.permute(0, 2, 3, 4, 1).reshape(n, rows, x, c)
    tr = torch.cat([tr, torch.zeros((n, chunks * rpc - rows, x, c), dtype=F)], 1).view(n, chunks, rpc, x, c)
    part = torch.zeros((n, chunks, x, c), dtype=F)
    for r in range(rpc):
        part = part + tr[:, :, r]
    if keep_x:
        terms = [part[:, k] for k in range(chunks)]                                     # each (n, x, c)
    else:
        terms = [part[:, k, xx].unsqueeze(1) for k in range(chunks) for xx in range(1 if one_column else x)]

    def seq(ts):
        s = torch.zeros_like(terms[0])
        for v in ts:
            s = s + v
        return s
    if c >= 256:
        return seq(terms)
    KL = 256 // c
    return seq([seq(terms[q::KL]) for q in range(KL)])


def emulate(inp, mutant=None):
    """the five entry points in float32 on the CPU -> the `dev` dict of se_ref.stage_checks.  mutant: one wrong formula."""
    y, res, g, se, scale = inp["y"], inp["res"], inp["g"], inp["se"], inp["scale"]
    keep_x, dtype = inp["keep_x"], inp["dtype"]
    n, c = y.shape[:2]
    L, R, V = se_ref.geometry(y.shape, keep_x)
    Rf, slope = torch.tensor(float(R), dtype=F), torch.tensor(inp["slope"], dtype=F)
    stats = se_ref.stats64(y).to(F)
    mean, rstd = stats[..., 0], stats[..., 1]
    m5, r5 = mean[:, :, None, None, None], rstd[:, :, None, None, None]
    s = (torch.ones(n) if scale is None else scale).to(F).view(n, 1, 1)
    dev = {"stats": stats}
    yf, gf = y.to(F), g.to(F)
    if se is not None:
        w1, b1, w2, b2 = (t.to(F) for t in se)
        pooled = (_line_sums(yf, keep_x, c, mutant == "pool_one_column") / Rf - mean.unsqueeze(1)) * rstd.unsqueeze(1)
        hidden = torch.relu((s * pooled) @ w1.T + b1)
        gate = 1 / (1 + torch.exp(-(hidden @ w2.T + b2)))
        mult = s * gate
        dev.update(pooled=pooled, hidden=hidden, gate=gate)
    else:
        mult = s.expand(n, L, c).clone()
    dev["mult"] = mult
    sp = lambda m: se_ref.spread(m if mutant != "apply_line0" else m[:, :1].expand_as(m), keep_x)      # noqa: E731
    xh = (yf - m5) * r5
    pre = xh * sp(mult)
    if res is not None:
        pre = pre + res.to(F)
    out = (pre if inp["slope"] == 1.0 else torch.where(pre > 0, pre, pre * slope)).to(dtype)
    dev["out"] = out
    gp = gf if inp["slope"] == 1.0 else torch.where(out.to(F) > 0, gf, gf * slope)
    L1, L2 = _line_sums(gp, keep_x, c), _line_sums(gp * xh, keep_x, c)
    if se is not None:
        dz2 = s * L2 * gate * ((1 - gate) if mutant != "gate_no_1mg" else 1)
        dh = dz2 @ w2
        if mutant != "no_relu_mask":
            dh = torch.where(hidden > 0, dh, torch.zeros_like(dh))
        D = s * (dh @ w1) / Rf
        t1 = mult * L1 + (Rf * D if mutant != "m1_no_RD" else 0)
        t2 = mult * L2 + (D * Rf * pooled if mutant != "m2_no_R" else D * pooled)
        rows = lambda t: t.reshape(-1, t.shape[-1]).double()                                           # noqa: E731
        dev.update(dw1=rows(dh).T @ rows(s * pooled if mutant != "dw1_no_scale" else pooled), db1=rows(dh).sum(0),
                   dw2=rows(dz2).T @ rows(hidden), db2=rows(dz2).sum(0))
    else:
        D = torch.zeros_like(mult)
        t1, t2 = mult * L1, mult * L2
    dev["dadd"] = D
    m12 = (torch.stack([t1.double().sum(1), t2.double().sum(1)], -1) / V).to(F)
    dev["m12"] = m12
    dx = gp * sp(mult) + sp(D)
    dev["dy"] = (r5 * (dx - m12[..., 0][:, :, None, None, None] - xh * m12[..., 1][:, :, None, None, None])).to(dtype)
    if inp["has_dres"]:
        old = inp["old_dres"] if mutant != "dres_ignore_old" else None
        dev["dres"] = (gp + old.to(F) if old is not None else gp).to(dtype)
    return {k: v.to(F).double() if k in ("dw1", "db1", "dw2", "db2") else v.double() for k, v in dev.items()}


def run_checks(inp, mutant=None):
    """name -> number of elements outside the bound; asserts the exempt cap of `out`"""
    bad = {}
    for chk in se_ref.stage_checks(inp, emulate(inp, mutant)):
        name, got, ref, bound, exempt = chk
        assert got.shape == ref.shape == bound.shape, (name, got.shape, ref.shape, bound.shape)
        if exempt is not None:
            assert int(exempt.sum()) <= 1e-3 * ref.numel(), (name, int(exempt.sum()), ref.numel())
        bad[name] = se_ref.violations(chk)
    return bad


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[-1])
@pytest.mark.parametrize("case", MATRIX, ids=case_id)
def test_emulation_within_bounds(case, dtype):
    bad = run_checks(make_inputs(case, dtype))
    assert not any(bad.values()), bad


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[-1])
@pytest.mark.parametrize("case", CROSS, ids=case_id)
def test_emulation_within_bounds_options(case, dtype):
    for opts in OPTIONS:
        bad = run_checks(make_inputs(case, dtype, opts))
        assert not any(bad.values()), (opts, bad)


def test_dropped_sample_is_exactly_zero():
    case = MATRIX[0]
    inp = make_inputs(case, torch.bfloat16)
    dev = emulate(inp)
    drop = inp["scale"] == 0
    assert drop.any() and all((dev[k][drop] == 0).all() for k in ("mult", "dadd", "dy"))
    refs = {c[0]: c for c in se_ref.stage_checks(inp, dev)}
    for k in ("mult", "dadd", "dy"):                                  # ... and the reference asks for exactly that
        assert (refs[k][2][drop] == 0).all() and (refs[k][3][drop] < 1e-40).all(), k


# ---- 3. the bounds reject wrong formulas -------------------------------------------------------------------------------------
MUTANTS = [
    # (mutant, case, options, the outputs that must leave their bound)
    ("m1_no_RD", MATRIX[0], Opts(), ["m12"]),
    ("m2_no_R", MATRIX[0], Opts(), ["m12"]),
    ("gate_no_1mg", MATRIX[0], Opts(), ["dadd", "dw1", "db1", "dw2", "db2"]),
    ("no_relu_mask", MATRIX[0], Opts(), ["dadd", "dw1", "db1"]),
    ("gate_no_1mg", MATRIX[10], Opts(), ["dadd", "dw1", "db1", "dw2", "db2"]),
    ("no_relu_mask", MATRIX[10], Opts(), ["dadd", "dw1", "db1"]),
    ("dw1_no_scale", MATRIX[0], Opts(), ["dw1"]),
    ("pool_one_column", MATRIX[15], Opts(), ["pooled"]),
    ("apply_line0", MATRIX[0], Opts(), ["out", "dy"]),
    ("dres_ignore_old", MATRIX[0], Opts(), ["dres"]),
]


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[-1])
@pytest.mark.parametrize("mutant,case,opts,must", MUTANTS, ids=[m[0] + "-" + case_id(m[1]) for m in MUTANTS])
def test_bounds_reject_wrong_formula(mutant, case, opts, must, dtype):
    inp = make_inputs(case, dtype, opts)
    assert not any(run_checks(inp).values())
    bad = run_checks_mutant(inp, mutant)
    for name in must:
        assert bad[name] > 0, (mutant, name, bad)


def run_checks_mutant(inp, mutant):
    """the checks of a mutated run, each stage given the mutated run's own upstream outputs (so only the wrong stage fails, and a stage
    downstream of a wrong but self-consistent value does not)"""
    dev = emulate(inp, mutant)
    return {chk[0]: se_ref.violations(chk) for chk in se_ref.stage_checks(inp, dev)}
