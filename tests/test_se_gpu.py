"""GPU (-m gpu): SqueezeExcite / DropPath kernels (csrc/rx_se.hip) through the C ABI.

PARITY UNPINNED: the two classes live in the un-vendored dynamic_network_architectures package (absent from the reference
tree and from this image; no reference test or fixture covers them).  The checker here is the oracle's restatement of
their published source (oracle/resenc_oracle.py::SqueezeExcite / DropPath) run in fp64 on the CPU with autograd.

Every output of the five entry points is held per element to the staged fp64 reference of tests/se_ref.py (each stage given the
device's own upstream outputs and LeakyReLU mask; bounds from the fp32 error analysis, entitled by tests/test_se_ref_cpu.py) over
the case matrix of tests/se_cases.py: one row per dispatch path, the gate kernel of each row pinned, activations read and written
through channel slices between guard channels, every output NaN-poisoned."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import resenc_oracle as oracle  # noqa: F401
import se_ref
from exact_ops import NAMES5, Guarded, assert_within, poisoned
from helpers import rel_l2
from se_cases import CROSS, DETERMINISM, DTYPES, MATRIX, OPTIONS, Opts, case_id, make_inputs

TOL = {torch.float32: 2e-5, torch.bfloat16: 1.5e-2, torch.float16: 3e-3}
dt_id = lambda d: str(d).split(".")[-1]      # noqa: E731


@pytest.fixture(scope="module")
def ops():
    import mt3d_amd  # noqa: F401
    from mt3d_amd.engine import ops as o
    return o


def to_act(ops, t, dtype, pad=32):
    """NCDHW fp64 (values representable in dtype) -> an Act on channels [pad, pad + c) of a (c + pad)-wide buffer"""
    if t is None:
        return None
    n, c, z, y, x = t.shape
    buf = torch.full((n, z, y, x, c + pad), 7.0, dtype=dtype, device="cuda")      # poison the unused channels
    buf[..., pad:] = t.permute(0, 2, 3, 4, 1).to(dtype).cuda()
    return ops.Act(buf, pad, c)


def last_kernel(ops):
    return ops.load().rx_last_conv_kernel().decode()


def device_weights(se, misaligned):
    """fp32 device copies of (w1, b1, w2, b2); misaligned: w1 and w2 as views 4 bytes into larger buffers"""
    dev = [t.float().cuda().contiguous() for t in se]
    if misaligned:
        for i in (0, 2):
            buf = torch.zeros(dev[i].numel() + 1, dtype=torch.float32, device="cuda")
            buf[1:] = dev[i].flatten()
            dev[i] = buf[1:].view(dev[i].shape)
            assert dev[i].data_ptr() % 16 != 0 and dev[i].is_contiguous()
    return dev


def run_block(ops, inp, misaligned=False):
    """the five entry points on one input set -> (dev: every output as fp64 CPU tensors, bits: the raw device outputs, kernels)"""
    y, dtype, keep_x, slope = inp["y"], inp["dtype"], inp["keep_x"], inp["slope"]
    n, c, dims = y.shape[0], y.shape[1], tuple(y.shape[2:])
    L = se_ref.geometry(y.shape, keep_x)[0]
    ya, ra, ga = to_act(ops, y, dtype), to_act(ops, inp["res"], dtype), to_act(ops, inp["g"], dtype)
    out, dy = Guarded(n, dims, c, dtype), Guarded(n, dims, c, dtype)
    dres = Guarded(n, dims, c, dtype, init_ncdhw=inp["old_dres"]) if inp["has_dres"] else None
    small = dict(stats=poisoned((n, c, 2)), mult=poisoned((n, L, c)), dadd=poisoned((n, L, c)), m12=poisoned((n, c, 2)))
    se, grads = None, [None] * 4
    if inp["se"] is not None:
        w = device_weights(inp["se"], misaligned)
        rd = w[0].shape[0]
        se = dict(w1=w[0], b1=w[1], w2=w[2], b2=w[3], rd=rd, keep_x=keep_x)
        small.update(pooled=poisoned((n, L, c)), hidden=poisoned((n, L, rd)), gate=poisoned((n, L, c)))
        grads = [poisoned(t.shape) for t in w]
        small.update(zip(("dw1", "db1", "dw2", "db2"), grads))
    sc = inp["scale"].float().cuda() if inp["scale"] is not None else None
    oa = out.act(ops)
    kernels = {}
    ops.instnorm_stats(ya, small["stats"])
    ops.se_gate_fwd(ya, small["stats"], se, small.get("pooled"), small.get("hidden"), small.get("gate"), small["mult"], sc)
    kernels["fwd"] = last_kernel(ops)
    ops.instnorm_gate_act_fwd(ya, small["stats"], small["mult"], keep_x, oa, slope, ra)
    ops.se_gate_bwd(ga, ya, small["stats"], oa, slope, se, small.get("pooled"), small.get("hidden"), small.get("gate"), small["mult"],
                    small["dadd"], small["m12"], *grads, path_scale=sc)
    kernels["bwd"] = last_kernel(ops)
    ops.instnorm_gate_act_bwd(ga, ya, small["stats"], oa, slope, small["mult"], small["dadd"], small["m12"], keep_x, dy.act(ops),
                              dres.act(ops) if dres is not None else None, inp["old_dres"] is not None)
    torch.cuda.synchronize()
    out.check("out"), dy.check("dy")
    bits = dict(small, out=out.buf, dy=dy.buf)
    if dres is not None:
        dres.check("d_residual")
        bits["dres"] = dres.buf
    dev = {k: v.detach().double().cpu() for k, v in small.items()}
    # (contiguous NCDHW: torch's CPU autograd mistakes a permuted view of a batch of one for channels-last and returns other gradients)
    dev.update(out=out.ncdhw().double().cpu().contiguous(), dy=dy.ncdhw().double().cpu().contiguous())
    if dres is not None:
        dev["dres"] = dres.ncdhw().double().cpu().contiguous()
    return dev, bits, kernels


def assert_stages(inp, dev, what=""):
    """every stage per element; the exact zeros of a dropped sample; returns (exempt share of `out`, largest gate error in ulps)"""
    share = 0.0
    for name, got, ref, bound, exempt in se_ref.stage_checks(inp, dev):
        assert got.shape == ref.shape, (name, got.shape, ref.shape)
        assert_within(got, ref, bound, f"{what} {name}", names=NAMES5 if got.dim() == 5 else se_ref.NAMES[name], exempt=exempt)
        if exempt is not None:
            share = exempt.double().mean().item()
        if name == "gate":
            ulps = ((got - ref).abs() / se_ref.ulp32(ref)).max().item()
    if inp["scale"] is not None:
        drop = inp["scale"] == 0
        for k in ("mult", "dadd", "dy"):
            assert (dev[k][drop] == 0).all(), f"{what} {k}: a sample with path_scale 0 is not exactly 0"
    return share, (ulps if inp["se"] is not None else 0.0)


def expected_fwd(case):
    return "se_gate_fwd_kernel" if case.rd else "se_fill_mult_kernel"


MATRIX_RUNS = [(c, d) for c in MATRIX for d in DTYPES if not (d == torch.float32 and c.c > 1024)]     # fp32 statistics stop at 1024 channels


@pytest.mark.parametrize("case,dtype", MATRIX_RUNS, ids=[f"{case_id(c)}-{dt_id(d)}" for c, d in MATRIX_RUNS])
def test_se_matrix(ops, case, dtype):
    inp = make_inputs(case, dtype)
    dev, _, kernels = run_block(ops, inp, misaligned=case.flag == "misaligned")
    assert kernels == {"fwd": expected_fwd(case), "bwd": case.bwd}, (case, kernels)
    share, ulps = assert_stages(inp, dev, case_id(case))
    print(f"{case_id(case)} {dt_id(dtype)}: {kernels['bwd']}, exempt share {share:.2e}, gate error {ulps:.2f} ulp")


@pytest.mark.parametrize("dtype", DTYPES, ids=dt_id)
@pytest.mark.parametrize("case", CROSS, ids=case_id)
def test_se_options(ops, case, dtype):
    """slope x forward residual x d_residual mode x path_scale on a small-kernel, a general-kernel and a DropPath-only case"""
    for opts in OPTIONS:
        inp = make_inputs(case, dtype, opts)
        dev, _, kernels = run_block(ops, inp)
        assert kernels == {"fwd": expected_fwd(case), "bwd": case.bwd}, (case, opts, kernels)
        assert_stages(inp, dev, f"{case_id(case)} {opts}")


@pytest.mark.parametrize("dtype", DTYPES, ids=dt_id)
@pytest.mark.parametrize("case", DETERMINISM, ids=case_id)
def test_se_deterministic(ops, case, dtype):
    """fixed-order sums, no atomics: two runs into fresh poisoned outputs agree bit for bit"""
    inp = make_inputs(case, dtype)
    _, a, _ = run_block(ops, inp)
    _, b, _ = run_block(ops, inp)
    assert set(a) == set(b)
    for k in a:
        ib = {4: torch.int32, 2: torch.int16}[a[k].element_size()]
        assert torch.equal(a[k].view(ib), b[k].view(ib)), f"{k} differs between two runs"


def _reference(y, res, g, w1, b1, w2, b2, scale, keep_x, slope, mask=None, eps=1e-5):
    """fp64 autograd restatement: a = lrelu(SE(DropPath(IN(y))) + res); returns a, dy, dres, fc gradients.  mask: the LeakyReLU
    branch of every element as the device's saved output has it (None: the sign of the fp64 pre-activation)"""
    y = y.clone().requires_grad_(True)
    res = res.clone().requires_grad_(True)
    ps = [p.clone().requires_grad_(True) for p in (w1, b1, w2, b2)] if w1 is not None else None
    xh = F.instance_norm(y, eps=eps)
    if scale is not None:
        xh = xh * scale.view(-1, 1, 1, 1, 1)
    if ps is not None:
        if keep_x:
            p = xh.mean((2, 3), keepdim=True)                 # the published forward: dims 2 and 3 of a 5-D tensor
        else:
            p = xh.mean((2, 3, 4), keepdim=True)              # a 4-D tensor (2-D net): (y, x) = every spatial axis here
        h = torch.relu(F.conv3d(p, ps[0], ps[1]))
        xh = xh * torch.sigmoid(F.conv3d(h, ps[2], ps[3]))
    pre = xh + res
    a = F.leaky_relu(pre, slope) if mask is None else torch.where(mask, pre, slope * pre)
    a.backward(g)
    return a.detach(), y.grad, res.grad, [p.grad for p in ps] if ps is not None else None


CASES = [
    # (n, c, (z, y, x), rd, keep_x, with_se, with_scale)
    (2, 32, (6, 5, 16), 8, 1, True, False),
    (2, 64, (4, 4, 12), 8, 1, True, True),
    (1, 256, (3, 3, 4), 16, 1, True, False),
    (2, 512, (2, 2, 2), 32, 1, True, True),
    (2, 32, (1, 12, 20), 8, 0, True, False),       # 2-D net: unit z axis, pooled over everything
    (3, 32, (4, 4, 8), 0, 1, False, True),         # DropPath only
    (2, 320, (2, 3, 5), 24, 1, True, False),       # C > 256 and not a power of two
]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", CASES)
def test_se_block_fwd_bwd(ops, dtype, case):
    n, c, dims, rd, keep_x, with_se, with_scale = case
    gen = torch.Generator().manual_seed(7)
    rnd = lambda *s, k=1.0: (torch.randn(*s, generator=gen) * k).to(dtype).double()
    y, res, g = rnd(n, c, *dims), rnd(n, c, *dims), rnd(n, c, *dims, k=0.1)
    slope = 0.01
    if with_se:
        w1, b1 = torch.randn(rd, c, 1, 1, 1, generator=gen).double() * 0.3, torch.randn(rd, generator=gen).double() * 0.1
        w2, b2 = torch.randn(c, rd, 1, 1, 1, generator=gen).double() * 0.3, torch.randn(c, generator=gen).double() * 0.1
        se = tuple(t.float().double() for t in (w1.view(rd, c), b1, w2.view(c, rd), b2))       # as the device holds them
        w1, b1, w2, b2 = se[0].view(rd, c, 1, 1, 1), se[1], se[2].view(c, rd, 1, 1, 1), se[3]
    else:
        w1 = b1 = w2 = b2 = se = None
    scale = torch.tensor([0.0, 1.25, 1.25][:n] if n <= 3 else [1.25] * n).double() if with_scale else None
    if with_scale and n == 2:
        scale = torch.tensor([1.25, 0.0]).double()
    old = torch.full_like(y, 0.5)                            # accumulate into an existing gradient
    inp = dict(y=y, res=res, g=g, se=se, scale=scale, keep_x=keep_x, slope=slope, dtype=dtype, old_dres=old, has_dres=True)
    dev, _, _ = run_block(ops, inp)
    # the backward kernels take the LeakyReLU mask from the saved output: so does the reference
    a_r, dy_r, dres_r, pg_r = _reference(y, res, g, w1, b1, w2, b2, scale, keep_x, slope, mask=dev["out"] > 0)
    tol = TOL[dtype]
    a_fwd = _reference(y, res, g, w1, b1, w2, b2, scale, keep_x, slope)[0]
    assert rel_l2(dev["out"], a_fwd) < tol
    assert_stages(inp, dev, str(case))
    assert rel_l2(dev["dy"], dy_r) < 20 * tol + 2e-2 * (dtype != torch.float32)
    assert rel_l2(dev["dres"] - 0.5, dres_r) < 20 * tol + 2e-2 * (dtype != torch.float32)
    if with_se:
        for k, want in zip(("dw1", "db1", "dw2", "db2"), pg_r):
            # (with keep_x = 0 the pooled value is the mean of an InstanceNorm output, i.e. ~0: dw1 is rounding noise there)
            err = (dev[k] - want.view(dev[k].shape)).norm().item()
            assert err < (20 * tol + 2e-2 * (dtype != torch.float32)) * want.norm().item() + 1e-5


def test_se_error_paths(ops):
    """every refusal raises RxError and launches nothing: the poisoned outputs stay NaN"""
    from mt3d_amd.engine.lib import RxError
    f32 = dict(dtype=torch.float32, device="cuda")
    bf = dict(dtype=torch.bfloat16, device="cuda")

    def world(c, rd, x=4):
        y = ops.Act(torch.zeros((1, 2, 2, x, c), **bf))
        w = dict(y=y, g=ops.Act(torch.zeros((1, 2, 2, x, c), **bf)), out=ops.Act(torch.zeros((1, 2, 2, x, c), **bf)),
                 stats=torch.zeros((1, c, 2), **f32), mult=torch.zeros((1, x, c), **f32),
                 se=dict(w1=torch.zeros(rd, c, **f32), b1=torch.zeros(rd, **f32), w2=torch.zeros(c, rd, **f32), b2=torch.zeros(c, **f32),
                         rd=rd, keep_x=1))
        w["outs"] = {k: poisoned(s) for k, s in dict(pooled=(1, x, c), hidden=(1, x, rd), gate=(1, x, c), mult_o=(1, x, c), dadd=(1, x, c),
                                                     m12=(1, c, 2), dw1=(rd, c), db1=(rd,), dw2=(c, rd), db2=(c,), stats_o=(1, c, 2)).items()}
        w["dy"], w["dres"], w["o"] = (ops.Act(poisoned((1, 2, 2, x, c), torch.bfloat16)) for _ in range(3))
        return w

    def fwd(w, ws=None, se="se"):
        o = w["outs"]
        ops.se_gate_fwd(w["y"], w["stats"], w[se] if se else None, o["pooled"], o["hidden"], o["gate"], o["mult_o"], None, ws)

    def bwd(w, ws=None, out="out", slope=0.01):
        o = w["outs"]
        ops.se_gate_bwd(w["g"], w["y"], w["stats"], w[out] if out else None, slope, w["se"], o["pooled"], o["hidden"], o["gate"], w["mult"],
                        o["dadd"], o["m12"], o["dw1"], o["db1"], o["dw2"], o["db2"], ws=ws)

    def act_fwd(w, out=None):
        ops.instnorm_gate_act_fwd(w["y"], w["stats"], w["mult"], 1, out or w["o"], 0.01, None)

    def act_bwd(w, out="out", slope=0.01, dy=None):
        ops.instnorm_gate_act_bwd(w["g"], w["y"], w["stats"], w[out] if out else None, slope, w["mult"], w["mult"], w["stats"], 1,
                                  dy or w["dy"], w["dres"], False)

    def refused(w, call, *a, **k):
        with pytest.raises(RxError):
            call(w, *a, **k)
        torch.cuda.synchronize()
        for name, t in list(w["outs"].items()) + [(k, w[k].t) for k in ("dy", "dres", "o")]:
            assert torch.isnan(t).all(), f"{call.__name__}: {name} was written by a refused call"

    w = world(32, 80)
    refused(w, fwd)                                   # more reduction channels than the gate kernel holds
    bad = ops.Act(poisoned((1, 2, 2, 4, 64), torch.bfloat16))
    refused(w, act_fwd, bad)                          # geometry mismatch between y and out
    assert torch.isnan(bad.t).all()
    w = world(32, 8)
    refused(w, bwd, out=None)                         # slope != 1 without the saved output: a gated block's mask needs it
    assert b"saved output" in ops.load().rx_last_error()
    refused(w, act_bwd, out=None)
    assert b"saved output" in ops.load().rx_last_error()
    refused(w, act_bwd, dy=bad)                       # a dy whose geometry differs from y
    need = ops.se_workspace_bytes(w["y"])
    short = torch.empty(need - 1, dtype=torch.uint8, device="cuda")
    refused(w, fwd, short)                            # a workspace one byte short
    refused(w, bwd, short)
    refused(world(32, 65), bwd)                       # rd = 65 on the backward
    w = world(2056, 8, x=2)                           # above RX_SE_MAX_C, on each of the five entry points
    with pytest.raises(RxError):
        ops.instnorm_stats(w["y"], w["outs"]["stats_o"])
    for call in (fwd, act_fwd, bwd, act_bwd):
        refused(w, call)
