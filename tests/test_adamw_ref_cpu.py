"""CPU: tests/adamw_ref.py means something -- (a) its fp64 reference is torch.optim.AdamW, (b) an honest fp32 evaluation of
`adamw_update` (rx_pack_optim.hip), with every rounding and with the a*b+c pairs fused, stays inside `adamw_bound` on the inputs of
the GPU tests, and (c) each planted fault leaves the bound in at least 10 % of the elements."""
import pytest
import torch

from adamw_ref import CLIP, HYPERS, STEPS, adam_args, adamw_bound, adamw_ref, exact_args, f32, make_inputs

N = 8192
CASES = [(h, s) for h in HYPERS for s in STEPS]


@pytest.mark.parametrize("wd", [0.0, 0.01])
def test_reference_is_torch_adamw_in_fp64(wd):
    """(a) five steps of adamw_ref fed the UNROUNDED arguments against torch.optim.AdamW on fp64 CPU tensors: 1e-12 relative"""
    torch.manual_seed(0)
    lr, b1, b2, eps = 1e-3, 0.9, 0.999, 1e-8
    p = torch.nn.Parameter(torch.randn(4096, dtype=torch.float64))
    opt = torch.optim.AdamW([p], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd)
    q, m, v = p.detach().clone(), torch.zeros(4096, dtype=torch.float64), torch.zeros(4096, dtype=torch.float64)
    for step in range(1, 6):
        g = torch.randn(4096, dtype=torch.float64) * torch.exp2(torch.randint(-12, 5, (4096,)).double())
        p.grad = g.clone()
        opt.step()
        q, m, v = adamw_ref(q, g, m, v, None, exact_args(lr, b1, b2, eps, wd, step))
        st = opt.state[p]
        for name, a, b in (("p", q, p.detach()), ("m", m, st["exp_avg"]), ("v", v, st["exp_avg_sq"])):
            assert ((a - b).abs() <= 1e-12 * b.abs()).all(), (step, name, ((a - b).abs() / b.abs().clamp(min=1e-300)).max().item())


def test_adam_args_round_like_the_host():
    """every field is an fp32 value; 1 - beta is rounded from the double difference, not formed from the rounded beta; the bias
    corrections reach exactly 1 at a large step"""
    a = adam_args(1e-3, 0.9, 0.999, 1e-8, 0.01, 3)
    for x in a:
        assert f32(x) == x
    assert a.omb1 == f32(1.0 - 0.9) and a.omb1 != 1.0 - a.beta1
    assert a.bc1 == f32(1.0 - 0.9 ** 3) and a.bc2_sqrt == f32((1.0 - 0.999 ** 3) ** 0.5)
    big = adam_args(1e-3, 0.9, 0.999, 1e-8, 0.01, 200000)
    assert big.bc1 == 1.0 and big.bc2_sqrt == 1.0


# ---- fp32 emulation of adamw_update, operation by operation ----------------------------------------------------------------------
def _t(x):
    return torch.tensor(x, dtype=torch.float32)


def _fma(a, b, c):
    """a * b + c rounded once: the product of two fp32 values is exact in fp64"""
    return (a.double() * b.double() + c.double()).float()


def emulate(p, g, m, v, clip, a, fused=False, fault=None):
    """`adamw_update` in fp32 (torch's CPU fp32 +, -, *, /, sqrt are correctly rounded); fused: every a*b+c pair as one FMA.
    fault: one of FAULTS, planted the way such a bug would be written"""
    lr, wd, b2, eps = _t(a.lr), _t(a.weight_decay), _t(a.beta2), _t(a.eps)
    omb1, omb2, bc1, bc2s = _t(a.omb1), _t(a.omb2), _t(a.bc1), _t(a.bc2_sqrt)
    if fault == "bc1":
        bc1 = _t(1.0)
    if fault == "bc2":
        bc2s = _t(1.0)
    if fault == "omb2":
        omb2 = omb1
    if clip is not None and fault != "noclip":
        g = g * _t(clip)
    if fault == "coupled_wd":                     # weight decay added to the gradient (Adam + L2) instead of decoupled
        g = g + wd * p
    else:
        p = _fma(-(lr * wd), p, p) if fused else p - lr * wd * p
    m = _fma(omb1, g - m, m) if fused else m + omb1 * (g - m)
    v = _fma(b2, v, omb2 * g * g) if fused else b2 * v + omb2 * g * g
    if fault == "eps_in_sqrt":
        denom = (v + eps).sqrt() / bc2s
    else:
        denom = v.sqrt() / bc2s + eps
    s, r = lr / bc1, m / denom
    p = _fma(-s, r, p) if fused else p - s * r
    if fault == "swap_mv":
        m, v = v, m
    return p, m, v


def _inputs(hyper, step):
    return make_inputs(N, 100 + STEPS.index(step) + 10 * HYPERS.index(hyper), step, hyper)


def _outside(got, p, g, m, v, clip, a):
    """share of the elements in which any of the three outputs leaves the bound; and the largest error / bound"""
    ref, bound = adamw_ref(p, g, m, v, clip, a), adamw_bound(p, g, m, v, clip, a)
    bad = torch.zeros(p.numel(), dtype=torch.bool)
    worst = 0.0
    for o, r, b in zip(got, ref, bound):
        err = (o.double() - r).abs()
        bad |= ~(err <= b)
        worst = max(worst, (err / b.clamp(min=1e-300)).max().item())
    return bad.double().mean().item(), worst


@pytest.mark.parametrize("clip", [None, CLIP])
@pytest.mark.parametrize("fused", [False, True])
def test_honest_fp32_stays_inside_the_bound(fused, clip):
    """(b) every hyper-parameter set at steps 1, 2, 1000 and 200000, zero-gradient / zero-parameter blocks included"""
    worst = 0.0
    for hyper, step in CASES:
        p, g, m, v = _inputs(hyper, step)
        a = adam_args(*hyper, step)
        share, w = _outside(emulate(p, g, m, v, clip, a, fused=fused), p, g, m, v, clip, a)
        assert share == 0.0, (hyper, step, share, w)
        worst = max(worst, w)
    print(f"honest fp32 (fused={fused}, clip={clip}): largest error / bound {worst:.3f}")
    assert worst > 0.05          # the bound is within a factor 20 of what fp32 arithmetic does: not a vacuous one


# fault -> the cases (hyper, step) in which it is a fault at all
FAULTS = {
    "bc1": lambda h, s: adam_args(*h, s).bc1 != 1.0,                    # the correction itself reaches 1 at step 200000
    "bc2": lambda h, s: adam_args(*h, s).bc2_sqrt != 1.0,
    "eps_in_sqrt": lambda h, s: True,
    "coupled_wd": lambda h, s: h[4] != 0.0,
    "omb2": lambda h, s: True,
    "noclip": lambda h, s: True,
    "step_off_by_one": lambda h, s: s in (1, 2),
    "swap_mv": lambda h, s: True,
}


@pytest.mark.parametrize("fault", list(FAULTS))
def test_planted_fault_leaves_the_bound(fault):
    """(c) in every case where the fault changes the arithmetic, at least 10 % of the elements leave the bound"""
    shares = {}
    for hyper, step in CASES:
        if not FAULTS[fault](hyper, step):
            continue
        p, g, m, v = _inputs(hyper, step)
        a = adam_args(*hyper, step)
        if fault == "step_off_by_one":
            got = emulate(p, g, m, v, CLIP, adam_args(*hyper, step + 1))
        else:
            got = emulate(p, g, m, v, CLIP, a, fault=fault)
        shares[(HYPERS.index(hyper), step)] = _outside(got, p, g, m, v, CLIP, a)[0]
    print(f"{fault}: smallest share outside the bound {min(shares.values()):.3f} at (hyper, step) {min(shares, key=shares.get)}")
    assert len(shares) >= 3
    assert min(shares.values()) >= 0.10, (fault, shares)
