"""CPU: tests/sgd_ref.py means something -- (a) its fp64 reference is torch.optim.SGD, (b) torch's own fp32 CPU step (every operation
rounded, `_single_tensor_sgd`) stays inside `sgd_bound` on the inputs of the GPU tests and comes within a factor 20 of it, and (c) a
planted fault leaves the bound in at least 10 % of the elements."""
import pytest
import torch

from sgd_ref import CLIP, HYPERS, exact_args, make_inputs, next_grad, sgd_args, sgd_bound, sgd_ref
from adamw_ref import f32

N = 8192
IDS = ["lr%g_mu%g_damp%g_wd%g_%s" % (h[0], h[1], h[2], h[3], "nesterov" if h[4] else "plain") for h in HYPERS]


def _torch_sgd(p, hyper, dtype):
    lr, mu, damp, wd, nesterov = hyper
    q = torch.nn.Parameter(p.to(dtype).clone())
    return q, torch.optim.SGD([q], lr=lr, momentum=mu, dampening=damp, weight_decay=wd, nesterov=nesterov, foreach=False)


@pytest.mark.parametrize("hyper", HYPERS, ids=IDS)
def test_reference_is_torch_sgd_in_fp64(hyper):
    """(a) five steps of torch.optim.SGD on fp64 CPU tensors; each step of sgd_ref, fed torch's own (p, buf) from before that step
    and the UNROUNDED arguments, equals torch's result to 1e-15 relative per element -- the first step (no buffer) and later ones"""
    p0, g0, _ = make_inputs(N, 3, True, hyper)
    q, opt = _torch_sgd(p0, hyper, torch.float64)
    for step in range(5):
        g = (g0 if step == 0 else next_grad(N, 3, step)).double()
        st = opt.state[q]
        before = (q.detach().clone(), st["momentum_buffer"].clone() if st.get("momentum_buffer") is not None else None)
        q.grad = g.clone()
        opt.step()
        first = before[1] is None
        assert first == (step == 0 or hyper[1] == 0)
        a = exact_args(*hyper, first)
        p2, b2 = sgd_ref(before[0], g, before[1], None, a)
        # each output is a sum of two terms, and two correctly rounded fp64 evaluations of it (torch's vectorised CPU kernels contract
        # a * b + c, plain tensor arithmetic does not) differ by roundings of the TERMS: 1e-15 relative is taken against the sum of
        # the terms' magnitudes (|d| <= |g| + wd |p|, |buf'| <= mu |buf| + omd that, ..., |p'| <= |p| + lr that), which is the output's own
        # magnitude wherever nothing cancels
        dmag = g.abs() + a.wd * before[0].abs()
        bmag = dmag if first or a.mu == 0 else a.mu * before[1].abs() + a.omd * dmag
        umag = dmag + a.mu * bmag if a.nesterov else bmag
        pairs = [("p", p2, q.detach(), before[0].abs() + a.lr * umag)]
        if hyper[1] != 0:
            pairs.append(("buf", b2, opt.state[q]["momentum_buffer"], bmag))
        else:
            assert b2 is None and "momentum_buffer" not in opt.state[q]
        for name, x, y, mag in pairs:
            assert ((x - y).abs() <= 1e-15 * mag).all(), (step, name, ((x - y).abs() / mag.clamp(min=1e-300)).max().item())


def test_sgd_args_round_like_the_host():
    """every field is an fp32 value; 1 - dampening is rounded from the double difference, not formed from the rounded dampening"""
    a = sgd_args(1e-2, 0.9, 0.1, 0.01, False, True)
    for x in a[:4]:
        assert f32(x) == x
    assert a.omd == f32(1.0 - 0.1) and a.omd != 1.0 - f32(0.1)
    assert a.first is True and a.nesterov is False


def _fp32_step(p, g, buf, clip, hyper, first, fault=None):
    """torch.optim.SGD's fp32 CPU step (`_single_tensor_sgd`: +, *, rounded one by one) from fp32 (p, g, buf); the clip coefficient
    multiplied into the gradient in fp32 first, as the kernel does.  fault: a planted bug, written the way it would be"""
    lr, mu, damp, wd, nesterov = hyper
    if fault == "no_dampening":
        damp = 0.0
    if fault == "no_nesterov":
        nesterov = False
    if fault == "no_wd":
        wd = 0.0
    if fault == "lr_sign":
        lr = -lr
    q, opt = _torch_sgd(p, (abs(lr), mu, damp, wd, nesterov), torch.float32)
    if lr < 0:
        opt.param_groups[0]["lr"] = lr
    if mu != 0 and not first and fault != "first_always":
        opt.state[q]["momentum_buffer"] = buf.clone()
    gg = g.clone()
    if clip is not None and fault != "noclip":
        gg = gg * torch.tensor(clip, dtype=torch.float32)
    q.grad = gg
    opt.step()
    return q.detach(), (opt.state[q]["momentum_buffer"] if mu != 0 else None)


def _outside(got, p, g, buf, clip, a):
    """share of the elements in which any output leaves the bound; and the largest error / bound.  (The reference gets the clip
    coefficient as the fp32 value the step multiplies by -- on the GPU it is read back from the device.)"""
    clip = None if clip is None else f32(clip)
    ref, bound = sgd_ref(p, g, buf, clip, a), sgd_bound(p, g, buf, clip, a)
    bad = torch.zeros(p.numel(), dtype=torch.bool)
    worst = 0.0
    for o, r, b in zip(got, ref, bound):
        if r is None:
            continue
        err = (o.double() - r).abs()
        bad |= ~(err <= b)
        worst = max(worst, (err / b.clamp(min=1e-300)).max().item())
    return bad.double().mean().item(), worst


@pytest.mark.parametrize("clip", [None, CLIP])
@pytest.mark.parametrize("first", [True, False])
def test_torch_fp32_step_stays_inside_the_bound(first, clip):
    """(b) every hyper-parameter row, first and later steps, zero-gradient / zero-parameter blocks included"""
    worst = 0.0
    for i, hyper in enumerate(HYPERS):
        p, g, buf = make_inputs(N, 100 + i, first, hyper)
        a = sgd_args(*hyper, first)
        share, w = _outside(_fp32_step(p, g, buf, clip, hyper, first), p, g, buf, clip, a)
        assert share == 0.0, (hyper, first, share, w)
        worst = max(worst, w)
    print(f"torch fp32 (first={first}, clip={clip}): largest error / bound {worst:.3f}")
    assert worst > 0.05          # the bound is within a factor 20 of what fp32 arithmetic does: not a vacuous one


# fault -> the cases (hyper, first) in which it is a fault at all
FAULTS = {
    "no_dampening": lambda h, first: h[1] != 0 and h[2] != 0 and not first,
    "no_nesterov": lambda h, first: h[4],
    "no_wd": lambda h, first: h[3] != 0,
    "lr_sign": lambda h, first: True,
    "noclip": lambda h, first: True,
    "first_always": lambda h, first: h[1] != 0 and not first,
}


@pytest.mark.parametrize("fault", list(FAULTS))
def test_planted_fault_leaves_the_bound(fault):
    """(c) in every case where the fault changes the arithmetic, at least 10 % of the elements leave the bound"""
    shares = {}
    for i, hyper in enumerate(HYPERS):
        for first in (True, False):
            if not FAULTS[fault](hyper, first):
                continue
            p, g, buf = make_inputs(N, 100 + i, first, hyper)
            got = _fp32_step(p, g, buf, CLIP, hyper, first, fault=fault)
            shares[(i, first)] = _outside(got, p, g, buf, CLIP, sgd_args(*hyper, first))[0]
    print(f"{fault}: smallest share outside the bound {min(shares.values()):.3f} at (hyper, first) {min(shares, key=shares.get)}")
    assert len(shares) >= 2
    assert min(shares.values()) >= 0.10, (fault, shares)
