"""fp64 AdamW reference and per-element bounds for the optimizer kernels of rx_pack_optim.hip (a plain module, imported by the test
files, like norm_bounds.py): `adam_args` restates the host's roundings of the hyper-parameters, `adamw_ref` is the update in fp64
from the fp32 inputs and those rounded arguments, `adamw_bound` the fp32 error analysis of `adamw_update`, `make_inputs` the data
the CPU and GPU tests share.  `check_step` holds one device call to the bound, given the device's own previous (p, m, v)."""
import math
from collections import namedtuple

import torch

from exact_ops import U32, assert_within

AdamArgs = namedtuple("AdamArgs", "lr beta1 beta2 eps weight_decay bc1 bc2_sqrt omb1 omb2")

# (lr, beta1, beta2, eps, weight_decay)
HYPERS = [(1e-3, 0.9, 0.999, 1e-8, 0.01), (1e-2, 0.9, 0.99, 1e-8, 0.0), (3e-4, 0.95, 0.999, 1e-6, 0.5)]
STEPS = (1, 2, 1000, 200000)
CLIP = 0.37
ETA = 2.0 ** -149            # smallest fp32 subnormal: the absolute error of an operation whose result underflows
SECOND_ORDER = 1 + 64 * U32  # products of two roundings, dropped from the first-order terms below (fewer than 64 pairs)


def f32(x):
    """the double x rounded to fp32 (round to nearest even, like a C cast), returned as a double"""
    return torch.tensor(float(x), dtype=torch.float64).to(torch.float32).item()


def adam_args(lr, b1, b2, eps, wd, step):
    """`adam_args()` of rx_pack_optim.hip: every hyper-parameter cast to fp32; 1 - beta and the bias corrections formed in double
    and cast once"""
    return AdamArgs(lr=f32(lr), beta1=f32(b1), beta2=f32(b2), eps=f32(eps), weight_decay=f32(wd),
                    bc1=f32(1.0 - math.pow(b1, float(step))), bc2_sqrt=f32(math.sqrt(1.0 - math.pow(b2, float(step)))),
                    omb1=f32(1.0 - b1), omb2=f32(1.0 - b2))


def exact_args(lr, b1, b2, eps, wd, step):
    """the same fields without any rounding to fp32 (what torch.optim.AdamW computes with on fp64 tensors)"""
    return AdamArgs(lr=lr, beta1=b1, beta2=b2, eps=eps, weight_decay=wd, bc1=1.0 - b1 ** step, bc2_sqrt=math.sqrt(1.0 - b2 ** step),
                    omb1=1.0 - b1, omb2=1.0 - b2)


def _d(t):
    return t.detach().double().cpu()


def _terms(p, g, m, v, clip, a):
    p, g, m, v = _d(p), _d(g), _d(m), _d(v)
    gp = g * (1.0 if clip is None else float(clip))
    p1 = p - a.lr * a.weight_decay * p
    m2 = m + a.omb1 * (gp - m)
    v2 = a.beta2 * v + a.omb2 * gp * gp
    denom = v2.sqrt() / a.bc2_sqrt + a.eps
    r = m2 / denom
    s = a.lr / a.bc1
    return p, gp, m, v, p1, m2, v2, denom, r, s, p1 - s * r


def adamw_ref(p, g, m, v, clip, args):
    """one AdamW step (decoupled weight decay, bias correction; the order of operations of `adamw_update`) in fp64 from fp32
    p, g, m, v, the clip coefficient (None: 1) and the rounded `args` -> (p', m', v') as fp64 CPU tensors"""
    t = _terms(p, g, m, v, clip, args)
    return t[10], t[5], t[6]


def adamw_bound(p, g, m, v, clip, args):
    """per-element absolute bounds (p', m', v') on the fp32 evaluation of `adamw_update` against `adamw_ref`, first order in
    u = 2^-24 (every operation rounded to nearest) times SECOND_ORDER.  An FMA contraction only removes one of the roundings
    counted here.  With g' = g clip, s = lr / bc1, the roundings counted are

      g'      the product g * clip:                                                  dg' = u |g'|        (0 without a clip)
      p1      = p - (lr wd) p: lr * wd (u), its product with p (u), the subtraction:  dp1 = 2u lr wd |p| + u |p1|
      m'      = m + omb1 (g' - m): the subtraction (u |g' - m| <= u (|g'| + |m|), and dg' carried), the product (u), the sum:
                                                                                     dm' = omb1 (dg' + 2u (|g'| + |m|)) + u |m'|
      v'      = beta2 v + (omb2 g') g', all terms non-negative: beta2 * v (u of that term); omb2 * g' and * g' (2u) with g'
              rounded in both factors (2u) -> 4u of that term; the sum (u):         dv' = 5u v'
      denom   = sqrt(v') / bc2_sqrt + eps, both terms non-negative: dv' moves the root by 2.5u; sqrtf 2u, the division 2u; the
              sum u.  (The build has no fast-math flag, so hipcc's default of correctly rounded fp32 sqrt and division holds and
              each is u; the bound counts 2u each and does not depend on that.)        ddenom = 7.5u denom
      r       = m' / denom: dm' carried, ddenom carried (7.5u |r|), the division 2u:  dr = dm' / denom + 9.5u |r|
      p'      = p1 - s r: the division lr / bc1 (2u), the product (u), the subtraction (u |p'|):
                                                                                     dp' = dp1 + s (dr + 3u |r|) + u |p'|

    and each of the at most four operations behind an output adds ETA where its result underflows (g'^2 on a tiny gradient)."""
    a = args
    p, gp, m, v, p1, m2, v2, denom, r, s, p2 = _terms(p, g, m, v, clip, a)
    u = U32
    dg = u * gp.abs() if clip is not None else torch.zeros_like(gp)
    dp1 = 2 * u * a.lr * a.weight_decay * p.abs() + u * p1.abs()
    dm = a.omb1 * (dg + 2 * u * (gp.abs() + m.abs())) + u * m2.abs() + 4 * ETA
    dv = 5 * u * v2 + 4 * ETA
    dr = dm / denom + 9.5 * u * r.abs()
    dp = dp1 + s * (dr + 3 * u * r.abs()) + u * p2.abs() + 4 * ETA
    return dp * SECOND_ORDER, dm * SECOND_ORDER, dv * SECOND_ORDER


def make_inputs(n, seed, step, hyper):
    """fp32 CPU (p, g, m, v) for a call at `step`: p ~ N(0, 1); g ~ N(0, 1) 2^k with k uniform in [-12, 4] per element (drawn once:
    the warm-up gradients share the element's scale); m, v from two warm-up reference steps rounded to fp32, zero at step 1.  Three
    blocks of max(1, n // 16) elements at the end of the first half, where n allows: g = 0 with v = 0 (denom = eps), g = +-0.0
    (alternating), p = 0."""
    gen = torch.Generator().manual_seed(seed)
    p = torch.randn(n, generator=gen, dtype=torch.float64)
    scale = torch.exp2(torch.randint(-12, 5, (n,), generator=gen).double())
    gs = [torch.randn(n, generator=gen, dtype=torch.float64) * scale for _ in range(3)]
    blk = max(1, n // 16)
    b0 = max(0, n // 2 - 3 * blk)
    zg, sg, zp = (slice(b0 + i * blk, min(n, b0 + (i + 1) * blk)) for i in range(3))
    if n >= 3:
        p[zp] = 0.0
    p = p.float()
    m = torch.zeros(n, dtype=torch.float32)
    v = torch.zeros(n, dtype=torch.float32)
    if step > 1:
        q = p.clone()
        for t in (1, 2):
            q, m, v = (x.float() for x in adamw_ref(q, gs[t].float(), m, v, None, adam_args(*hyper, t)))
    g = gs[0].float()
    if n >= 3:
        g[zg] = 0.0
        v[zg] = 0.0
        g[sg] = 0.0
        g[sg][1::2] = -0.0
    return p, g, m, v


def next_grad(n, seed, k):
    """the gradient of the k-th following step of a multi-step test: N(0, 1) 2^j, j uniform in [-12, 4]"""
    gen = torch.Generator().manual_seed(seed * 1000 + 17 * k + 1)
    scale = torch.exp2(torch.randint(-12, 5, (n,), generator=gen).double())
    return (torch.randn(n, generator=gen, dtype=torch.float64) * scale).float()


RATIOS = {}                  # what -> largest error / bound seen per output (informational: printed by the tests)


def check_step(got, before, g, clip, args, what, names=("i",)):
    """got = the device's (p', m', v') after one call, before = its (p, m, v) read back BEFORE that call: each output per element
    within adamw_bound of adamw_ref (no exemptions).  Returns the largest error / bound ratio per output."""
    ref = adamw_ref(before[0], g, before[1], before[2], clip, args)
    bound = adamw_bound(before[0], g, before[1], before[2], clip, args)
    ratios = []
    for name, o, r, b in zip(("p", "m", "v"), got, ref, bound):
        o = _d(o).reshape(r.shape)
        err = (o - r).abs()
        ratios.append(torch.where(b > 0, err / b.clamp(min=1e-300), (err > 0).double() * float("inf")).max().item())
        assert_within(o, r, b, f"{what}: {name}'", names=names)
    key = what.split(":")[0]
    old = RATIOS.get(key, (0.0, 0.0, 0.0))
    RATIOS[key] = tuple(max(x, y) for x, y in zip(old, ratios))
    return ratios
