"""fp64 SGD reference and per-element bounds for the SGD kernels of rx_pack_optim.hip (a plain module, imported by the test files,
like adamw_ref.py): `sgd_args` restates the host's roundings of the hyper-parameters, `sgd_ref` is the update in fp64 from the fp32
inputs and those rounded arguments, `sgd_bound` the fp32 error analysis of `sgd_update`, `make_inputs` the data the CPU and GPU
tests share.  `check_step` holds one device call to the bound, given the device's own previous (p, buf)."""
from collections import namedtuple

import torch

from adamw_ref import ETA, SECOND_ORDER, f32
from exact_ops import U32, assert_within

SgdArgs = namedtuple("SgdArgs", "lr mu omd wd nesterov first")

# (lr, momentum, dampening, weight_decay, nesterov): nesterov on / off, momentum 0 / 0.9, dampening 0 / 0.1, weight_decay 0 / 0.01
# -- all ten combinations torch accepts (nesterov needs momentum and no dampening)
HYPERS = [(1e-2, 0.9, 0.0, 0.01, True), (1e-2, 0.9, 0.0, 0.0, True), (1e-3, 0.9, 0.1, 0.01, False), (3e-2, 0.9, 0.0, 0.0, False),
          (1e-2, 0.9, 0.1, 0.0, False), (1e-2, 0.9, 0.0, 0.01, False), (1e-2, 0.0, 0.0, 0.01, False), (1e-3, 0.0, 0.0, 0.0, False),
          (1e-2, 0.0, 0.1, 0.0, False), (1e-2, 0.0, 0.1, 0.01, False)]
CLIP = 0.37


def sgd_args(lr, momentum, dampening, wd, nesterov, first):
    """`sgd_args()` of rx_pack_optim.hip: every hyper-parameter cast to fp32; 1 - dampening formed in double and cast once"""
    return SgdArgs(lr=f32(lr), mu=f32(momentum), omd=f32(1.0 - dampening), wd=f32(wd), nesterov=bool(nesterov), first=bool(first))


def exact_args(lr, momentum, dampening, wd, nesterov, first):
    """the same fields without any rounding to fp32 (what torch.optim.SGD computes with on fp64 tensors)"""
    return SgdArgs(lr=lr, mu=momentum, omd=1.0 - dampening, wd=wd, nesterov=bool(nesterov), first=bool(first))


def _d(t):
    return t.detach().double().cpu()


def _terms(p, g, buf, clip, a):
    p, g = _d(p), _d(g)
    gp = g * (1.0 if clip is None else float(clip))
    d = gp + a.wd * p if a.wd != 0 else gp
    if a.mu == 0:
        return p, gp, None, d, None, d, p - a.lr * d
    b = None if a.first else _d(buf)
    b2 = d.clone() if a.first else a.mu * b + a.omd * d
    u = d + a.mu * b2 if a.nesterov else b2
    return p, gp, b, d, b2, u, p - a.lr * u


def sgd_ref(p, g, buf, clip, args):
    """one SGD step (torch's `_single_tensor_sgd`, the order of operations of `sgd_update`) in fp64 from fp32 p, g, buf (ignored on a
    first step and without momentum), the clip coefficient (None: 1) and the rounded `args` -> (p', buf') as fp64 CPU tensors, buf'
    None without momentum"""
    t = _terms(p, g, buf, clip, args)
    return t[6], t[4]


def sgd_bound(p, g, buf, clip, args):
    """per-element absolute bounds (p', buf') on the fp32 evaluation of `sgd_update` against `sgd_ref`, first order in u = 2^-24 (every
    operation rounded to nearest) times SECOND_ORDER.  An FMA contraction only removes one of the roundings counted here.  With
    g' = g clip, the roundings counted are

      g'     the product g * clip:                                                       dg' = u |g'|            (0 without a clip)
      d      = g' + wd p (wd != 0): the product wd * p (u |wd p|), the sum (u |d|), dg' carried:
                                                                                         dd  = dg' + u wd |p| + u |d|
             = g' (wd == 0):                                                             dd  = dg'
      buf'   = mu buf + omd d (not first): the product mu * buf (u mu |buf|), the product omd * d (u omd |d|, and dd carried times
             omd), the sum (u |buf'|):                                                   db  = u mu |buf| + omd (dd + u |d|) + u |buf'|
             = d (first: a copy):                                                        db  = dd
      upd    = d + mu buf' (nesterov): dd carried, db carried times mu, the product (u mu |buf'|), the sum (u |upd|):
                                                                                         du  = dd + mu (db + u |buf'|) + u |upd|
             = buf' (momentum, no nesterov):                                             du  = db
             = d (mu == 0):                                                              du  = dd
      p'     = p - lr upd: du carried times lr, the product (u lr |upd|), the subtraction (u |p'|):
                                                                                         dp' = lr (du + u |upd|) + u |p'|

    and each of the at most six operations behind an output adds ETA where its result underflows (wd * p on a tiny parameter)."""
    a = args
    p, gp, b, d, b2, upd, p2 = _terms(p, g, buf, clip, a)
    u = U32
    dg = u * gp.abs() if clip is not None else torch.zeros_like(gp)
    dd = dg + u * a.wd * p.abs() + u * d.abs() if a.wd != 0 else dg
    if a.mu == 0:
        db, du = None, dd
    else:
        db = dd.clone() if a.first else u * a.mu * b.abs() + a.omd * (dd + u * d.abs()) + u * b2.abs()
        du = dd + a.mu * (db + u * b2.abs()) + u * upd.abs() if a.nesterov else db
    dp = a.lr * (du + u * upd.abs()) + u * p2.abs() + 6 * ETA
    return dp * SECOND_ORDER, None if db is None else (db + 6 * ETA) * SECOND_ORDER


def make_inputs(n, seed, first, hyper):
    """fp32 CPU (p, g, buf): p ~ N(0, 1); g ~ N(0, 1) 2^k with k uniform in [-12, 4] per element (drawn once: the warm-up gradients
    share the element's scale); buf from two warm-up reference steps rounded to fp32 -- zero when `first` or without momentum (the
    kernel must not read it then).  Three blocks of max(1, n // 16) elements at the end of the first half, where n allows: g = 0 with
    buf = 0, g = +-0.0 (alternating), p = 0."""
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
    buf = torch.zeros(n, dtype=torch.float32)
    if not first and hyper[1] != 0:
        q = p.clone()
        for t in (1, 2):
            q, buf = (x.float() for x in sgd_ref(q, gs[t].float(), buf, None, sgd_args(*hyper, t == 1)))
    g = gs[0].float()
    if n >= 3:
        g[zg] = 0.0
        buf[zg] = 0.0
        g[sg] = 0.0
        g[sg][1::2] = -0.0
    return p, g, buf


def next_grad(n, seed, k):
    """the gradient of the k-th following step of a multi-step test: N(0, 1) 2^j, j uniform in [-12, 4]"""
    gen = torch.Generator().manual_seed(seed * 1000 + 17 * k + 1)
    scale = torch.exp2(torch.randint(-12, 5, (n,), generator=gen).double())
    return (torch.randn(n, generator=gen, dtype=torch.float64) * scale).float()


RATIOS = {}                  # what -> largest error / bound seen per output (informational: printed by the tests)


def check_step(got, before, g, clip, args, what, names=("i",)):
    """got = the device's (p', buf') after one call (buf' None without momentum), before = its (p, buf) read back BEFORE that call
    (buf ignored on a first step): each output per element within sgd_bound of sgd_ref (no exemptions).  Returns the largest
    error / bound ratio per output."""
    ref = sgd_ref(before[0], g, before[1], clip, args)
    bound = sgd_bound(before[0], g, before[1], clip, args)
    ratios = []
    for name, o, r, b in zip(("p", "buf"), got, ref, bound):
        if r is None:
            assert o is None, f"{what}: a momentum buffer without momentum"
            ratios.append(0.0)
            continue
        o = _d(o).reshape(r.shape)
        err = (o - r).abs()
        ratios.append(torch.where(b > 0, err / b.clamp(min=1e-300), (err > 0).double() * float("inf")).max().item())
        assert_within(o, r, b, f"{what}: {name}'", names=names)
    key = what.split(":")[0]
    old = RATIOS.get(key, (0.0, 0.0))
    RATIOS[key] = tuple(max(x, y) for x, y in zip(old, ratios))
    return ratios
