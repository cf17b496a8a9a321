"""The fp64 reference of the eight losses of `LOSS_FN_MAP` (plain torch on the CPU, no project kernel), the per-element error
bounds the kernels of csrc/rx_loss.hip are held to, and the case table shared by tests/test_loss_ops_gpu.py (the kernels) and
tests/test_loss_ref_cpu.py (fp32 CPU torch on the same table: the evidence that the bounds are neither vacuous nor too tight).

`host(name, x, t, kw, dtype)` is the host formulation of training/losses/losses.py -- the `torch.nn` class, or the explicit expression
for the label-smoothing, Z-smooth, Dice and cosine losses -- evaluated in `dtype`.  `reference()` runs it in fp64 on inputs that are
exact fp32 values (smoothing constants and the Z-smooth table included: both are fp32 in the kernels and in the fp32 host path) and
takes d loss / d pred by fp64 autograd times the upstream scalar.

Bound per element:  |got - ref| <= rel_i * M_i + FLOOR.
  M_i   the sum of the absolute values of the terms the formula adds to form element i (fp64), so cancellation costs nothing;
  rel_i SAFETY * n_i * 2^-24, n_i the number of fp32 roundings on the kernel's path to the element, derived per family below;
  FLOOR 2^-125 * max(1, |g k|): an intermediate or a result under the smallest normal fp32 number may flush to zero.
SAFETY = 4.  n_i * 2^-24 is the worst case of ONE fp32 evaluation of the formula.  Another fp32 evaluation with an operation sequence
of about the same length (CPU torch's) has the same worst case, so the issue's demand that fp32 CPU torch stay within a quarter of
the bound can only hold for a bound of at least 4 n_i 2^-24; that is the bound.  A correct kernel sits within a quarter of it too
(test_loss_ref_cpu.py asserts the quarter for CPU torch; DESIGN section 15 records the largest ratio measured on the device)."""
import math

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

U = 2.0 ** -24
SAFETY = 4.0
FLOOR = 2.0 ** -125
G_UP = -2.5                     # the upstream gradient of every case unless stated
EXP_SAT = 104.0                 # beyond |x| = 104 exp(-|x|) is 0 in fp32 whatever the argument's rounding


def f32(v):
    """the fp32 value of a python scalar, as a python float (what a c_float argument / an fp32 torch scalar holds)"""
    return float(np.float32(v))


# ---- fast-exp error -----------------------------------------------------------------------------------------------------------------
# __expf(x) = v_exp_f32(x * log2(e)).  The product is rounded once and log2(e) itself is an fp32 constant: the argument y = x log2(e)
# carries an absolute error of 2 |y| 2^-24, i.e. a relative error of 2 ln2 |y| 2^-24 < 2 |x| 2^-24 = |x| 2^-23 in 2^y (the
# argument-scaling term).  v_exp_f32 is accurate to 1 ulp = 2 * 2^-24 (the CDNA ISA manuals' figure; the guides give no other).
def exp_err_units(absx):
    """relative error of __expf(x) in units of 2^-24"""
    return 2.0 + 2.0 * absx.clamp(max=EXP_SAT)


def zsmooth_table(d, center, edge):
    """the reference's fp32 expression for the per-slice smoothing (losses.py:277-288): what the kernel's table holds"""
    z = torch.arange(d, dtype=torch.float32)
    return center + (edge - center) * ((z - (d - 1) / 2.0).abs() / (d // 2))


ELEMENTWISE = ("BCEWithLogitsLoss", "BCEWithLogitsLossLabelSmoothing", "BCEWithLogitsLossZSmooth", "BCELoss", "MSELoss")
LOGIT_NAMES = ("BCEWithLogitsLoss", "BCEWithLogitsLossLabelSmoothing", "BCEWithLogitsLossZSmooth")


def _alpha(name, kw, shape, dtype):
    """per-element smoothing of the three BCE-with-logits names, broadcastable to `shape`, exact fp32 values in `dtype`"""
    if name == "BCEWithLogitsLossZSmooth":
        d = shape[2]
        return zsmooth_table(d, kw.get("center_smoothing", 0.1), kw.get("edge_smoothing", 0.4)).to(dtype).view(1, 1, d, 1, 1)
    s = f32(kw.get("smoothing", 0.1)) if name == "BCEWithLogitsLossLabelSmoothing" else 0.0
    return torch.tensor(s, dtype=dtype)


def dice_sums(x, t):
    """per channel (I, D) = (sum p t, sum p^2 + sum t^2) over (N, spatial), p = sigmoid(x)"""
    c = x.shape[1]
    p = torch.sigmoid(x).transpose(0, 1).reshape(c, -1)
    tt = t.transpose(0, 1).reshape(c, -1)
    return (p * tt).sum(-1), (p * p).sum(-1) + (tt * tt).sum(-1)


def host(name, x, t, kw, dtype=torch.float64):
    """the host formulation of training/losses/losses.py in `dtype`.  x may require grad."""
    red = kw.get("reduction", "mean")
    if name in LOGIT_NAMES:
        if name == "BCEWithLogitsLoss":
            return nn.BCEWithLogitsLoss(reduction=red)(x, t)
        a = _alpha(name, kw, x.shape, dtype)
        return F.binary_cross_entropy_with_logits(x, t * (1.0 - 2.0 * a) + a, reduction=red)
    if name == "BCELoss":
        return nn.BCELoss(reduction=red)(x, t)
    if name == "MSELoss":
        return nn.MSELoss(reduction=red)(x, t)
    if name == "BCEDiceLoss":
        s = f32(kw.get("smoothing", 0.1))
        bce = F.binary_cross_entropy_with_logits(x, t * (1.0 - 2.0 * s) + s)
        inter, den = dice_sums(x, t)
        dice = 1.0 - (2 * (inter / den.clamp(min=1e-6))).mean()
        return kw["alpha"] * bce + kw["beta"] * dice
    if name == "MaskedCosineLoss":
        mask = (torch.norm(t, dim=1) > 1e-6).to(dtype)
        unit = x / torch.norm(x, dim=1, keepdim=True).clamp(min=1e-8)
        cos = F.cosine_similarity(unit, t, dim=1, eps=1e-8)
        return 1.0 - (cos * mask).sum() / (mask.sum() + 1e-8)
    if name == "CrossEntropyLoss":
        return nn.CrossEntropyLoss(reduction=red, ignore_index=kw.get("ignore_index", -100))(x, t)
    raise KeyError(name)


def ce_sanitize(t, c, ignore):
    """index targets as torch accepts them: an index outside [0, C) is skipped by the kernel like an ignored one; torch refuses it"""
    if t.dtype != torch.int64:
        return t
    return torch.where((t < 0) | (t >= c), torch.full_like(t, ignore), t)


def run_host(name, x, t, kw, dtype, g=G_UP):
    """(loss, g * d loss / d x) of the host formulation in `dtype`"""
    xx = x.to(dtype).requires_grad_(True)
    tt = ce_sanitize(t, x.shape[1], kw.get("ignore_index", -100)) if name == "CrossEntropyLoss" else t
    tt = tt if tt.dtype == torch.int64 else tt.to(dtype)
    loss = host(name, xx, tt, kw, dtype)
    (grad,) = torch.autograd.grad(loss, xx)
    return loss.detach(), grad * g


# ---- rounding counts n_i (units of 2^-24) per family ------------------------------------------------------------------------------
# BCE-with-logits gradient  g k (p - ts),  ts = t (1 - 2a) + a,  p = 1 / (1 + __expf(-x)):
#   ts: 2a exact, 1 - 2a, t *, + a                      3 roundings on |ts|   (counted 4: a itself is the fp32 value of the constant)
#   p : __expf (exp_err_units, enters p as (1 - p) <= 1 times it), 1 + e, 1 / .        2 + exp_err on p
#   p - ts, k = (float)(1 / E), g * k, (g k) * (.)       4 on the whole
#   n_i = 4 + 4 + exp_err(|x_i|) = 10 + 2 min(|x_i|, 104)
def n_bce_logits(x):
    return 8.0 + exp_err_units(x.abs())


# BCELoss gradient  g k (x - t) / max(x (1 - x), 1e-12):  x - t, 1 - x, x * (.), the division, k, g k, the product = 7, and 1 for
# the fp32 value of the 1e-12 constant:  n = 8
N_BCE_PROB = 8.0
# MSE gradient  g k 2 (x - t):  x - t, k, g k, the product (the factor 2 is exact) = 4, counted 5
N_MSE = 5.0
# Dice part of BCE+Dice  g k_dice (a t - b p) p (1 - p):
#   coefficients: I, D are sums of non-negative fp32 terms: 32 serial adds per thread, 6 shuffle levels, 4 waves = 42 roundings, the terms'
#     own (p t: 1 + p's 2; p^2: 1 + 2 * 2; exp_err weighted by p (1 - p) |x| < 0.3: 2 more) 8:  50 on a sum, relative to the sum.
#     a = 2 / D (fp64, cast: 1): 51.   b = 4 I / D^2: 50 + 2 * 50 + 1 = 151.
#   a t, b p, the difference, * p, 1 - p, * (.), k_dice = beta / C, * k_dice, g *, the outer difference: 10;  p enters three times:
#     3 (2 + exp_err)
#   n_i = 151 + 10 + 3 (2 + exp_err(|x_i|)) = 173 + 6 min(|x_i|, 104); the BCE part keeps n_bce_logits.
N_DICE_A, N_DICE_B = 51.0, 151.0


def n_dice(x):
    return N_DICE_B + 10.0 + 3.0 * (2.0 + exp_err_units(x.abs()))


# Masked cosine gradient  k (t_c / |t| - cos p_c / |pred|) * scale,  scale = 1 / (uc pc)  (= 1 / |pred| from |pred| = 1e-16 up):
#   pp, tt, pt: C products and C - 1 sums each: C + 1 (pt: relative to sum |p_j t_j|, which is why M expands the cosine)
#   |pred|, |t|: (C + 1) / 2 + 1 (sqrt);  1 / |t|: + 1;  1 / |pred|: + 1;  scale: + 1, and below 1e-8: pn / pc, * pc: + 2
#   t_c / |t|: (C + 1) / 2 + 3.   cos p_c / |pred|: pt (C + 1), scale ((C + 1) / 2 + 4), 1 / |t| ((C + 1) / 2 + 2), two products, * p_c,
#   * 1 / |pred| ((C + 1) / 2 + 2 + 1): 2.5 (C + 1) + 12.   The difference, k (cast of coef, - g coef: 2), * k, * scale ((C + 1) / 2 + 4 + 1): 9 + (C + 1) / 2
#   n = 3 (C + 1) + 21
def n_cosine(c):
    return 3.0 * (c + 1) + 21.0


# Cross entropy  g k (exp(x_c - lse) s - t_c):
#   online sum of exponentials over C classes: per class one __expf of |d| <= R (R = max - min of the voxel's logits), one product or
#   sum, at worst a rescale of the whole sum every class: (C - 1) (2 + exp_err(R)) relative on the sum = absolute on its log;
#   logf (1, relative to |log sum| <= log C), m + log (1, relative to |lse|):
#   lse_err = (C - 1) (2 + exp_err(R)) + log C + |lse| + 1                      (absolute, units of 2^-24: the bound on `saved`)
#   x_c - lse: 1 relative to the difference, then __expf: (1 + exp_err(|x_c - lse|)) ... as a relative error of the softmax term
#   s = sum of C targets (C), * s, - t, k (cast), g k, the product: C + 5
#   n_i = lse_err + 1 + |x_c - lse|' + exp_err(|x_c - lse|) + C + 5
def ce_lse_err_units(x64, lse):
    c = x64.shape[1]
    r = (x64.amax(1) - x64.amin(1)).clamp(max=EXP_SAT)
    return (c - 1) * (2.0 + 2.0 + 2.0 * r) + math.log(c) + lse.abs() + 1.0


def n_ce(x64, lse):
    d = (x64 - lse.unsqueeze(1)).abs()
    return ce_lse_err_units(x64, lse).unsqueeze(1) + 1.0 + d.clamp(max=EXP_SAT) + exp_err_units(d) + x64.shape[1] + 5.0


# ---- the reference -----------------------------------------------------------------------------------------------------------------
def reference(name, x, t, kw, g=G_UP):
    """x, t: fp32 CPU tensors (t int64 for class indices).  -> dict: loss (0-dim fp64), grad (fp64), M, rel (broadcastable to grad),
    floor, and per family: lse / tsum (cross entropy), a / b (BCE+Dice coefficients), with their bounds."""
    assert x.dtype == torch.float32 and (t.dtype in (torch.float32, torch.int64))
    loss, grad = run_host(name, x, t, kw, torch.float64, g)
    x64 = x.double()
    t64 = t if t.dtype == torch.int64 else t.double()
    e = x.numel()
    k = 1.0 / e if kw.get("reduction", "mean") == "mean" else 1.0
    out = {"loss": loss, "grad": grad}
    if name in LOGIT_NAMES:
        a = _alpha(name, kw, x.shape, torch.float64)
        ts = t64 * (1.0 - 2.0 * a) + a
        out["M"] = abs(g) * k * (torch.sigmoid(x64) + ts.abs())
        out["rel"] = SAFETY * U * n_bce_logits(x64)
    elif name == "BCELoss":
        out["M"] = abs(g) * k * (x64.abs() + t64.abs()) / (x64 * (1.0 - x64)).clamp(min=1e-12)
        out["rel"] = SAFETY * U * N_BCE_PROB
    elif name == "MSELoss":
        out["M"] = abs(g) * k * 2.0 * (x64.abs() + t64.abs())
        out["rel"] = SAFETY * U * N_MSE
    elif name == "BCEDiceLoss":
        s, c = f32(kw.get("smoothing", 0.1)), x.shape[1]
        p = torch.sigmoid(x64)
        inter, den = dice_sums(x64, t64)
        dcl = den.clamp(min=1e-6)
        a_c = 2.0 / dcl
        b_c = torch.where(den > 1e-6, 4.0 * inter / (dcl * dcl), torch.zeros_like(den))
        view = (1, c) + (1,) * (x.dim() - 2)
        m_bce = abs(g) * abs(kw["alpha"]) / e * (p + (t64 * (1.0 - 2.0 * s) + s).abs())
        m_dice = abs(g) * abs(kw["beta"]) / c * ((a_c.view(view) * t64).abs() + (b_c.view(view) * p).abs()) * p * (1.0 - p)
        out["M"] = m_bce + m_dice
        out["rel"] = SAFETY * U * (n_bce_logits(x64) * m_bce + n_dice(x64) * m_dice) / out["M"].clamp(min=1e-300)
        out["a"], out["b"] = a_c, b_c
        out["rel_a"], out["rel_b"] = SAFETY * U * N_DICE_A, SAFETY * U * N_DICE_B
        k = max(abs(kw["alpha"]) / e, abs(kw["beta"]) / c * float(a_c.max()))
    elif name == "MaskedCosineLoss":
        c = x.shape[1]
        pn, tn = x64.norm(dim=1, keepdim=True), t64.norm(dim=1, keepdim=True)
        on = tn > 1e-6
        kk = 1.0 / (float(on.sum()) + 1e-8)
        pc = pn.clamp(min=1e-8)
        scale = torch.where(pn >= 1e-8, 1.0 / pn.clamp(min=1e-300), 1.0 / ((pn / pc).clamp(min=1e-8) * pc))
        ph = torch.where(pn > 0, x64 / pn.clamp(min=1e-300), torch.zeros_like(x64))
        th = t64 / tn.clamp(min=1e-300)
        cos_abs = (ph.abs() * th.abs()).sum(1, keepdim=True) * (scale * pn).clamp(max=1.0)       # sum_j |p_j t_j| / (uc pc |t|)
        out["M"] = torch.where(on, abs(g) * kk * (th.abs() + cos_abs * ph.abs()) * scale, torch.zeros_like(x64))
        out["rel"] = SAFETY * U * n_cosine(c)
        k = kk * 1e16
    elif name == "CrossEntropyLoss":
        c, ignore = x.shape[1], kw.get("ignore_index", -100)
        lse = torch.logsumexp(x64, dim=1)
        sm = torch.softmax(x64, dim=1)
        if t.dtype == torch.int64:
            ts_ = ce_sanitize(t, c, ignore)
            valid = ts_ != ignore
            onehot = F.one_hot(torch.where(valid, ts_, torch.zeros_like(ts_)), c).movedim(-1, 1).double() * valid.unsqueeze(1)
            tsum = valid.double()
            count = float(valid.sum())
            k = (1.0 / count if count else 0.0) if kw.get("reduction", "mean") == "mean" else 1.0
        else:
            onehot, tsum = t64, t64.sum(1)
            k = 1.0 / (x.shape[0] * lse[0].numel()) if kw.get("reduction", "mean") == "mean" else 1.0
        out["M"] = abs(g) * k * (sm * tsum.unsqueeze(1).abs() + onehot.abs())
        out["rel"] = SAFETY * U * n_ce(x64, lse)
        out["lse"], out["tsum"] = lse, tsum
        out["lse_bound"] = SAFETY * U * ce_lse_err_units(x64, lse)
        out["tsum_bound"] = SAFETY * U * c * (onehot.abs().sum(1)) if t.dtype != torch.int64 else None
    else:
        raise KeyError(name)
    out["floor"] = FLOOR * max(1.0, abs(g) * k)
    return out


def worst_ratio(got, ref, M, rel, floor=FLOOR):
    """largest |got - ref| / (rel M + floor) and its flat index; a NaN in `got` counts as infinite"""
    g, r = got.detach().double().cpu(), ref.detach().double().cpu()
    bound = torch.as_tensor(rel, dtype=torch.float64) * M + floor
    ratio = ((g - r).abs() / bound.expand_as(r))
    ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, float("inf")), ratio)
    i = int(ratio.flatten().argmax())
    return float(ratio.flatten()[i]), i


RATIOS = {}          # family -> largest ratio seen by assert_elementwise in this process


def assert_elementwise(got, ref, M, rel, what, floor=FLOOR, family=None, limit=1.0):
    """|got - ref| <= limit * (rel * M + floor) for every element.  On failure: the worst element's index, the values and the ratio
    |got - ref| / (rel M + floor)."""
    assert tuple(got.shape) == tuple(ref.shape), (what, tuple(got.shape), tuple(ref.shape))
    ratio, i = worst_ratio(got, ref, M, rel, floor)
    if family is not None:
        RATIOS[family] = max(RATIOS.get(family, 0.0), ratio)
    if not ratio <= limit:
        idx = np.unravel_index(i, tuple(ref.shape)) if ref.dim() else ()
        gi, ri = got.detach().double().cpu().flatten()[i].item(), ref.detach().double().cpu().flatten()[i].item()
        mi = torch.as_tensor(M, dtype=torch.float64).expand_as(ref).flatten()[i].item()
        li = torch.as_tensor(rel, dtype=torch.float64).expand_as(ref).flatten()[i].item()
        n_bad = int((((got.detach().double().cpu() - ref.detach().double().cpu()).abs()
                      <= limit * (torch.as_tensor(rel, dtype=torch.float64) * M + floor)) == 0).sum())
        raise AssertionError(f"{what}: {n_bad} of {ref.numel()} elements outside the bound; worst at {tuple(int(j) for j in idx)}: got {gi!r} "
                             f"want {ri!r}, M {mi:.6g}, rel {li:.3g}, |got-ref| / (rel M) = {ratio:.4g} (limit {limit})")


def sum_margin(loss32, loss64):
    """bound of a sum-reduced loss, relative to the fp64 value: 4x the relative error of torch's own fp32 CPU result, never below
    2e-6 (the rule of scripts/make_losses_fixture.py)"""
    return max(4.0 * abs(loss32 - loss64) / abs(loss64), 2e-6) if loss64 != 0 else 2e-6


MEAN_ABS = 2e-6


def loss_ok(got, ref64, kw, loss32=None):
    """(ok, text): mean-reduced 2e-6 absolute against the fp64 value; sum-reduced the sum_margin rule.  NaN matches NaN only."""
    if math.isnan(ref64) or math.isnan(got):
        return math.isnan(ref64) and math.isnan(got), f"loss {got!r} reference {ref64!r}"
    if kw.get("reduction", "mean") == "sum":
        margin = sum_margin(loss32, ref64)
        err = abs(got - ref64) / abs(ref64) if ref64 != 0 else abs(got)
        return err <= margin, f"sum loss {got!r} fp64 {ref64!r} rel err {err:.3e} margin {margin:.3e}"
    return abs(got - ref64) <= MEAN_ABS, f"loss {got!r} fp64 {ref64!r} |diff| {abs(got - ref64):.3e} bound {MEAN_ABS}"


# ---- the case table ------------------------------------------------------------------------------------------------------------------
# A case: dict(id, name, kw, make) -- make() -> (x, t) fp32 CPU tensors from seeded generators.  Shapes: the smallest that reach each
# path (chunk of the element-wise / BCE+Dice kernels: 8192 elements of a plane; of cross entropy: 2048 voxels; 16-byte path: V % 4 == 0).
LOGIT_GRID = [0.0, 1e-8, -1e-8, 1.0, -1.0, 20.0, -20.0, 87.0, -87.0, 89.0, -89.0, 104.0, -104.0, 1e4, -1e4]
TARGET_GRID = [0.0, 1.0, 0.25]
PROB_GRID = [0.0, 2.0 ** -149, 1e-12, 0.5, 1.0 - 2.0 ** -24, 1.0]
PROB_TARGET_GRID = [0.0, 1.0, 0.3]
ELEM_V = [1, 3, 4, 8191, 8192, 8193, 8196]
ZS_SHAPE_OF_V = {3: (3, 1, 1), 4: (2, 1, 2), 8191: (8191, 1, 1), 8192: (2, 64, 64), 8193: (3, 1, 2731), 8196: (4, 3, 683)}
ZS_EDGE_SHAPES = [(2, 1, 2), (3, 1, 4), (4, 1, 3), (5, 2, 2), (4, 3, 1), (3, 2, 683 * 2)]
ZS_KW = [{"center_smoothing": 0.1, "edge_smoothing": 0.4}, {"center_smoothing": 0.0, "edge_smoothing": 0.5}]


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def rand_pair(name, shape, seed):
    g = _gen(seed)
    x = torch.randn(shape, generator=g) * 2.0
    t = (torch.rand(shape, generator=g) > 0.7).float()
    return (torch.sigmoid(x) if name == "BCELoss" else x), t


def grid_pair(name, shape, seed):
    """random fill with the value grid (every logit x every target) written at scattered places of every plane's first half.  The
    fill keeps a mean-reduced loss small enough for the 2e-6 absolute bound to be representable in fp32 at all."""
    x, t = rand_pair(name, shape, seed)
    xs, tsv = (PROB_GRID, PROB_TARGET_GRID) if name == "BCELoss" else (LOGIT_GRID, TARGET_GRID)
    combos = [(a, b) for a in xs for b in tsv]
    xf, tf = x.view(-1), t.view(-1)
    pos = 5 + 89 * torch.arange(len(combos))
    assert int(pos[-1]) < xf.numel()
    xf[pos] = torch.tensor([c[0] for c in combos], dtype=torch.float32)
    tf[pos] = torch.tensor([c[1] for c in combos], dtype=torch.float32)
    return x, t


def _shape5(name, v):
    return (1, 1) + (ZS_SHAPE_OF_V[v] if name == "BCEWithLogitsLossZSmooth" else (1, 1, v))


def elem_cases():
    """per (name, reduction): the sizes around the chunk edge on both paths, odd planes, 600 blocks, the value grid, the Z-smooth
    boundary shapes.  BCEWithLogitsLossZSmooth has no V = 1 case: Z = 1 divides by zero in the reference's expression."""
    out = []
    seed = 1000
    for name in ELEMENTWISE:
        zs = name == "BCEWithLogitsLossZSmooth"
        for red in ("mean", "sum"):
            def add(tag, shape, kw=None, fn=rand_pair):
                nonlocal seed
                seed += 1
                kw = dict(kw or {}, reduction=red)
                out.append({"id": f"{name}-{red}-{tag}", "name": name, "kw": kw, "group": (name, red),
                            "make": (lambda fn=fn, shape=shape, s=seed, name=name: fn(name, shape, s))})
            for v in ELEM_V:
                if not (zs and v == 1):
                    add(f"V{v}", _shape5(name, v))
            add("odd_planes", (1, 3, 5, 7, 9))
            add("600_blocks", (200, 3, 5, 1, 1))
            if name == "BCEWithLogitsLossLabelSmoothing":
                for s in (0.0, 0.1, 0.5):
                    add(f"grid_s{s}", (1, 4, 2, 64, 64), {"smoothing": s}, grid_pair)
                    add(f"grid_scalar_s{s}", (1, 4, 1, 1, 8193), {"smoothing": s}, grid_pair)
            elif zs:
                for i, kw in enumerate(ZS_KW):
                    add(f"grid_kw{i}", (1, 4, 2, 64, 64), kw, grid_pair)
                    for shp in ZS_EDGE_SHAPES:
                        add(f"zyx{'x'.join(map(str, shp))}_kw{i}", (2, 2) + shp, kw)
            elif name != "MSELoss":            # the value grids are logits (BCEWithLogitsLoss) and probabilities (BCELoss)
                add("grid", (1, 4, 2, 64, 64), None, grid_pair)
                add("grid_scalar", (1, 4, 1, 1, 8193), None, grid_pair)
    return out


def _dice_clamp(name, shape, seed):
    """logits -20 everywhere.  Channel 0: target all zero, den = V p^2 ~ 1e-14 <= 1e-6: the clamp is active (a = 2e6, b = 0 exactly).
    Channel 1: one voxel at 1e-3, den just above 1e-6: clamp inactive.  Channel 2: one voxel at 1."""
    x = torch.full(shape, -20.0)
    t = torch.zeros(shape)
    t[0, 1].view(-1)[3] = 1e-3
    t[0, 2].view(-1)[5] = 1.0
    return x, t


def _dice_empty_channel(name, shape, seed):
    x, t = rand_pair("BCEDiceLoss", shape, seed)
    t[:, 1] = 0.0
    return x, t


def dice_cases():
    out = []
    seed = 3000

    def add(tag, shape, kw=None, fn=rand_pair):
        nonlocal seed
        seed += 1
        kw = dict({"alpha": 0.3, "beta": 0.7}, **(kw or {}))
        out.append({"id": f"BCEDiceLoss-{tag}", "name": "BCEDiceLoss", "kw": kw, "group": ("BCEDiceLoss", "mean"),
                    "make": (lambda fn=fn, shape=shape, s=seed: fn("BCEDiceLoss", shape, s))})
    for v in ELEM_V:
        add(f"V{v}", (1, 1, v))
    add("odd_planes", (1, 3, 5, 7, 9))
    add("300_quadruples", (300, 2, 3, 4))
    add("N3_V8193", (3, 2, 8193))
    for s in (0.0, 0.1, 0.5):
        add(f"grid_s{s}", (1, 4, 8192), {"smoothing": s}, grid_pair)
        add(f"grid_scalar_s{s}", (1, 4, 8193), {"smoothing": s}, grid_pair)
    add("clamp_active", (1, 3, 24), {"alpha": 0.5, "beta": 0.5}, _dice_clamp)
    add("alpha0", (2, 2, 5, 7), {"alpha": 0.0, "beta": 1.0})
    add("beta0", (2, 2, 5, 7), {"alpha": 1.0, "beta": 0.0})
    add("empty_channel", (2, 3, 5, 7, 9), None, _dice_empty_channel)
    return out


COS_T_NORMS = [0.0, 5e-7, 2e-6, 1.0]
COS_P_NORMS = [0.0, 1e-12, 5e-9, 2e-8, 1.0, 1e15]


def _unit(shape, g):
    v = torch.randn(shape, generator=g, dtype=torch.float64)
    return v / v.norm(dim=1, keepdim=True)


def cosine_pair(shape, seed, all_masked=False):
    """every voxel draws its target norm from COS_T_NORMS and its prediction norm from COS_P_NORMS (norm 1 twice as often)"""
    g = _gen(seed)
    n, c = shape[0], shape[1]
    vox = (n, 1) + tuple(shape[2:])
    tn = torch.tensor(COS_T_NORMS[:2] if all_masked else COS_T_NORMS + [1.0], dtype=torch.float64)
    pn = torch.tensor(COS_P_NORMS + [1.0], dtype=torch.float64)
    t = _unit(shape, g) * tn[torch.randint(0, len(tn), vox, generator=g)]
    x = _unit(shape, g) * pn[torch.randint(0, len(pn), vox, generator=g)]
    return x.float(), t.float()


def cosine_cases():
    out = []
    seed = 4000
    for c in (1, 2, 3, 8):
        for v in (1, 8192, 8193):
            seed += 1
            out.append({"id": f"MaskedCosineLoss-C{c}-V{v}", "name": "MaskedCosineLoss", "kw": {}, "group": ("MaskedCosineLoss", "mean"),
                        "make": (lambda c=c, v=v, s=seed: cosine_pair((3, c, v), s))})
    out.append({"id": "MaskedCosineLoss-all_masked", "name": "MaskedCosineLoss", "kw": {}, "group": ("MaskedCosineLoss", "mean"),
                "make": lambda: cosine_pair((3, 3, 8193), 4100, all_masked=True)})
    return out


CE_CV = {1: [1, 4, 2049], 2: [1, 3, 4, 2047, 2048, 2049, 2052], 3: [1, 3, 4, 2047, 2048, 2049, 2052], 64: [3, 4, 2049, 2052],
         1024: [1, 3, 4, 260]}       # C = 1024 stays under 3M elements (N = 3)


def ce_logits(n, c, v, g):
    """voxel i takes pattern i % 4: the maximum at class 0; at the last class; all classes equal; one class at +1e4 and the rest at
    -1e4.  -> (x, hot): hot = the class of the +1e4 (pattern 3), -1 elsewhere"""
    x = torch.randn((n, c, v), generator=g) * 1.5
    pat = (torch.arange(n * v).view(n, v)) % 4
    top = x.amax(1) + 1.0
    x[:, 0] = torch.where(pat == 0, top, x[:, 0])
    x[:, c - 1] = torch.where(pat == 1, top, x[:, c - 1])
    x = torch.where((pat == 2).unsqueeze(1), x[:, :1].expand(n, c, v), x)
    hot = torch.randint(0, c, (n, v), generator=g)
    sat = torch.where(F.one_hot(hot, c).movedim(-1, 1).bool(), torch.tensor(1e4), torch.tensor(-1e4))
    x = torch.where((pat == 3).unsqueeze(1), sat, x)
    return x.contiguous(), torch.where(pat == 3, hot, torch.full_like(hot, -1))


def ce_pair(n, c, v, seed, mode, ignore=-100, oor=False):
    """mode "prob": rows summing to 1, 0 and 2 in turn; "index".  On the +-1e4 voxels the target is the hot class except at voxel
    4103 of the case, where there is one (a miss costs 2e4: more of them, or one among few voxels, and a mean-reduced loss leaves the
    range where fp32 can hold it to 2e-6)."""
    g = _gen(seed)
    x, hot = ce_logits(n, c, v, g)
    i = torch.arange(n * v).view(n, v)
    keep_hot = (hot >= 0) & (i != 4103)
    if mode == "prob":
        t = torch.softmax(torch.randn((n, c, v), generator=g) * 2.0, dim=1)
        t = torch.where(keep_hot.unsqueeze(1), F.one_hot(hot.clamp(min=0), c).movedim(-1, 1).float(), t)
        scale = torch.tensor([1.0, 0.0, 2.0])[(i // 4) % 3]
        return x, (t * scale.unsqueeze(1)).contiguous()
    t = torch.randint(0, c, (n, v), generator=g)
    t = torch.where(keep_hot, hot, t)
    t[torch.rand((n, v), generator=g) < 0.3] = ignore
    if oor:
        bad = torch.tensor([c, -1, 2 ** 40])[torch.randint(0, 3, (n, v), generator=g)]
        t = torch.where(torch.rand((n, v), generator=g) < 0.2, bad, t)
    return x, t


def ce_cases():
    out = []
    seed = 5000

    def add(tag, c, v, mode, kw, **extra):
        nonlocal seed
        seed += 1
        out.append({"id": f"CrossEntropyLoss-{mode}-{tag}", "name": "CrossEntropyLoss", "kw": kw, "group": ("CrossEntropyLoss", mode),
                    "make": (lambda s=seed: ce_pair(3, c, v, s, mode, kw.get("ignore_index", -100), **extra))})
    for mode in ("prob", "index"):
        k = 0
        for c, vs in CE_CV.items():
            for v in vs:
                k += 1
                reds = ("mean", "sum") if c == 3 else (("mean", "sum")[k % 2],)
                for red in reds:
                    add(f"C{c}-V{v}-{red}", c, v, mode, {"reduction": red})
    for red in ("mean", "sum"):
        add(f"ignore255-{red}", 3, 2049, "index", {"reduction": red, "ignore_index": 255})
        add(f"ignore1_in_range-{red}", 3, 2052, "index", {"reduction": red, "ignore_index": 1})
        add(f"out_of_range-{red}", 3, 2052, "index", {"reduction": red}, oor=True)
        add(f"out_of_range_scalar-{red}", 3, 2049, "index", {"reduction": red}, oor=True)
    return out


def all_cases():
    return elem_cases() + dice_cases() + cosine_cases() + ce_cases()
