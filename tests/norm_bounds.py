"""Per-element bounds for the InstanceNorm kernel family (a plain module, imported by the op test files): the fp32 error analysis
of (mean, rstd), the apply pass and the backward pass, each checked given the device's own statistics.  Not exact: fp32
statistics, a normalised value, a cancellation."""
import torch

from exact_ops import U32, assert_within, gamma, half_ulp


def _ncdhw(t):
    """an Act, a (n, c, z, y, x) tensor or None -> fp64 CPU NCDHW"""
    if t is None:
        return None
    return (t.to_ncdhw() if hasattr(t, "to_ncdhw") else t).detach().double().cpu()


def _mr(stats, n, c):
    st = stats.detach().double().cpu().view(n, c, 2)
    return st[..., 0].view(n, c, 1, 1, 1), st[..., 1].view(n, c, 1, 1, 1)


def check_stats(stats, y, eps=1e-5, what="stats", keep=None):
    """(mean, rstd) of every (n, c) plane against fp64.  The sums of y and y^2 are fp32 sums of V terms in some order, each within
    gamma_V of the sum of magnitudes; so |mean - mean64| <= (gamma_V + 4u) mean|y| and the variance errs by at most
    (gamma_V + 8u) (E[y^2] + 2 |mean| mean|y|), which moves rstd = (var + eps)^-1/2 by at most half that over var + eps, plus 4u.
    keep: (n, c) 0/1 of a channel dropout -- dropped planes must have rstd exactly 0."""
    y = _ncdhw(y)
    n, c = y.shape[:2]
    V = y[0, 0].numel()
    mean_d, rstd_d = _mr(stats, n, c)
    mean, var = y.mean((2, 3, 4), keepdim=True), y.var((2, 3, 4), unbiased=False, keepdim=True)
    rstd = (var + eps).rsqrt()
    am, a2 = y.abs().mean((2, 3, 4), keepdim=True), (y * y).mean((2, 3, 4), keepdim=True)
    names = ("n", "c", "_", "_", "_")
    assert_within(mean_d, mean, (gamma(V) + 4 * U32) * am + 1e-30, f"{what}: mean", names=names)
    b_r = rstd * ((gamma(V) + 8 * U32) * (a2 + 2 * mean.abs() * am) / (2 * (var + eps)) + 4 * U32)
    if keep is not None:
        k = keep.double().cpu().view(n, c, 1, 1, 1)
        assert (rstd_d[k == 0] == 0).all(), f"{what}: a dropped plane has rstd != 0"
        rstd_d = torch.where(k == 0, rstd, rstd_d)
    assert_within(rstd_d, rstd, b_r, f"{what}: rstd", names=names)


def check_norm_fwd(got, y, stats, res, slope, dtype, what="norm fwd"):
    """out = lrelu((y - mean) * rstd + res), per element, given the device statistics (check_stats bounds them on their own).  In
    fp32 the subtraction, the product, the residual add, the slope (fl(slope)) and its product make at most 5 roundings of u
    relative to |y - mean| * rstd + |res|; then one rounding into the storage type (half an ulp).  A pre-activation strictly
    within that fp32 bound of 0 may take either LeakyReLU branch: those elements are exempt, and at most 0.1 % of the tensor may
    be (a pre-activation of exactly 0 with a zero bound -- a dropped plane -- is 0 on both)."""
    y, res = _ncdhw(y), _ncdhw(res)
    mean, rstd = _mr(stats, *y.shape[:2])
    t = (y - mean) * rstd
    pre = t + (res if res is not None else 0)
    e32 = 5 * U32 * (t.abs() + (res.abs() if res is not None else 0))
    ref = pre if slope == 1.0 else torch.where(pre > 0, pre, pre * slope)
    exempt = (pre.abs() < e32) if slope != 1.0 else None
    assert_within(_ncdhw(got), ref, e32 + half_ulp(ref.abs() + e32, dtype), what, exempt=exempt)


def norm_bwd_ref(g, y, stats, mask, slope):
    """fp64 dy = rstd (g' - mean g' - xhat mean(g' xhat)), g' = g * (mask ? 1 : slope), from the device statistics; with the bound
    of its fp32 evaluation.  The two means are fp32 sums of V terms (gamma_V of the sums of magnitudes, plus 6u for g' = g *
    fl(slope), xhat, the product and the division by V); per element, g' (2u), xhat (2u), xhat * mean(g' xhat), the two
    subtractions and the product by rstd add 8u of the magnitude terms |g'| + |mean g'| + |xhat| |mean(g' xhat)| (scaled by rstd;
    not by the result, which cancels)."""
    g, y = _ncdhw(g), _ncdhw(y)
    n, c = y.shape[:2]
    V = y[0, 0].numel()
    mean, rstd = _mr(stats, n, c)
    xh = (y - mean) * rstd
    gp = g if mask is None else torch.where(mask, g, g * slope)
    m1 = gp.mean((2, 3, 4), keepdim=True)
    m2 = (gp * xh).mean((2, 3, 4), keepdim=True)
    ref = rstd * (gp - m1 - xh * m2)
    s1, s2 = gp.abs().mean((2, 3, 4), keepdim=True), (gp * xh).abs().mean((2, 3, 4), keepdim=True)
    e32 = rstd * ((gamma(V) + 6 * U32) * (s1 + xh.abs() * s2) + 8 * U32 * (gp.abs() + m1.abs() + xh.abs() * m2.abs()))
    return ref, e32, gp


def check_norm_bwd(got, g, y, stats, mask, slope, dtype, what="norm bwd", d_g=None):
    """per element within norm_bwd_ref's fp32 bound plus half an ulp of the storage type (got: one output or a tuple of them, all
    of the same reference).  d_g: a per-element bound on the error of g itself (a gradient the kernel forms on the fly), carried
    through rstd (g' - mean g' - xhat mean(g' xhat))"""
    ref, e32, _ = norm_bwd_ref(g, y, stats, mask, slope)
    if d_g is not None:
        yd = _ncdhw(y)
        mean, rstd = _mr(stats, *yd.shape[:2])
        xa = ((yd - mean) * rstd).abs()
        e32 = e32 + rstd * (d_g + d_g.mean((2, 3, 4), keepdim=True) + xa * (d_g * xa).mean((2, 3, 4), keepdim=True))
    bound = e32 + half_ulp(ref.abs() + e32, dtype)
    for one in (got if isinstance(got, tuple) else (got,)):
        assert_within(_ncdhw(one), ref, bound, what)


def lrelu_mask(out, y, stats, slope):
    """the LeakyReLU mask the backward kernels use: out > 0 from the saved output, else xhat > 0 (the sign of y - mean is exact
    in fp32); None for slope 1"""
    if slope == 1.0:
        return None
    if out is not None:
        return _ncdhw(out) > 0
    y = _ncdhw(y)
    mean, rstd = _mr(stats, *y.shape[:2])
    return (y - mean) * rstd > 0


def check_dres(got, g, mask, slope, dtype, what="d_residual", old=None):
    """the residual gradient of rx_instnorm_act_bwd: g' = g * lrelu'(out) -- fl(slope) and the product, 2u -- then one rounding
    into the storage type; accumulating (old: the destination before the call, fp64 NCDHW) adds one fp32 rounding of the sum.
    Returns g'."""
    g = _ncdhw(g)
    gp = g if mask is None else torch.where(mask, g, g * slope)       # g' = g * lrelu'(out): fl(slope) and the product
    if old is None:
        e = 2 * U32 * gp.abs()
        assert_within(_ncdhw(got), gp, e + half_ulp(gp.abs() + e, dtype), what)
    else:
        want = old + gp
        e = U32 * (want.abs() + 2 * gp.abs())
        assert_within(_ncdhw(got), want, e + half_ulp(want.abs() + e, dtype), what)
    return gp


def check_norm_bwd_res(d_res, dy, g, pool_dy, pool, out, y, stats, slope, dtype, what="bwd_res"):
    """rx_instnorm_act_bwd_res per element: g' = (g + pool term) * lrelu'(out) in fp32 -- the pool scale and product, the add and the
    slope product, 4u of |g| + |pool term| -- then one rounding into d_residual.  dy: the norm-backward bound of g', plus the error
    of g' itself carried through rstd (g' - mean g' - xhat mean(g' xhat)), counting half an ulp more in case the sums read g' as
    stored.  g, out, y, pool_dy: as the launch read them; pool: the stride of the deferred AvgPool or None."""
    g, outd, yd = _ncdhw(g), _ncdhw(out), _ncdhw(y)
    n, c = yd.shape[:2]
    up = 0
    if pool:
        up = _ncdhw(pool_dy)
        for ax, s in enumerate(pool):
            up = up.repeat_interleave(s, dim=2 + ax)
        up = up / (pool[0] * pool[1] * pool[2])
    gd_c = g + up
    gd_c = torch.where(outd > 0, gd_c, gd_c * slope)
    e_c = 4 * U32 * (g.abs() + (up.abs() if pool else 0))
    assert_within(_ncdhw(d_res), gd_c, e_c + half_ulp(gd_c.abs() + e_c, dtype), f"{what}: d_residual")
    ref_c, e32, _ = norm_bwd_ref(gd_c, yd, stats, None, 1.0)
    mean, rstd_c = _mr(stats, n, c)
    xh_c = (yd - mean) * rstd_c
    d_g = e_c + half_ulp(gd_c.abs() + e_c, dtype)
    e_dy = e32 + rstd_c * (d_g + d_g.mean((2, 3, 4), keepdim=True) + xh_c.abs() * (d_g * xh_c.abs()).mean((2, 3, 4), keepdim=True))
    assert_within(_ncdhw(dy), ref_c, e_dy + half_ulp(ref_c.abs() + e_dy, dtype), f"{what}: dy")
