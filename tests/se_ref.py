"""Staged fp64 reference of the SqueezeExcite / DropPath block (csrc/rx_se.hip) with per-element bounds from the fp32 error analysis
of each formula (a plain module: torch on the CPU, no device code, nothing of the package).

The block is   a = lrelu(mult * xhat + res),  xhat = (y - mean) * rstd,  mult[n][line][c] = s_n * gate,  line = x (keep_x) or 0:
    pooled = line mean of xhat = (linesum(y) / R - mean) * rstd            R = voxels per line
    hidden = relu(W1 (s pooled) + b1);   gate = sigmoid(W2 hidden + b2);   mult = s * gate         (DropPath only: mult = s)
and, with g' = g * lrelu'(out),  L1 = linesum(g'),  L2 = linesum(g' xhat):
    dz2 = s L2 gate (1 - gate);   dh = W2^T dz2 where hidden > 0;   dp = W1^T dh;   dadd = D = s dp / R
    m1 = sum_lines(mult L1 + R D) / V;   m2 = sum_lines(mult L2 + D R pooled) / V
    dw1 = sum_rows dh (s pooled)^T;  db1 = sum_rows dh;  dw2 = sum_rows dz2 hidden^T;  db2 = sum_rows dz2     (rows = (n, line))
    dy = rstd (g' mult + dadd - m1 - xhat m2);   d_residual (+)= g'

Every stage is evaluated GIVEN THE DEVICE'S OWN UPSTREAM OUTPUTS (statistics, pooled, hidden, gate, mult, dadd, m12 and the LeakyReLU
mask out > 0 of the saved output, which is exactly what the kernels read), so no stage inherits another's error and the backward
has no branch ambiguity.  Each stage returns fp64 (ref, bound) pairs; u = 2^-24, gamma(n) bounds an fp32 sum of n terms in any
order.  Layouts: activations NCDHW, line tensors (n, L, c), hidden (n, L, rd), stats and m12 (n, c, 2), w1 (rd, C), w2 (C, rd).

SIGMOID_ULPS.  The gate is 1 / (1 + expf(-z)).  The ROCm install ships no HIP math-API accuracy table (none of its documents
names the ulp error of expf), so the constant is measured: the largest error of the device gate against fp64 sigmoid of
fp64 (W2 hidden + b2) on the device's own hidden, over the whole case matrix of tests/test_se_gpu.py in the three dtypes, was
MEASURED_GATE_ULPS = 5.06 ulps of the gate on the MI355X (the next largest cases: 4.76 and 4.71); twice that is allowed."""
import torch

from exact_ops import U32, gamma, half_ulp

MEASURED_GATE_ULPS = 5.06
SIGMOID_ULPS = 2 * MEASURED_GATE_ULPS


def ulp32(v):
    """one fp32 ulp at |v| (fp64 tensor)"""
    e = torch.floor(torch.log2(v.abs().clamp(min=2.0 ** -126)))
    return torch.exp2(e - 23)


def geometry(shape, keep_x):
    """(L, R, V) of an NCDHW shape: lines per sample, voxels per line, voxels per sample"""
    z, y, x = shape[2:]
    return (x, z * y, z * y * x) if keep_x else (1, z * y * x, z * y * x)


def line_sum(t, keep_x):
    """NCDHW -> (n, L, c): the sum over the voxels of every line"""
    if keep_x:
        return t.sum((2, 3)).permute(0, 2, 1)
    return t.sum((2, 3, 4)).unsqueeze(1)


def spread(m, keep_x):
    """(n, L, c) -> broadcastable against NCDHW"""
    if keep_x:
        return m.permute(0, 2, 1)[:, :, None, None, :]
    return m.permute(0, 2, 1)[:, :, :, None, None]


def _mr(stats):
    st = stats.detach().double().cpu()
    return st[..., 0][:, :, None, None, None], st[..., 1][:, :, None, None, None]


def _scale(scale, n):
    return (torch.ones(n, dtype=torch.float64) if scale is None else scale.detach().double().cpu()).view(n, 1, 1)


def xhat_of(y, stats):
    mean, rstd = _mr(stats)
    return (y - mean) * rstd


def gprime(g, mask, slope):
    """g' = g * lrelu'(out): g where the mask holds, g * slope elsewhere (mask None: slope 1)"""
    return g if mask is None else torch.where(mask, g, g * slope)


def pool_stage(y, stats, keep_x):
    """pooled = (linesum(y) / R - mean) * rstd.  The line sum is an fp32 sum of R stored values in some order (gamma_R of the sum of
    magnitudes); the division, the subtraction and the product round once each.  The subtraction cancels, so the bound is relative
    to rstd * mean|y| over the line, not to |pooled|:  rstd (gamma_R + 2u) mean|y| + 3u |pooled|."""
    L, R, _ = geometry(y.shape, keep_x)
    st = stats.detach().double().cpu()
    mean, rstd = st[..., 0].unsqueeze(1), st[..., 1].unsqueeze(1)           # (n, 1, c)
    ref = (line_sum(y, keep_x) / R - mean) * rstd
    bound = rstd * (gamma(R) + 2 * U32) * line_sum(y.abs(), keep_x) / R + 3 * U32 * ref.abs()
    return ref, bound


def gate_stage(pooled, hidden, gate, se, scale):
    """hidden from the device pooled, gate from the device hidden, mult from the device gate.
    hidden = relu(W1 (s pooled) + b1): s * pooled rounds once, the C products and the C + 1 term sum give gamma_(C+2) of
    sum|w1||s pooled| + |b1|; relu does not amplify it.
    gate = 1 / (1 + expf(-z)), z = b2 + W2 hidden: z errs by dz = gamma_(rd+1) (|b2| + |w2| |hidden|), which moves the sigmoid by at
    most dz / 4; expf, the add and the divide are SIGMOID_ULPS ulps of the gate (see the module docstring).
    mult = s * gate: one rounding (none for s in {0, 1}: s = 0 gives exactly 0).
    se None (DropPath only): mult = s exactly, nothing else is written."""
    n = pooled.shape[0] if pooled is not None else gate.shape[0]
    s = _scale(scale, n)
    if se is None:
        ref = s.expand_as(gate).clone()
        return {"mult": (ref, torch.zeros_like(ref))}
    w1, b1, w2, b2 = se
    C, rd = w1.shape[1], w1.shape[0]
    sp = s * pooled
    h_ref = torch.relu(sp @ w1.T + b1)
    h_b = gamma(C + 2) * (sp.abs() @ w1.abs().T + b1.abs())
    z = hidden @ w2.T + b2
    dz = gamma(rd + 1) * (hidden.abs() @ w2.abs().T + b2.abs())
    g_ref = torch.sigmoid(z)
    g_b = dz / 4 + SIGMOID_ULPS * ulp32(g_ref)
    m_ref = s * gate
    m_b = U32 * m_ref.abs()
    return {"hidden": (h_ref, h_b), "gate": (g_ref, g_b), "mult": (m_ref, m_b)}


def apply_fwd_stage(y, res, stats, mult, keep_x, slope, dtype):
    """out = lrelu(mult * xhat + res) given the device statistics and mult -> (ref, bound, exempt).  In fp32 the subtraction, the two
    products, the residual add, fl(slope) and its product are at most 6 roundings of u relative to |mult xhat| + |res|; then one
    rounding into the storage type.  A pre-activation strictly within that fp32 bound of 0 may take either LeakyReLU branch: exempt
    (None for slope 1)."""
    t = xhat_of(y, stats) * spread(mult, keep_x)
    pre = t + (res if res is not None else 0)
    e32 = 6 * U32 * (t.abs() + (res.abs() if res is not None else 0))
    ref = pre if slope == 1.0 else torch.where(pre > 0, pre, pre * slope)
    exempt = (pre.abs() < e32) if slope != 1.0 else None
    return ref, e32 + half_ulp(ref.abs() + e32, dtype), exempt


def _fin(ref, e):
    """a sum formed in fp64 from fp32 terms with carried error e, rounded once to fp32"""
    return e + U32 * (ref.abs() + e)


def gate_bwd_stage(g, y, mask, stats, pooled, hidden, gate, mult, se, scale, keep_x, slope):
    """dadd, m12 and the four fc gradients given the device mask, statistics, pooled, hidden, gate and mult.
    g' = g * fl(slope) (2u) and xhat (2u) are formed per element; L1 = linesum(g') is an fp32 sum of R terms: (gamma_R + 3u) sum|g'|;
    L2 = linesum(g' xhat), one more product: (gamma_R + 6u) sum|g' xhat|.
    dz2 = s L2 gate (1 - gate): four roundings, 5u |dz2| plus the carried |s| gate (1 - gate) eL2.
    dh = W2^T dz2 under the device's hidden > 0: |w2|^T e_dz2 + gamma_(C+1) |w2|^T |dz2|;  dp = W1^T dh: |w1|^T e_dh + gamma_(rd+1) |w1|^T |dh|.
    D = s dp / R: 3u |D| + |s| e_dp / R.   Line terms t1 = mult L1 + R D and t2 = mult L2 + D R pooled: the carried errors plus 3u
    (4u) of the magnitudes of their two products.   m12 = fp64 sum over the lines / V, rounded once.
    The fc gradients are fp64 sums over the (n, line) rows of fp32 factors, rounded once: the carried e_dh / e_dz2 against the
    magnitude of the other factor (s * pooled rounds once more), plus u of the result.
    A sample with s = 0 has dz2 = dh = D = 0 with zero bounds: it contributes exactly nothing.  se None: dadd = 0, t = mult L."""
    n = y.shape[0]
    L, R, V = geometry(y.shape, keep_x)
    s = _scale(scale, n)
    xh = xhat_of(y, stats)
    gp = gprime(g, mask, slope)
    L1, L2 = line_sum(gp, keep_x), line_sum(gp * xh, keep_x)
    eL1 = (gamma(R) + 3 * U32) * line_sum(gp.abs(), keep_x)
    eL2 = (gamma(R) + 6 * U32) * line_sum((gp * xh).abs(), keep_x)
    out = {}
    if se is None:
        D, eD = torch.zeros_like(mult), torch.zeros_like(mult)
        p = torch.zeros_like(mult)
    else:
        w1, b1, w2, b2 = se
        C, rd = w1.shape[1], w1.shape[0]
        gg = gate * (1 - gate)
        dz2 = s * L2 * gg
        e_dz2 = s.abs() * gg * eL2 + 5 * U32 * dz2.abs()
        live = (hidden > 0).double()
        dh = (dz2 @ w2) * live
        e_dh = (e_dz2 @ w2.abs() + gamma(C + 1) * (dz2.abs() @ w2.abs())) * live
        dp = dh @ w1
        e_dp = e_dh @ w1.abs() + gamma(rd + 1) * (dh.abs() @ w1.abs())
        D = s * dp / R
        eD = s.abs() * e_dp / R + 3 * U32 * D.abs()
        p = pooled
        sp = s * pooled
        f = lambda t: t.reshape(-1, t.shape[-1])                       # rows = (n, line)          # noqa: E731
        out["dw1"] = (f(dh).T @ f(sp), _fin(f(dh).T @ f(sp), f(e_dh).T @ f(sp).abs() + U32 * (f(dh).abs().T @ f(sp).abs())))
        out["db1"] = (f(dh).sum(0), _fin(f(dh).sum(0), f(e_dh).sum(0)))
        out["dw2"] = (f(dz2).T @ f(hidden), _fin(f(dz2).T @ f(hidden), f(e_dz2).T @ f(hidden).abs()))
        out["db2"] = (f(dz2).sum(0), _fin(f(dz2).sum(0), f(e_dz2).sum(0)))
    out["dadd"] = (D, eD)
    t1 = mult * L1 + R * D
    e1 = mult.abs() * eL1 + R * eD + 3 * U32 * ((mult * L1).abs() + R * D.abs())
    t2 = mult * L2 + D * R * p
    e2 = mult.abs() * eL2 + R * p.abs() * eD + 4 * U32 * ((mult * L2).abs() + (D * R * p).abs())
    m12 = torch.stack([t1.sum(1), t2.sum(1)], -1) / V                       # (n, c, 2)
    e12 = torch.stack([e1.sum(1), e2.sum(1)], -1) / V
    out["m12"] = (m12, _fin(m12, e12))
    return out


def apply_bwd_stage(g, y, mask, stats, mult, dadd, m12, keep_x, slope, dtype, old_dres=None):
    """dy = rstd (g' mult + dadd - m1 - xhat m2) and d_residual = g' (+ the old value) given the device mask, statistics, mult, dadd
    and m12.  g' (2u), its product with mult, the add of dadd, the two subtractions, xhat (2u), xhat * m2 and the product by rstd: at
    most 8u of the magnitude terms |g' mult| + |dadd| + |m1| + |xhat| |m2|, scaled by rstd (not by the result, which cancels); then
    one rounding into the storage type.  d_residual: fl(slope) and the product (2u |g'|), or with the old value the add (u |old +
    g'|) on top; then the storage rounding.  No exemptions: the mask is the device's."""
    mean, rstd = _mr(stats)
    xh = (y - mean) * rstd
    gp = gprime(g, mask, slope)
    m, d = spread(mult, keep_x), spread(dadd, keep_x)
    mm = m12.detach().double().cpu()
    m1, m2 = mm[..., 0][:, :, None, None, None], mm[..., 1][:, :, None, None, None]
    ref = rstd * (gp * m + d - m1 - xh * m2)
    e32 = rstd * 8 * U32 * ((gp * m).abs() + d.abs() + m1.abs() + xh.abs() * m2.abs())
    out = {"dy": (ref, e32 + half_ulp(ref.abs() + e32, dtype))}
    want = gp if old_dres is None else old_dres + gp
    e = 2 * U32 * gp.abs() + (U32 * want.abs() if old_dres is not None else 0)
    out["dres"] = (want, e + half_ulp(want.abs() + e, dtype))
    return out


def stats64(y, eps=1e-5):
    """(n, c, 2) fp64 (mean, rstd) of every plane"""
    mean, var = y.mean((2, 3, 4)), y.var((2, 3, 4), unbiased=False)
    return torch.stack([mean, (var + eps).rsqrt()], -1)


def chain(y, res, g, se, scale, keep_x, slope, mask, eps=1e-5):
    """the stages chained end to end in fp64, each fed the previous one's reference values -> dict(a, dy, dres, dw1, db1, dw2, db2)
    (mask: the LeakyReLU branch of every element, as the backward will read it)"""
    n = y.shape[0]
    stats = stats64(y, eps)
    L = geometry(y.shape, keep_x)[0]
    if se is not None:
        pooled, _ = pool_stage(y, stats, keep_x)
        zl = torch.zeros_like(pooled)
        hidden = gate_stage(pooled, torch.zeros((n, L, se[0].shape[0]), dtype=torch.float64), zl, se, scale)["hidden"][0]
        gate = gate_stage(pooled, hidden, zl, se, scale)["gate"][0]
        mult = gate_stage(pooled, hidden, gate, se, scale)["mult"][0]
    else:
        pooled = hidden = gate = None
        mult = gate_stage(None, None, torch.zeros((n, L, y.shape[1]), dtype=torch.float64), None, scale)["mult"][0]
    pre = xhat_of(y, stats) * spread(mult, keep_x) + (res if res is not None else 0)
    a = pre if mask is None else torch.where(mask, pre, slope * pre)
    gb = gate_bwd_stage(g, y, mask, stats, pooled, hidden, gate, mult, se, scale, keep_x, slope)
    ab = apply_bwd_stage(g, y, mask, stats, mult, gb["dadd"][0], gb["m12"][0], keep_x, slope, torch.float32)
    out = {"a": a, "dy": ab["dy"][0], "dres": ab["dres"][0]}
    for k in ("dw1", "db1", "dw2", "db2"):
        if k in gb:
            out[k] = gb[k][0]
    return out


LINE, M12 = ("n", "line", "c"), ("n", "c", "m")
NAMES = {"pooled": LINE, "hidden": ("n", "line", "j"), "gate": LINE, "mult": LINE, "dadd": LINE, "m12": M12, "dw1": ("j", "c"),
         "db1": ("j",), "dw2": ("c", "j"), "db2": ("c",)}


def stage_checks(inp, dev):
    """every stage of one run against its reference: [(name, got, ref, bound, exempt)].
    inp: y, res (or None), g (fp64 NCDHW, as stored), se ((w1, b1, w2, b2) fp64 or None), scale ((n,) or None), keep_x, slope, dtype,
    old_dres (the d_residual an accumulating call started from, or None), has_dres.
    dev: the outputs of the run as fp64 CPU tensors (stats, pooled, hidden, gate, mult, out, dadd, m12, dw1, db1, dw2, db2, dy, dres)"""
    y, res, g, se, scale = inp["y"], inp["res"], inp["g"], inp["se"], inp["scale"]
    keep_x, slope, dtype = inp["keep_x"], inp["slope"], inp["dtype"]
    mask = None if slope == 1.0 else dev["out"] > 0
    checks = []
    if se is not None:
        checks.append(("pooled", dev["pooled"], *pool_stage(y, dev["stats"], keep_x), None))
    for k, (ref, b) in gate_stage(dev.get("pooled"), dev.get("hidden"), dev["gate"] if se is not None else dev["mult"], se,
                                  scale).items():
        checks.append((k, dev[k], ref, b, None))
    checks.append(("out", dev["out"], *apply_fwd_stage(y, res, dev["stats"], dev["mult"], keep_x, slope, dtype)))
    gb = gate_bwd_stage(g, y, mask, dev["stats"], dev.get("pooled"), dev.get("hidden"), dev.get("gate"), dev["mult"], se, scale,
                        keep_x, slope)
    for k, (ref, b) in gb.items():
        checks.append((k, dev[k], ref, b, None))
    ab = apply_bwd_stage(g, y, mask, dev["stats"], dev["mult"], dev["dadd"], dev["m12"], keep_x, slope, dtype, inp["old_dres"])
    checks.append(("dy", dev["dy"], *ab["dy"], None))
    if inp["has_dres"]:
        checks.append(("dres", dev["dres"], *ab["dres"], None))
    return checks


def violations(check):
    """how many elements of one stage_checks entry leave their bound (exempt ones aside; NaN counts)"""
    _, got, ref, bound, exempt = check
    ok = (got - ref).abs() <= bound
    if exempt is not None:
        ok = ok | exempt
    return int((~ok).sum())
