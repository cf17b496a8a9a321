"""fp64 references, per-element bounds and the shared case tables of the streaming-inference kernels (csrc/rx_infer.hip), written
from the contract in include/rxunet.h (a plain module: numpy on the CPU, no device code; the package is imported only for the
record enumeration `tta_views`).  Used by tests/test_infer_ref_cpu.py (an fp32 numpy twin and a list of wrong variants through
every checker) and by tests/test_infer_ops_gpu.py (the C ABI through the same checkers).  u = 2^-24, gamma(n) as in exact_ops.

Volumes are (C, Z, Y, X) with absolute rows; `ring_of` makes the (C, R, Y, X) ring slab the kernels read.  Records are the 12
integers of rx_geom_sample (src_axis, flip, ch_src, ch_neg), applied as the gather out[o] = in[i(o)],
i[src_axis[d]] = flip[d] ? n_d - 1 - o_d : o_d.

GATHER / SCALE is exact: uint8 / 255 and uint16 / 65535 are one correctly rounded fp32 division, fp32 passes through; the
checker compares uint32 views, so NaN payloads, -0.0 and subnormals count.

GATHER / ZSCORE.  Reference z = (v - mean) / max(std, 1e-10) in fp64 over all channels of the patch, population std.  The kernel
sums v and v^2 in fp64 and then rounds four times: m = fl32(mean) (|m - mean| <= u |mean|), s = fl32(std) (relative u),
d = fl32(v - m) (relative u of v - m), got = fl32(d / s) (relative u).  To first order
    got - z = z (e_d + e_div - e_s) - (m - mean) / std        =>        |got - z| <= 3u |z| + u |mean| / std.
The variance is formed as E[v^2] - mean^2 in fp64: each of the two terms carries a relative 2^-53, so var errs by 2^-52 E[v^2]
and std = sqrt(var) by the relative 2^-52 E[v^2] / (2 var), which multiplies |z|.  That is the whole bound; there is no flat
epsilon.  A constant patch has var = 0: the fp64 sums of n equal fp32 values are exact (n < 2^29), so fl32(mean) = v and every
output is (v - v) / s = +0 whatever s is -- `check_zscore` demands exact zeros there instead of a bound.

ACCUMULATE.  Reference: the first `valid` slots added in slot order in fp64, p the fp64 activation.  A voxel covered by K slots is
a_K = fl(...fl(fl(a_0 + t_1) + t_2)... + t_K), t_k = fl(w p_k): K additions, so
    |got - ref| <= gamma_K (|a_0| + sum |w p_k|) + sum eps_p |w p_k|,
eps_p the relative error of the activated p_k (0 for act = none; the product's own rounding u is far inside the factor two of
eps_p, and act = none is tested with integer logits and dyadic weights, where every product and sum is exact and the demand is
bit equality).  wsum: gamma_K (|w_0| + sum w).  Voxels no slot covers (K = 0) must keep their bits, NaN and -0.0 included.
    sigmoid: eps_p = SIGMOID_ULPS ulps of p -- se_ref's measured constant for the same expression 1 / (1 + expf(-x)).
    softmax: eps_p = SOFTMAX_ULPS ulps of p, SOFTMAX_ULPS = 2 * MEASURED_SOFTMAX_ULPS.  The ROCm install documents no ulp error
    for expf, so, as in se_ref, it is measured: the largest error of the device's p = expf(x - max) / sum expf(. - max) against
    the fp64 softmax over the large-logit table `SOFTMAX_TABLE` (uniform weight 1 onto a zero accumulator, K = 1, so the
    accumulator holds p itself) was MEASURED_SOFTMAX_ULPS = 2.283 ulps of p on the MI355X, at the row (500, 490.125, 490.875),
    channel 1 (p = 5.14e-5); twice that, 4.566 ulps, is allowed.  (Over the 12 hand-written rows alone the largest error was 0.671
    ulps, at (1.5, 0.25, -inf): three dozen values of p are too few to see the tail, which is why the table has 120 rows.)
    tests/test_infer_ops_gpu.py repeats the measurement on every run.  The
    logits of every softmax case are multiples of 1/8, so the fp32 difference x - max is exact; where it is not, the contract's
    own rounding of it adds u |x - max| (`eps_act`).
An ulp of p is 2^(floor(log2 p) - 23), at least 2^-149.  The sigmoid reference is 0 where expf(-x) leaves fp32 (x < -88.72): the
contract is the fp32 expression 1 / (1 + expf(-x)), which is 1 / inf there; the table demands exactly 0 and 1 at its saturated ends.

FINALIZE is exact against the fp32 numpy statement of oracle/inference_oracle.py:54-68 (`finalize_ref`): contraction is off in the
kernel and every operation is correctly rounded.  The only data-dependent branch is wsum > 0, which is exact.  `finalize_ref` also
states the accumulators after the call (reset 0 / 1 / 2) and the optional weight rows.

OCCUPANCY is exact against inference.occupancy_numpy (the test calls it directly)."""
import itertools

import numpy as np

from exact_ops import U32, gamma
from se_ref import SIGMOID_ULPS

# the largest |p_device - p_fp64| in fp32 ulps of p over SOFTMAX_TABLE on the MI355X, and the table row that produced it
MEASURED_SOFTMAX_ULPS = 2.283
MEASURED_SOFTMAX_CASE = "logits (500, 490.125, 490.875), channel 1 (p = 5.14e-5)"
SOFTMAX_ULPS = 2 * MEASURED_SOFTMAX_ULPS

NP_DT = {"u8": np.uint8, "u16": np.uint16, "f32": np.float32}
DIV = {"u8": np.float32(255.0), "u16": np.float32(65535.0), "f32": None}
IDENT = (0, 1, 2, 0, 0, 0, 0, 1, 2, 0, 0, 0)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def ulp32(v):
    """one fp32 ulp at |v| (fp64 array), subnormal spacing below 2^-126"""
    e = np.floor(np.log2(np.maximum(np.abs(v), 2.0 ** -126)))
    return np.exp2(e - 23)


def ring_of(vol, R, z_lo):
    """the (C, R, Y, X) ring slab holding the rows [z_lo, z_lo + R) of a (C, Z, Y, X) volume, row z at z % R; rows past the volume
    stay zero"""
    C, Z, Y, X = vol.shape
    ring = np.zeros((C, R, Y, X), vol.dtype)
    for z in range(z_lo, min(z_lo + R, Z)):
        ring[:, z % R] = vol[:, z]
    return ring


def apply_record(row, arr, vector=False):
    """out[c][o] = (+/-) arr[cs(c)][i(o)] for a (C, z, y, x) array: the gather form of rx_geom_apply, by index arrays"""
    src, flip, chs, neg = row[0:3], row[3:6], row[6:9], row[9:12]
    ext = arr.shape[1:]
    out_ext = [0, 0, 0]
    for d in range(3):
        out_ext[d] = ext[src[d]]
    o = np.meshgrid(*[np.arange(n) for n in out_ext], indexing="ij")
    i = [None, None, None]
    for d in range(3):
        i[src[d]] = (out_ext[d] - 1 - o[d]) if flip[d] else o[d]
    out = arr[:, i[0], i[1], i[2]]
    if vector:
        assert arr.shape[0] == 3
        out = np.stack([np.negative(out[chs[c]]) if neg[c] else out[chs[c]] for c in range(3)])
    return np.ascontiguousarray(out)


def records_for(patch):
    """every record inference.tta_views admits for a patch shape (flips about all axes, quarter turns about the axes whose plane
    is square), as the INVERSE rows rx_sw_accumulate_geom applies"""
    import mt3d_amd  # noqa: F401
    from mt3d_amd import inference as inf
    from mt3d_amd.dataloading.geometry_device import allowed_rot90_axes
    spec = {"flip": ["z", "y", "x"], "rot90": list(allowed_rot90_axes(patch))}
    return [tuple(v.inverse().row()) for v in inf.tta_views(spec, patch)]


# ---- gather -------------------------------------------------------------------------------------------------------------------
def scale_ref(raw):
    """the SCALE statement: numpy's float32 division (fp32 input as it is, bits included)"""
    if raw.dtype == np.float32:
        return raw.copy()
    return raw.astype(np.float32) / (np.float32(255.0) if raw.dtype == np.uint8 else np.float32(65535.0))


def gather_scale_ref(vol, origins, patch, rows=None):
    """(B, cin, pz, py, px) fp32: slot b is the scaled patch of `vol` at origins[b], moved by rows[b] if given"""
    pz, py, px = patch
    out = []
    for b, (z, y, x) in enumerate(origins):
        p = scale_ref(vol[:, z:z + pz, y:y + py, x:x + px])
        out.append(apply_record(rows[b], p) if rows is not None else p)
    return np.stack(out)


def zscore_ref(p32):
    """one scaled patch (all its channels) -> (z, bound, constant) in fp64; see the module docstring"""
    v = p32.astype(np.float64)
    mean, var = v.mean(), v.var()
    std = max(np.sqrt(var), 1e-10)
    z = (v - mean) / std
    e2 = (v * v).mean()
    cancel = 2.0 ** -52 * e2 / (2 * max(var, 1e-20))
    bound = (3 * U32 + cancel) * np.abs(z) + U32 * abs(mean) / std
    return z, bound, bool(var == 0.0)


def check_zscore(got, scaled, what=""):
    """got, scaled: (B, cin, pz, py, px).  Returns the largest error / bound over the non-constant slots."""
    assert got.shape == scaled.shape, (what, got.shape, scaled.shape)
    worst = 0.0
    for b in range(scaled.shape[0]):
        z, bound, const = zscore_ref(scaled[b])
        g = got[b].astype(np.float64)
        if const:
            assert (g == 0).all(), f"{what}: slot {b} is constant, its zscore must be exactly 0 (got {g.ravel()[:4]})"
            continue
        err = np.abs(g - z)
        ok = err <= bound                                   # NaN fails
        assert ok.all(), (f"{what}: slot {b}: {int((~ok).sum())} of {ok.size} beyond the bound, worst err/bound "
                          f"{np.nanmax(err / bound):.3f} at {np.unravel_index(np.argmax(~ok), ok.shape)}")
        worst = max(worst, float((err / bound).max()))
    return worst


def _gvol(dt, shape, seed, kind="random"):
    rng = np.random.default_rng(seed)
    if dt == "f32":
        if kind == "const":
            return np.full(shape, 0.3, np.float32)
        v = (rng.normal(size=shape) * 3 + 1).astype(np.float32)
        v += np.arange(shape[2], dtype=np.float32)[None, None, :, None]      # the statistics differ from origin to origin
        if kind == "step":
            v = np.full(shape, 0.3, np.float32)
            v[0, shape[1] // 2, 1, 1] = np.float32(0.3) + np.float32(1 / 255)       # one uint8 level, as the integer kinds
        return v
    top = int(np.iinfo(NP_DT[dt]).max)
    if kind == "const":
        return np.full(shape, 77, NP_DT[dt])
    if kind == "step":
        v = np.full(shape, 77, NP_DT[dt])
        v[0, shape[1] // 2, 1, 1] = 78
        return v
    if kind == "band":                                      # mean ~ 0.99, std ~ 1e-3: an fp32 sum of squares would lose the variance
        return rng.integers(int(top * 0.9885), int(top * 0.9915) + 1, size=shape).astype(NP_DT[dt])
    v = rng.integers(0, top + 1, size=shape)
    v = np.clip(v // 2 + (np.arange(shape[2])[None, None, :, None] * top) // (2 * shape[2]), 0, top)
    return v.astype(NP_DT[dt])


def _g(name, dt, cin, zyx, R, z_lo, patch, origins, kind="random", zscore=True):
    return dict(name=f"{name}-{dt}", dt=dt, cin=cin, zyx=zyx, R=R, z_lo=z_lo, patch=patch, origins=origins, kind=kind, zscore=zscore)


def gather_cases(big=True):
    """the gather table.  Small slab (20, 11, 13), ring 8 holding rows [7, 15): every patch row range wraps or touches the seam."""
    cases = []
    for dt in ("u8", "u16", "f32"):
        for cin in (1, 3):
            for patch in ((3, 2, 1), (2, 4, 3), (3, 5, 4), (4, 3, 5), (2, 3, 10)):      # px 1, 3, 4, 5, 10; three distinct extents
                pz, py, px = patch
                org = [(7, 0, 0), (15 - pz, 11 - py, 13 - px), (9, 3, 2)]
                cases.append(_g(f"c{cin}-p{pz}x{py}x{px}", dt, cin, (20, 11, 13), 8, 7, patch, org))
        cases.append(_g("whole-slab", dt, 3, (20, 5, 6), 8, 7, (8, 5, 6), [(7, 0, 0)]))
        org32 = [(7 + b % 7, (b * 3) % 9, (b * 5) % 10) for b in range(32)]
        cases.append(_g("batch32", dt, 1, (20, 11, 13), 8, 7, (2, 3, 4), org32))
        cases.append(_g("odd-n", dt, 1, (20, 11, 13), 8, 7, (3, 3, 5), [(8, 1, 2), (12, 8, 8)]))
        cases.append(_g("constant", dt, 3, (20, 11, 13), 8, 7, (3, 3, 5), [(8, 1, 2), (12, 8, 8)], kind="const"))
        cases.append(_g("one-step", dt, 1, (8, 5, 7), 8, 0, (8, 5, 7), [(0, 0, 0)], kind="step"))
    cases.append(_g("narrow-band", "u16", 1, (20, 11, 13), 8, 7, (3, 3, 5), [(8, 1, 2), (12, 8, 8)], kind="band"))
    if big:
        cases.append(_g("chunk-cap-41", "u8", 1, (43, 42, 43), 41, 2, (41, 41, 41), [(2, 1, 2)]))             # n = 68 921
        cases.append(_g("grid-cap-104", "u8", 1, (104, 101, 100), 104, 0, (104, 101, 100), [(0, 0, 0)]))      # n = 1 050 400
    return cases


def gather_volume(case):
    seed = sum(ord(ch) for ch in case["name"])
    vol = _gvol(case["dt"], (case["cin"],) + tuple(case["zyx"]), seed, case["kind"])
    if case["kind"] == "random" and case["dt"] != "f32":       # the top of the range inside the first patch: exactly 1.0
        z, y, x = case["origins"][0]
        vol[0, z, y, x] = np.iinfo(vol.dtype).max
    return vol


F32_SPECIALS = np.array([np.nan, np.inf, -np.inf, -0.0, 1e-41, -1e-45, 0.0, 1.5], np.float32)


# ---- accumulate ---------------------------------------------------------------------------------------------------------------
SIGMOID_TABLE = np.array([30, -30, 88, -88, 100, -100, np.inf, -np.inf, 0.0, 0.37, -5.25, 17.5], np.float32)
# rows of c = 3 logits: channels 90 apart, all equal at 1000, one channel at -inf -- and, so that the largest error is taken over
# a few hundred values of p and not a few dozen, 108 more rows of large logits: a base of +-1000, +-90 or 500 on one channel, the
# others below it by multiples of 1/8 up to 12 (every difference exact in fp32)
_FIXED_ROWS = [[0, 90, -90], [90, 0, -90], [-90, 90, 0], [3.25, 93.75, -86.125], [45.25, -44.875, 135.5], [1000, 1000, 1000],
               [-np.inf, 2, 1], [5, -np.inf, 5], [1.5, 0.25, -np.inf], [10.125, 11.75, 9.25], [-1000, -1001.5, -1003.25],
               [88.5, 87.25, 89.125]]


def _softmax_table():
    rng = np.random.default_rng(2)
    rows = list(_FIXED_ROWS)
    for i in range(108):
        base = (1000.0, -1000.0, 90.0, -90.0, 500.0)[i % 5]
        row = base - rng.integers(0, 97, size=3) / 8.0
        row[i % 3] = base
        rows.append(row.tolist())
    return np.array(rows, np.float32)


SOFTMAX_TABLE = _softmax_table()


def act_ref(lg, act):
    """fp64 activation of (c, ...) logits over the channel axis"""
    lg = lg.astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        if act == 1:
            # the contract is the fp32 expression 1 / (1 + expf(-x)): where expf(-x) leaves fp32 (x < -88.72...) it is 1 / inf = 0
            # exactly; the true value there is below 2^-128, under half the smallest normal number
            return np.where(-lg > np.log(float(np.finfo(np.float32).max)), 0.0, 1.0 / (1.0 + np.exp(-lg)))
        if act == 2:
            e = np.exp(lg - lg.max(0, keepdims=True))
            return e / e.sum(0, keepdims=True)
    return lg


def eps_act(p, act, lg=None):
    """the relative error allowed to an activated fp32 p (fp64 array): ulps of p over |p|.  Softmax (lg: the logits): where the
    fp32 difference d = x - max is itself rounded, exp(d (1 + e)) = p (1 + d e) adds u |d| to the numerator and sum_k p_k u |d_k| to
    the denominator -- zero for the dyadic logits of the case tables, whose differences are exact."""
    ulps = {0: 0.0, 1: SIGMOID_ULPS, 2: SOFTMAX_ULPS}[act]
    if ulps == 0.0:
        return np.zeros_like(p)
    eps = np.where(p != 0, ulps * ulp32(p) / np.where(p != 0, np.abs(p), 1.0), 0.0)
    if act == 2 and lg is not None:
        with np.errstate(invalid="ignore", over="ignore"):
            d = lg.astype(np.float64) - lg.astype(np.float64).max(0, keepdims=True)
            cond = np.where(np.isfinite(d) & (d.astype(np.float32).astype(np.float64) != d), U32 * np.abs(d), 0.0)
        eps = eps + cond + (p * cond).sum(0, keepdims=True)
    return eps


def accumulate_ref(sum0, wsum0, logits, origins, valid, w, act, R, rows=None, vector=0):
    """-> dict(s, s_bound, w, w_bound, K): fp64 accumulators after the call, their per-voxel bounds and the cover count K (R, Y, X).
    sum0 (c, R, Y, X), wsum0 (R, Y, X) or None, logits (B, c, pz, py, px), w (pz, py, px)."""
    c, _, Y, X = sum0.shape
    pz, py, px = w.shape
    s = sum0.astype(np.float64)
    ws = wsum0.astype(np.float64) if wsum0 is not None else np.zeros((R, Y, X))
    mag_s = np.zeros_like(s)
    err_s = np.zeros_like(s)
    mag_w = np.zeros_like(ws)
    K = np.zeros((R, Y, X), np.int64)
    w64 = w.astype(np.float64)
    for b in range(valid):
        z, y, x = origins[b]
        p = act_ref(logits[b], act)
        e = eps_act(p, act, logits[b])
        if rows is not None:
            p, e = apply_record(rows[b], p, bool(vector)), apply_record(rows[b], e, bool(vector))
            e = np.abs(e)
        t = w64[None] * p
        for i in range(pz):
            r = (z + i) % R
            sl = np.s_[r, y:y + py, x:x + px]
            s[(slice(None),) + sl] += t[:, i]
            mag_s[(slice(None),) + sl] += np.abs(t[:, i])
            err_s[(slice(None),) + sl] += e[:, i] * np.abs(t[:, i])
            ws[sl] += w64[i]
            mag_w[sl] += w64[i]
            K[sl] += 1
    with np.errstate(invalid="ignore"):
        g = gamma(K.astype(np.float64))
        a0 = np.where(K > 0, np.abs(np.nan_to_num(sum0.astype(np.float64), nan=0.0, posinf=0.0, neginf=0.0)), 0.0)
        s_bound = g[None] * (a0 + mag_s) + err_s
        w0 = np.abs(wsum0.astype(np.float64)) if wsum0 is not None else 0.0
        w_bound = g * (np.where(K > 0, np.nan_to_num(w0, nan=0.0), 0.0) + mag_w)
    return dict(s=s, s_bound=s_bound, w=ws, w_bound=w_bound, K=K)


def check_accumulate(got_s, got_w, ref, sum0, wsum0, what="", exact=False):
    """covered voxels within their bound (bit-equal to the fp32 value of the reference if `exact`), uncovered voxels bit-identical
    to what they held.  got_w / wsum0 None: the call had no wsum.  Returns the largest err / bound of (sum, wsum)."""
    worst = []
    for got, base, r, bound, cov in ((got_s, sum0, ref["s"], ref["s_bound"], np.broadcast_to(ref["K"] > 0, sum0.shape)),
                                     (got_w, wsum0, ref["w"], ref["w_bound"], ref["K"] > 0)):
        if got is None:
            worst.append(0.0)
            continue
        same = bits(got) == bits(base)
        assert same[~cov].all(), (f"{what}: {int((~same[~cov]).sum())} voxels no slot covers changed, first at "
                                  f"{np.unravel_index(np.argmax(~same & ~cov), same.shape)}")
        with np.errstate(invalid="ignore", divide="ignore"):
            err = np.abs(got.astype(np.float64) - r)
            ok = (err <= bound) | ~cov
            if exact:
                ok &= (bits(got) == bits(r.astype(np.float32))) | ~cov
            ratio = np.where(cov & (bound > 0), err / np.where(bound > 0, bound, 1.0), 0.0)
        assert ok.all(), (f"{what}: {int((~ok).sum())} covered voxels beyond the bound, first at "
                          f"{np.unravel_index(np.argmax(~ok), ok.shape)}: got {got[np.unravel_index(np.argmax(~ok), ok.shape)]!r}, "
                          f"want {r[np.unravel_index(np.argmax(~ok), ok.shape)]!r} +- {bound[np.unravel_index(np.argmax(~ok), ok.shape)]:.3e}")
        worst.append(float(np.nanmax(ratio)) if ratio.size else 0.0)
    return tuple(worst)


def softmax_ulps(got_p, logits):
    """the error of fp32 softmax values against fp64, in ulps of p, per element ((c, ...) arrays)"""
    p = act_ref(logits, 2)
    return np.abs(got_p.astype(np.float64) - p) / ulp32(p)


def _a(name, c, patch, Y, X, origins, valid, weights, act, logits="random", rows=None, vector=0, R=16, zero_acc=False):
    return dict(name=name, c=c, patch=patch, Y=Y, X=X, R=R, origins=origins, valid=valid, weights=weights, act=act, logits=logits,
                rows=rows, vector=vector, zero_acc=zero_acc)


def _spread(patch, X, Y=14):
    """five slots: z origins 10, 12, 15 (ring 16: with pz = 8 the rows 10..22 wrap), the smallest x origin 5 (X % 4 == 0) or 6, a
    repeated position, and a padding slot that `valid` = 4 leaves out; the largest x end is no multiple of 4"""
    pz, py, px = patch
    x0 = 5 if X % 4 == 0 else 6
    x1 = X - px - (1 if (X - 1) % 4 else 2)
    assert (x1 + px) % 4 != 0 and x1 >= x0
    return [(10, 1, x0), (12, Y - py, x1), (15, 2, x0 + 1), (12, Y - py, x1), (10, 0, 0)]


ACTS = {0: "none", 1: "sigmoid", 2: "softmax"}


def accumulate_cases(geom=True):
    cases = []
    for X in (24, 22):
        for weights in ("uniform", "gauss"):
            for c in (1, 2, 3, 5):
                for act in (0, 1, 2):
                    cases.append(_a(f"span-c{c}-{ACTS[act]}-{weights}-X{X}", c, (8, 5, 6), 14, X, _spread((8, 5, 6), X), 4, weights, act))
            for patch in ((5, 6, 7), (3, 3, 3), (4, 4, 4)):
                cases.append(_a(f"patch{patch[0]}{patch[1]}{patch[2]}-{weights}-X{X}", 3, patch, 14, X, _spread(patch, X), 4, weights, 1))
            cases.append(_a(f"K32-{weights}-X{X}", 2, (3, 3, 3), 14, X, [(14, 5, 6)] * 32, 32, weights, 2))
            cases.append(_a(f"valid1-{weights}-X{X}", 3, (4, 4, 4), 14, X, _spread((4, 4, 4), X), 1, weights, 1))
            cases.append(_a(f"valid0-{weights}-X{X}", 3, (4, 4, 4), 14, X, _spread((4, 4, 4), X), 0, weights, 1))
        cases.append(_a(f"sigmoid-table-X{X}", 1, (2, 3, 4), 14, X, [(15, 3, 6), (13, 9, 9)], 2, "uniform", 1, logits="sigmoid-table",
                        zero_acc=True))
        cases.append(_a(f"softmax-table-X{X}", 3, (4, 5, 6), 14, X, [(15, 3, 6), (11, 8, 9)], 2, "uniform", 2, logits="softmax-table",
                        zero_acc=True))
        cases.append(_a(f"softmax-c1-X{X}", 1, (3, 3, 3), 14, X, [(15, 3, 6)], 1, "uniform", 2, zero_acc=True))
        if geom:
            for patch in ((5, 6, 6), (6, 5, 6), (6, 6, 5), (5, 6, 7)):
                recs = records_for(patch)
                assert 8 <= len(recs) <= 32
                pz, py, px = patch
                x0 = 5 if X % 4 == 0 else 6
                spots = [(10, 1, x0), (12, 14 - py, X - px - 1), (15, 2, x0 + 1), (11, 3, x0 + 2)]
                org = [spots[b % 4] for b in range(len(recs))]       # every record of the shape in one batch, mixed
                for vector in (0, 1):
                    for act in ((0, 1, 2) if patch == (5, 6, 6) else (0,)):
                        cases.append(_a(f"geom{pz}{py}{px}-v{vector}-{ACTS[act]}-X{X}", 3, patch, 14, X, org, len(recs), "gauss", act,
                                        rows=recs, vector=vector))
    return cases


def accumulate_data(case, gaussian=None):
    """-> (sum0, wsum0, logits, w).  act = none: integer logits and dyadic weights (every product and sum exact).  Uncovered voxels of
    both accumulators hold NaN, -0.0 and integers in turn, inside the bounding box and outside it.  gaussian: patch -> fp32 weights
    (inference.gaussian_importance_map); without it a smooth non-dyadic table of the same kind."""
    rng = np.random.default_rng(sum(ord(ch) for ch in case["name"]))
    c, patch, R, Y, X = case["c"], case["patch"], case["R"], case["Y"], case["X"]
    B = len(case["origins"])
    if case["logits"] == "sigmoid-table":
        logits = np.resize(SIGMOID_TABLE, (B, 1) + patch).astype(np.float32)
    elif case["logits"] == "softmax-table":
        n = int(np.prod(patch))
        t = np.resize(SOFTMAX_TABLE, (B * n, 3))
        logits = np.ascontiguousarray(t.reshape(B, n, 3).transpose(0, 2, 1).reshape((B, 3) + patch))
    elif case["act"] == 0:
        logits = rng.integers(-4, 5, size=(B, c) + patch).astype(np.float32)
        logits[0, :, 0, 0, :2] = 0.0                                    # exact zeros: a negated one is -0.0
    elif case["act"] == 2:
        logits = (rng.integers(-128, 129, size=(B, c) + patch) / 8).astype(np.float32)      # dyadic: x - max is exact in fp32
    else:
        logits = (rng.normal(size=(B, c) + patch) * 4).astype(np.float32)
    if case["weights"] == "uniform":
        w = np.ones(patch, np.float32)
    elif case["act"] == 0:
        w = (rng.integers(1, 9, size=patch) / 8).astype(np.float32)
    elif gaussian is not None:
        w = gaussian(patch)
    else:
        g = [np.exp(-0.5 * ((np.arange(n) - n // 2) / (n / 8 + 0.5)) ** 2) for n in patch]
        w = (g[0][:, None, None] * g[1][None, :, None] * g[2][None, None, :]).astype(np.float32)
    K = np.zeros((R, Y, X), bool)
    for b in range(case["valid"]):
        z, y, x = case["origins"][b]
        for i in range(patch[0]):
            K[(z + i) % R, y:y + patch[1], x:x + patch[2]] = True
    if case["zero_acc"]:
        sum0, wsum0 = np.zeros((c, R, Y, X), np.float32), np.zeros((R, Y, X), np.float32)
    else:
        sum0 = rng.integers(-3, 4, size=(c, R, Y, X)).astype(np.float32)
        wsum0 = rng.integers(0, 3, size=(R, Y, X)).astype(np.float32)
    mark = np.arange(R * Y * X).reshape(R, Y, X) % 3
    for arr in (sum0, wsum0):
        arr[..., ~K & (mark == 0)] = np.nan
        arr[..., ~K & (mark == 1)] = -0.0
    return sum0, wsum0, logits, w


# ---- finalize -----------------------------------------------------------------------------------------------------------------
def finalize_ref(s, ws, R, z0, rows, blend, cast, reset):
    """-> (blended, final, wsum_rows, sum_after, wsum_after): oracle/inference_oracle.py:54-68 on the ring rows (z0 + i) % R, fp32"""
    rr = [(z0 + i) % R for i in range(rows)]
    v, wr = s[:, rr].copy(), ws[rr].copy()
    mask = wr > 0
    if blend == 1:
        with np.errstate(over="ignore"):                    # sums beyond the clip ends: 1e30^2 is inf, as in the kernel
            mag = np.sqrt(v[0] ** 2 + v[1] ** 2 + v[2] ** 2) + np.float32(1e-8)
        for k in range(3):
            v[k][mask] /= mag[mask]
    elif blend == 0:
        v[..., mask] /= wr[mask]
    with np.errstate(invalid="ignore"):
        if cast == 1:
            fin = np.clip((v + np.float32(1.0)) / np.float32(2.0) * np.float32(65535.0), 0, 65535).astype(np.uint16)
        else:
            fin = np.clip(v * np.float32(255.0), 0, 255).astype(np.uint8)
    s_after, w_after = s.copy(), ws.copy()
    if reset >= 1:
        s_after[:, rr] = 0
    if reset == 2:
        w_after[rr] = 0
    return v, fin, wr, s_after, w_after


def check_finalize(got, want, what=""):
    """five arrays each, compared exactly: the floats by their bits (the sign of a zero counts)"""
    names = ("blended", "final", "wsum_out", "sum after", "wsum after")
    for n, g, w in zip(names, got, want):
        if g is None:
            continue
        assert g.shape == w.shape and g.dtype == w.dtype, (what, n, g.shape, w.shape, g.dtype, w.dtype)
        same = (bits(g) == bits(w)) if g.dtype == np.float32 else (g == w)
        assert same.all(), (f"{what}: {n}: {int((~same).sum())} of {same.size} differ, first at "
                            f"{np.unravel_index(np.argmax(~same), same.shape)}: got {g[np.unravel_index(np.argmax(~same), same.shape)]!r}, "
                            f"want {w[np.unravel_index(np.argmax(~same), same.shape)]!r}")


FIN_MODES = [(0, 0, c) for c in (1, 2, 3, 4)] + [(0, 1, c) for c in (1, 2, 3, 4)] + [(2, 0, c) for c in (1, 2, 3, 4)] + \
            [(2, 1, c) for c in (1, 2, 3, 4)] + [(1, 0, 3), (1, 1, 3)]


def _f(name, Y, X, R, z0, rows, reset=2):
    return dict(name=name, Y=Y, X=X, R=R, z0=z0, rows=rows, reset=reset)


def finalize_cases():
    """geometry x reset; every case runs every (blend, cast, c) of FIN_MODES"""
    cases = []
    for reset in (0, 1, 2):
        cases.append(_f(f"plane9x7-reset{reset}", 9, 7, 6, 4, 4, reset))             # 63 voxels: a tail of 3, rows 4, 5, 0, 1
        cases.append(_f(f"plane5x6-reset{reset}", 5, 6, 6, 5, 3, reset))             # 30 voxels: a tail of 2
        cases.append(_f(f"plane12x20-reset{reset}", 12, 20, 6, 4, 4, reset))         # 240 voxels: whole quads
    cases.append(_f("all-rows-off-zero", 9, 7, 5, 3, 5, 1))                          # rows = R, z0 % R != 0
    cases.append(_f("z0-beyond-2R", 5, 6, 5, 13, 3, 2))                              # z0 >= 2R
    cases.append(_f("no-rows", 5, 6, 5, 2, 0, 2))
    cases.append(_f("all-rows-240", 12, 20, 4, 9, 4, 1))
    return cases


def finalize_data(case, blend, cast, c):
    """-> (sum, wsum) fp32 ring accumulators.  Weights 0, 1, 2 and 0.375; sums on both sides of both clip ends; ring row z0 % R
    carries the edge values at weight 1: one fp32 ulp either side of k / 255 and of the uint16 steps 2m / 65535 - 1, values beyond
    both clip ends, a zero vector where wsum > 0; non-zero sums where wsum == 0 occur throughout."""
    rng = np.random.default_rng(sum(ord(ch) for ch in case["name"]) + 7 * blend + 3 * cast + c)
    R, Y, X = case["R"], case["Y"], case["X"]
    ws = rng.integers(0, 4, size=(R, Y, X)).astype(np.float32)
    ws[ws == 3] = 0.375
    s = ((rng.normal(size=(c, R, Y, X)) * 1.5).astype(np.float32) * np.maximum(ws, 1)).astype(np.float32)
    one, up, dn = np.float32(1), np.float32(np.inf), np.float32(-np.inf)
    edge = [np.float32(0), one, -one, np.float32(2), np.float32(-0.5), np.float32(-3), np.float32(1e30), np.float32(-1e30)]
    for k in (1, 2, 127, 128, 254, 255):
        q = np.float32(k) / np.float32(255)
        edge += [q, np.nextafter(q, up), np.nextafter(q, dn)]
    for m in (1, 2, 32767, 32768, 65534):
        q = np.float32(2 * m / 65535 - 1)
        edge += [q, np.nextafter(q, up), np.nextafter(q, dn)]
    edge = np.array(edge, np.float32)
    r = case["z0"] % R
    flat_s, flat_w = s[:, r].reshape(c, -1), ws[r].reshape(-1)
    n = min(edge.size, flat_w.size - 2)
    flat_s[:, :n] = edge[:n]
    flat_w[:n] = 1.0
    flat_s[:, n] = 0.0                                      # a zero vector where wsum > 0
    flat_w[n] = 2.0
    flat_s[:, n + 1] = 0.75                                 # a non-zero sum where wsum == 0
    flat_w[n + 1] = 0.0
    s[:, r], ws[r] = flat_s.reshape(c, Y, X), flat_w.reshape(Y, X)
    return s, ws


def product(*a):
    return list(itertools.product(*a))
