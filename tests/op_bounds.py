"""Per-element bounds of the convolution, head and pooling kernels (a plain module, imported by the op test files and by
tests/plan_audit.py): each function restates one fp32 error analysis once, so that an op test and the per-launch audit of a whole
plan hold a kernel to the same bound.  The InstanceNorm family has its own module, tests/norm_bounds.py."""
import torch
import torch.nn.functional as F

from exact_ops import U32, assert_within, gamma, half_ulp


# ---- convolutions ---------------------------------------------------------------------------------------------------------------
def check(got, ref, a, terms, dtype, what, names=("n", "c", "z", "y", "x")):
    """|got - ref| <= gamma(terms - 1 [+ 1 in fp32 mode]) * sum|a b|, then half an ulp of the storage type"""
    e = gamma(terms - 1 + (dtype == torch.float32)) * a
    out16 = got.dtype != torch.float32
    assert_within(got, ref, e + (half_ulp(ref.abs() + e, dtype) if out16 else 0), what, names=names)


def check_m12(m12, g, xh, slope, dtype, what):
    """the two backward means an epilogue leaves behind (rx_conv3d_bwd_data_instats), per (n, c), against the fp64 sums over the
    stored gradient g (fp64 NCDHW) and xhat: fp32 sums of V terms -> gamma_V (+ 6u for xhat and the products) of the sums of
    magnitudes; the epilogue may sum g' before its rounding into the storage type: half an ulp of each term more"""
    g = torch.where(xh > 0, g, g * slope)
    want = torch.stack([g.mean((2, 3, 4)), (g * xh).mean((2, 3, 4))], -1)
    V = g[0, 0].numel()
    hu = half_ulp(g.abs(), dtype)
    bnd = torch.stack([g.abs().mean((2, 3, 4)), (g * xh).abs().mean((2, 3, 4))], -1) * (gamma(V) + 6 * U32) + \
        torch.stack([hu.mean((2, 3, 4)), (hu * xh.abs()).mean((2, 3, 4))], -1)
    assert_within(m12, want, bnd, what, names=("n", "c", "m"))


# ---- task head (fp64 NCDHW operands; a: the activated input as stored) ------------------------------------------------------------
def head_logits_ref(a, w64, b64):
    """(logits, bound): an fp32 sum of c products and the bias, gamma_(c+1) of the magnitudes (the logits are fp32: no rounding)"""
    k, c = w64.shape
    bb = b64.view(1, k, 1, 1, 1)
    want = torch.einsum("nczyx,kc->nkzyx", a, w64) + bb
    e = gamma(c + 1) * (torch.einsum("nczyx,kc->nkzyx", a.abs(), w64.abs()) + bb.abs())
    return want, e


def head_grads_ref(d64, a):
    """(dw, db, bound of dw, bound of db): fp32 sums of n * V terms in some order"""
    nV = d64.shape[0] * d64[0, 0].numel()
    dw_ref, db_ref = torch.einsum("nkzyx,nczyx->kc", d64, a), d64.sum((0, 2, 3, 4))
    e_dw, e_db = gamma(nV) * torch.einsum("nkzyx,nczyx->kc", d64.abs(), a.abs()), gamma(nV) * d64.abs().sum((0, 2, 3, 4))
    return dw_ref, db_ref, e_dw, e_db


def head_dx_ref(d64, w64, dtype):
    """(g, bound): g = dout x w is an fp32 sum of k products (gamma_k of the magnitudes), rounded into the storage type (half an
    ulp)"""
    k = w64.shape[0]
    g_un = torch.einsum("nkzyx,kc->nczyx", d64, w64)
    e_g = gamma(k) * torch.einsum("nkzyx,kc->nczyx", d64.abs(), w64.abs())
    return g_un, e_g + half_ulp(g_un.abs() + e_g, dtype)


# ---- average pooling ---------------------------------------------------------------------------------------------------------------
def pool_fwd_bound(x, s):
    """an fp32 sum of K terms, the scale 1/K and its product"""
    K = s[0] * s[1] * s[2]
    return (gamma(K) + 2 * U32) * F.avg_pool3d(x.abs(), s, s)


def pool_bwd_bound(de, old=None):
    """dx = g / K (`de`): fl(1/K) and the product each err by u relative; dx += adds one fp32 rounding of the sum old + de"""
    return 2.0001 * U32 * de.abs() + (U32 * (old + de).abs() if old is not None else 0)
