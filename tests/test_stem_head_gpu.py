"""GPU (-m gpu): the stem convolution and the task head -- the two full-resolution ends of the network -- per element against fp64
torch on the CPU, at geometries where a workgroup owns several tiles (stem) or a sample is cut into several chunks (head).  Every
assertion is bit equality on exact integer data (tests/exact_ops.py) or a bound derived from the fp32 error analysis; every
geometry that claims a regime recomputes that regime from the dispatch arithmetic and asserts it, so a later change of a cap
fails here instead of dropping coverage.

Which test reaches which path:
  stem_wgrad_mfma_kernel NB=1 / NB=2, per = 2, a workgroup across a sample boundary   test_stem_tiles[big-*-32|64-*] (16-bit, Cin <= 4)
  stem_fwd_mfma_kernel plain (per = 2, straddling) and STATS (per_s = 3, ragged last block), KSM 2 / 7, output in a channel slice
                                                                                      test_stem_tiles[big-*-32-*] (16-bit, Cin <= 4)
  stem_fwd32_kernel (two 32-channel passes)                                           test_stem_tiles[*-64-*] (16-bit), [*-5-k-32-*]
  stem_fwd_kernel                                                                     test_stem_tiles[*-16-*], every fp32 case
  stem_wgrad_kernel (CQ = 4 / 8 / 16, several voxels per thread)                      test_stem_tiles[big-*-16-*], fp32, Cin = 5
  head_bwd_kernel multi-chunk, ragged last chunk, C = 16 / 48 / 64, ld = 2C           test_head_chunks
  rx_reduce_plan's 512-chunk cap                                                      test_head_chunk_cap
  head_fwd_kernel's second grid-stride pass                                           test_head_fwd_grid_stride
  rx_instnorm_act_head_fwd / rx_instnorm_act_bwd_head, C = 16 / 32 / 64, K = 1..4     test_fused_head_pair
"""
import math
import zlib

import pytest
import torch
import torch.nn.functional as F

from exact_ops import (NAMES5, Guarded, assert_bits, assert_exact_precondition, assert_within, exact_tensor, gamma, half_ulp,
                       poisoned)
from norm_bounds import check_norm_bwd, check_norm_fwd, check_stats, lrelu_mask
from op_bounds import head_dx_ref, head_grads_ref, head_logits_ref

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16, torch.float16]
DW_NAMES = ("co", "ci", "kz", "ky", "kx")
BITS = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.float16: torch.int16}


@pytest.fixture(scope="module")
def ops():
    import mt3d_amd  # noqa: F401
    from mt3d_amd.engine import lib, ops as _ops
    lib.require_device()
    return _ops


def _seed(key):
    return zlib.crc32(repr(key).encode()) % 100000


def rnd16(shape, seed, scale=1.0):
    """normal values representable in bf16, fp16 AND fp32 (rounded to bf16, the few below fp16's normal range set to 0), in fp64:
    one reference then serves the three storage types"""
    g = torch.Generator().manual_seed(seed)
    t = (torch.randn(shape, generator=g) * scale).to(torch.bfloat16).double()
    t = torch.where(t.abs() < 2.0 ** -14, torch.zeros_like(t), t)
    assert torch.equal(t.to(torch.float16).double(), t)
    return t


def rnd32(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).double()


def to_act(ops, x_ncdhw, dtype, ld=None, c0=0):
    """NCDHW fp64 (values representable in dtype) -> device Act, optionally a channel slice of a wider buffer"""
    n, c, z, y, x = x_ncdhw.shape
    ld = c if ld is None else ld
    buf = torch.full((n, z, y, x, ld), 7.0, dtype=dtype, device="cuda")
    buf[..., c0:c0 + c] = x_ncdhw.permute(0, 2, 3, 4, 1).to(dtype).cuda()
    return ops.Act(buf, c0, c)


def ncdhw(act):
    return act.tensor().permute(0, 4, 1, 2, 3)


# The big stem tensors have 15 M elements; the comparison runs on the device and exact_ops' assert only has to speak (with the
# coordinates of the first wrong elements) when it fails.
def fast_bits(got, want, dtype, what, names=NAMES5):
    w = want.to(torch.float32).to(dtype).to(got.device)
    if got.dtype == dtype and got.shape == w.shape and torch.equal(got, w):       # (NaN is never equal; -0 == +0 as in assert_bits)
        return
    assert_bits(got, want, dtype, what, names)


def fast_within(got, ref, bound, what, names=NAMES5):
    if got.shape == ref.shape and ((got.double() - ref.to(got.device)).abs() <= bound.to(got.device)).all():
        return
    assert_within(got, ref, bound, what, names)


class Out:
    """an output activation in one of the layouts the plan uses: dense (ld == c, NaN-poisoned) or one half of a 2c-channel region
    between guard channels, the other half pre-filled with a per-channel pattern that must come back bit-unchanged"""

    def __init__(self, ops, n, dims, c, dtype, layout):
        self.g = None
        if layout == "dense":
            self.act = ops.Act(poisoned((n, *dims, c), dtype))
            return
        half = {"lo": 0, "hi": 1}[layout]
        self.g = g = Guarded(n, dims, 2 * c, dtype)                     # NaN over both halves
        self.o0 = g.c0 + (1 - half) * c
        g.buf[..., self.o0:self.o0 + c] = ((torch.arange(c, dtype=torch.float64) - 7.0) * 0.25).to(dtype).cuda()
        self.other = g.buf[..., self.o0:self.o0 + c].clone()
        self.act = ops.Act(g.buf, g.c0 + half * c, c)

    def check(self, what):
        if self.g is None:
            return
        self.g.check(what)                                               # guard bands intact, nothing left NaN
        now = self.g.buf[..., self.o0:self.o0 + self.act.c]
        b = BITS[now.dtype]
        assert torch.equal(now.contiguous().view(b), self.other.view(b)), f"{what}: the other half of the buffer was written"


LAYOUTS = ("dense", "lo", "hi")


def in_layout(ops, t, dtype, layout):
    c = t.shape[1]
    if layout == "dense":
        return to_act(ops, t, dtype)
    return to_act(ops, t, dtype, ld=2 * c, c0=c if layout == "hi" else 0)


# ---- stem -------------------------------------------------------------------------------------------------------------------
GEOMS = {"big": (3, (18, 42, 104)), "one": (2, (6, 9, 10))}
_STEM = {}


def cdiv(a, b):
    return -(-a // b)


def stem_regime(n, dims, co):
    """the dispatch arithmetic of rx_stem_wgrad_mfma_try / rx_stem_fwd_mfma_try / rx_stem_conv_bwd_weight, recomputed"""
    z, y, x = dims
    NT = n * cdiv(z, 4) * cdiv(y, 4) * cdiv(x, 16)             # 4x4x16 tiles
    NTs = NT // n
    wb = min(NT, 1024, 768)                                     # weight gradient: RX_STEM_CHUNKS partial rows, 768 workgroups
    w_per = cdiv(NT, wb)
    fb = min(NT, 1024)                                          # forward: 1024 workgroups
    f_per = cdiv(NT, fb)
    bps = max(cdiv(NT, f_per) // n, 1)                          # STATS: whole blocks per sample
    per_s = cdiv(NTs, bps)
    vpb = 256 // (co // 4)                                      # VALU weight gradient: voxels per pass of a workgroup
    chunk = cdiv(cdiv(n * z * y * x, 1024), vpb) * vpb
    return dict(NT=NT, NTs=NTs, w_per=w_per, w_blocks=cdiv(NT, w_per), f_per=f_per, per_s=per_s, bps=cdiv(NTs, per_s),
                valu_passes=chunk // vpb)


def stem_ref(geom, cin, k, co):
    key = (geom, cin, k, co)
    if key in _STEM:
        return _STEM[key]
    _STEM.clear()                                               # one reference at a time (the three dtypes of a case share it)
    n, dims = GEOMS[geom]
    V, taps, pad = math.prod(dims), math.prod(k), [(kk - 1) // 2 for kk in k]
    sd = _seed(("stem2",) + key)
    wgrad = lambda x_, g_: torch.nn.grad.conv3d_weight(x_, (co, cin, *k), g_, padding=pad)          # noqa: E731
    # exact pass: integer image, dyadic weights / bias / dy
    xe = exact_tensor((n, cin, *dims), sd, -4, 4, 0.5, 2.0 ** -2)
    we = exact_tensor((co, cin, *k), sd + 1, -4, 4, 0.5, 2.0 ** -3)
    be = exact_tensor((co,), sd + 2, -16, 16, 1.0, 2.0 ** -5)
    ge = exact_tensor((n, co, *dims), sd + 3, -4, 4, 0.5, 2.0 ** -2)
    assert_exact_precondition(None, (xe, we), 2.0 ** -5, terms=cin * taps, extra=be, what="stem y")
    assert_exact_precondition(wgrad, (xe, ge), 2.0 ** -4, terms=n * V, out16=False, what="stem dw")
    ye, dwe = F.conv3d(xe, we, be, padding=pad), wgrad(xe, ge)
    assert torch.equal(ye.float().double(), ye) and torch.equal(dwe.float().double(), dwe)
    # random pass: image, weights and dy representable in every storage type (the MFMA kernels convert the weights to it)
    xr, wr, br = rnd16((n, cin, *dims), sd + 4), rnd16((co, cin, *k), sd + 5, 0.3), rnd32((co,), sd + 6).float().double()
    gr = rnd16((n, co, *dims), sd + 7)
    yr, dwr = F.conv3d(xr, wr, br, padding=pad), wgrad(xr, gr)
    e_y = gamma(cin * taps + 1) * F.conv3d(xr.abs(), wr.abs(), br.abs(), padding=pad)
    e_dw = gamma(n * V) * wgrad(xr.abs(), gr.abs())
    r = _STEM[key] = dict(xe=xe, we=we, be=be, ge=ge, ye=ye, dwe=dwe, xr=xr, wr=wr, br=br, gr=gr, yr=yr, dwr=dwr, e_y=e_y, e_dw=e_dw,
                          b_y={})
    return r


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("co", [32, 64, 16])
@pytest.mark.parametrize("cin,k", [(1, (3, 3, 3)), (3, (1, 3, 3)),        # K = Cin * taps <= 32: KSM = 2
                                   (2, (3, 3, 3)), (4, (3, 3, 3)),        # K = 54 / 108: KSM = 7
                                   (5, (3, 3, 3))])                       # more than 4 input channels: the VALU kernels
@pytest.mark.parametrize("geom", ["big", "one"])
def test_stem_tiles(ops, dtype, geom, cin, k, co):
    n, dims = GEOMS[geom]
    g = stem_regime(n, dims, co)
    if geom == "big":
        # 1155 tiles, ragged on all three axes; 385 per sample is odd, so with two tiles per workgroup one workgroup owns the last
        # tile of a sample and the first of the next
        assert g["NT"] == 1155 and g["NTs"] == 385
        assert g["w_per"] >= 2 and g["w_blocks"] == 578, g            # weight gradient: accumulators persist over two tiles
        assert g["f_per"] >= 2, g                                     # plain forward
        assert any((s * g["NTs"]) % g["w_per"] for s in range(1, n)) and any((s * g["NTs"]) % g["f_per"] for s in range(1, n)), g
        assert g["per_s"] >= 2 and g["NTs"] % g["per_s"] != 0 and g["bps"] == 129, g      # STATS: ragged last block per sample
        assert g["valu_passes"] >= 2, g                               # VALU weight gradient: several voxels per thread
    else:
        assert g["w_per"] == 1 and g["f_per"] == 1 and g["per_s"] == 1, g
    r = stem_ref(geom, cin, k, co)
    tag = f"{geom} cin={cin} k={k} co={co}"
    if dtype not in r["b_y"]:
        r["b_y"][dtype] = r["e_y"] + half_ulp(r["yr"].abs() + r["e_y"], dtype)
    xe, xr = r["xe"].float().cuda().contiguous(), r["xr"].float().cuda().contiguous()
    we, be = r["we"].float().cuda(), r["be"].float().cuda()
    wr, br = r["wr"].float().cuda(), r["br"].float().cuda()
    checked = []
    for layout in LAYOUTS:
        what = f"stem {tag} {layout}"
        # exact pass: y of both entry points rounded once and equal to each other, dw bit for bit
        ya, yb = Out(ops, n, dims, co, dtype, layout), Out(ops, n, dims, co, dtype, layout)
        ops.stem_conv_fwd(xe, we, be, ya.act, k)
        ops.stem_conv_fwd_stats(xe, we, be, yb.act, k, poisoned((n, co, 2)))
        for yy, nm in ((ya, "fwd"), (yb, "fwd_stats")):
            yy.check(f"{what} y ({nm})")
            fast_bits(ncdhw(yy.act), r["ye"], dtype, f"{what} y ({nm}, exact data)")
        assert torch.equal(ya.act.tensor(), yb.act.tensor()), f"{what}: fwd and fwd_stats differ"
        dw = poisoned((co, cin, *k))
        ops.stem_conv_bwd_weight(xe, in_layout(ops, r["ge"], dtype, layout), dw, k)
        assert_bits(dw, r["dwe"], torch.float32, f"{what} dw (exact data)", names=DW_NAMES)
        # random pass: per element within the fp32 summation bound
        ya, yb = Out(ops, n, dims, co, dtype, layout), Out(ops, n, dims, co, dtype, layout)
        st_f, st_s = poisoned((n, co, 2)), poisoned((n, co, 2))
        ops.stem_conv_fwd(xr, wr, br, ya.act, k)
        ops.stem_conv_fwd_stats(xr, wr, br, yb.act, k, st_f)
        for yy, nm in ((ya, "fwd"), (yb, "fwd_stats")):
            yy.check(f"{what} y ({nm})")
            fast_within(ncdhw(yy.act), r["yr"], r["b_y"][dtype], f"{what} y ({nm})")
        assert torch.equal(ya.act.tensor(), yb.act.tensor()), f"{what}: fwd and fwd_stats differ"
        ops.instnorm_stats(yb.act, st_s)
        assert torch.allclose(st_f, st_s, rtol=2e-5, atol=2e-6), (what, (st_f - st_s).abs().max().item())
        # (mean, rstd) against the values as stored; the same y bits with the same statistics bits are checked once
        for st in (st_f, st_s):
            if any(torch.equal(yb.act.tensor(), y0) and torch.equal(st, s0) for y0, s0 in checked):
                continue
            check_stats(st, ncdhw(yb.act).double().cpu(), what=f"{what} stats")
            checked.append((yb.act.tensor().clone(), st.clone()))
        dw = poisoned((co, cin, *k))
        ops.stem_conv_bwd_weight(xr, in_layout(ops, r["gr"], dtype, layout), dw, k)
        assert_within(dw, r["dwr"], r["e_dw"], f"{what} dw", names=DW_NAMES)


# ---- head -------------------------------------------------------------------------------------------------------------------
def reduce_plan(V, C, per16):
    """rx_reduce_plan (rx_reduce.h), recomputed: (chunks wanted before the cap, nchunks, chunk_vox)"""
    vp = max(256 // (C // per16), 1)
    want = max(V // (vp * 8), 1)
    nch = min(want, 512)
    cvx = cdiv(cdiv(V, nch), vp) * vp
    return want, cdiv(V, cvx), cvx


def per16(dtype):
    return 4 if dtype == torch.float32 else 8


_HEAD = {}


def head_ref(n, c, k, dims, exact_only=False, fwd_only=False):
    key = (n, c, k, dims)
    if key in _HEAD:
        return _HEAD[key]
    _HEAD.clear()
    V = math.prod(dims)
    sd = _seed(("head2",) + key)
    xe = exact_tensor((n, c, *dims), sd, -4, 4, 0.5, 2.0 ** -2)
    we = exact_tensor((k, c), sd + 1, -4, 4, 0.5, 2.0 ** -3)
    be = exact_tensor((k,), sd + 2, -16, 16, 1.0, 2.0 ** -5)
    assert_exact_precondition(None, (xe, we), 2.0 ** -5, terms=c, extra=be, out16=False, what="logits")
    r = dict(xe=xe, we=we, be=be, le=torch.einsum("nczyx,kc->nkzyx", xe, we) + be.view(1, k, 1, 1, 1))
    if not fwd_only:
        ge = exact_tensor((n, k, *dims), sd + 3, -4, 4, 0.5, 2.0 ** -2)
        assert_exact_precondition(None, (ge, we), 2.0 ** -5, terms=k, what="head dx")
        assert_exact_precondition(None, (ge, xe), 2.0 ** -4, terms=n * V, out16=False, what="head dw")
        r.update(ge=ge, dxe=torch.einsum("nkzyx,kc->nczyx", ge, we), dwe=torch.einsum("nkzyx,nczyx->kc", ge, xe), dbe=ge.sum((0, 2, 3, 4)))
    if not exact_only:
        xr, wr, br, gr = rnd16((n, c, *dims), sd + 4), rnd32((k, c), sd + 5, 0.3).float().double(), rnd32((k,), sd + 6).float().double(), \
            rnd32((n, k, *dims), sd + 7).float().double()
        r.update(xr=xr, wr=wr, br=br, gr=gr,
                 lr=torch.einsum("nczyx,kc->nkzyx", xr, wr) + br.view(1, k, 1, 1, 1),
                 e_l=gamma(c + 1) * (torch.einsum("nczyx,kc->nkzyx", xr.abs(), wr.abs()) + br.abs().view(1, k, 1, 1, 1)),
                 dxr=torch.einsum("nkzyx,kc->nczyx", gr, wr), e_dx=gamma(k) * torch.einsum("nkzyx,kc->nczyx", gr.abs(), wr.abs()),
                 dwr=torch.einsum("nkzyx,nczyx->kc", gr, xr), e_dw=gamma(n * V) * torch.einsum("nkzyx,nczyx->kc", gr.abs(), xr.abs()),
                 dbr=gr.sum((0, 2, 3, 4)), e_db=gamma(n * V) * gr.abs().sum((0, 2, 3, 4)))
    _HEAD[key] = r
    return r


def head_exact_pass(ops, r, dtype, layout, what, dx_guarded=True):
    """logits, dw, db (fp32) bit for bit, dx rounded once, on the exact data of `r`"""
    n, c = r["xe"].shape[:2]
    k, dims = r["we"].shape[0], tuple(r["xe"].shape[2:])
    xa = in_layout(ops, r["xe"], dtype, layout)
    w, b, g = r["we"].float().cuda(), r["be"].float().cuda(), r["ge"].float().cuda().contiguous()
    lg = poisoned((n, k, *dims))
    ops.head_fwd(xa, w, b, lg)
    fast_bits(lg, r["le"], torch.float32, f"{what} logits (exact data)")
    dx, dw, db = Guarded(n, dims, c, dtype), poisoned((k, c)), poisoned((k,))
    ops.head_bwd(g, xa, w, dx.act(ops), dw, db)
    dx.check(f"{what} dx")
    fast_bits(dx.ncdhw(), r["dxe"], dtype, f"{what} dx (exact data)")
    assert_bits(dw, r["dwe"], torch.float32, f"{what} dw (exact data)", names=("k", "c"))
    assert_bits(db, r["dbe"], torch.float32, f"{what} db (exact data)", names=("k",))
    dw2, db2 = poisoned((k, c)), poisoned((k,))
    ops.head_bwd(g, xa, w, None, dw2, db2)                                  # without a data gradient: the same parameter gradients
    assert_bits(dw2, r["dwe"], torch.float32, f"{what} dw (dx = None, exact data)", names=("k", "c"))
    assert_bits(db2, r["dbe"], torch.float32, f"{what} db (dx = None, exact data)", names=("k",))


HEAD_DIMS = [(12, 20, 24),      # 5760 voxels: several chunks at every width (asserted below)
             (11, 19, 23),      # 4807 voxels: no multiple of any chunk length, so the last chunk is ragged at every width
             (5, 7, 9)]         # 315 voxels: one chunk


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("k", [1, 3, 17])
@pytest.mark.parametrize("c", [16, 32, 48, 64])      # 48: CV = 6 / 12 channel vectors, a non-power-of-two split of the 256 threads
@pytest.mark.parametrize("dims", HEAD_DIMS)
def test_head_chunks(ops, dtype, dims, c, k):
    n, V = 2, math.prod(dims)
    _, nch, cvx = reduce_plan(V, c, per16(dtype))
    if dims == (12, 20, 24):
        assert nch >= 2, (nch, cvx)
        if c == 32:
            assert nch == (10 if dtype != torch.float32 else 20)
    elif dims == (11, 19, 23):
        assert nch >= 2 and V % cvx != 0, (nch, cvx)                 # ragged last chunk
    else:
        assert nch == (2 if (c, dtype) == (64, torch.float32) else 1)    # (16 channel vectors: 16 voxels per pass, 315 / 128 = 2)
    r = head_ref(n, c, k, dims)
    for layout in ("dense", "lo", "hi"):
        what = f"head c={c} k={k} {dims} {layout}"
        head_exact_pass(ops, r, dtype, layout, what)
        xa = in_layout(ops, r["xr"], dtype, layout)
        w, b, g = r["wr"].float().cuda(), r["br"].float().cuda(), r["gr"].float().cuda().contiguous()
        lg = poisoned((n, k, *dims))
        ops.head_fwd(xa, w, b, lg)
        assert_within(lg, r["lr"], r["e_l"], f"{what} logits")
        dx, dw, db = Guarded(n, dims, c, dtype), poisoned((k, c)), poisoned((k,))
        ops.head_bwd(g, xa, w, dx.act(ops), dw, db)
        dx.check(f"{what} dx")
        assert_within(dx.ncdhw(), r["dxr"], r["e_dx"] + half_ulp(r["dxr"].abs() + r["e_dx"], dtype), f"{what} dx")
        assert_within(dw, r["dwr"], r["e_dw"], f"{what} dw", names=("k", "c"))
        assert_within(db, r["dbr"], r["e_db"], f"{what} db", names=("k",))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("dims", [(64, 64, 65),      # 266 240 voxels: more chunks wanted than the cap gives, ragged last chunk
                                  (64, 64, 72)])     # 294 912 = 512 * 576 voxels: exactly 512 chunks after the cap
def test_head_chunk_cap(ops, dtype, dims):
    n, c, k, V = 1, 32, 3, math.prod(dims)
    want, nch, cvx = reduce_plan(V, c, per16(dtype))
    assert want > 512, want                                          # rx_reduce_plan's cap is what sets the chunk length
    if dims == (64, 64, 65):
        # 520 (16-bit) / 1040 (fp32) chunks wanted; the cap gives 520 voxels per chunk, rounded up to whole passes of VP voxels
        # (576 / 544), which leaves 463 / 490 chunks, the last one ragged
        assert (want, nch, cvx) == ((520, 463, 576) if dtype != torch.float32 else (1040, 490, 544)) and V % cvx != 0
    else:
        assert nch == 512 and cvx == 576
    r = head_ref(n, c, k, dims, exact_only=True)
    head_exact_pass(ops, r, dtype, "dense", f"head cap {dims}")


def test_head_fwd_grid_stride(ops):
    """head_fwd_kernel's grid is capped at 4096 workgroups of 256 voxels; past 1 048 576 voxels a thread takes a second voxel"""
    from mt3d_amd.engine import lib
    dtype, n, c, k, dims = torch.bfloat16, 1, 32, 3, (104, 104, 100)
    V = math.prod(dims)
    G = min(cdiv(V, 256), 4096)
    assert G == 4096 and V > G * 256                                 # a second grid-stride pass
    r = head_ref(n, c, k, dims, exact_only=True, fwd_only=True)
    xa = to_act(ops, r["xe"], dtype)
    w, b = r["we"].float().cuda(), r["be"].float().cuda()
    lg = poisoned((n, k, *dims))
    ops.head_fwd(xa, w, b, lg, lib.RX_ACT_NONE)
    fast_bits(lg, r["le"], torch.float32, "head fwd 1M voxels logits (exact data)")
    sm = poisoned((n, k, *dims))
    ops.head_fwd(xa, w, b, sm, lib.RX_ACT_SOFTMAX)
    want = torch.softmax(r["le"], 1)
    ulp = torch.exp2(torch.floor(torch.log2(want)) - 23)             # an ulp of fp32 at the reference
    fast_within(sm, want, 8 * ulp, "head fwd 1M voxels softmax")


# ---- the fused pair under a head ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("slope", [0.01, 1.0])
@pytest.mark.parametrize("k", [1, 2, 3, 4])
@pytest.mark.parametrize("c", [16, 32, 64])
def test_fused_head_pair(ops, dtype, c, k, slope):
    """rx_instnorm_act_head_fwd == rx_instnorm_act_fwd + rx_head_fwd and rx_instnorm_act_bwd_head == rx_head_bwd + rx_instnorm_act_bwd,
    bit for bit where they state it; logits, dw and db of BOTH against fp64 products with the activated output as stored"""
    n, dims = 2, (12, 20, 24)
    V = math.prod(dims)
    assert reduce_plan(V, c, 8)[1] >= 2                              # several chunks in the reduce pass
    sd = _seed(("fused", c, k, slope))
    y = to_act(ops, rnd16((n, c, *dims), sd), dtype)
    w64, b64 = rnd32((k, c), sd + 1, 0.3).float().double(), rnd32((k,), sd + 2).float().double()
    d64 = rnd32((n, k, *dims), sd + 3, 0.01).float().double()
    w, b, dout = w64.float().cuda(), b64.float().cuda(), d64.float().cuda().contiguous()
    what = f"fused c={c} k={k} slope={slope}"
    stats = poisoned((n, c, 2))
    ops.instnorm_stats(y, stats)
    # forward
    o1, o2 = ops.Act(poisoned((n, *dims, c), dtype)), ops.Act(poisoned((n, *dims, c), dtype))
    l1, l2, l3 = poisoned((n, k, *dims)), poisoned((n, k, *dims)), poisoned((n, k, *dims))
    ops.instnorm_act_fwd(y, stats, o1, slope)
    ops.head_fwd(o1, w, b, l1)
    ops.instnorm_act_head_fwd(y, stats, o2, w, b, l2, 0, slope)
    ops.instnorm_act_head_fwd(y, stats, None, w, b, l3, 0, slope)        # nobody needs the activated output: not stored
    assert torch.equal(o1.t, o2.t), f"{what}: activated output differs from the two calls"
    assert torch.equal(l2, l3), f"{what}: logits depend on whether the output is stored"
    check_norm_fwd(o1, y, stats, None, slope, dtype, f"{what} out")
    a = ncdhw(o1).double().cpu()                                      # the activated output as stored
    want, e = head_logits_ref(a, w64, b64)
    for lg, nm in ((l1, "head_fwd"), (l2, "fused")):
        assert_within(lg, want, e, f"{what} logits ({nm})")
    # backward
    g = ops.Act(poisoned((n, *dims, c), dtype))
    dw1, db1 = poisoned((k, c)), poisoned((k,))
    dy1, dy2, dy3 = (ops.Act(poisoned((n, *dims, c), dtype)) for _ in range(3))
    ops.head_bwd(dout, o1, w, g, dw1, db1)
    ops.instnorm_act_bwd(g, y, stats, None, dy1, slope)
    dw2, db2 = poisoned((k, c)), poisoned((k,))
    ops.head_bwd(dout, o1, w, None, dw2, db2)
    ops.instnorm_act_bwd_head(dout, w, y, stats, dy2, slope)
    dw3, db3 = poisoned((k, c)), poisoned((k,))
    ops.instnorm_act_bwd_head(dout, w, y, stats, dy3, slope, dw=dw3, db=db3)
    assert torch.equal(dy1.t, dy2.t) and torch.equal(dy3.t, dy2.t), f"{what}: dy differs from the two calls"
    assert torch.equal(dw1, dw2) and torch.equal(db1, db2), f"{what}: head_bwd's dw / db depend on dx"
    dw_ref, db_ref, e_dw, e_db = head_grads_ref(d64, a)
    for dw, db, nm in ((dw1, db1, "head_bwd"), (dw3, db3, "fused")):
        assert_within(dw, dw_ref, e_dw, f"{what} dw ({nm})", names=("k", "c"))
        assert_within(db, db_ref, e_db, f"{what} db ({nm})", names=("k",))
    # dy: g = dout x w is an fp32 sum of k products (gamma_k of the magnitudes), rounded into the storage type (half an ulp)
    g_un, d_g = head_dx_ref(d64, w64, dtype)
    assert_within(ncdhw(g), g_un, d_g, f"{what} g")
    mask = lrelu_mask(None, y, stats, slope)
    check_norm_bwd((dy1, dy2, dy3), g_un, y, stats, mask, slope, dtype, f"{what} dy", d_g=d_g)


def test_head_widths_the_library_refuses(ops):
    """the widths these kernels do not take are refused with a message, not computed: the fused forward wants C / 8 to divide 64 (the
    lanes of a voxel hand their sums along inside one wave), which excludes 48 -- the plan asks the same before it fuses
    (engine/plan.py::_fuse_head) -- and rx_head_bwd wants at least 16 channels"""
    from mt3d_amd.engine.lib import RxError
    n, dims, k = 1, (4, 4, 4), 3
    w, b = torch.zeros((k, 48), device="cuda"), torch.zeros((k,), device="cuda")
    y = ops.Act.zeros(n, *dims, 48, torch.bfloat16)
    stats = torch.zeros((n, 48, 2), device="cuda")
    with pytest.raises(RxError, match="rx_instnorm_act_head_fwd: 16-bit types, K <= 4, C / 8 dividing 64"):
        ops.instnorm_act_head_fwd(y, stats, None, w, b, poisoned((n, k, *dims)), 0, 0.01)
    x8 = ops.Act.zeros(n, *dims, 8, torch.bfloat16)
    with pytest.raises(RxError, match="rx_head_bwd: 1 <= K <= 1024"):
        ops.head_bwd(torch.zeros((n, k, *dims), device="cuda"), x8, torch.zeros((k, 8), device="cuda"), None, poisoned((k, 8)), poisoned((k,)))
