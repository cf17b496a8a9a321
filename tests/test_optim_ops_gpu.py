"""GPU (-m gpu): the C entries of rx_pack_optim.hip one by one -- rx_adamw_pack, rx_adamw_flat, rx_adamw_flat_multi and
rx_grad_norm_clip -- and EngineAdamW's step bookkeeping, each output held per element to the fp32 error bound of
tests/adamw_ref.py around an fp64 AdamW evaluated from the device's own previous (p, m, v).  Every tensor sits between sentinel
fences inside a larger buffer; outputs that a call must write completely are NaN-filled first."""
import copy
import ctypes
from ctypes import c_void_p

import pytest
import torch

from adamw_ref import CLIP, HYPERS, RATIOS, adam_args, check_step, f32, make_inputs, next_grad
from exact_ops import U32, _report

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16, torch.float32]
BITS = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.float16: torch.int16}


@pytest.fixture(scope="module")
def L():
    import mt3d_amd  # noqa: F401
    from mt3d_amd.engine import lib
    lib.require_device()
    return lib


def _ptr(t):
    return c_void_p(t.data_ptr()) if t is not None else c_void_p(0)


def _sync():
    torch.cuda.synchronize()


class Arena:
    """tensors of `sizes` elements inside ONE device buffer, each 64-byte aligned (plus `shifts[i]` elements) with at least `pad`
    sentinel elements on both sides; check() holds every element outside the tensors to its bits"""

    def __init__(self, sizes, dtype=torch.float32, shifts=None, pad=64):
        offs, o = [], pad
        for i, n in enumerate(sizes):
            o = (o + 31) // 32 * 32 + (shifts[i] if shifts else 0)
            offs.append(o)
            o += n + pad
        self.buf = (-(97 + torch.arange(o, device="cuda") % 128)).to(dtype)                    # integers up to 224: exact in bf16
        inside = torch.zeros(o + 1, dtype=torch.int32)
        for off, n in zip(offs, sizes):
            inside[off] += 1
            inside[off + n] -= 1
        self.guard = (inside[:o].cumsum(0) == 0).cuda()
        self.buf[~self.guard] = float("nan")
        self.views = [self.buf[off:off + n] for off, n in zip(offs, sizes)]
        self.snap = self.buf.clone()

    def check(self, what):
        b = BITS[self.buf.dtype]
        bad = (self.buf.view(b) != self.snap.view(b)) & self.guard
        assert not bad.any(), _report(f"{what}: fence written", bad.cpu(), self.buf.double().cpu(), self.snap.double().cpu(), ("offset",))

    def bits(self):
        return self.buf.view(BITS[self.buf.dtype]).clone()


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(BITS[a.dtype]), b.contiguous().view(BITS[b.dtype]))


def _dev_clip(with_clip):
    """(device scalar or None, the fp32 value it holds or None)"""
    if not with_clip:
        return None, None
    t = torch.tensor([CLIP], dtype=torch.float32, device="cuda")
    return t, t.item()


def _print_ratios(key):
    r = RATIOS.get(key)
    if r:
        print(f"{key}: largest error / bound p' {r[0]:.3f} m' {r[1]:.3f} v' {r[2]:.3f}")


# ---- 3a rx_adamw_pack ------------------------------------------------------------------------------------------------------------
# (kind, A, B, taps, w_bwd given): the 16-byte path; convT; TT == 1; ragged tiles of multiples of 8; not multiples of 8; below one
# tile; 2-D 3x3 over several tiles; convT ragged; the 16-byte path of a forward-only plan (w_bwd NULL)
PACK_CASES = [(0, 64, 32, 27, True), (1, 32, 64, 8, True), (0, 64, 32, 1, True), (0, 40, 24, 27, True), (0, 33, 31, 3, True),
              (0, 16, 16, 27, True), (0, 96, 64, 9, True), (1, 24, 40, 4, True), (0, 64, 32, 27, False)]
START_STEPS = (1, 1000, 200000, 2)


def _expect_packs(pnew, kind, A, B, taps):
    """fp32 (w_fwd [T][Co][Ci], w_bwd [T][Ci][Co]): the plain permutation of the weight (A, B, T)"""
    w = pnew.view(A, B, taps)
    same, swp = w.permute(2, 0, 1).contiguous(), w.permute(2, 1, 0).contiguous()
    return (same, swp) if kind == 0 else (swp, same)


def _assert_pack(got, src, dtype, what, names):
    """got (NaN before the call) is bit for bit `src` (fp32, already permuted) cast to dtype"""
    got, want = got.view(src.shape), src.to(dtype)
    nan = torch.isnan(got)
    assert not nan.any(), _report(f"{what}: left unwritten (NaN)", nan.cpu(), got.double().cpu(), want.double().cpu(), names)
    bad = got.view(BITS[dtype]) != want.view(BITS[dtype])
    assert not bad.any(), _report(f"{what}: not the permutation of p' cast to {dtype} (bound column: p' in fp32)", bad.cpu(),
                                  got.double().cpu(), want.double().cpu(), names, extra=src.double().cpu())


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[-1])
@pytest.mark.parametrize("ci", range(len(PACK_CASES)), ids=lambda i: "k%d_%dx%dx%d%s" % (PACK_CASES[i][:4] + ("" if PACK_CASES[i][4] else "_nobwd",)))
def test_adamw_pack_per_element(L, dtype, ci):
    """three consecutive rx_adamw_pack calls: p', m', v' per element inside the bound, grad untouched, both packed copies bit-equal
    to the permutation of the device's own p', fences intact; then taps = 28 and step = 0 are refused and write nothing"""
    kind, A, B, taps, with_bwd = PACK_CASES[ci]
    hyper, start = HYPERS[ci % 3], START_STEPS[ci % 4]
    clip_t, clip = _dev_clip(ci % 2 == 1 or ci == 0)
    n = A * B * taps
    p0, g0, m0, v0 = make_inputs(n, 40 + ci, start, hyper)
    f = Arena([n, n, n, n])
    p, g, m, v = f.views
    for dst, src in zip((p, g, m, v), (p0, g0, m0, v0)):
        dst.copy_(src)
    packs = Arena([n, n], dtype)
    wf, wb = packs.views[0], (packs.views[1] if with_bwd else None)
    code = L.DTYPE_CODE[dtype]
    what = "adamw_pack"

    def call(step, t=taps):
        rc = L.load().rx_adamw_pack(code, _ptr(p), _ptr(g), _ptr(m), _ptr(v), _ptr(clip_t), *hyper, step, kind, A, B, t, _ptr(wf), _ptr(wb),
                                    L.stream_ptr())
        _sync()
        return rc

    for k in range(3):
        if k:
            g.copy_(next_grad(n, 40 + ci, k))
        for w in packs.views:
            w.fill_(float("nan"))
        before, gbits = (p.cpu(), m.cpu(), v.cpu()), g.view(torch.int32).clone()
        L.check(call(start + k), "rx_adamw_pack")
        check_step((p, m, v), before, g.cpu(), clip, adam_args(*hyper, start + k), f"{what}: case {ci} {dtype} step {start + k}")
        assert torch.equal(g.view(torch.int32), gbits), "grad written"
        ef, eb = _expect_packs(p, kind, A, B, taps)
        _assert_pack(wf, ef, dtype, f"{what}: case {ci} step {start + k} w_fwd", ("t", "co", "ci"))
        if with_bwd:
            _assert_pack(wb, eb, dtype, f"{what}: case {ci} step {start + k} w_bwd", ("t", "ci", "co"))
        else:
            assert torch.isnan(packs.views[1]).all(), "a NULL w_bwd was written somewhere"
        f.check(what), packs.check(what)
    snap, psnap = f.bits(), packs.bits()
    assert call(start + 3, 28) != 0 and call(0) != 0
    assert torch.equal(f.bits(), snap) and torch.equal(packs.bits(), psnap), "a refused call wrote something"
    _print_ratios(what)


# ---- 3b rx_adamw_flat / rx_adamw_flat_multi --------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 255, 4095, 4096, 4097, 12289, 1048576 + 257])
def test_adamw_flat_per_element(L, n):
    """rx_adamw_flat: sizes around the 256-thread block and, above 4096 blocks of 256, the second trip of the grid-stride loop"""
    i = [1, 255, 4095, 4096, 4097, 12289, 1048576 + 257].index(n)
    hyper, start = HYPERS[i % 3], START_STEPS[i % 4]
    clip_t, clip = _dev_clip(i % 2 == 0)
    f = Arena([n, n, n, n])
    p, g, m, v = f.views
    for dst, src in zip(f.views, make_inputs(n, 70 + i, start, hyper)):
        dst.copy_(src)
    for k in range(2):
        if k:
            g.copy_(next_grad(n, 70 + i, k))
        before, gbits = (p.cpu(), m.cpu(), v.cpu()), g.view(torch.int32).clone()
        L.check(L.load().rx_adamw_flat(_ptr(p), _ptr(g), _ptr(m), _ptr(v), _ptr(clip_t), *hyper, start + k, n, L.stream_ptr()), "rx_adamw_flat")
        _sync()
        check_step((p, m, v), before, g.cpu(), clip, adam_args(*hyper, start + k), f"adamw_flat: n {n} step {start + k}")
        assert torch.equal(g.view(torch.int32), gbits), "grad written"
        f.check("adamw_flat")
    snap = f.bits()
    assert L.load().rx_adamw_flat(_ptr(p), _ptr(g), _ptr(m), _ptr(v), _ptr(clip_t), *hyper, 0, n, L.stream_ptr()) != 0
    _sync()
    assert torch.equal(f.bits(), snap)
    _print_ratios("adamw_flat")


def _flat_multi(L, arenas, hyper, step, clip_t):
    ps, gs, ms, vs = (a.views for a in arenas)
    k = len(ps)
    VP, LP = ctypes.c_void_p * k, ctypes.c_long * k
    L.check(L.load().rx_adamw_flat_multi(k, VP(*[t.data_ptr() for t in ps]), VP(*[t.data_ptr() for t in gs]), VP(*[t.data_ptr() for t in ms]),
                                         VP(*[t.data_ptr() for t in vs]), LP(*[t.numel() for t in ps]), _ptr(clip_t), *hyper, step,
                                         L.stream_ptr()), "rx_adamw_flat_multi")
    _sync()


def _run_flat_multi(L, sizes, shifts, hyper, start, with_clip, seed, what, steps=2):
    """shifts: per array (p, g, m, v) a list of element shifts or None.  All tensors of one array share one fenced arena."""
    clip_t, clip = _dev_clip(with_clip)
    arenas = [Arena(sizes, shifts=s) for s in shifts]
    ins = [make_inputs(n, seed + j, start, hyper) for j, n in enumerate(sizes)]
    for a, which in zip(arenas, range(4)):
        for view, t in zip(a.views, ins):
            view.copy_(t[which])
    P, G, M, V = (a.views for a in arenas)
    for k in range(steps):
        if k:
            for j, gv in enumerate(G):
                gv.copy_(next_grad(gv.numel(), seed + j, k))
        before = [(p.cpu(), m.cpu(), v.cpu()) for p, m, v in zip(P, M, V)]
        gbits = arenas[1].bits()
        _flat_multi(L, arenas, hyper, start + k, clip_t)
        args = adam_args(*hyper, start + k)
        for j in range(len(sizes)):
            check_step((P[j], M[j], V[j]), before[j], G[j].cpu(), clip, args, f"{what}: tensor {j} of {sizes[j]} step {start + k}")
        assert torch.equal(arenas[1].bits(), gbits), "grad written"
        for a in arenas:
            a.check(what)
    _print_ratios(what)


@pytest.mark.parametrize("count", [48, 49, 97])
def test_adamw_flat_multi_table_boundaries(L, count):
    """exactly one full table (48 tensors), one more, and two full tables plus one; sizes around the 4096-element chunk"""
    base = [1, 3, 255, 4095, 4096, 4097, 8192, 12289]
    sizes = [base[j % 8] if j % 3 == 0 else 17 + 131 * j for j in range(count)]
    i = [48, 49, 97].index(count)
    _run_flat_multi(L, sizes, [None] * 4, HYPERS[i], START_STEPS[i], True, 200 + 100 * i, "adamw_flat_multi")


@pytest.mark.parametrize("which", range(4), ids=["p", "g", "m", "v"])
def test_adamw_flat_multi_one_misaligned_array(L, which):
    """`vec` ORs the four pointers: ONE of p, g, m, v 4 bytes off a 16-byte boundary must send the whole tensor (n = 8192) down the
    scalar path, between aligned neighbours that take the 16-byte path in the same launch"""
    sizes = [4096, 8192, 4097]
    shifts = [[0, 1, 0] if a == which else None for a in range(4)]
    _run_flat_multi(L, sizes, shifts, HYPERS[which % 3], START_STEPS[which], which % 2 == 0, 500 + 10 * which, "adamw_flat_multi")


# ---- 3d rx_grad_norm_clip --------------------------------------------------------------------------------------------------------
# One partial is an fp32 sum of squares in a fixed order: 16 terms per thread (16 adds, and 1 rounding of the product unless it is
# contracted), 6 shuffle adds, 2 adds of the four wave sums: every term passes through at most 16 + 1 + 6 + 2 = 25 roundings, all
# terms are non-negative, so a partial is within 25u of its sum (first order).  The partials are added in fp64 (2^-53 per add: nothing
# at this scale), the root halves the relative error (12.5u) and sqrt + the cast to fp32 add one rounding: 13.5u, with 1 + 2^-10 for
# the second-order terms and the fp64 sums.
NORM_BOUND = (0.5 * (16 + 1 + 6 + 2) + 1) * U32 * (1 + 2.0 ** -10)


def _norm_clip(L, grads, max_norm):
    k = len(grads)
    VP, LP = ctypes.c_void_p * k, ctypes.c_long * k
    numel = LP(*[g.numel() for g in grads])
    need = L.load().rx_grad_norm_clip_partials(k, numel)
    ws = Arena([need, 2])
    L.check(L.load().rx_grad_norm_clip(k, VP(*[g.data_ptr() for g in grads]), numel, float(max_norm), _ptr(ws.views[0]), need,
                                       _ptr(ws.views[1]), L.stream_ptr()), "rx_grad_norm_clip")
    _sync()
    ws.check("grad_norm_clip")
    assert not torch.isnan(ws.views[0]).any(), "a partial was left unwritten"
    return need, ws.views[1].cpu()


def _check_norm(L, grads, ref_sq, max_norm, what):
    need, out = _norm_clip(L, grads, max_norm)
    _, out2 = _norm_clip(L, grads, max_norm)
    assert torch.equal(out.view(torch.int32), out2.view(torch.int32)), "not deterministic"          # fixed summation order
    norm, coef = out[0].double().item(), out[1].double().item()
    ref = ref_sq ** 0.5
    print(f"{what}: {need} partials, norm error / bound {abs(norm - ref) / (NORM_BOUND * ref) if ref else 0.0:.3f}")
    assert abs(norm - ref) <= NORM_BOUND * ref, (what, norm, ref)
    # the coefficient from the DEVICE norm: fl(norm + 1e-6f) and a correctly rounded division, each within u / (1 + u): 2u exactly
    cref = min(1.0, f32(max_norm) / (norm + f32(1e-6)))
    assert abs(coef - cref) <= 2 * U32 * cref and coef <= 1.0, (what, coef, cref)
    return need


@pytest.mark.parametrize("max_norm", [3.0, 1e6])
def test_grad_norm_clip_large_gradient(L, max_norm):
    """8193 * 4096 + 5 elements (8194 partials: the finalize kernel's 8-way unrolled loop runs) plus a few small tensors"""
    gen = torch.Generator(device="cuda").manual_seed(5)
    sizes = [8193 * 4096 + 5, 1, 4097, 300]
    a = Arena(sizes)
    ref_sq = 0.0
    for v in a.views:
        v.copy_(torch.randn(v.numel(), generator=gen, device="cuda") * 0.3)
        ref_sq += torch.linalg.vector_norm(v, 2, dtype=torch.float64).item() ** 2
    need = _check_norm(L, a.views, ref_sq, max_norm, f"grad_norm_clip large, max_norm {max_norm}")
    assert need == 8194 + 1 + 2 + 1
    a.check("grad_norm_clip")


@pytest.mark.parametrize("partials", [7168, 7169])
def test_grad_norm_clip_finalize_loop_boundary(L, partials):
    """`i + 7 * 1024 < nblocks`: at 7168 partials no thread takes the unrolled loop, at 7169 thread 0 alone does.  One partial per
    tensor of 5 elements (150 table launches)"""
    gen = torch.Generator().manual_seed(partials)
    a = Arena([5] * partials, pad=3)
    vals = torch.randn(partials, 5, generator=gen) * 0.3
    for v, t in zip(a.views, vals.cuda()):
        v.copy_(t)
    need = _check_norm(L, a.views, (vals.double() ** 2).sum().item(), 3.0, f"grad_norm_clip {partials} partials")
    assert need == partials
    a.check("grad_norm_clip")


def test_grad_norm_clip_all_zero(L):
    a = Arena([4097, 1, 300])
    for v in a.views:
        v.zero_()
    _, out = _norm_clip(L, a.views, 3.0)
    assert out[0].item() == 0.0 and out[1].item() == 1.0


# ---- 3e EngineAdamW bookkeeping --------------------------------------------------------------------------------------------------
def _params(sizes, seed):
    torch.manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(s, device="cuda")) for s in sizes]


def _set_grads(ps, seed, k, skip=()):
    for j, p in enumerate(ps):
        p.grad = None if j in skip else next_grad(p.numel(), seed + j, k).view(p.shape).cuda()


def test_engine_adamw_late_gradient_keeps_its_own_step(L):
    """a parameter whose .grad is None for two steps and appears at the third: its step is 1 while the others' is 3 (`_flat_update`
    splits the group by step), and each follows its own reference"""
    from mt3d_amd.training.optim import EngineAdamW
    hyper = HYPERS[0]
    ps = _params([(64, 32, 3), (4097,), (7, 5), (300,)], 11)
    opt = EngineAdamW(ps, model=None, lr=hyper[0], betas=hyper[1:3], eps=hyper[3], weight_decay=hyper[4])
    late = 1
    for k in range(3):
        _set_grads(ps, 900, k, skip=(late,) if k < 2 else ())
        before = [(p.detach().cpu(), opt.state[p]["exp_avg"].cpu(), opt.state[p]["exp_avg_sq"].cpu()) if opt.state.get(p)
                  else (p.detach().cpu(), torch.zeros(p.shape), torch.zeros(p.shape)) for p in ps]
        opt.step()
        _sync()
        for j, p in enumerate(ps):
            if p.grad is None:
                assert torch.equal(p.detach().cpu(), before[j][0]) and not opt.state.get(p)
                continue
            st = opt.state[p]
            want = (1 if k == 2 else None) if j == late else k + 1
            assert st["step"] == want, (j, k, st["step"])
            check_step((p.detach().flatten(), st["exp_avg"].flatten(), st["exp_avg_sq"].flatten()), [b.flatten() for b in before[j]],
                       p.grad.flatten().cpu(), None, adam_args(*hyper, st["step"]), f"engine_adamw: parameter {j} step {st['step']}")


@pytest.mark.parametrize("source", ["engine", "torch"])
def test_engine_adamw_state_dict_round_trip_is_bit_exact(L, source):
    """state_dict() -> a new EngineAdamW -> load_state_dict() continues bit for bit; also when the state comes from torch.optim.AdamW,
    whose `step` is a tensor"""
    from mt3d_amd.training.optim import EngineAdamW
    hyper = HYPERS[0]
    kw = dict(lr=hyper[0], betas=hyper[1:3], eps=hyper[3], weight_decay=hyper[4])
    sizes = [(64, 32, 3), (4097,), (7, 5)]
    pa = _params(sizes, 12)
    oa = EngineAdamW(pa, model=None, **kw) if source == "engine" else torch.optim.AdamW(pa, **kw)
    for k in range(2):
        _set_grads(pa, 950, k)
        oa.step()
    sd = copy.deepcopy(oa.state_dict())
    if source == "torch":
        assert all(torch.is_tensor(s["step"]) for s in sd["state"].values())
        ints = copy.deepcopy(sd)
        for s in ints["state"].values():
            s["step"] = int(s["step"])
        # the optimizer that continues `pa`: an EngineAdamW given the same state with plain integer steps
        pa = [torch.nn.Parameter(p.detach().clone()) for p in pa]
        oa = EngineAdamW(pa, model=None, **kw)
        oa.load_state_dict(ints)
    pb = [torch.nn.Parameter(p.detach().clone()) for p in pa]
    ob = EngineAdamW(pb, model=None, **kw)
    ob.load_state_dict(sd)
    for k in range(2, 4):
        _set_grads(pa, 950, k)
        _set_grads(pb, 950, k)
        before = [(p.detach().cpu(), ob.state[p]["exp_avg"].cpu(), ob.state[p]["exp_avg_sq"].cpu()) for p in pb]
        oa.step(), ob.step()
        _sync()
        for j, (a, b) in enumerate(zip(pa, pb)):
            sa, sb = oa.state[a], ob.state[b]
            assert int(sa["step"]) == int(sb["step"]) == k + 1
            assert _same_bits(a.detach(), b.detach()) and _same_bits(sa["exp_avg"], sb["exp_avg"]) and _same_bits(sa["exp_avg_sq"], sb["exp_avg_sq"]), (j, k)
            check_step((b.detach().flatten(), sb["exp_avg"].flatten(), sb["exp_avg_sq"].flatten()), [t.flatten() for t in before[j]],
                       b.grad.flatten().cpu(), None, adam_args(*hyper, k + 1), f"engine_adamw: loaded from {source}, parameter {j} step {k + 1}")
