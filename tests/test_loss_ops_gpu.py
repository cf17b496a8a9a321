"""GPU (-m gpu): the C entries of csrc/rx_loss.hip one by one -- BCE+Dice, masked cosine, the element-wise family and cross entropy --
each gradient element held to the bound of tests/loss_ref.py around the fp64 host formulation, the scalar loss to 2e-6 (mean) or the
sum_margin rule (sum), cross entropy's `saved` per voxel to the fp64 logsumexp / target sum and BCE+Dice's `coef` to a_c, b_c.  The
kernels are called through the C ABI with explicit pointers: every output (loss, coef, saved, the gradient) is carved out of one
NaN-poisoned buffer between sentinel fences, every input at a chosen element offset (0-3) from a 16-byte boundary.  After each call
the fences are intact, no NaN is left in an output and the bounds hold.  Cases: loss_ref.all_cases(); on every one of them fp32 CPU
torch stays within a quarter of the same bound (tests/test_loss_ref_cpu.py).  A few cases go through the autograd classes for what
only they decide: the torch fallbacks and contiguous views at odd storage offsets."""
import math
from ctypes import c_void_p

import pytest
import torch

import loss_ref as R

pytestmark = pytest.mark.gpu

RX_EINVAL = -1


@pytest.fixture(scope="module")
def L():
    import mt3d_amd  # noqa: F401
    from mt3d_amd.engine import lib
    lib.require_device()
    return lib


def _ptr(t):
    return c_void_p(t.data_ptr()) if t is not None else c_void_p(0)


class Arena:
    """fp32 tensors of `sizes` elements inside ONE device buffer: tensor i starts `shifts[i]` elements after a 16-byte boundary with
    at least 64 sentinel elements on both sides; the tensors hold NaN until written.  check() holds every sentinel to its bits."""

    def __init__(self, sizes, shifts=None, pad=64):
        offs, o = [], pad
        for i, n in enumerate(sizes):
            o = (o + 31) // 32 * 32 + (shifts[i] if shifts else 0)
            offs.append(o)
            o += n + pad
        self.buf = (-(97.0 + torch.arange(o, device="cuda") % 128)).float()
        assert self.buf.data_ptr() % 16 == 0
        inside = torch.zeros(o + 1, dtype=torch.int32)
        for off, n in zip(offs, sizes):
            inside[off] += 1
            inside[off + n] -= 1
        self.guard = (inside[:o].cumsum(0) == 0).cuda()
        self.buf[~self.guard] = float("nan")
        self.views = [self.buf[off:off + n] for off, n in zip(offs, sizes)]
        self.snap = self.buf.clone()

    def check(self, what):
        bad = (self.buf.view(torch.int32) != self.snap.view(torch.int32)) & self.guard
        assert not bad.any(), f"{what}: {int(bad.sum())} fence words written, first at offset {int(bad.nonzero()[0])}"

    def untouched(self):
        return torch.equal(self.buf.view(torch.int32), self.snap.view(torch.int32))


def _filled(out, what):
    nan = torch.isnan(out)
    assert not nan.any(), f"{what}: {int(nan.sum())} of {out.numel()} elements left unwritten (NaN), first at {int(nan.flatten().nonzero()[0])}"


def _ncv(x):
    n, c = x.shape[0], x.shape[1]
    return n, c, x.numel() // (n * c)


def _ws(nbytes):
    return torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device="cuda")


def _upstream(g):
    return torch.tensor([g], dtype=torch.float32, device="cuda")


ELEM_KIND = {"BCEWithLogitsLoss": 0, "BCEWithLogitsLossLabelSmoothing": 0, "BCEWithLogitsLossZSmooth": 0, "BCELoss": 1, "MSELoss": 2}
REDUCE = {"mean": 0, "sum": 1}


def run_kernel(L, name, x, t, kw, g=R.G_UP, shifts=(0, 0, 0), poison_check=True, coef_in=None):
    """forward + backward of one family through the C ABI.  shifts: element offsets of (x, t, gradient) -- cross entropy: (logits,
    probability target, dlogits, saved) -- from a 16-byte boundary.  -> dict(loss, grad, coef / saved where the family has them),
    CPU tensors, after the fence and poison checks.  coef_in (BCE+Dice): the backward takes these coefficients instead of the ones its
    own forward left (which stay in the result)"""
    so = L.load()
    n, c, v = _ncv(x)
    e = x.numel()
    st = L.stream_ptr()
    gl = _upstream(g)
    what = f"{name} {tuple(x.shape)} {kw} shifts {shifts}"
    index = t.dtype == torch.int64
    ins = Arena([e] if index else [e, t.numel()], shifts=[shifts[0]] if index else list(shifts[:2]))
    ins.views[0].copy_(x.reshape(-1))
    xd = ins.views[0]
    td = t.cuda() if index else ins.views[1].copy_(t.reshape(-1))
    ins_bits = ins.buf.view(torch.int32).clone()
    out = {}
    if name in ELEM_KIND:
        outs = Arena([1, e], shifts=[0, shifts[2]])
        loss, dx = outs.views
        table, z = None, 0
        if name == "BCEWithLogitsLossZSmooth":
            z = x.shape[2]
            table = R.zsmooth_table(z, kw.get("center_smoothing", 0.1), kw.get("edge_smoothing", 0.4)).cuda().contiguous()
        s = float(kw.get("smoothing", 0.1)) if name == "BCEWithLogitsLossLabelSmoothing" else 0.0
        ws = _ws(so.rx_loss_workspace(n, c, v))
        red = REDUCE[kw.get("reduction", "mean")]
        L.check(so.rx_elem_loss_fwd(ELEM_KIND[name], _ptr(xd), _ptr(td), n, c, v, s, _ptr(table), z, red, _ptr(loss), _ptr(ws), ws.numel(), st),
                "rx_elem_loss_fwd")
        L.check(so.rx_elem_loss_bwd(ELEM_KIND[name], _ptr(xd), _ptr(td), n, c, v, s, _ptr(table), z, red, _ptr(gl), _ptr(dx), st),
                "rx_elem_loss_bwd")
    elif name == "BCEDiceLoss":
        outs = Arena([1, e, 2 * c], shifts=[0, shifts[2], 0])
        loss, dx, coef = outs.views
        s = float(kw.get("smoothing", 0.1))
        ws = _ws(so.rx_loss_workspace(n, c, v))
        L.check(so.rx_bce_dice_loss_fwd(_ptr(xd), _ptr(td), n, c, v, kw["alpha"], kw["beta"], s, 1e-6, _ptr(loss), _ptr(coef), _ptr(ws),
                                        ws.numel(), st), "rx_bce_dice_loss_fwd")
        cb = coef if coef_in is None else coef_in.cuda()
        L.check(so.rx_bce_dice_loss_bwd(_ptr(xd), _ptr(td), n, c, v, kw["alpha"], kw["beta"], s, _ptr(cb), _ptr(gl), _ptr(dx), st),
                "rx_bce_dice_loss_bwd")
        out["coef"] = coef
    elif name == "MaskedCosineLoss":
        outs = Arena([1, e, 1], shifts=[0, shifts[2], 0])
        loss, dx, coef = outs.views
        ws = _ws(so.rx_loss_workspace(n, c, v))
        L.check(so.rx_masked_cosine_loss_fwd(_ptr(xd), _ptr(td), n, c, v, _ptr(loss), _ptr(coef), _ptr(ws), ws.numel(), st),
                "rx_masked_cosine_loss_fwd")
        L.check(so.rx_masked_cosine_loss_bwd(_ptr(xd), _ptr(td), n, c, v, _ptr(coef), _ptr(gl), _ptr(dx), st), "rx_masked_cosine_loss_bwd")
    else:
        p = n * v
        nsaved = p if index else 2 * p
        outs = Arena([1, e, 1, nsaved], shifts=[0, shifts[2], 0, shifts[3] if len(shifts) > 3 else 0])
        loss, dx, coef, saved = outs.views
        ws = _ws(so.rx_cross_entropy_loss_workspace(n, c, v))
        tp, ti = (None, td) if index else (td, None)
        ignore, red = kw.get("ignore_index", -100), REDUCE[kw.get("reduction", "mean")]
        L.check(so.rx_cross_entropy_loss_fwd(_ptr(xd), _ptr(tp), _ptr(ti), ignore, n, c, v, red, _ptr(loss), _ptr(coef), _ptr(saved), _ptr(ws),
                                             ws.numel(), st), "rx_cross_entropy_loss_fwd")
        L.check(so.rx_cross_entropy_loss_bwd(_ptr(xd), _ptr(tp), _ptr(ti), ignore, n, c, v, _ptr(coef), _ptr(saved), _ptr(gl), _ptr(dx), st),
                "rx_cross_entropy_loss_bwd")
        out["saved"] = saved
    torch.cuda.synchronize()
    outs.check(what)
    assert torch.equal(ins.buf.view(torch.int32), ins_bits), f"{what}: an input or its fences were written"
    if poison_check:
        for key, view in [("gradient", dx)] + [(k, out[k]) for k in out]:
            _filled(view, f"{what} {key}")
    out = {k: w.cpu().clone() for k, w in out.items()}
    out["loss"], out["grad"] = loss.cpu().clone()[0], dx.cpu().clone().view(x.shape)
    return out


def check_case(L, case, shifts=(0, 0, 0)):
    """one case of the table: kernel against the fp64 reference, every check of the module docstring"""
    name, kw = case["name"], case["kw"]
    x, t = case["make"]()
    ref = R.reference(name, x, t, kw)
    got = run_kernel(L, name, x, t, kw, shifts=shifts)
    what = case["id"]
    loss32 = float(R.run_host(name, x, t, kw, torch.float32)[0]) if kw.get("reduction") == "sum" else None
    ok, text = R.loss_ok(float(got["loss"]), float(ref["loss"]), kw, loss32)
    print(f"{what}: {text}")
    R.assert_elementwise(got["grad"], ref["grad"], ref["M"], ref["rel"], f"{what} gradient", ref["floor"], family=case["group"][0])
    assert ok, f"{what}: {text}"
    if name == "BCEDiceLoss":
        coef = got["coef"].double().view(-1, 2)
        R.assert_elementwise(coef[:, 0], ref["a"], ref["a"], ref["rel_a"], f"{what} coef a_c", family="BCEDiceLoss coef")
        R.assert_elementwise(coef[:, 1], ref["b"], ref["b"], ref["rel_b"], f"{what} coef b_c", family="BCEDiceLoss coef")
        assert torch.equal(coef[:, 1] == 0, ref["b"] == 0), f"{what}: b_c is zero exactly where the reference's is: {coef[:, 1]} {ref['b']}"
    if name == "CrossEntropyLoss":
        p = ref["lse"].numel()
        R.assert_elementwise(got["saved"][:p].view(ref["lse"].shape), ref["lse"], 1.0, ref["lse_bound"], f"{what} saved logsumexp",
                             family="CrossEntropyLoss saved")
        if t.dtype != torch.int64:
            R.assert_elementwise(got["saved"][p:].view(ref["tsum"].shape), ref["tsum"], 1.0, ref["tsum_bound"], f"{what} saved target sum",
                                 family="CrossEntropyLoss saved")
    return got, ref


def _report_ratios():
    for fam, r in sorted(R.RATIOS.items()):
        print(f"largest |got - ref| / bound so far, {fam}: {r:.4f}")


def _groups(cases):
    out = {}
    for c in cases:
        out.setdefault(c["group"], []).append(c)
    return out


ELEM_GROUPS = _groups(R.elem_cases())
CE_GROUPS = _groups(R.ce_cases())


# ---- the case table --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", list(ELEM_GROUPS), ids=lambda g: "-".join(g))
def test_elementwise_family_per_element(L, group):
    """sizes 1 .. 8196 around the chunk edge on the vector and the scalar path, odd planes, 600 blocks through the finalize, the
    logit / probability value grids (saturating exp, both BCELoss clamps), Z-smooth slice boundaries inside a 4-vector"""
    for case in ELEM_GROUPS[group]:
        check_case(L, case)
    _report_ratios()


def test_bce_dice_per_element(L):
    """the same sizes, 300 and 600 partial quadruples per channel, Dice sums over N, the value grid, alpha = 0, beta = 0, an empty
    channel, and the Dice clamp: a_c = 2e6 and b_c == 0 exactly where den <= 1e-6"""
    for case in R.dice_cases():
        got, ref = check_case(L, case)
        if case["id"].endswith("clamp_active"):
            coef = got["coef"].view(-1, 2)
            assert coef[0, 0].item() == 2e6 and coef[0, 1].item() == 0.0, coef
            assert coef[1, 1].item() > 0.0 and coef[2, 1].item() > 0.0, coef
    _report_ratios()


def test_masked_cosine_per_element(L):
    """C 1, 2, 3, 8; one voxel, one chunk, one more; target norms on both sides of the 1e-6 mask threshold; prediction norms 0, 1e-12
    and 5e-9 (under the 1e-8 clamp, where the gradient is the ordinary one, not zero), 2e-8, 1, 1e15; every voxel masked"""
    for case in R.cosine_cases():
        got, ref = check_case(L, case)
        if case["id"].endswith("all_masked"):
            assert got["loss"].item() == 1.0 and (got["grad"] == 0).all()
    _report_ratios()


@pytest.mark.parametrize("group", list(CE_GROUPS), ids=lambda g: "-".join(g))
def test_cross_entropy_per_element(L, group):
    """C 1 .. 1024, V around the 2048-voxel chunk on both paths, both branches of the online max, equal logits, +-1e4; probability
    rows summing to 1, 0, 2; index targets with ~30 % ignored, ignore_index 255 and 1 (in range), indices C, -1, 2^40 mixed in"""
    for case in CE_GROUPS[group]:
        check_case(L, case)
    _report_ratios()


def test_cross_entropy_all_ignored(L):
    """loss NaN (0 / 0, as torch), gradient exactly 0, saved still the logsumexp"""
    x, _ = R.ce_pair(3, 3, 2049, 77, "index")
    t = torch.full((3, 2049), -100, dtype=torch.int64)
    for red, want_nan in (("mean", True), ("sum", False)):
        got = run_kernel(L, "CrossEntropyLoss", x, t, {"reduction": red})
        assert math.isnan(got["loss"].item()) == want_nan and (want_nan or got["loss"].item() == 0.0), got["loss"]
        assert (got["grad"] == 0).all()


# ---- misaligned operands: the scalar fallback, bit-identical to the aligned call ------------------------------------------------------
SHIFTS3 = [(1, 0, 0), (0, 2, 0), (0, 0, 3), (1, 2, 3)]


@pytest.mark.parametrize("name", list(R.ELEMENTWISE) + ["BCEDiceLoss"])
def test_misaligned_operands_match_aligned_bit_for_bit(L, name):
    """V = 8196 (a multiple of 4, more than one chunk) with x, t and the gradient 1, 2, 3 elements off a 16-byte boundary, one at a
    time and together: the per-element arithmetic is the same, so the gradient is the aligned one bit for bit.  The loss: the same
    terms in another summation order (bound as everywhere).  BCE+Dice's gradient also takes a_c, b_c, which are such sums: its
    backward is compared bit for bit on the aligned call's coefficients, and once more on its own forward's within the bound."""
    shape = (1, 1) + (R.ZS_SHAPE_OF_V[8196] if name == "BCEWithLogitsLossZSmooth" else (8196,))
    kw = {"alpha": 0.3, "beta": 0.7} if name == "BCEDiceLoss" else {"reduction": "mean"}
    x, t = R.rand_pair(name, shape, 611)
    ref = R.reference(name, x, t, kw)
    base = run_kernel(L, name, x, t, kw)
    for sh in SHIFTS3:
        got = run_kernel(L, name, x, t, kw, shifts=sh, coef_in=base.get("coef"))
        assert torch.equal(got["grad"].view(torch.int32), base["grad"].view(torch.int32)), f"{name} shifts {sh}: gradient differs from aligned"
        ok, text = R.loss_ok(float(got["loss"]), float(ref["loss"]), kw)
        assert ok, f"{name} shifts {sh}: {text}"
        R.assert_elementwise(got["grad"], ref["grad"], ref["M"], ref["rel"], f"{name} shifts {sh}", ref["floor"])
        if name == "BCEDiceLoss":
            own = run_kernel(L, name, x, t, kw, shifts=sh)
            R.assert_elementwise(own["grad"], ref["grad"], ref["M"], ref["rel"], f"{name} shifts {sh}, own coefficients", ref["floor"])
            coef = own["coef"].double().view(-1, 2)
            R.assert_elementwise(coef[:, 0], ref["a"], ref["a"], ref["rel_a"], f"{name} shifts {sh} a_c")
            R.assert_elementwise(coef[:, 1], ref["b"], ref["b"], ref["rel_b"], f"{name} shifts {sh} b_c")
            if sh[:2] == (0, 0):        # a misaligned gradient alone does not change the forward
                assert torch.equal(own["coef"].view(torch.int32), base["coef"].view(torch.int32))


@pytest.mark.parametrize("mode", ["prob", "index"])
def test_cross_entropy_misaligned_operands_take_w1_bit_identical(L, mode):
    """V = 2052: logits, probability targets, dlogits and saved off a 16-byte boundary one at a time: the W = 1 instantiation, whose
    per-voxel arithmetic is the W = 4 one's"""
    x, t = R.ce_pair(3, 3, 2052, 612, mode)
    kw = {"reduction": "mean"}
    base = run_kernel(L, "CrossEntropyLoss", x, t, kw, shifts=(0, 0, 0, 0))
    for sh in [(1, 0, 0, 0), (0, 2, 0, 0), (0, 0, 3, 0), (0, 0, 0, 1)]:
        if mode == "index" and sh[1]:
            continue
        got = run_kernel(L, "CrossEntropyLoss", x, t, kw, shifts=sh)
        for key in ("grad", "saved"):
            assert torch.equal(got[key].view(torch.int32), base[key].view(torch.int32)), f"cross entropy {mode} shifts {sh}: {key} differs"
        assert abs(got["loss"].item() - base["loss"].item()) <= R.MEAN_ABS


# ---- NaN, the grid-y limit ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(R.LOGIT_NAMES) + ["MSELoss", "BCEDiceLoss", "MaskedCosineLoss", "CrossEntropyLoss"])
def test_nan_logit_gives_nan_loss(L, name):
    """as the reference does (BCELoss is not here: torch rejects the input)"""
    shape = (1, 3, 2, 5, 7)
    kw = {"alpha": 0.5, "beta": 0.5} if name == "BCEDiceLoss" else {"reduction": "mean"}
    if name == "CrossEntropyLoss":
        x, t = R.ce_pair(1, 3, 70, 5, "prob")
    elif name == "MaskedCosineLoss":
        x, t = R.cosine_pair((1, 3, 70), 6)
        t = torch.ones_like(t)
    else:
        x, t = R.rand_pair(name, shape, 7)
    x.view(-1)[11] = float("nan")
    assert math.isnan(float(R.run_host(name, x, t, kw, torch.float64)[0]))
    got = run_kernel(L, name, x, t, kw, poison_check=False)
    assert math.isnan(got["loss"].item())


def test_grid_y_limit(L):
    """N * C = 65535 planes of one element run; 65536 are refused with RX_EINVAL before any launch: outputs keep their poison"""
    so, st = L.load(), L.stream_ptr()
    for name, kw in (("BCEWithLogitsLoss", {"reduction": "mean"}), ("BCEDiceLoss", {"alpha": 0.3, "beta": 0.7})):
        x, t = R.rand_pair(name, (21845, 3, 1), 801)
        ref = R.reference(name, x, t, kw)
        got = run_kernel(L, name, x, t, kw)
        R.assert_elementwise(got["grad"], ref["grad"], ref["M"], ref["rel"], f"{name} 65535 planes", ref["floor"])
        assert R.loss_ok(float(got["loss"]), float(ref["loss"]), kw)[0]
    n, c = 16384, 4
    ins, outs = Arena([n * c, n * c]), Arena([1, n * c, 2 * c])
    ins.views[0].fill_(0.5), ins.views[1].fill_(1.0)
    ins.snap = ins.buf.clone()
    x, t = ins.views
    loss, dx, coef = outs.views
    ws, gl = _ws(so.rx_loss_workspace(n, c, 1)), _upstream(1.0)
    rcs = [so.rx_elem_loss_fwd(0, _ptr(x), _ptr(t), n, c, 1, 0.0, None, 0, 0, _ptr(loss), _ptr(ws), ws.numel(), st),
           so.rx_elem_loss_bwd(0, _ptr(x), _ptr(t), n, c, 1, 0.0, None, 0, 0, _ptr(gl), _ptr(dx), st),
           so.rx_bce_dice_loss_fwd(_ptr(x), _ptr(t), n, c, 1, 0.5, 0.5, 0.1, 1e-6, _ptr(loss), _ptr(coef), _ptr(ws), ws.numel(), st),
           so.rx_bce_dice_loss_bwd(_ptr(x), _ptr(t), n, c, 1, 0.5, 0.5, 0.1, _ptr(coef), _ptr(gl), _ptr(dx), st),
           so.rx_masked_cosine_loss_fwd(_ptr(x), _ptr(t), n, c, 1, _ptr(loss), _ptr(coef), _ptr(ws), ws.numel(), st),
           so.rx_masked_cosine_loss_bwd(_ptr(x), _ptr(t), n, c, 1, _ptr(coef), _ptr(gl), _ptr(dx), st)]
    torch.cuda.synchronize()
    assert rcs == [RX_EINVAL] * 6, rcs
    assert outs.untouched() and ins.untouched()


# ---- what only the autograd classes decide -----------------------------------------------------------------------------------------------
def _classes():
    from mt3d_amd.training.losses.losses import LOSS_FN_MAP
    return LOSS_FN_MAP


def test_cosine_nine_channels_takes_torch_exactly(L):
    x, t = R.cosine_pair((2, 9, 70), 901)
    x, t = x.cuda(), t.cuda()
    a = x.clone().requires_grad_(True)
    la = _classes()["MaskedCosineLoss"]()(a, t)
    assert "_MaskedCosineFn" not in type(la.grad_fn).__name__
    (la * R.G_UP).backward()
    b = x.clone().requires_grad_(True)
    lb = R.host("MaskedCosineLoss", b, t, {}, torch.float32)
    (lb * R.G_UP).backward()
    assert torch.equal(la, lb) and torch.equal(a.grad, b.grad)


def test_cross_entropy_1025_classes_takes_torch(L):
    x, t = R.ce_pair(2, 1025, 5, 902, "index")
    x, t = x.cuda(), t.cuda()
    a = x.clone().requires_grad_(True)
    la = _classes()["CrossEntropyLoss"]()(a, t)
    assert "_CrossEntropyFn" not in type(la.grad_fn).__name__
    la.backward()
    b = x.clone().requires_grad_(True)
    lb = torch.nn.CrossEntropyLoss()(b, t)
    lb.backward()
    assert torch.equal(la, lb) and torch.equal(a.grad, b.grad)


@pytest.mark.parametrize("name", ["BCEDiceLoss", "MaskedCosineLoss", "BCEWithLogitsLoss", "CrossEntropyLoss"])
def test_classes_on_contiguous_views_at_odd_storage_offsets(L, name):
    """a contiguous view one element into its storage reaches the kernels as a misaligned pointer with V % 4 == 0: the class's result
    is held to the same bounds (the upstream gradient -2.5 arrives through autograd)"""
    shape = {"BCEDiceLoss": (2, 2, 8196), "MaskedCosineLoss": (2, 3, 8196), "BCEWithLogitsLoss": (2, 2, 8196), "CrossEntropyLoss": (3, 3, 2052)}[name]
    kw = {"alpha": 0.3, "beta": 0.7} if name == "BCEDiceLoss" else {}
    if name == "CrossEntropyLoss":
        x, t = R.ce_pair(*shape, 903, "prob")
    elif name == "MaskedCosineLoss":
        x, t = R.cosine_pair(shape, 904)
    else:
        x, t = R.rand_pair(name, shape, 905)
    ref = R.reference(name, x, t, kw)

    def odd(v):
        buf = torch.empty(v.numel() + 1, device="cuda")
        buf[1:].copy_(v.reshape(-1))
        w = buf[1:].view(v.shape)
        assert w.is_contiguous() and w.data_ptr() % 16 == 4
        return w
    a = odd(x).requires_grad_(True)
    loss = _classes()[name](**kw)(a, odd(t))
    assert "Fn" in type(loss.grad_fn).__name__, type(loss.grad_fn).__name__
    (loss * R.G_UP).backward()
    ok, text = R.loss_ok(loss.item(), float(ref["loss"]), kw)
    assert ok, text
    R.assert_elementwise(a.grad.cpu(), ref["grad"], ref["M"], ref["rel"], f"{name} class on an odd view", ref["floor"])
