"""The six remaining names of the loss map -- BCEWithLogitsLoss, BCEWithLogitsLossLabelSmoothing, BCEWithLogitsLossZSmooth, BCELoss,
MSELoss, CrossEntropyLoss -- against vectors produced by the reference's classes / torch.nn on the CPU
(tests/golden/losses_extra.npz, written by scripts/make_losses_fixture.py).

  * CPU: the host formulation reproduces the fixture; the fixture regenerates identically where the reference is present; the
    C ABI exports the new entry points, which validate their arguments before touching a device.
  * GPU (`-m gpu`): the element-wise and cross-entropy HIP kernels (csrc/rx_loss.hip) against the same vectors, with the bounds
    of tests/test_losses.py -- 2e-6 absolute on a mean-reduced loss, 2e-5 rel-L2 on the gradient.  A sum-reduced loss is judged
    relative to the float64 value of the fixture (`loss64`): within 4x the relative error of torch's own fp32 CPU result for
    that case (another summation order of the same fp32 terms), floor 2e-6.  Then the fallbacks, the dtype rule, and larger
    shapes against the torch formulation evaluated on the device.

These bounds judge a whole tensor.  The per-element checks of the same kernels -- every dispatch path, guarded and NaN-poisoned
outputs, value edges, each gradient element against an fp64 reference -- are in tests/test_loss_ops_gpu.py (reference and bounds:
tests/loss_ref.py)."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest
import torch

from helpers import rel_l2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "losses_extra.npz"))


def _fixture_script():
    spec = importlib.util.spec_from_file_location("make_losses_fixture", os.path.join(ROOT, "scripts", "make_losses_fixture.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


FIX = _fixture_script()
CASES = FIX.CASES          # name -> (kind, shape, seed, kwargs, upstream weight, target mode)
ENGINE_NODE = {"CrossEntropyLoss": "_CrossEntropyFn"}


def _losses():
    import mt3d_amd  # noqa: F401
    from mt3d_amd.training.losses.losses import LOSS_FN_MAP
    return LOSS_FN_MAP


def _run(name, device):
    kind, _, _, kw, weight, _ = CASES[name]
    fn = _losses()[kind](**kw)
    pred = torch.from_numpy(GOLD[f"{name}.pred"]).to(device).requires_grad_(True)
    target = torch.from_numpy(GOLD[f"{name}.target"]).to(device)
    loss = fn(pred, target)
    (loss * weight).backward()
    return loss, pred.grad.cpu()


def test_fixture_covers_the_case_table():
    assert sorted({k.split(".")[0] for k in GOLD.files}) == sorted(CASES)
    assert {c[0] for c in CASES.values()} == set(FIX.ELEMENTWISE) | {"CrossEntropyLoss"}


@pytest.mark.parametrize("name", list(CASES))
def test_host_formulation_matches_reference(name):
    loss, grad = _run(name, "cpu")
    assert abs(loss.item() - float(GOLD[f"{name}.loss"])) < 1e-6
    ref = torch.from_numpy(GOLD[f"{name}.grad"])
    assert (grad - ref).abs().max().item() <= 1e-7 + 1e-5 * ref.abs().max().item()


def test_loss_map_classes_are_the_torch_classes():
    import torch.nn as nn
    m = _losses()
    for name in ("BCEWithLogitsLoss", "BCELoss", "MSELoss", "CrossEntropyLoss"):
        assert isinstance(m[name](), getattr(nn, name)) and m[name] is not getattr(nn, name)
    assert m["CrossEntropyLoss"](ignore_index=7, label_smoothing=0.1).label_smoothing == 0.1
    assert m["BCEWithLogitsLoss"](pos_weight=torch.ones(3)).pos_weight is not None


def test_fixture_regenerates_from_the_reference():
    import ref_shim
    if not ref_shim.reference_available():
        pytest.skip("reference tree not present")
    arrays = FIX.generate(FIX.reference_classes())
    assert sorted(arrays) == sorted(GOLD.files)
    for k, v in arrays.items():
        assert np.array_equal(np.asarray(v), GOLD[k]), k


NEW_SYMBOLS = ("rx_elem_loss_fwd", "rx_elem_loss_bwd", "rx_cross_entropy_loss_workspace", "rx_cross_entropy_loss_fwd",
               "rx_cross_entropy_loss_bwd")


def test_cabi_exports_and_validates_the_new_entry_points():
    """no device is touched: the size query is host arithmetic and validation precedes every launch"""
    import __graft_entry__
    __graft_entry__.build()
    import mt3d_amd  # noqa: F401
    from mt3d_amd.engine import lib
    raw = ctypes.CDLL(lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert hasattr(raw, name), name
        assert name in lib.exported_symbols()
    so = lib.load()
    assert so.rx_cross_entropy_loss_workspace(2, 5, 8400) > 0
    for bad in ((0, 5, 8400), (2, 0, 8400), (2, 5, 0), (-1, 5, 8400)):
        assert so.rx_cross_entropy_loss_workspace(*bad) == 0
    calls = {
        "rx_elem_loss_fwd": lambda: so.rx_elem_loss_fwd(0, None, None, 2, 5, 8400, 0.0, None, 0, 0, None, None, 0, None),
        "rx_elem_loss_bwd": lambda: so.rx_elem_loss_bwd(0, None, None, 2, 5, 8400, 0.0, None, 0, 0, None, None, None),
        "rx_cross_entropy_loss_fwd": lambda: so.rx_cross_entropy_loss_fwd(None, None, None, -100, 2, 5, 8400, 0, None, None, None, None,
                                                                          0, None),
        "rx_cross_entropy_loss_bwd": lambda: so.rx_cross_entropy_loss_bwd(None, None, None, -100, 2, 5, 8400, None, None, None, None,
                                                                          None),
    }
    for name, call in calls.items():
        assert call() < 0, name
        assert name.encode() in so.rx_last_error(), (name, so.rx_last_error())


# ---- GPU ------------------------------------------------------------------------------------------------------------
def _node(kind):
    return ENGINE_NODE.get(kind, "_ElemLossFn")


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_hip_kernels_match_reference(name):
    """Bounds as stated in the module docstring.  Measured on an MI355X: see DESIGN, "The remaining task losses"."""
    from mt3d_amd.engine import lib
    lib.require_device()
    kind, _, _, kw, _, _ = CASES[name]
    loss, grad = _run(name, "cuda")
    assert _node(kind) in type(loss.grad_fn).__name__, type(loss.grad_fn).__name__
    want, want64 = float(GOLD[f"{name}.loss"]), float(GOLD[f"{name}.loss64"])
    ref = torch.from_numpy(GOLD[f"{name}.grad"])
    r = rel_l2(grad, ref)
    if kw.get("reduction") == "sum":
        margin = FIX.sum_margin(want, want64)
        err = abs(loss.item() - want64) / abs(want64)
        print(f"{name}: sum loss {loss.item():.6f} rel err vs loss64 {err:.3e} (margin {margin:.2e}), grad rel-L2 {r:.3e}")
        assert err < margin, (loss.item(), want64, err, margin)
    else:
        print(f"{name}: loss {loss.item():.7f} |diff| {abs(loss.item() - want):.3e}, grad rel-L2 {r:.3e}")
        assert abs(loss.item() - want) < 2e-6, (loss.item(), want)
    assert r < 2e-5, r


def _pair(shape, seed=5, prob=False):
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn(shape, device="cuda", generator=g)
    t = (torch.rand(shape, device="cuda", generator=g) > 0.7).float()
    return (torch.sigmoid(x) if prob else x), t


FALLBACKS = {    # name -> (class, kwargs, probabilities in?, index targets?)
    "bcel_none": ("BCEWithLogitsLoss", {"reduction": "none"}, False, False),
    "bcel_pos_weight": ("BCEWithLogitsLoss", {"pos_weight": "ones3"}, False, False),
    "bcel_weight": ("BCEWithLogitsLoss", {"weight": "ones3"}, False, False),
    "bce_none": ("BCELoss", {"reduction": "none"}, True, False),
    "bce_weight": ("BCELoss", {"weight": "ones3"}, True, False),
    "mse_none": ("MSELoss", {"reduction": "none"}, False, False),
    "ce_none": ("CrossEntropyLoss", {"reduction": "none"}, False, True),
    "ce_weight": ("CrossEntropyLoss", {"weight": "w3"}, False, True),
    "ce_label_smoothing": ("CrossEntropyLoss", {"label_smoothing": 0.1}, False, False),
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(FALLBACKS))
def test_unsupported_arguments_take_the_torch_path(name):
    import torch.nn as nn
    kind, kw, prob, index = FALLBACKS[name]
    shape = (2, 3, 4, 6, 8)
    consts = {"ones3": torch.full((3, 1, 1, 1), 1.5, device="cuda"), "w3": torch.tensor([0.5, 1.0, 2.0], device="cuda")}
    kw = {k: consts.get(v, v) if isinstance(v, str) and v in consts else v for k, v in kw.items()}
    x, t = _pair(shape, prob=prob)
    if index:
        t = torch.randint(0, 3, (2, 4, 6, 8), device="cuda")
    out = []
    for cls in (_losses()[kind], getattr(nn, kind)):
        xa = x.clone().requires_grad_(True)
        l = cls(**kw)(xa, t)
        l.sum().backward()
        out.append((l, xa.grad))
    assert "_ElemLossFn" not in type(out[0][0].grad_fn).__name__ and "_CrossEntropyFn" not in type(out[0][0].grad_fn).__name__
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])


@pytest.mark.gpu
def test_zsmooth_falls_back_where_it_is_not_eligible():
    """reduction="none" keeps the torch expression; the eligible call next to it takes the kernel"""
    fn_none = _losses()["BCEWithLogitsLossZSmooth"](reduction="none")
    x, t = _pair((1, 2, 5, 6, 8))
    xa = x.clone().requires_grad_(True)
    l = fn_none(xa, t)
    assert l.shape == x.shape and "_ElemLossFn" not in type(l.grad_fn).__name__
    lm = _losses()["BCEWithLogitsLossZSmooth"]()(xa, t)
    assert "_ElemLossFn" in type(lm.grad_fn).__name__
    assert abs(lm.item() - l.mean().item()) < 2e-6


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["BCEWithLogitsLossLabelSmoothing", "BCEWithLogitsLossZSmooth", "BCELoss", "MSELoss", "CrossEntropyLoss"])
def test_bf16_prediction_gets_a_bf16_gradient(kind):
    """`_as_f32c`: the kernels see fp32; the gradient comes back in the prediction's dtype, the fp32 result rounded once"""
    x, t = _pair((1, 3, 5, 7, 9), prob=kind == "BCELoss")
    xb = x.to(torch.bfloat16)
    fn = _losses()[kind]()
    a = xb.clone().requires_grad_(True)
    la = fn(a, t); la.backward()
    b = xb.float().requires_grad_(True)
    lb = fn(b, t); lb.backward()
    assert a.grad.dtype == torch.bfloat16 and la.dtype == torch.float32
    assert torch.equal(la, lb) and torch.equal(a.grad, b.grad.to(torch.bfloat16))


def _torch_formulation(kind, kw, x, t):
    """the formulation the CPU path uses, on whatever device x lives"""
    import torch.nn as nn
    import torch.nn.functional as F
    if kind in ("BCEWithLogitsLoss", "BCELoss", "MSELoss", "CrossEntropyLoss"):
        return getattr(nn, kind)(**kw)(x, t)
    if kind == "BCEWithLogitsLossLabelSmoothing":
        s = kw.get("smoothing", 0.1)
        return F.binary_cross_entropy_with_logits(x, t * (1.0 - 2.0 * s) + s)
    d = x.shape[2]
    z = torch.arange(d, device=x.device, dtype=x.dtype)
    alpha = (0.1 + (0.4 - 0.1) * ((z - (d - 1) / 2.0).abs() / (d // 2))).view(1, 1, d, 1, 1)
    return F.binary_cross_entropy_with_logits(x, t * (1.0 - 2.0 * alpha) + alpha)


LARGE = {    # name -> (class, shape, target mode)
    "bcel": ("BCEWithLogitsLoss", (2, 3, 40, 48, 56), "binary"),
    "bcels": ("BCEWithLogitsLossLabelSmoothing", (2, 3, 40, 48, 56), "binary"),
    "zs": ("BCEWithLogitsLossZSmooth", (2, 3, 40, 48, 56), "binary"),
    "bce": ("BCELoss", (2, 3, 40, 48, 56), "binary"),
    "mse": ("MSELoss", (2, 3, 40, 48, 56), "binary"),
    "ce_prob_c3": ("CrossEntropyLoss", (2, 3, 40, 48, 56), "prob"),
    "ce_idx_c3": ("CrossEntropyLoss", (2, 3, 40, 48, 56), "index"),
    "ce_prob_c12": ("CrossEntropyLoss", (1, 12, 40, 48, 56), "prob"),
    "ce_idx_c12": ("CrossEntropyLoss", (1, 12, 40, 48, 56), "index"),
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(LARGE))
def test_larger_shapes_against_device_torch_formulation(name):
    kind, shape, mode = LARGE[name]
    x, t = _pair(shape, seed=9, prob=kind == "BCELoss")
    g = torch.Generator(device="cuda").manual_seed(10)
    if mode == "prob":
        t = torch.softmax(torch.randn(shape, device="cuda", generator=g) * 2.0, dim=1)
    elif mode == "index":
        t = torch.randint(0, shape[1], (shape[0], *shape[2:]), device="cuda", generator=g)
        t[torch.rand(t.shape, device="cuda", generator=g) < 0.3] = -100
    xa = x.clone().requires_grad_(True)
    la = _losses()[kind]()(xa, t); (la * 0.5).backward()
    assert _node(kind) in type(la.grad_fn).__name__
    xb = x.clone().requires_grad_(True)
    lb = _torch_formulation(kind, {}, xb, t); (lb * 0.5).backward()
    r = rel_l2(xa.grad.cpu(), xb.grad.cpu())
    print(f"{name}: loss {la.item():.7f} torch {lb.item():.7f} |diff| {abs(la.item() - lb.item()):.3e}, grad rel-L2 {r:.3e}")
    assert abs(la.item() - lb.item()) < 2e-6
    assert r < 2e-5
