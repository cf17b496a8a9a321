"""CPU: the fp64 loss reference of tests/loss_ref.py and its per-element bounds, checked without a device.

  * the reference reproduces tests/golden/losses.npz and tests/golden/losses_extra.npz (vectors of the reference's own classes), loss
    and gradient, with the bounds the existing CPU tests use for the host formulation;
  * over the WHOLE case table of tests/test_loss_ops_gpu.py, fp32 CPU torch on the host formulation stays within a quarter of the
    per-element bound and meets the scalar bound: the bounds are not too tight; a single element moved by 1e-4 of its magnitude M
    breaks them: they are not vacuous;
  * the masked-cosine gradient under the 1e-8 clamp is the ordinary one, and finite at pred == 0 (what the kernel must follow).

No element of any case is left out of a comparison (the cap is 0 % of the elements): the reference is asserted finite everywhere."""
import pytest
import torch

import loss_ref as R
import test_losses as T0
import test_losses_extra as T1

CASES = R.all_cases()


def _golden(name):
    if name in T0.CASES:
        kind, kw, weight = T0.CASES[name]
        return T0.GOLD, kind, kw, weight
    kind, _, _, kw, weight, _ = T1.CASES[name]
    return T1.GOLD, kind, kw, weight


@pytest.mark.parametrize("name", list(T0.CASES) + list(T1.CASES))
def test_reference_reproduces_the_golden_vectors(name):
    gold, kind, kw, weight = _golden(name)
    x, t = torch.from_numpy(gold[f"{name}.pred"]), torch.from_numpy(gold[f"{name}.target"])
    ref = R.reference(kind, x, t, kw, g=weight)
    if kw.get("reduction") == "sum":        # an fp32 sum of ~1000 against the fp64 one: the floor of the sum_margin rule, relative
        assert abs(float(ref["loss"]) - float(gold[f"{name}.loss"])) < 2e-6 * abs(float(gold[f"{name}.loss"]))
    else:
        assert abs(float(ref["loss"]) - float(gold[f"{name}.loss"])) < 1e-6
    want = torch.from_numpy(gold[f"{name}.grad"]).double()
    assert (ref["grad"] - want).abs().max().item() <= 1e-7 + 1e-5 * want.abs().max().item()
    if f"{name}.loss64" in gold.files:      # the fixture's fp64 run holds the smoothing constants as doubles, this one as fp32 values
        assert abs(float(ref["loss"]) - float(gold[f"{name}.loss64"])) <= 1e-8 * max(1.0, abs(float(gold[f"{name}.loss64"])))


def test_case_table_is_the_issues():
    ids = [c["id"] for c in CASES]
    assert len(set(ids)) == len(ids)
    assert {c["name"] for c in CASES} == {"BCEDiceLoss", "MaskedCosineLoss", "CrossEntropyLoss", *R.ELEMENTWISE}
    assert max(c["make"]()[0].numel() for c in CASES if "C1024" in c["id"] or "600" in c["id"]) <= 3.2e6


@pytest.mark.parametrize("group", sorted({c["group"] for c in CASES}), ids=lambda g: "-".join(g))
def test_fp32_cpu_torch_within_a_quarter_of_the_bound(group):
    worst = (0.0, "")
    for case in (c for c in CASES if c["group"] == group):
        name, kw = case["name"], case["kw"]
        x, t = case["make"]()
        assert torch.equal(x.double().float(), x)
        ref = R.reference(name, x, t, kw)
        assert torch.isfinite(ref["grad"]).all() and torch.isfinite(ref["M"]).all(), case["id"]     # nothing is left out
        loss32, grad32 = R.run_host(name, x, t, kw, torch.float32)
        R.assert_elementwise(grad32, ref["grad"], ref["M"], ref["rel"], f"{case['id']} fp32 CPU torch", ref["floor"], limit=0.25)
        ok, text = R.loss_ok(float(loss32), float(ref["loss"]), kw, float(loss32))
        assert ok, f"{case['id']}: {text}"
        ratio = R.worst_ratio(grad32, ref["grad"], ref["M"], ref["rel"], ref["floor"])[0]
        worst = max(worst, (ratio, case["id"]))
    print(f"{group}: fp32 CPU torch largest |got - ref| / bound {worst[0]:.3f} ({worst[1]})")


@pytest.mark.parametrize("name", ["BCEWithLogitsLossLabelSmoothing", "BCELoss", "MSELoss", "BCEDiceLoss", "MaskedCosineLoss", "CrossEntropyLoss"])
def test_bound_is_not_vacuous(name):
    """one element moved by 1e-4 of its own magnitude M (where M > 0) is outside the bound"""
    case = next(c for c in CASES if c["name"] == name and ("odd_planes" in c["id"] or "C3-V8193" in c["id"] or "prob-C3-V2049-mean" in c["id"]))
    x, t = case["make"]()
    ref = R.reference(name, x, t, case["kw"])
    i = int((ref["M"].flatten() > 0).nonzero()[-1])
    bad = ref["grad"].clone()
    bad.view(-1)[i] += 1e-4 * ref["M"].flatten()[i]
    with pytest.raises(AssertionError, match="outside the bound"):
        R.assert_elementwise(bad, ref["grad"], ref["M"], ref["rel"], "moved", ref["floor"])


# ---- the masked-cosine gradient under the clamps -------------------------------------------------------------------------------------
def _cos_grad(p, t, dtype=torch.float64):
    x = p.to(dtype).view(1, -1, 1)
    return R.run_host("MaskedCosineLoss", x, t.to(dtype).view(1, -1, 1), {}, dtype, g=1.0)[1].view(-1).double()


@pytest.mark.parametrize("pn", [1e-15, 3e-13, 2e-9, 9.9e-9])
def test_cosine_gradient_below_the_clamp_is_the_ordinary_one(pn):
    """|pred| in [1e-15, 1e-8): unit = pred / 1e-8 is linear in pred and the cosine is scale-invariant, so torch's graph gives
    -(t^ - cos p^) / |pred| / (sum m + 1e-8), components of 1e7 and more -- not zero.  fp32 autograd agrees."""
    d = torch.tensor([0.3, -0.5, 0.81], dtype=torch.float64)
    p = (d / d.norm() * pn).float().double()
    t = torch.tensor([0.2, 0.9, -0.4], dtype=torch.float64)
    ph, th = p / p.norm(), t / t.norm()
    want = -(th - (ph * th).sum() * ph) / p.norm() / (1.0 + 1e-8)
    got = _cos_grad(p, t)
    assert (got - want).abs().max() <= 1e-9 * want.abs().max()
    assert want.abs().max() >= 1e7
    got32 = _cos_grad(p, t, torch.float32)
    assert (got32 - want).abs().max() <= 1e-5 * want.abs().max()


def test_cosine_gradient_at_zero_prediction_is_finite():
    """pred == 0: -t^ * 1e16 / (sum m + 1e-8)"""
    t = torch.tensor([0.2, 0.9, -0.4], dtype=torch.float64)
    want = -(t / t.norm()) * 1e16 / (1.0 + 1e-8)
    got = _cos_grad(torch.zeros(3, dtype=torch.float64), t)
    assert (got - want).abs().max() <= 1e-9 * want.abs().max()


def test_reference_magnitude_follows_the_cosine_clamps():
    """M of loss_ref at |pred| = 0, 5e-9, 1: the closed form's own scale factor (1e16, 1/|pred|, 1/|pred|)"""
    t = torch.tensor([[0.0], [1.0], [0.0]]).view(1, 3, 1)
    for pn, scale in ((0.0, 1e16), (5e-9, 1.0 / float(torch.tensor(5e-9, dtype=torch.float32))), (1.0, 1.0)):
        x = (torch.tensor([[1.0], [0.0], [0.0]]).view(1, 3, 1) * pn).float()
        m = R.reference("MaskedCosineLoss", x, t, {}, g=1.0)["M"].view(-1)
        assert abs(m[1].item() / (scale / (1.0 + 1e-8)) - 1.0) < 1e-6, (pn, m)
