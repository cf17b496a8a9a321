"""GPU: rx_seg_counts, rx_class_counts and rx_normal_stats (csrc/rx_metrics.hip) through engine.ops against the numpy statements of
training/metrics, and `ValidationMetrics` on a 16^3 two-head model.  Every count is compared with `==`.

The float sums of normal_stats have a MEASURED tolerance: the per-voxel formula evaluated in numpy float32 (summed in float64)
deviates from the float64 statement by e0 on the very inputs of the test -- that is what float32 costs there, acos' conditioning
near parallel vectors included -- and the kernel, which differs from that evaluation by acosf and a few ulp per voxel, may deviate
from the statement by 4 * e0, per sample and sum."""
import math
import os

import numpy as np
import pytest
import torch

import mt3d_amd  # noqa: F401
from mt3d_amd.training import metrics as M

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "tasks", "synthetic_sheet.yaml")
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
NAN, INF = float("nan"), float("inf")
# smallest input; V = 385: head and tail, odd V; V = 88440: several workgroups per row, so the atomics combine
SHAPES = [(1, 1, 1, 1, 1), (2, 3, 5, 7, 11), (2, 2, 33, 40, 67)]
CLASS_SHAPES = [(1, 64, 3, 5, 7), (2, 2, 9, 9, 9), (2, 3, 5, 7, 11), (2, 5, 33, 40, 67)]
# ... and V = 599760: more 16-byte units than 512 chunks of 256 hold, so the chunks of a sample grow instead of their number
NORMAL_SHAPES = [(1, 3, 1, 1, 1), (2, 3, 5, 7, 11), (2, 3, 33, 40, 67), (1, 3, 84, 84, 85)]
_CASES = {}


def ops():
    from mt3d_amd.engine import ops as E
    return E


def host(t):
    """what the oracle sees: the tensor's exact values as float32 (int64 stays)"""
    return t.numpy() if t.dtype == torch.int64 else t.float().numpy()


def rows(t):
    return t.reshape(t.shape[0], t.shape[1], -1)


def seg_case(shape, dtype):
    """prediction in `dtype` (generated there), float32 target, thresholds, oracle; made once, never written to"""
    key = ("seg", shape, dtype)
    if key not in _CASES:
        g = torch.Generator().manual_seed(sum(shape) + DTYPES.index(dtype))
        thr_p, thr_t = 0.25, 0.5           # both exact in every dtype
        pred = torch.randn(shape, generator=g).to(dtype)
        target = (torch.rand(shape, generator=g) > 0.6).float() * torch.rand(shape, generator=g)
        r, t = rows(pred), rows(target)
        if r.shape[2] > 1:
            # non-finite and threshold-equal values at the first and the last voxel of rows
            r[0, 0, 0], r[0, 0, -1], r[-1, -1, 0], r[-1, -1, -1] = NAN, thr_p, INF, -INF
            t[0, 0, 0], t[0, 0, -1], t[-1, -1, 0], t[-1, -1, -1] = 1.0, 1.0, NAN, INF
            t[-1, 0, 0], t[-1, 0, -1], r[-1, 0, 0], r[-1, 0, -1] = thr_t, INF, 1.0, 1.0
        want = M.seg_counts_numpy(host(pred), host(target), thr_p, thr_t)
        _CASES[key] = (pred, target, thr_p, thr_t, want)
    return _CASES[key]


def class_case(shape, dtype, index):
    key = ("class", shape, dtype, index)
    if key not in _CASES:
        g = torch.Generator().manual_seed(7 * sum(shape) + DTYPES.index(dtype))
        n, c = shape[:2]
        pred = (torch.randn(shape, generator=g) * 2).to(dtype)          # 16-bit values tie now and then: the first maximum wins
        r = rows(pred)
        r[0, :, 0] = 1.5                       # a full tie at the first voxel
        r[-1, 0, -1], r[-1, 1, -1] = NAN, -3.0  # a NaN in class 0 at the last voxel: never chosen over a number
        r[0, c - 1, -1] = INF
        if index:
            target = torch.randint(0, c, (n,) + shape[2:], generator=g)
            flat = target.reshape(n, -1)
            flat[:, ::5] = -100
            flat[0, 0], flat[-1, -1] = 1, 0
            if flat.shape[1] > 3:
                flat[0, 1], flat[0, 2] = c, -7          # no class at all: skipped
        else:
            target = torch.rand(shape, generator=g)
            rows(target)[0, :, 0] = 0.25
            rows(target)[-1, c - 1, -1] = NAN
        want = M.class_counts_numpy(host(pred), host(target), -100)
        _CASES[key] = (pred, target, want)
    return _CASES[key]


def normal_case(shape, dtype, same=False):
    """random vectors, about half the targets zeroed; `same`: pred == target, where acos is ill-conditioned.  -> pred, target,
    count, the float64 sums, e0"""
    key = ("normal", shape, dtype, same)
    if key not in _CASES:
        g = torch.Generator().manual_seed(3 * sum(shape) + DTYPES.index(dtype))
        target = torch.randn(shape, generator=g)
        target = target * (torch.rand((shape[0], 1) + shape[2:], generator=g) > 0.5)
        if same:
            target = target.to(dtype).float()
            pred = target.to(dtype)
        else:
            pred = torch.randn(shape, generator=g).to(dtype)
        count, sums = M.normal_stats_numpy(host(pred), host(target))
        c32, s32 = M.normal_stats_numpy(host(pred), host(target), dtype=np.float32)
        assert np.array_equal(count, c32)
        _CASES[key] = (pred, target, count, sums, np.abs(s32 - sums))
    return _CASES[key]


def check_sums(got, want, e0, what):
    dev = np.abs(got - want)
    print(f"normal_stats {what}: deviation {dev.tolist()} e0 {e0.tolist()} bound {(4 * e0).tolist()}")
    assert (dev <= 4 * e0).all(), (what, dev, e0)


# ---- seg_counts -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_seg_counts_equal_the_statement(shape, dtype):
    pred, target, thr_p, thr_t, want = seg_case(shape, dtype)
    got = ops().seg_counts(pred.cuda(), target.cuda(), thr_p, thr_t)
    assert got.dtype == torch.int64 and got.shape == want.shape
    assert np.array_equal(got.cpu().numpy(), want)
    v = pred.numel() // (pred.shape[0] * pred.shape[1])
    assert (want.sum(-1) <= v).all() and (shape[-1] == 1 or want.sum() > 0)


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_seg_counts_on_bases_that_are_only_element_aligned(dtype):
    """views of flat buffers at element offset 1 (4 bytes for float32, 2 for the 16-bit types): the prediction alone, the target
    alone (its 16-byte loads then straddle the prediction's), and both"""
    shape = SHAPES[1]
    pred, target, thr_p, thr_t, want = seg_case(shape, dtype)
    n = pred.numel()

    def off1(t):
        flat = torch.full((n + 9,), -9.0 if t.dtype != torch.float32 else NAN, dtype=t.dtype, device="cuda")
        flat[1:n + 1] = t.reshape(-1).cuda()
        v = flat[1:n + 1].view(shape)
        assert v.data_ptr() % 16 == t.element_size() and v.is_contiguous()
        return v
    for p, t in ((off1(pred), target.cuda()), (pred.cuda(), off1(target)), (off1(pred), off1(target))):
        assert np.array_equal(ops().seg_counts(p, t, thr_p, thr_t).cpu().numpy(), want)
    big = seg_case(SHAPES[2], dtype)
    flat = torch.zeros(big[0].numel() + 3, dtype=dtype, device="cuda")
    flat[3:] = big[0].reshape(-1).cuda()
    assert np.array_equal(ops().seg_counts(flat[3:].view(SHAPES[2]), big[1].cuda(), big[2], big[3]).cpu().numpy(), big[4])


def test_seg_counts_add_into_out_and_repeat_bit_for_bit():
    E = ops()
    a, b = seg_case(SHAPES[2], torch.float32), seg_case(SHAPES[2], torch.bfloat16)
    out = torch.zeros(a[4].shape, dtype=torch.int64, device="cuda")
    assert E.seg_counts(a[0].cuda(), a[1].cuda(), a[2], a[3], out=out) is out
    E.seg_counts(b[0].cuda(), b[1].cuda(), b[2], b[3], out=out)
    assert np.array_equal(out.cpu().numpy(), a[4] + b[4])
    again = E.seg_counts(a[0].cuda(), a[1].cuda(), a[2], a[3])
    assert torch.equal(again, E.seg_counts(a[0].cuda(), a[1].cuda(), a[2], a[3])) and np.array_equal(again.cpu().numpy(), a[4])
    # a non-contiguous prediction is made contiguous; other thresholds, -0.0 included
    wide = torch.zeros(SHAPES[1][:-1] + (SHAPES[1][-1] + 5,), device="cuda")
    c = seg_case(SHAPES[1], torch.float32)
    view = wide[..., 5:]
    view.copy_(c[0])
    assert not view.is_contiguous() and np.array_equal(E.seg_counts(view, c[1].cuda(), c[2], c[3]).cpu().numpy(), c[4])
    for tp_, tt_ in ((-0.0, 0.0), (math.log(0.3 / 0.7), 0.1), (INF, -INF)):
        assert np.array_equal(E.seg_counts(c[0].cuda(), c[1].cuda(), tp_, tt_).cpu().numpy(), M.seg_counts_numpy(host(c[0]), host(c[1]), tp_, tt_))


# ---- class_counts -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index", [False, True], ids=["prob", "index"])
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("shape", CLASS_SHAPES, ids=str)
def test_class_counts_equal_the_statement(shape, dtype, index):
    pred, target, want = class_case(shape, dtype, index)
    got = ops().class_counts(pred.cuda(), target.cuda())
    assert got.dtype == torch.int64 and np.array_equal(got.cpu().numpy(), want)
    assert want.sum() > 0 and (want[..., 1].sum(1) == want[..., 2].sum(1)).all()


def test_class_counts_offset_views_accumulation_and_repeats():
    E = ops()
    shape = CLASS_SHAPES[2]
    for dtype in DTYPES:
        for index in (False, True):
            pred, target, want = class_case(shape, dtype, index)
            fp = torch.zeros(pred.numel() + 1, dtype=dtype, device="cuda")
            fp[1:] = pred.reshape(-1).cuda()
            ft = torch.zeros(target.numel() + 1, dtype=target.dtype, device="cuda")
            ft[1:] = target.reshape(-1).cuda()
            assert np.array_equal(E.class_counts(fp[1:].view(shape), ft[1:].view(target.shape)).cpu().numpy(), want)
    a, b = class_case(CLASS_SHAPES[3], torch.float32, False), class_case(CLASS_SHAPES[3], torch.float16, True)
    out = torch.zeros(a[2].shape, dtype=torch.int64, device="cuda")
    E.class_counts(a[0].cuda(), a[1].cuda(), out=out)
    E.class_counts(b[0].cuda(), b[1].cuda(), out=out)
    assert np.array_equal(out.cpu().numpy(), a[2] + b[2])
    assert torch.equal(E.class_counts(b[0].cuda(), b[1].cuda()), E.class_counts(b[0].cuda(), b[1].cuda()))
    other = E.class_counts(b[0].cuda(), b[1].cuda(), ignore_index=1)
    assert np.array_equal(other.cpu().numpy(), M.class_counts_numpy(host(b[0]), host(b[1]), 1))


# ---- normal_stats -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("same", [False, True], ids=["random", "pred==target"])
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("shape", NORMAL_SHAPES, ids=str)
def test_normal_stats_count_is_exact_and_sums_are_within_the_measured_bound(shape, dtype, same):
    pred, target, count, sums, e0 = normal_case(shape, dtype, same)
    c, s = ops().normal_stats(pred.cuda(), target.cuda())
    assert c.dtype == torch.int64 and s.dtype == torch.float64 and s.shape == (shape[0], 2)
    assert np.array_equal(c.cpu().numpy(), count)
    check_sums(s.cpu().numpy(), sums, e0, f"{shape} {dtype} same={same}")
    c2, s2 = ops().normal_stats(pred.cuda(), target.cuda())
    assert torch.equal(c, c2) and torch.equal(s.view(torch.int64), s2.view(torch.int64))          # the same bits


def test_normal_stats_offset_views_specials_and_accumulation():
    E = ops()
    shape = NORMAL_SHAPES[1]
    for dtype in DTYPES:
        pred, target, count, sums, e0 = normal_case(shape, dtype)
        fp = torch.zeros(pred.numel() + 1, dtype=dtype, device="cuda")
        fp[1:] = pred.reshape(-1).cuda()
        ft = torch.zeros(target.numel() + 1, device="cuda")
        ft[1:] = target.reshape(-1).cuda()
        c, s = E.normal_stats(fp[1:].view(shape), ft[1:].view(shape))
        assert np.array_equal(c.cpu().numpy(), count)
        check_sums(s.cpu().numpy(), sums, e0, f"offset 1 {dtype}")
    # the mask's edge and the clamps at the first and last voxel of a sample: count exact, sums under the bound measured on them
    pred, target, *_ = normal_case(NORMAL_SHAPES[2], torch.float32)
    pred, target = pred.clone(), target.clone()
    p, t = rows(pred), rows(target)
    t[0, :, 0] = torch.tensor([1e-7, 1e-7, 1e-7])           # below the mask
    t[0, :, -1] = torch.tensor([1e-6, 1e-6, 0.0])            # just inside
    p[0, :, -1] = 0.0                                        # |p| under its clamp: cos = 0
    t[1, :, 0], p[1, :, 0] = torch.tensor([0.0, 2.0, 0.0]), torch.tensor([0.0, -5.0, 0.0])      # cos = -1 exactly
    t[1, :, -1], p[1, :, -1] = torch.tensor([3.0, 0.0, 0.0]), torch.tensor([0.5, 0.0, 0.0])     # cos = 1 exactly
    count, sums = M.normal_stats_numpy(host(pred), host(target))
    e0 = np.abs(M.normal_stats_numpy(host(pred), host(target), dtype=np.float32)[1] - sums)
    out = (torch.zeros(2, dtype=torch.int64, device="cuda"), torch.zeros((2, 2), dtype=torch.float64, device="cuda"))
    got = E.normal_stats(pred.cuda(), target.cuda(), out=out)
    assert got[0] is out[0] and got[1] is out[1] and np.array_equal(out[0].cpu().numpy(), count)
    check_sums(out[1].cpu().numpy(), sums, e0, "planted")
    first = out[1].clone()
    E.normal_stats(pred.cuda(), target.cuda(), out=out)      # a second call into the same buffers: the sum of the two
    assert np.array_equal(out[0].cpu().numpy(), 2 * count) and torch.equal(out[1], first + first)


def test_wrappers_refuse_what_the_kernels_do_not_take():
    E = ops()
    from mt3d_amd.engine.lib import RxError
    pred, target, thr_p, thr_t, want = seg_case(SHAPES[1], torch.float32)
    p, t = pred.cuda(), target.cuda()
    out = torch.zeros(want.shape, dtype=torch.int64, device="cuda")
    for bad in (lambda: E.seg_counts(pred, t), lambda: E.seg_counts(p, target), lambda: E.seg_counts(p.double(), t),
                lambda: E.seg_counts(p, t.half()), lambda: E.seg_counts(p, t[:, :2]), lambda: E.seg_counts(p, t, out=out.int()),
                lambda: E.seg_counts(p, t, out=out[:1]), lambda: E.seg_counts(p, t, out=out.cpu()),
                lambda: E.seg_counts(p, t, NAN), lambda: E.class_counts(p[:, :1], t[:, :1]),
                lambda: E.class_counts(p, t[:, 0].long()[:, :2]), lambda: E.class_counts(p, t.double()),
                lambda: E.normal_stats(p[:, :2], t[:, :2]), lambda: E.normal_stats(p, t, out=out),
                lambda: E.normal_stats(p, t, out=(out, out)), lambda: E.normal_stats(p.cpu(), t)):
        with pytest.raises(RxError):
            bad()
    torch.cuda.synchronize()
    assert int(out.abs().sum()) == 0
    with pytest.raises(RxError, match="rx_class_counts.*status -1"):
        E.class_counts(torch.zeros((1, 65, 4), device="cuda"), torch.zeros((1, 65, 4), device="cuda"))


# ---- ValidationMetrics on a 16^3 two-head model -------------------------------------------------------------------------------------
def _model(tmp_path, sheet_activation):
    import yaml
    from mt3d_amd.train import BaseTrainer
    cfg = yaml.safe_load(open(CFG))
    cfg["tr_config"]["patch_size"] = [16, 16, 16]
    cfg["dataset_config"]["targets"] = {
        "sheet": {"channels": 1, "activation": sheet_activation, "weight": 1, "loss_fn": "BCEDiceLoss", "loss_kwargs": {"alpha": 0.5, "beta": 0.5}},
        "normals": {"channels": 3, "activation": "none", "weight": 1, "loss_fn": "MaskedCosineLoss"},
    }
    p = tmp_path / f"cfg_{sheet_activation}.yaml"
    yaml.safe_dump(cfg, open(p, "w"))
    tr = BaseTrainer(str(p), verbose=False)
    return tr, tr._build_model().to("cuda").eval()


def test_validation_metrics_equal_the_statements_over_three_batches(tmp_path):
    tr, model = _model(tmp_path, "sigmoid")
    tr_none, model_none = _model(tmp_path, "none")
    model_none.load_state_dict(model.state_dict())
    thr = 0.4
    vm = M.ValidationMetrics(tr.mgr.tasks, {"threshold": thr, "target_threshold": 0.5})
    vm_none = M.ValidationMetrics(tr_none.mgr.tasks, {"threshold": thr})
    assert vm.kinds == {"sheet": "binary", "normals": "normals"} and vm.thr_pred["sheet"] == thr
    assert vm_none.thr_pred["sheet"] == math.log(thr / (1 - thr))
    ds = tr._configure_dataset()
    seen = []
    mode = torch.cuda.get_sync_debug_mode()
    for b in range(3):
        items = [ds[2 * b], ds[2 * b + 1]]
        batch = {k: torch.stack([it[k] for it in items]).to("cuda", dtype=torch.float32) for k in items[0]}
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            out = model(batch["image"])
            out_none = model_none(batch["image"])
        targets = {k: v for k, v in batch.items() if k != "image"}
        torch.cuda.set_sync_debug_mode("error")          # a host synchronisation inside update raises
        try:
            vm.update(out, targets)
            vm_none.update(out_none, targets)
        finally:
            torch.cuda.set_sync_debug_mode(mode)
        seen.append(({k: v.float().cpu().numpy() for k, v in out.items()}, {k: v.cpu().numpy() for k, v in targets.items()}))
    got, got_none = vm.compute(), vm_none.compute()
    # the statements on the same outputs
    counts = sum(M.seg_counts_numpy(o["sheet"], t["sheet"], thr, 0.5) for o, t in seen)
    assert np.array_equal(vm.counts("sheet"), counts.sum(0)) and counts.sum() > 0
    want = M.scores_from_counts(*counts.sum((0, 1)))
    for k in M.RATES:
        assert got["sheet"][k] == want[k] or (math.isnan(got["sheet"][k]) and math.isnan(want[k])), k
    per = np.concatenate([M.seg_counts_numpy(o["sheet"], t["sheet"], thr, 0.5).sum(1) for o, t in seen]).astype(np.float64)      # six patches
    den = 2 * per[:, 0] + per[:, 1] + per[:, 2]
    assert got["sheet"]["dice_per_patch"] == pytest.approx(float((2 * per[:, 0] / den)[den > 0].mean()), rel=1e-12)
    assert set(got["sheet"]) == set(M.metric_names("binary")) and set(got["normals"]) == set(M.metric_names("normals"))
    # logits against the threshold in logit space: the same voxels as the probabilities against the threshold
    assert np.array_equal(vm_none.counts("sheet"), vm.counts("sheet"))
    assert got_none["sheet"] == got["sheet"] or all(math.isnan(v) for v in got["sheet"].values())
    stats = [M.normal_stats_numpy(o["normals"], t["normals"]) for o, t in seen]
    stats32 = [M.normal_stats_numpy(o["normals"], t["normals"], dtype=np.float32) for o, t in seen]
    cnt = int(sum(c.sum() for c, _ in stats))
    sums = sum(s.sum(0) for _, s in stats)
    e0 = np.abs(sum(s.sum(0) for _, s in stats32) - sums)
    assert cnt > 0 and got["normals"]["masked_voxels"] == cnt
    dev = np.abs(np.array([got["normals"]["mean_cos"], got["normals"]["mean_angle_deg"]]) * cnt - sums)
    print(f"ValidationMetrics normals: deviation {dev.tolist()} e0 {e0.tolist()}")
    assert (dev <= 4 * e0 + 4 * np.spacing(np.abs(sums))).all(), (dev, e0)      # (+ the rounding of mean * count in this very line)
    assert 0.0 <= got["normals"]["mean_angle_deg"] <= 180.0 and -1.0 <= got["normals"]["mean_cos"] <= 1.0
    # reset clears the state; an epoch of one batch is that batch's statement
    vm.reset()
    assert all(math.isnan(v) for v in vm.compute()["sheet"].values()) and vm.compute()["normals"]["masked_voxels"] == 0.0
    o, t = seen[0]
    vm.update({k: torch.from_numpy(v).cuda() for k, v in o.items()}, {k: torch.from_numpy(v).cuda() for k, v in t.items()})
    assert np.array_equal(vm.counts("sheet"), M.seg_counts_numpy(o["sheet"], t["sheet"], thr, 0.5).sum(0))


def test_validation_metrics_multiclass_through_class_counts():
    tasks = {"classes": {"channels": 5, "activation": "softmax", "loss_fn": "CrossEntropyLoss"}}
    vm = M.ValidationMetrics(tasks, True)
    assert vm.kinds == {"classes": "multiclass"}
    total = 0
    for index in (False, True):
        pred, target, want = class_case(CLASS_SHAPES[3], torch.float32, index)
        vm.update({"classes": pred.cuda()}, {"classes": target.cuda()})
        total = total + want
    got = vm.compute()["classes"]
    assert np.array_equal(vm.counts("classes"), total.sum(0))
    pooled = M.scores_from_counts(*total.sum((0, 1)))
    per_class = M.scores_from_counts(*(total.sum(0)[:, i] for i in range(3)))
    for r in M.RATES:
        assert got[r] == pooled[r] and got[f"{r}_class_mean"] == pytest.approx(float(np.nanmean(per_class[r])), rel=1e-12)
    assert 0.0 < got["dice_per_patch"] < 1.0
