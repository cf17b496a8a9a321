"""CPU: the numpy statements of the validation metrics against brute-force loops, the scores, kind inference, the threshold rule,
config rejection, the C ABI's argument checks (no device is touched) and the name of the best checkpoint."""
import ctypes
import math
import os

import numpy as np
import pytest

import mt3d_amd  # noqa: F401
from mt3d_amd.training import metrics as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "tasks", "synthetic_sheet.yaml")
NAN, INF = float("nan"), float("inf")


# ---- brute force ------------------------------------------------------------------------------------------------------------------
def brute_seg(pred, target, tp_, tt_):
    n, c = pred.shape[:2]
    p, t = pred.reshape(n, c, -1), target.reshape(n, c, -1)
    out = np.zeros((n, c, 3), dtype=np.int64)
    for i in range(n):
        for k in range(c):
            for v in range(p.shape[2]):
                a = bool(np.float32(p[i, k, v]) > np.float32(tp_))
                b = bool(np.float32(t[i, k, v]) > np.float32(tt_))
                out[i, k] += (a and b, a and not b, b and not a)
    return out


def brute_argmax(x):
    best = 0
    for k in range(1, len(x)):
        if x[k] > x[best] or (math.isnan(x[best]) and not math.isnan(x[k])):
            best = k
    return best


def brute_class(pred, target, ignore_index):
    n, c = pred.shape[:2]
    p = pred.reshape(n, c, -1)
    index = target.dtype.kind in "iu"
    t = target.reshape(n, -1) if index else target.reshape(n, c, -1)
    out = np.zeros((n, c, 3), dtype=np.int64)
    for i in range(n):
        for v in range(p.shape[2]):
            q = brute_argmax([float(a) for a in p[i, :, v]])
            if index:
                lab = int(t[i, v])
                if lab == ignore_index or not 0 <= lab < c:
                    continue
            else:
                lab = brute_argmax([float(a) for a in t[i, :, v]])
            if q == lab:
                out[i, lab, 0] += 1
            else:
                out[i, q, 1] += 1
                out[i, lab, 2] += 1
    return out


def brute_normals(pred, target):
    n = pred.shape[0]
    p, t = pred.reshape(n, 3, -1), target.reshape(n, 3, -1)
    count, sums = np.zeros(n, dtype=np.int64), np.zeros((n, 2))
    for i in range(n):
        for v in range(p.shape[2]):
            tx, ty, tz = (np.float32(a) for a in t[i, :, v])
            if not np.sqrt((tx * tx + ty * ty) + tz * tz) > np.float32(1e-6):
                continue
            a, b = [float(q) for q in p[i, :, v]], [float(q) for q in t[i, :, v]]
            pn = math.sqrt((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2])
            tn = math.sqrt((b[0] * b[0] + b[1] * b[1]) + b[2] * b[2])
            cos = ((a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]) / (max(pn, 1e-8) * max(tn, 1e-8))
            cos = min(max(cos, -1.0), 1.0)
            count[i] += 1
            sums[i] += (cos, math.acos(cos) * (180.0 / math.pi))
    return count, sums


# ---- the statements ---------------------------------------------------------------------------------------------------------------
def test_seg_counts_numpy_is_the_brute_force_count():
    rng = np.random.default_rng(0)
    pred = rng.standard_normal((2, 3, 2, 3, 5)).astype(np.float32)
    target = (rng.random((2, 3, 2, 3, 5)) > 0.5).astype(np.float32)
    specials = [NAN, INF, -INF, -0.0, 0.0, 0.25, np.nextafter(np.float32(0.25), np.float32(1)), np.nextafter(np.float32(0.25), np.float32(0))]
    pred.reshape(-1)[:len(specials)] = specials
    target.reshape(-1)[5:5 + len(specials)] = specials          # overlaps the prediction's specials: NaN against NaN, inf against 0.25 ...
    target.reshape(-1)[40:44] = [0.5, np.nextafter(np.float32(0.5), np.float32(1)), NAN, INF]
    for tp_, tt_ in ((0.25, 0.5), (0.0, 0.25), (-0.0, 0.0), (math.log(0.3 / 0.7), 0.5)):
        assert np.array_equal(M.seg_counts_numpy(pred, target, tp_, tt_), brute_seg(pred, target, tp_, tt_)), (tp_, tt_)
    got = M.seg_counts_numpy(pred, target, 0.25, 0.5)
    assert got.dtype == np.int64 and got.shape == (2, 3, 3)
    # a value exactly at the threshold is negative, the next float up is positive; a NaN is negative on either side
    one = np.array([0.25, np.nextafter(np.float32(0.25), np.float32(1)), NAN, INF], dtype=np.float32).reshape(1, 1, 4)
    lab = np.array([1.0, 1.0, 1.0, NAN], dtype=np.float32).reshape(1, 1, 4)
    assert M.seg_counts_numpy(one, lab, 0.25, 0.5).tolist() == [[[1, 1, 2]]]


def test_class_counts_numpy_is_the_brute_force_count():
    rng = np.random.default_rng(1)
    pred = rng.standard_normal((2, 4, 3, 7)).astype(np.float32)
    pred[0, :, 0, 0] = [1.0, 1.0, 0.5, 1.0]             # ties: the first maximum wins
    pred[0, :, 0, 1] = [NAN, 0.0, -1.0, NAN]            # a NaN is never chosen over a number
    pred[0, :, 0, 2] = [NAN, NAN, NAN, NAN]             # all NaN: class 0
    pred[0, :, 0, 3] = [-INF, -INF, INF, INF]
    pred[0, :, 0, 4] = [-0.0, 0.0, -0.0, 0.0]           # 0.0 > -0.0 is false: class 0
    pred[0, :, 0, 5] = [0.0, NAN, 3.0, 3.0]
    assert [brute_argmax([float(a) for a in pred[0, :, 0, j]]) for j in range(6)] == [0, 1, 0, 2, 0, 2]
    assert M.argmax_numpy(pred.reshape(2, 4, -1))[0, :6].tolist() == [0, 1, 0, 2, 0, 2]
    prob = rng.random((2, 4, 3, 7)).astype(np.float32)
    prob[1, :, 2, 6] = [0.5, 0.5, NAN, 0.25]
    index = rng.integers(0, 4, size=(2, 3, 7))
    index[0, 0, :3] = [-100, 7, -1]                     # ignore_index, and labels that are no class
    index[1, 2, 6] = -100
    for target, ig in ((prob, -100), (index, -100), (index, 2), (index.astype(np.int32), 3)):
        got = M.class_counts_numpy(pred, target, ig)
        assert got.dtype == np.int64 and np.array_equal(got, brute_class(pred, target, ig)), ig
    full = M.class_counts_numpy(pred, prob)
    assert (full[..., 0].sum(1) + full[..., 1].sum(1) == 21).all() and (full[..., 1].sum(1) == full[..., 2].sum(1)).all()


def test_normal_stats_numpy_is_the_brute_force_sum():
    rng = np.random.default_rng(2)
    pred = rng.standard_normal((2, 3, 4, 9)).astype(np.float32)
    target = rng.standard_normal((2, 3, 4, 9)).astype(np.float32)
    target[:, :, ::2, ::2] = 0.0                       # outside the mask
    target[0, :, 1, 1] = [1e-7, 1e-7, 1e-7]            # |t| = 1.7e-7: outside
    target[0, :, 1, 3] = [1e-6, 1e-6, 0.0]             # |t| = 1.4e-6: inside
    pred[0, :, 1, 3] = 0.0                             # |p| below its clamp: cos = 0
    pred[1, :, 3, 1] = target[1, :, 3, 1]              # parallel, and anti-parallel: the clamp to [-1, 1]
    pred[1, :, 3, 3] = -3.0 * target[1, :, 3, 3]
    count, sums = M.normal_stats_numpy(pred, target)
    bc, bs = brute_normals(pred, target)
    assert count.dtype == np.int64 and np.array_equal(count, bc) and 0 < count[0] < 36
    assert sums.dtype == np.float64 and np.allclose(sums, bs, rtol=1e-13, atol=1e-11)
    c32, s32 = M.normal_stats_numpy(pred, target, dtype=np.float32)
    assert np.array_equal(c32, count) and np.allclose(s32, sums, rtol=1e-5) and not np.array_equal(s32, sums)
    # 16-bit predictions are taken at their exact float32 values
    assert np.array_equal(M.seg_counts_numpy(pred.astype(np.float16), target), M.seg_counts_numpy(pred.astype(np.float16).astype(np.float32), target))


def test_scores_from_counts_and_its_nan_cases():
    s = M.scores_from_counts(6, 2, 4)
    assert s == {"dice": 12 / 18, "iou": 6 / 12, "precision": 6 / 8, "recall": 6 / 10}
    s = M.scores_from_counts(0, 0, 0)
    assert all(math.isnan(s[k]) for k in M.RATES)
    s = M.scores_from_counts(0, 3, 0)                   # predictions but no label: recall has nothing to divide by
    assert s["dice"] == 0.0 and s["iou"] == 0.0 and s["precision"] == 0.0 and math.isnan(s["recall"])
    s = M.scores_from_counts(0, 0, 5)
    assert s["dice"] == 0.0 and math.isnan(s["precision"]) and s["recall"] == 0.0
    s = M.scores_from_counts(np.array([1, 0]), np.array([1, 0]), np.array([0, 0]))
    assert s["dice"][0] == 2 / 3 and np.isnan(s["dice"][1]) and s["recall"][0] == 1.0


# ---- configuration ----------------------------------------------------------------------------------------------------------------
TASKS = {
    "sheet": {"channels": 1, "activation": "none", "loss_fn": "BCEDiceLoss"},
    "prob": {"channels": 2, "activation": "sigmoid"},
    "normals": {"channels": 3, "activation": "none", "loss_fn": "MaskedCosineLoss"},
    "dirs": {"channels": 3, "activation": "none"},
    "classes": {"channels": 3, "activation": "none", "loss_fn": "CrossEntropyLoss"},
    "soft": {"channels": 4, "activation": "softmax"},
    "soft1": {"channels": 1, "activation": "softmax"},
    "many": {"channels": 65, "activation": "sigmoid"},
}


def test_kind_inference_and_the_threshold_rule():
    kinds = {k: M.infer_kind(k, v) for k, v in TASKS.items()}
    assert kinds == {"sheet": "binary", "prob": "binary", "normals": "normals", "dirs": "binary", "classes": "multiclass",
                     "soft": "multiclass", "soft1": "binary", "many": "binary"}
    assert M.infer_kind("dirs", TASKS["dirs"], normal_keys=("dirs",)) == "normals"
    assert M.infer_kind("normals", TASKS["normals"], normal_keys=("dirs",)) == "binary"
    assert M.infer_kind("normals", {"channels": 2}) == "binary"
    assert M.pred_threshold(TASKS["prob"], 0.3) == 0.3
    assert M.pred_threshold(TASKS["sheet"], 0.5) == 0.0
    assert M.pred_threshold(TASKS["sheet"], 0.3) == math.log(0.3 / 0.7)
    assert M.pred_threshold({"channels": 1}, 0.9) == math.log(0.9 / (1 - 0.9))          # no activation key: logits
    # the rule keeps the positive set: sigmoid(x) > thr  <=>  x > logit(thr), away from the rounding of the boundary itself
    x = np.linspace(-6, 6, 2001)
    for thr in (0.1, 0.5, 0.77):
        lt = M.pred_threshold(TASKS["sheet"], thr)
        far = np.abs(x - lt) > 1e-9
        assert np.array_equal((1 / (1 + np.exp(-x)) > thr)[far], (x > lt)[far])
    cfg = M.parse_config(True, TASKS)
    assert cfg["threshold"] == cfg["target_threshold"] == 0.5 and cfg["best"] is None and cfg["kinds"] == kinds
    assert M.parse_config(None, TASKS) is None and M.parse_config(False, TASKS) is None
    cfg = M.parse_config({"threshold": 0.3, "tasks": {"sheet": {"kind": "binary"}, "many": {"kind": "none"}, "dirs": {"kind": "normals"}},
                          "best": {"task": "sheet", "metric": "dice"}}, TASKS)
    assert cfg["threshold"] == 0.3 and cfg["kinds"]["many"] == "none" and cfg["kinds"]["dirs"] == "normals"
    assert cfg["best"] == {"task": "sheet", "metric": "dice", "mode": "max"}
    vm = M.ValidationMetrics(TASKS, cfg)
    assert "many" not in vm.kinds and vm.thr_pred["sheet"] == math.log(0.3 / 0.7) and vm.thr_pred["prob"] == 0.3
    assert set(vm.compute()["normals"]) == {"mean_cos", "mean_angle_deg", "masked_voxels"}
    assert set(vm.compute()["classes"]) == set(M.RATES) | {f"{r}_class_mean" for r in M.RATES} | {"dice_per_patch"}


REJECTED = [
    ({"treshold": 0.5}, "treshold"),
    ({"threshold": 0.0}, "threshold"),
    ({"threshold": 1.0}, "threshold"),
    ({"threshold": "high"}, "threshold"),
    ({"target_threshold": 1.5}, "target_threshold"),
    ({"tasks": {"sheets": {"kind": "binary"}}}, "sheets"),
    ({"tasks": {"sheet": {"kind": "dice"}}}, "kind"),
    ({"tasks": {"sheet": {"kinds": "binary"}}}, "kinds"),
    ({"tasks": {"many": {"kind": "multiclass"}}}, "many"),
    ({"tasks": {"prob": {"kind": "normals"}}}, "prob"),
    ({"best": {"task": "nope", "metric": "dice"}}, "best.task"),
    ({"best": {"task": "sheet", "metric": "mean_cos"}}, "best.metric"),
    ({"best": {"task": "normals", "metric": "dice"}}, "best.metric"),
    ({"best": {"task": "sheet", "metric": "dice", "mode": "up"}}, "best.mode"),
    ({"best": {"task": "sheet", "metric": "dice", "patience": 3}}, "patience"),
    ({"best": {"metric": "dice"}}, "best.task"),
    ("yes", "val_metrics"),
]


@pytest.mark.parametrize("cfg,key", REJECTED, ids=[k + str(i) for i, (_, k) in enumerate(REJECTED)])
def test_bad_configs_are_rejected_with_the_key_named(cfg, key):
    with pytest.raises(ValueError, match="val_metrics") as e:
        M.parse_config(cfg, TASKS)
    assert key in str(e.value)


def test_the_trainer_rejects_a_bad_config_at_construction(tmp_path):
    import yaml
    from mt3d_amd.train import BaseTrainer
    cfg = yaml.safe_load(open(CFG))
    cfg["tr_config"]["val_metrics"] = {"best": {"task": "sheet", "metric": "accuracy"}}
    p = tmp_path / "cfg.yaml"
    yaml.safe_dump(cfg, open(p, "w"))
    with pytest.raises(ValueError, match="best.metric.*accuracy"):
        BaseTrainer(str(p), verbose=False)
    cfg["tr_config"]["val_metrics"] = {"best": {"task": "sheet", "metric": "dice", "mode": "max"}}
    yaml.safe_dump(cfg, open(p, "w"))
    tr = BaseTrainer(str(p), verbose=False)
    assert tr.val_metrics_config["kinds"] == {"sheet": "binary"} and tr.last_val_metrics is None
    assert BaseTrainer(CFG, verbose=False).val_metrics_config is None


# ---- the C ABI: arguments are checked on the host before anything is launched -------------------------------------------------------
def test_entry_points_refuse_bad_arguments_without_a_device():
    import __graft_entry__
    __graft_entry__.build()
    from mt3d_amd.engine import lib
    so = lib.load()
    A, B, O, S = 0x10000, 0x20000, 0x30000, 0x40000          # never dereferenced: every call below is refused on the host

    def refused(fn, rc, status=-1):
        assert rc == status, (fn, rc)
        msg = so.rx_last_error().decode()
        assert msg.startswith(fn + ":"), msg
        return msg
    for args in ((None, 0, B, 1, 1, 8, 0.5, 0.5, O), (A, 0, None, 1, 1, 8, 0.5, 0.5, O), (A, 0, B, 1, 1, 8, 0.5, 0.5, None),
                 (A, 0, B, 0, 1, 8, 0.5, 0.5, O), (A, 0, B, 1, 0, 8, 0.5, 0.5, O), (A, 0, B, 1, 1, 0, 0.5, 0.5, O),
                 (A, 0, B, 1, 1, -3, 0.5, 0.5, O), (A, 3, B, 1, 1, 8, 0.5, 0.5, O), (A + 2, 0, B, 1, 1, 8, 0.5, 0.5, O),
                 (A + 1, 1, B, 1, 1, 8, 0.5, 0.5, O), (A, 0, B + 2, 1, 1, 8, 0.5, 0.5, O), (A, 0, B, 1, 1, 8, 0.5, 0.5, O + 4),
                 (A, 0, B, 1, 1, 8, NAN, 0.5, O)):
        refused("rx_seg_counts", so.rx_seg_counts(*args, None))
    good = (A, 0, B, None, -100, 1, 4, 8, O)
    for i, v in ((0, None), (2, None), (3, S), (8, None), (5, 0), (6, 1), (6, 65), (6, 0), (7, 0), (1, 7), (0, A + 2), (2, B + 1), (8, O + 2)):
        args = list(good)
        args[i] = v
        msg = refused("rx_class_counts", so.rx_class_counts(*args, None))
        if i == 6:
            assert "2 to 64 classes" in msg and f"got {v}" in msg
    refused("rx_class_counts", so.rx_class_counts(A, 0, None, S + 4, -100, 1, 4, 8, O, None))
    assert so.rx_normal_stats_workspace(2, 1000) >= 2 * 2 * 8
    for n, v in ((0, 10), (-1, 10), (2, 0), (2, -5)):
        assert so.rx_normal_stats_workspace(n, v) == 0
    need = so.rx_normal_stats_workspace(1, 8)
    good = (A, 0, B, 1, 8, O, S, 0x50000, need)
    for i, v in ((0, None), (2, None), (5, None), (6, None), (7, None), (3, 0), (4, 0), (1, 9), (0, A + 2), (2, B + 2), (5, O + 4), (6, S + 4),
                 (7, 0x50004)):
        args = list(good)
        args[i] = v
        refused("rx_normal_stats", so.rx_normal_stats(*args, None))
    refused("rx_normal_stats", so.rx_normal_stats(A, 0, B, 1, 8, O, S, 0x50000, need - 1, None), status=-4)
    assert ctypes.sizeof(ctypes.c_long) == 8


def test_the_best_checkpoint_is_out_of_reach_of_the_pruning_glob(tmp_path):
    """BaseTrainer.train prunes `ckpt_dir.glob(f"{model_name}_*.pth")` down to the ten newest files"""
    import inspect
    from mt3d_amd import train
    src = inspect.getsource(train.BaseTrainer)
    assert 'glob(f"{self.mgr.model_name}_*.pth")' in src and '{self.mgr.model_name}.best.pth' in src
    for name in ("synthetic_sheet", "m", "run_best"):
        d = tmp_path / name
        d.mkdir()
        for f in [f"{name}_{i}.pth" for i in range(1, 4)] + [f"{name}.best.pth"]:
            (d / f).write_bytes(b"")
        assert sorted(p.name for p in d.glob(f"{name}_*.pth")) == [f"{name}_{i}.pth" for i in range(1, 4)]
