"""CPU: the numpy statements of the surface-distance metrics (training/metrics/surface.py) against scipy where it is importable and
against hand-made cases, `surface_scores` on hand-made histograms, the `tr_config.val_metrics.surface` block, and the C ABI's
argument checks (no device is touched)."""
import ctypes
import math

import numpy as np
import pytest

import mt3d_amd  # noqa: F401
from mt3d_amd.training import metrics as M
from mt3d_amd.training.metrics import surface as S

SHAPES = [(9, 10, 12), (1, 7, 65), (5, 1, 3), (33, 17, 70)]
DENSITIES = [0.02, 0.3, 0.9]
TASKS = {"sheet": {"channels": 1, "activation": "none"}, "prob": {"channels": 1, "activation": "sigmoid"},
         "normals": {"channels": 3, "activation": "none"}, "classes": {"channels": 4, "loss_fn": "CrossEntropyLoss"}}


def random_mask(shape, density, seed=0):
    return np.random.default_rng(seed + sum(shape)).random(shape) < density


# ---- the statements against scipy ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=str)
@pytest.mark.parametrize("density", DENSITIES)
def test_edt_sq_numpy_equals_scipy(shape, density):
    ndi = pytest.importorskip("scipy.ndimage")
    f = random_mask(shape, density)
    assert f.any()
    want = np.rint(ndi.distance_transform_edt(~f) ** 2).astype(np.int32)
    got = S.edt_sq_numpy(f)
    assert got.dtype == np.int32 and np.array_equal(got, want)


@pytest.mark.parametrize("shape", SHAPES, ids=str)
@pytest.mark.parametrize("density", DENSITIES)
def test_edges_numpy_equals_scipy(shape, density):
    ndi = pytest.importorskip("scipy.ndimage")
    m = random_mask(shape, density, seed=1)
    assert np.array_equal(S.edges_numpy(m), m & ~ndi.binary_erosion(m))
    full = np.ones(shape, dtype=bool)
    assert np.array_equal(S.edges_numpy(full), full & ~ndi.binary_erosion(full))


# ---- the statements on hand-made cases ------------------------------------------------------------------------------------------------
def brute_edt(f):
    pts = np.argwhere(f)
    out = np.full(f.shape, S.EDT_NONE, dtype=np.int64)
    for idx in np.ndindex(*f.shape):
        if len(pts):
            out[idx] = ((pts - np.array(idx)) ** 2).sum(1).min()
    return out.astype(np.int32)


def test_edt_sq_numpy_against_brute_force_and_at_a_corner():
    f = np.zeros((9, 10, 12), dtype=bool)
    f[0, 0, 0] = True
    d = S.edt_sq_numpy(f)
    assert d[-1, -1, -1] == 8 ** 2 + 9 ** 2 + 11 ** 2 and d[0, 0, 0] == 0 and d[0, 0, 5] == 25
    for shape in [(5, 1, 3), (4, 6, 7), (1, 1, 1)]:
        g = random_mask(shape, 0.2, seed=3)
        assert np.array_equal(S.edt_sq_numpy(g), brute_edt(g))


def test_edt_sq_numpy_without_a_feature_is_none_everywhere():
    d = S.edt_sq_numpy(np.zeros((3, 4, 5), dtype=bool))
    assert d.dtype == np.int32 and (d == S.EDT_NONE).all() and S.EDT_NONE == 1 << 30 == M.EDT_NONE


def test_edges_numpy_by_hand():
    full = np.ones((4, 5, 6), dtype=bool)
    e = S.edges_numpy(full)
    assert not e[1:-1, 1:-1, 1:-1].any() and e.sum() == 4 * 5 * 6 - 2 * 3 * 4      # only the shell
    hole = full.copy()
    hole[2, 2, 3] = False
    e = S.edges_numpy(hole)
    assert e[1, 2, 3] and e[2, 1, 3] and e[2, 2, 2] and e[2, 2, 4] and not e[2, 2, 3] and not e[1, 1, 2]      # faces only, no diagonal
    assert np.array_equal(S.edges_numpy(np.ones((1, 1, 1), dtype=bool)), np.ones((1, 1, 1), dtype=bool))
    with pytest.raises(ValueError, match="2-D"):
        S.edges_numpy(np.ones((4, 4), dtype=bool))
    with pytest.raises(ValueError, match="2-D"):
        S.edt_sq_numpy(np.ones((4, 4), dtype=bool))


def plane(shape, z, thick=1):
    v = np.zeros(shape, dtype=np.float32)
    v[z:z + thick] = 1.0
    return v


def test_surface_hist_numpy_on_planes_and_empty_sides():
    shape = (12, 5, 6)
    a, b = plane(shape, 2), plane(shape, 5)
    hist, counts = S.surface_hist_numpy(a, b, 0.5, 0.5)
    assert hist.shape == (2, S.default_bins(shape)) and S.default_bins(shape) == 11 ** 2 + 4 ** 2 + 5 ** 2 + 1
    assert hist[0, 9] == hist[1, 9] == 30 and hist.sum() == 60 and counts.tolist() == [30, 30, 0, 0]
    hist, counts = S.surface_hist_numpy(a, np.zeros(shape, np.float32), 0.5, 0.5)
    assert hist.sum() == 0 and counts.tolist() == [30, 0, 30, 0]
    hist, counts = S.surface_hist_numpy(np.zeros(shape, np.float32), b, 0.5, 0.5)
    assert hist.sum() == 0 and counts.tolist() == [0, 30, 0, 30]
    hist, counts = S.surface_hist_numpy(np.zeros(shape, np.float32), np.zeros(shape, np.float32), 0.5, 0.5)
    assert hist.sum() == 0 and counts.tolist() == [0, 0, 0, 0]
    # a caller-given small `bins`: the distance 9 goes to the last bin; at the threshold is not above it; a NaN is negative
    hist, counts = S.surface_hist_numpy(a, b, 0.5, 0.5, bins=4)
    assert hist.tolist() == [[0, 0, 0, 30], [0, 0, 0, 30]]
    c = a.copy()
    c[7], c[8, 0, 0] = 0.5, np.nan
    assert S.surface_hist_numpy(c, b, 0.5, 0.5)[1].tolist() == [30, 30, 0, 0]


# ---- scores -------------------------------------------------------------------------------------------------------------------------
def test_surface_scores_identical_shifted_and_empty():
    hist = np.zeros((2, 50), dtype=np.int64)
    hist[:, 0] = 40
    s = S.surface_scores(hist, [40, 40, 0, 0], [0, 1])
    assert s == {"surface_dice_0": 1.0, "surface_dice_1": 1.0, "assd": 0.0, "hd95": 0.0, "surface_voxels": 80.0}
    hist = np.zeros((2, 50), dtype=np.int64)
    hist[:, 9] = 30      # a plane against the same plane shifted by 3
    s = S.surface_scores(hist, [30, 30, 0, 0], [2, 3, 1.5])
    assert s["assd"] == 3.0 and s["hd95"] == 3.0 and s["surface_dice_2"] == 0.0 and s["surface_dice_3"] == 1.0
    assert list(s) == ["surface_dice_2", "surface_dice_3", "surface_dice_1.5", "assd", "hd95", "surface_voxels"]
    s = S.surface_scores(np.zeros((2, 50), dtype=np.int64), [30, 0, 30, 0], [1, 2])      # one side empty
    assert s["surface_dice_1"] == 0.0 and s["surface_dice_2"] == 0.0 and math.isnan(s["assd"]) and math.isnan(s["hd95"])
    assert s["surface_voxels"] == 30.0
    s = S.surface_scores(np.zeros((2, 50), dtype=np.int64), [0, 0, 0, 0], [1, 2])      # both empty
    assert all(math.isnan(s[k]) for k in ("surface_dice_1", "surface_dice_2", "assd", "hd95")) and s["surface_voxels"] == 0.0


def test_surface_scores_mixed_rows_and_the_tolerance_rule():
    hist = np.zeros((2, 30), dtype=np.int64)
    hist[0, [0, 1, 2, 4]] = [5, 3, 2, 1]
    hist[1, [0, 3, 16]] = [4, 2, 1]
    s = S.surface_scores(hist, [12, 7, 1, 0], [0, 1, 1.5, 2])
    assert s["surface_voxels"] == 19.0
    assert s["surface_dice_0"] == 9 / 19 and s["surface_dice_1"] == 12 / 19 and s["surface_dice_1.5"] == 14 / 19      # 1.5^2 = 2.25: k <= 2
    assert s["surface_dice_2"] == 17 / 19
    want = 0.0
    for k in range(30):
        want += (float(hist[0, k]) + float(hist[1, k])) * math.sqrt(k)
    assert s["assd"] == want / 18.0
    assert s["hd95"] == 4.0      # row 0: rank ceil(10.45) = 11 -> k = 4 (2.0); row 1: rank 7 -> k = 16 (4.0)


def test_hd95_is_nearest_rank_on_a_bin_boundary():
    hist = np.zeros((2, 30), dtype=np.int64)
    hist[0, 1], hist[0, 25] = 19, 1      # n = 20: rank ceil(19.0) = 19 is reached by bin 1 exactly
    assert S.surface_scores(hist, [20, 0, 0, 0], [1])["hd95"] == 1.0
    hist[0, 1], hist[0, 25] = 18, 2      # ... and one voxel fewer in bin 1 moves it to bin 25
    assert S.surface_scores(hist, [20, 0, 0, 0], [1])["hd95"] == 5.0
    hist[0] = 0
    hist[0, 4], hist[0, 9] = 95, 5       # n = 100: rank 95 falls on the last voxel of bin 4
    assert S.surface_scores(hist, [100, 0, 0, 0], [1])["hd95"] == 2.0      # numpy's interpolating percentile would say 2.05
    with pytest.raises(ValueError, match="surface_scores"):
        S.surface_scores(np.zeros((3, 4)), [0, 0, 0, 0], [1])


# ---- configuration ------------------------------------------------------------------------------------------------------------------
def test_parse_config_surface_off_on_and_metric_names():
    base = M.parse_config(True, TASKS)
    assert base["surface"] is None and M.parse_config({"surface": False}, TASKS) == base and M.parse_config({"surface": None}, TASKS) == base
    assert set(base) == {"threshold", "target_threshold", "kinds", "best", "surface"}
    on = M.parse_config({"surface": True}, TASKS, patch_size=(16, 16, 16))
    assert on["surface"] == {"tolerances": (1.0, 2.0), "tasks": ("sheet", "prob")}
    assert {k: v for k, v in on.items() if k != "surface"} == {k: v for k, v in base.items() if k != "surface"}
    cfg = M.parse_config({"surface": {"tolerances": [0, 1, 1.5], "tasks": ["prob"]}, "best": {"task": "prob", "metric": "hd95", "mode": "min"}},
                         TASKS)
    assert cfg["surface"] == {"tolerances": (0.0, 1.0, 1.5), "tasks": ("prob",)} and cfg["best"]["metric"] == "hd95"
    # without `surface` the names are what they were
    assert M.metric_names("binary") == M.RATES + ("dice_per_patch",)
    assert M.metric_names("multiclass") == M.RATES + tuple(f"{r}_class_mean" for r in M.RATES) + ("dice_per_patch",)
    assert M.metric_names("normals") == ("mean_cos", "mean_angle_deg", "masked_voxels") and M.metric_names("none") == ()
    assert M.metric_names("binary", None) == M.metric_names("binary")
    extra = ("surface_dice_0", "surface_dice_1", "surface_dice_1.5", "assd", "hd95", "surface_voxels")
    assert M.metric_names("binary", cfg["surface"]) == M.metric_names("binary") + extra
    assert M.metric_names("normals", cfg["surface"]) == M.metric_names("normals")
    vm = M.ValidationMetrics(TASKS, cfg)
    got = vm.compute()
    assert list(got["prob"]) == list(M.metric_names("binary") + extra) and list(got["sheet"]) == list(M.metric_names("binary"))
    assert all(math.isnan(v) for v in got["prob"].values())
    assert list(M.ValidationMetrics(TASKS, True).compute()["prob"]) == list(M.metric_names("binary"))


REJECTED = [
    ({"surface": {"tolerance": [1]}}, "tolerance", None),
    ({"surface": "yes"}, "surface", None),
    ({"surface": {"tolerances": [1, -1]}}, "surface.tolerances", None),
    ({"surface": {"tolerances": [float("inf")]}}, "surface.tolerances", None),
    ({"surface": {"tolerances": [float("nan")]}}, "surface.tolerances", None),
    ({"surface": {"tolerances": ["1"]}}, "surface.tolerances", None),
    ({"surface": {"tolerances": [True]}}, "surface.tolerances", None),
    ({"surface": {"tolerances": [1, 2, 1.0]}}, "surface.tolerances", None),
    ({"surface": {"tolerances": []}}, "surface.tolerances", None),
    ({"surface": {"tasks": ["sheets"]}}, "sheets", None),
    ({"surface": {"tasks": ["normals"]}}, "normals", None),
    ({"surface": {"tasks": ["classes"]}}, "classes", None),
    ({"surface": {"tasks": "sheet"}}, "surface.tasks", None),
    ({"surface": True}, "train_patch_size", (64, 64)),
    ({"surface": True, "best": {"task": "normals", "metric": "hd95"}}, "best.metric", None),
    ({"surface": {"tasks": ["prob"]}, "best": {"task": "sheet", "metric": "assd"}}, "best.metric", None),
    ({"best": {"task": "sheet", "metric": "assd"}}, "best.metric", None),
]


@pytest.mark.parametrize("cfg,key,patch", REJECTED, ids=[f"{k}{i}" for i, (_, k, _) in enumerate(REJECTED)])
def test_bad_surface_blocks_are_rejected_with_the_key_named(cfg, key, patch):
    with pytest.raises(ValueError, match="val_metrics") as e:
        M.parse_config(cfg, TASKS, patch_size=patch)
    assert key in str(e.value)


def test_the_trainer_passes_the_block_through(tmp_path):
    import os
    import yaml
    from mt3d_amd.train import BaseTrainer
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg = yaml.safe_load(open(os.path.join(root, "tasks", "synthetic_sheet.yaml")))
    cfg["tr_config"]["val_metrics"] = {"surface": {"tolerances": [1, 3]}, "best": {"task": "sheet", "metric": "assd", "mode": "min"}}
    p = tmp_path / "cfg.yaml"
    yaml.safe_dump(cfg, open(p, "w"))
    tr = BaseTrainer(str(p), verbose=False)
    assert tr.val_metrics_config["surface"] == {"tolerances": (1.0, 3.0), "tasks": ("sheet",)}
    cfg["tr_config"]["patch_size"] = [32, 32]
    yaml.safe_dump(cfg, open(p, "w"))
    with pytest.raises(ValueError, match="val_metrics.surface.*train_patch_size"):
        BaseTrainer(str(p), verbose=False)


# ---- the C ABI: arguments are checked on the host before anything is launched -------------------------------------------------------
def test_the_entry_points_refuse_bad_arguments_before_any_launch():
    import __graft_entry__
    __graft_entry__.build()
    from mt3d_amd.engine import lib
    so = lib.load()
    p = ctypes.c_void_p(0x1000)
    q = ctypes.c_void_p(0x2000)

    def refused(rc, name, word):
        msg = so.rx_last_error().decode()
        assert rc == -1 and msg.startswith(name) and word in msg, (rc, msg)
    refused(so.rx_edt_sq(p, 1, 1025, 4, 4, q, None), "rx_edt_sq", "1024")
    refused(so.rx_edt_sq(p, 1, 4, 1025, 4, q, None), "rx_edt_sq", "1024")
    refused(so.rx_edt_sq(p, 1, 4, 4, 1025, q, None), "rx_edt_sq", "1024")
    refused(so.rx_edt_sq(p, 1, 4, 0, 4, q, None), "rx_edt_sq", "positive")
    refused(so.rx_edt_sq(None, 1, 4, 4, 4, q, None), "rx_edt_sq", "null")
    refused(so.rx_edt_sq(p, 1, 4, 4, 4, ctypes.c_void_p(0x2002), None), "rx_edt_sq", "aligned")
    refused(so.rx_edt_sq(p, 1, 4, 4, 4, p, None), "rx_edt_sq", "different")
    refused(so.rx_mask_edges(p, 0, 0.5, 1, 4, 4, 1025, q, None), "rx_mask_edges", "1024")
    refused(so.rx_mask_edges(p, 7, 0.5, 1, 4, 4, 4, q, None), "rx_mask_edges", "dtype")
    refused(so.rx_mask_edges(p, 0, float("nan"), 1, 4, 4, 4, q, None), "rx_mask_edges", "NaN")
    refused(so.rx_mask_edges(p, 0, 0.5, 65536, 4, 4, 4, q, None), "rx_mask_edges", "65535")
    refused(so.rx_mask_edges(p, 0, 0.5, 1, 4, 4, 4, None, None), "rx_mask_edges", "null")
    refused(so.rx_surface_hist(p, q, 0, 8, q, q, q, None), "rx_surface_hist", "positive")
    refused(so.rx_surface_hist(p, q, 8, 0, q, q, q, None), "rx_surface_hist", "positive")
    refused(so.rx_surface_hist(p, q, 8, 8, ctypes.c_void_p(0x2004), q, q, None), "rx_surface_hist", "aligned")
    refused(so.rx_surface_hist(p, None, 8, 8, q, q, q, None), "rx_surface_hist", "null")
    assert lib.RX_EDT_NONE == S.EDT_NONE and lib.RX_EDT_MAX_EXTENT == S.MAX_EXTENT
