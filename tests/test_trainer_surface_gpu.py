"""GPU: `tr_config.val_metrics.surface` through BaseTrainer.train on a synthetic 16^3 sheet + normals config, one epoch, two
validation steps: the new names in `last_val_metrics`, in the log lines and in the `val/{task}_{metric}` scalars, and a `best`
that watches one of them."""
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
SURFACE = ("surface_dice_1", "surface_dice_2.5", "assd", "hd95", "surface_voxels")


def test_surface_metrics_are_reported_by_the_trainer(tmp_path):
    import yaml
    from mt3d_amd.train import BaseTrainer
    cfg = yaml.safe_load(open(CFG))
    cfg["tr_setup"].update(model_name="sf_run", ckpt_out_base=str(tmp_path / "ckpt"), tensorboard_log_dir=str(tmp_path / "tb"))
    cfg["tr_config"].update(max_epoch=1, max_steps_per_epoch=2, max_val_steps_per_epoch=2, patch_size=[16, 16, 16], compile=False)
    cfg["tr_config"]["val_metrics"] = {"surface": {"tolerances": [1, 2.5]}, "best": {"task": "sheet", "metric": "surface_voxels", "mode": "min"}}
    cfg["dataset_config"]["targets"]["normals"] = {"channels": 3, "activation": "none", "weight": 1, "loss_fn": "MaskedCosineLoss"}
    p = tmp_path / "cfg.yaml"
    yaml.safe_dump(cfg, open(p, "w"))
    os.chdir(tmp_path)
    lines, scalars = [], {}

    class Rec(BaseTrainer):
        def _log(self, *a):
            lines.append(" ".join(str(x) for x in a))

        def _report_val_metrics(self, metrics, vrun, vsteps, epoch, writer, *rest):
            class Spy:      # what the writer is asked to record, passed on to the real one
                def add_scalar(self, tag, value, step):
                    scalars[tag] = value
                    if writer is not None:
                        writer.add_scalar(tag, value, step)
            return super()._report_val_metrics(metrics, vrun, vsteps, epoch, Spy(), *rest)

    torch.manual_seed(1234)
    np.random.seed(1234)
    tr = Rec(str(p), verbose=False)
    assert tr.val_metrics_config["surface"] == {"tolerances": (1.0, 2.5), "tasks": ("sheet",)}
    tr.train()
    torch.cuda.synchronize()
    got = tr.last_val_metrics
    assert list(got["sheet"]) == list(M.metric_names("binary") + SURFACE) and list(got["normals"]) == list(M.metric_names("normals"))
    s = got["sheet"]
    # a 16^3 target sheet has edge voxels, so there is something to score whatever the untrained head predicts
    assert s["surface_voxels"] > 0 and s["surface_voxels"] == int(s["surface_voxels"])
    for k in ("surface_dice_1", "surface_dice_2.5"):
        assert 0.0 <= s[k] <= 1.0
    assert s["surface_dice_1"] <= s["surface_dice_2.5"]
    if not math.isnan(s["assd"]):
        assert 0.0 <= s["assd"] <= math.sqrt(3 * 15 ** 2) and 0.0 <= s["hd95"] <= math.sqrt(3 * 15 ** 2)
    for name in SURFACE:
        assert sum(l.startswith(f"Task 'sheet', epoch 1 val {name}: ") for l in lines) == 1, name
        assert not any(l.startswith(f"Task 'normals', epoch 1 val {name}: ") for l in lines)
        if s[name] == s[name]:
            assert scalars[f"val/sheet_{name}"] == s[name]
        else:
            assert f"val/sheet_{name}" not in scalars      # nan skipped, as for every metric
    assert scalars["val/sheet_dice"] == s["dice"] or math.isnan(s["dice"])
    assert tr.best_val_metric == s["surface_voxels"] and "sf_run.best.pth" in os.listdir(tmp_path / "ckpt")
