"""GPU: `tr_config.val_preview` through BaseTrainer.train on the synthetic 16^3 sheet + normals config of the metrics test, one
epoch, two validation steps: the GIF at the reference's default path, its frames against the numpy statement on the tensors of
validation step 0, and -- without the key -- no file and no preview."""
import os

import numpy as np
import pytest
import torch

import mt3d_amd  # noqa: F401
from mt3d_amd.engine import ops
from mt3d_amd.training import visualization as V

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "tasks", "synthetic_sheet.yaml")


def _run(tmp_path, val_preview, monkeypatch):
    import yaml
    from mt3d_amd.train import BaseTrainer
    cfg = yaml.safe_load(open(CFG))
    cfg["tr_setup"].update(model_name="pv_run", ckpt_out_base=str(tmp_path / "ckpt"), tensorboard_log_dir=str(tmp_path / "tb"))
    cfg["tr_config"].update(max_epoch=1, max_steps_per_epoch=2, max_val_steps_per_epoch=2, patch_size=[16, 16, 16], compile=False)
    if val_preview is not None:
        cfg["tr_config"]["val_preview"] = val_preview
    cfg["dataset_config"]["targets"]["normals"] = {"channels": 3, "activation": "none", "weight": 1, "loss_fn": "MaskedCosineLoss"}
    tmp_path.mkdir(parents=True, exist_ok=True)
    p = tmp_path / "cfg.yaml"
    yaml.safe_dump(cfg, open(p, "w"))
    monkeypatch.chdir(tmp_path)
    calls = []
    real = ops.preview_frames

    def spy(image, targets, preds, **kw):      # what the trainer handed over, copied to the host before anything else runs
        out = real(image, targets, preds, **kw)
        calls.append((image.float().cpu().numpy(), {k: v.float().cpu().numpy() for k, v in targets.items()},
                      {k: v.float().cpu().numpy() for k, v in preds.items()}, kw))
        return out
    monkeypatch.setattr(ops, "preview_frames", spy)
    lines = []

    class Rec(BaseTrainer):
        def _log(self, *a):
            lines.append(" ".join(str(x) for x in a))

    torch.manual_seed(1234)
    np.random.seed(1234)
    tr = Rec(str(p), verbose=False)
    tr.train()
    torch.cuda.synchronize()
    return tr, lines, calls


def test_the_gif_is_written_and_its_frames_are_the_statement(tmp_path, monkeypatch):
    from PIL import Image
    tr, _, calls = _run(tmp_path / "on", {"every": 2}, monkeypatch)
    assert len(calls) == 1                                          # validation step 0 only, of two steps
    image, targets, preds, kw = calls[0]
    assert sorted(targets) == ["normals", "sheet"] and kw["every"] == 2 and kw["sample"] == 0 and tuple(kw["sigmoid_tasks"]) == ()
    z, h, w = image.shape[2:]
    t = len(targets)
    path = tmp_path / "on" / "pv_run_debug.gif"                     # the reference's name, in the working directory
    assert path.exists()
    with Image.open(path) as im:
        assert im.n_frames == -(-z // 2) and im.size == ((1 + t) * w, 2 * h) and im.info["duration"] == 200
    want = V.frames_numpy(image[0], {k: v[0] for k, v in targets.items()}, {k: v[0] for k, v in preds.items()}, every=2)
    got = tr.last_val_preview
    assert isinstance(got, np.ndarray) and got.dtype == np.uint8 and got.shape == (-(-z // 2), 2 * h, (1 + t) * w, 3)
    assert np.array_equal(got, want)
    assert not got[:, h:, :w].any() and got[:, :h].std() > 0


def test_without_the_key_nothing_is_drawn(tmp_path, monkeypatch):
    tr, lines, calls = _run(tmp_path / "off", None, monkeypatch)
    assert tr.val_preview_config is None and tr.last_val_preview is None and calls == []
    assert not [f for f in os.listdir(tmp_path / "off") if f.endswith(".gif")]
    assert not any("preview" in l.lower() or "gif" in l.lower() for l in lines)
    with pytest.raises(ValueError, match="every"):                  # a typo stops the run at construction
        _run(tmp_path / "bad", {"every": 0}, monkeypatch)
