"""`BaseTrainer._build_loss()` hands out the engine's losses for the names that used to be plain torch modules: a two-task table
(a 3-channel softmax head under CrossEntropyLoss, a sheet head under BCEWithLogitsLossZSmooth with loss_kwargs), one forward plus
backward of the smallest synthetic model the trainer tests use."""
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "tasks", "synthetic_sheet.yaml")


@pytest.mark.gpu
def test_two_task_table_runs_both_losses_on_the_engine(tmp_path):
    import yaml
    import mt3d_amd  # noqa: F401
    from mt3d_amd.train import BaseTrainer
    from mt3d_amd.training.losses import losses as L
    cfg = yaml.safe_load(open(CFG))
    cfg["tr_setup"].update(ckpt_out_base=str(tmp_path / "ckpt"), tensorboard_log_dir=str(tmp_path / "tb"))
    cfg["dataset_config"]["targets"] = {
        "classes": {"channels": 3, "activation": "softmax", "weight": 1, "loss_fn": "CrossEntropyLoss"},
        "sheet": {"channels": 1, "activation": "none", "weight": 0.5, "loss_fn": "BCEWithLogitsLossZSmooth",
                  "loss_kwargs": {"center_smoothing": 0.05, "edge_smoothing": 0.3}},
    }
    p = tmp_path / "cfg.yaml"
    yaml.safe_dump(cfg, open(p, "w"))
    tr = BaseTrainer(str(p), verbose=False)
    fns = tr._build_loss()
    assert isinstance(fns["classes"], L.CrossEntropyLoss) and isinstance(fns["classes"], torch.nn.CrossEntropyLoss)
    assert isinstance(fns["sheet"], L.BCEWithLogitsLossZSmooth) and fns["sheet"].edge_smoothing == 0.3
    ds = tr._configure_dataset()
    items = [ds[0], ds[1]]
    batch = {k: torch.stack([it[k] for it in items]).to("cuda", dtype=torch.float32) for k in items[0]}
    model = tr._build_model().to("cuda")
    model.train()
    with torch.autocast("cuda", dtype=torch.bfloat16):
        out = model(batch["image"])
        per = {name: fns[name](out[name], batch[name]) for name in fns}
        total = per["classes"] + 0.5 * per["sheet"]
    assert "_CrossEntropyFn" in type(per["classes"].grad_fn).__name__
    assert "_ElemLossFn" in type(per["sheet"].grad_fn).__name__
    total.backward()
    assert torch.isfinite(total).item()
    # parameters the reference leaves unused (deep-supervision heads) stay grad-less; every other gradient is finite and non-zero
    grads = {n: q.grad for n, q in model.named_parameters() if q.grad is not None}
    assert "shared_encoder.stages.0.blocks.0.conv1.conv.weight" in grads          # the gradient went all the way down
    for task in fns:
        assert any(task in n for n in grads), (task, sorted(grads))
    bad = [n for n, g in grads.items() if not torch.isfinite(g).all().item()]
    assert not bad, bad
    zero = [n for n, g in grads.items() if g.abs().sum().item() == 0.0]
    assert not zero, zero
