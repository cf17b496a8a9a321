"""TEST INFRASTRUCTURE ONLY -- run where the reference tree exists (oracle/ref_shim.py, $RX_REFERENCE_ROOT):

    python oracle/make_golden_parity.py

Records what the REAL reference computes for the checks of `tests/test_oracle_vs_reference.py` and
`tests/test_product_tree.py::test_reference_task_files_behave_as_upstream`, so that those tests run on any machine:

* `tests/golden/parity/<case>.npz`: per golden case (oracle/golden_cases.py) the reference's `state_dict` keys in
  order with a sha256 digest of every tensor's bytes, its train-mode outputs (channel-dropout masks drawn after
  `torch.manual_seed(77)`), its loss and every parameter gradient (in full up to GRAD_SAMPLE elements, beyond that a
  fixed sample of elements and the whole tensor's sum, sum of magnitudes and L2 norm).
* `tests/golden/parity/autoconfig.json`: the reference planner's strides / kernels / blocks per stage for a list of
  patch sizes.
* `tests/golden/reference_task_files.json`: per task file of the reference (`tasks/*.yaml`) the parsed configuration
  (data only, no YAML text), the outcome of the reference's `ConfigManager` on it, the attribute values it reads, and
  whether the reference's `NetworkFromConfig` refuses the configuration.
"""
import contextlib
import glob
import hashlib
import io
import json
import os
import sys

import numpy as np
import torch
import yaml

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_shim  # noqa: E402
from golden_cases import CASES  # noqa: E402
from resenc_oracle import synthetic_batch  # noqa: E402  (data generator only)

OUT = os.path.join(os.path.dirname(HERE), "tests", "golden")
PARITY = os.path.join(OUT, "parity")
THREADS = 4            # the tests compute with the same thread count
GRAD_SAMPLE = 512      # gradients larger than this are kept as a fixed sample of elements plus sum, sum |g| and L2 norm
AUTOCONFIG_PATCHES = [(64, 64, 64), (128, 128, 128), (160, 160, 160), (14, 256, 256), (8, 32, 32), (256, 256)]
CONFIG_ATTRS = ("model_name", "autoconfigure", "train_patch_size", "train_batch_size", "in_channels", "gradient_accumulation",
                "optimizer", "initial_lr", "weight_decay", "max_epoch", "tr_val_split", "min_labeled_ratio", "min_bbox_percent")


def tensor_digest(t):
    t = t.detach().contiguous()
    h = hashlib.sha256(f"{t.dtype}{tuple(t.shape)}".encode())
    h.update(t.numpy().tobytes())
    return h.hexdigest()


def grad_sample_index(numel):
    """the fixed element positions of a gradient with more than GRAD_SAMPLE elements that the fixture keeps"""
    return torch.randperm(numel, generator=torch.Generator().manual_seed(numel))[:GRAD_SAMPLE].sort().values


def case_arrays(c, ref_losses):
    """the inputs and seeds of test_oracle_vs_reference.py::test_state_dict_and_forward_backward_equal"""
    mgr = ref_shim.make_mgr(c["patch"], c["tasks"], c["in_channels"], 1, c["autoconfigure"], c["model_config"])
    torch.manual_seed(c["seed"])
    ref = ref_shim.build_reference_network(mgr)
    sd = ref.state_dict()
    arrays = {"state_dict_keys": np.array(json.dumps(list(sd.keys()))),
              "state_dict_sha256": np.array(json.dumps([tensor_digest(v) for v in sd.values()]))}
    x, targets = synthetic_batch(c["batch"], c["in_channels"], c["patch"], c["tasks"], c["data_seed"])
    ref.train()
    torch.manual_seed(77)
    out = ref(x)
    for k, v in out.items():
        arrays[f"out.{k}"] = v.detach().numpy()
    arrays["out_keys"] = np.array(json.dumps(list(out.keys())))
    loss = 0.0
    for name, gt in targets.items():
        info = c["tasks"][name]
        cls = getattr(ref_losses, info.get("loss_fn", "BCEDiceLoss"))
        loss = loss + cls(**info.get("loss_kwargs", {}))(out[name], gt) * info.get("weight", 1.0)
    arrays["loss"] = np.float64(loss.item())
    loss.backward()
    names, with_grad = [], []
    for n, p in ref.named_parameters():
        names.append(n)
        with_grad.append(p.grad is not None)
        if p.grad is not None:
            g = p.grad.flatten()
            if g.numel() > GRAD_SAMPLE:
                g = g[grad_sample_index(g.numel())]
            arrays[f"grad.{n}"] = g.numpy()
            gd = p.grad.double()
            arrays[f"grad_sums.{n}"] = np.array([gd.sum().item(), gd.abs().sum().item(), gd.norm().item()])
    arrays["param_names"] = np.array(json.dumps(names))
    arrays["param_has_grad"] = np.array(with_grad)
    return arrays


def autoconfig_table():
    import builders.utils as ru       # the reference's planner (importable once import_reference() ran)
    rows = []
    for patch in AUTOCONFIG_PATCHES:
        _, strides, kernels, _, _ = ru.get_pool_and_conv_props((1.0,) * len(patch), patch, 4, 999999)
        rows.append({"patch": list(patch), "strides": [list(s) for s in strides], "kernels": [list(k) for k in kernels],
                     "n_blocks_per_stage": list(ru.get_n_blocks_per_stage(len(strides)))})
    return rows


def task_file_records():
    from configuration.config_manager import ConfigManager as RefManager          # the reference's own
    records = []
    for f in sorted(glob.glob(os.path.join(ref_shim.REFERENCE_ROOT, "tasks", "*.yaml"))):
        with open(f) as fh:
            config = yaml.safe_load(fh)
        rec = {"file": os.path.basename(f), "config": config}
        try:
            with contextlib.redirect_stdout(io.StringIO()):
                try:
                    r = RefManager(f, verbose=False)
                except TypeError:
                    r = RefManager(f)
            rec["outcome"] = "ok"
        except Exception as e:      # noqa: BLE001
            rec["outcome"] = type(e).__name__
            records.append(rec)
            continue
        rec["attrs"] = {a: repr(getattr(r, a)) for a in CONFIG_ATTRS}
        rec["tasks"] = list(r.tasks)
        rec["model_config"] = repr(r.model_config)
        try:
            ref_shim.build_reference_network(r)
            rec["network"] = "ok"
        except Exception as e:      # noqa: BLE001  (ValueError: autoconfigure false without the manual topology keys)
            rec["network"] = type(e).__name__
        records.append(rec)
    return records


def main():
    torch.set_num_threads(THREADS)
    _, ref_losses = ref_shim.import_reference()
    os.makedirs(PARITY, exist_ok=True)
    for cname, c in CASES.items():
        path = os.path.join(PARITY, f"{cname}.npz")
        np.savez_compressed(path, **case_arrays(c, ref_losses))
        print(path, os.path.getsize(path) // 1024, "KiB")
    with open(os.path.join(PARITY, "autoconfig.json"), "w") as f:
        json.dump(autoconfig_table(), f, indent=1)
        f.write("\n")
    path = os.path.join(OUT, "reference_task_files.json")
    with open(path, "w") as f:
        json.dump(task_file_records(), f, indent=1)
        f.write("\n")
    print(path, os.path.getsize(path) // 1024, "KiB")


if __name__ == "__main__":
    main()
