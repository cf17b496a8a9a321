"""`inference.main` with an `inference_config.postprocess.components` block: `<task>_filtered` is filter_numpy of `<task>_final`, and
the arrays inference itself writes are byte-identical to a run without the block."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _cfg(tmp_path, name, ic):
    import yaml
    cfg = {"tr_setup": {}, "tr_config": {"patch_size": [16, 16, 16], "batch_size": 2}, "model_config": {},
           "dataset_config": {"targets": {"sheet": {"channels": 1, "activation": "sigmoid"}}}, "inference_config": ic}
    p = tmp_path / f"{name}.yaml"
    p.write_text(yaml.safe_dump(cfg))
    return str(p)


def test_inference_main_runs_the_component_filter(tmp_path, capsys):
    import mt3d_amd  # noqa: F401
    import mt3d_amd.inference as inf
    import mt3d_amd.postprocess as pp
    from mt3d_amd.builders.build_network_from_config import NetworkFromConfig
    from mt3d_amd.configuration.config_manager import ConfigManager
    from mt3d_amd.dataloading import zarr_lite
    from mt3d_amd.engine import lib as L
    L.require_device()
    vol = np.random.default_rng(11).integers(0, 256, size=(24, 20, 36)).astype(np.uint8)
    src = zarr_lite.write_array(str(tmp_path / "vol.zarr"), vol, (16, 16, 16), compressor="zlib")
    ckpt = str(tmp_path / "model.pt")
    base = {"checkpoint_path": ckpt, "input_path": str(src.path), "overlap": 0.5}
    torch.manual_seed(3)
    net = NetworkFromConfig(ConfigManager(_cfg(tmp_path, "plain", base), verbose=False)).cuda()
    torch.save({"model": net.state_dict()}, ckpt)

    plain = inf.main(["--config_path", _cfg(tmp_path, "plain", {**base, "output_path": str(tmp_path / "a")})])
    final = zarr_lite.open(os.path.join(plain, "sheet_final"))[...]
    level = min(int(np.median(final)), 254)      # a level that leaves speckle on both sides, whatever the random weights predict
    block = {"components": {"tasks": ["sheet"], "level": level, "connectivity": 6, "min_voxels": 4, "write_labels": True}}
    capsys.readouterr()
    filt = inf.main(["--config_path", _cfg(tmp_path, "filtered", {**base, "output_path": str(tmp_path / "b"), "postprocess": block})])
    printed = capsys.readouterr().out
    assert "'min_voxels': 4" in printed and "'components':" in printed      # the summary dict is printed
    for n in ("sheet_final", "sheet_sum", "sheet_count"):
        a, b = os.path.join(plain, n), os.path.join(filt, n)
        assert sorted(os.listdir(a)) == sorted(os.listdir(b)), n
        for f in os.listdir(a):
            assert open(os.path.join(a, f), "rb").read() == open(os.path.join(b, f), "rb").read(), (n, f)
    assert not os.path.exists(os.path.join(plain, "sheet_filtered"))
    want, _ = pp.filter_numpy(final, level, 6, 4)
    assert np.array_equal(zarr_lite.open(os.path.join(filt, "sheet_filtered"))[...], want)
    assert os.path.exists(os.path.join(filt, "sheet_labels"))
