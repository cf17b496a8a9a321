"""GPU: rx_label_dilate (csrc/rx_morph.hip) against the numpy statement `dilate_numpy`, through `ops.label_dilate`, `DeviceDilate`,
the feeder and the trainer.  Every comparison is exact: 0.0 / 1.0 float32 with +0.0 zeros, no tolerance anywhere."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import mt3d_amd  # noqa: F401
from mt3d_amd.dataloading import dilate_device as D

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "tasks", "synthetic_sheet.yaml")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_dilate_cpu import label, same_01  # noqa: E402

# (B, C, Z, Y, X): every extent below the radius; exactly one word; a 6-bit tail and two channels; three words and y beyond any
# plausible tile; z beyond a tile and a 1-bit tail; a single slice
SHAPES = [(1, 1, 3, 4, 5), (2, 1, 12, 13, 64), (1, 2, 13, 11, 70), (2, 1, 9, 37, 130), (1, 1, 37, 9, 129), (1, 1, 1, 20, 200)]
RADII = [1, 5, 8]
_ORACLE = {}


def oracle(a, r):
    """`dilate_numpy` of every sample of a (B, C, Z, Y, X) array"""
    return np.stack([D.dilate_numpy(s, r) for s in a])


def case(shape, r):
    """the input and its oracle, computed once per (shape, radius) and never written to"""
    if (shape, r) not in _ORACLE:
        a = label(shape, 11 * r + shape[-1])
        a.setflags(write=False)
        want = oracle(a, r)
        want.setflags(write=False)
        _ORACLE[(shape, r)] = (a, want)
    return _ORACLE[(shape, r)]


@pytest.mark.parametrize("r", RADII)
@pytest.mark.parametrize("shape", SHAPES)
def test_kernel_is_dilate_numpy_in_place_and_out_of_place(shape, r):
    from mt3d_amd.engine import ops as E
    a, want = case(shape, r)
    x = torch.from_numpy(a.copy()).cuda()
    keep = x.clone()
    out = torch.full_like(x, -7.0)
    got = E.label_dilate(x, r, out=out)
    assert got is out
    torch.cuda.synchronize()
    assert same_01(x.cpu().numpy(), a)                      # a separate `out` leaves the input alone (NaNs and -0.0 included)
    assert same_01(out.cpu().numpy(), want)
    back = E.label_dilate(keep, r)
    assert back is keep
    assert same_01(keep.cpu().numpy(), want) and torch.equal(keep, out)


@pytest.mark.parametrize("shape", SHAPES)
def test_lone_voxels_on_either_side_of_a_word_boundary(shape):
    """one voxel in the last x position of a word (or of the row, when it is shorter than a word) and one in the first position
    of the next word, in different rows: what crosses the boundary is the carry of the shifts"""
    from mt3d_amd.engine import ops as E
    B, C, Z, Y, X = shape
    a = np.zeros(shape, dtype=np.float32)
    a[0, 0, Z // 2, Y // 2, min(63, X - 1)] = 0.5
    if X > 64:
        a[-1, -1, Z - 1, 0, 64] = 1.0
        a[-1, -1, 0, Y - 1, X - 1] = 1.0 / 255.0
    for r in (5, 8):
        x = torch.from_numpy(a).cuda()
        assert same_01(E.label_dilate(x, r).cpu().numpy(), oracle(a, r)), r


def test_all_on_all_off_and_the_sign_of_zero():
    from mt3d_amd.engine import ops as E
    shape = (2, 1, 9, 37, 130)
    on = torch.full(shape, 1.0 / 255.0, device="cuda")
    assert same_01(E.label_dilate(on, 5).cpu().numpy(), np.ones(shape, dtype=np.float32))
    off = np.full(shape, -0.0, dtype=np.float32)
    off[0, 0, 1, 2, 3], off[1, 0, 8, 36, 129], off[1, 0, 0, 0, 64] = np.nan, -1.0, 0.0
    got = E.label_dilate(torch.from_numpy(off).cuda(), 8).cpu().numpy()
    assert same_01(got, np.zeros(shape, dtype=np.float32)) and not np.signbit(got).any()


def test_on_another_stream_and_through_a_non_contiguous_batch():
    from mt3d_amd.engine import ops as E
    shape, r = SHAPES[3], 5
    a, want = case(shape, r)
    s = torch.cuda.Stream()
    x = torch.from_numpy(a.copy()).cuda()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        got = E.label_dilate(x, r)
    s.synchronize()
    assert same_01(got.cpu().numpy(), want)
    wide = torch.zeros(shape[:-1] + (shape[-1] + 3,), device="cuda")
    view = wide[..., 3:]
    view.copy_(torch.from_numpy(a.copy()))
    back = E.label_dilate(view, r)                          # made contiguous for the kernel, handed back to the view's storage
    assert back is view and same_01(view.cpu().numpy(), want) and float(wide[..., :3].abs().sum()) == 0.0


def test_bad_arguments_are_refused_before_anything_is_launched():
    from mt3d_amd.engine import ops as E
    from mt3d_amd.engine.lib import RxError, load
    lib = load()
    sp = E.stream_ptr()
    shape, r = (1, 2, 13, 11, 70), 5
    a, want = case(shape, r)
    x = torch.from_numpy(a.copy()).cuda()
    out = torch.full_like(x, -7.0)
    need = lib.rx_dilate_workspace(*shape)
    assert need == 2 * 13 * 11 * 2 * 8
    scratch = torch.zeros(need // 8, dtype=torch.int64, device="cuda")
    xp, op_, wp = x.data_ptr(), out.data_ptr(), scratch.data_ptr()
    refused = {
        "radius 0": ((xp, op_, wp, need, 1, 2, 13, 11, 70, 0), -1),
        "radius 9": ((xp, op_, wp, need, 1, 2, 13, 11, 70, 9), -1),
        "x = 0": ((xp, op_, wp, need, 1, 2, 13, 11, 0, 5), -1),
        "batch 0": ((xp, op_, wp, need, 0, 2, 13, 11, 70, 5), -1),
        "null in": ((None, op_, wp, need, 1, 2, 13, 11, 70, 5), -1),
        "null out": ((xp, None, wp, need, 1, 2, 13, 11, 70, 5), -1),
        "null scratch": ((xp, op_, None, need, 1, 2, 13, 11, 70, 5), -1),
        "a sample beyond the index arithmetic": ((xp, op_, wp, need, 1, 1, 2048, 2048, 2048, 5), -1),
        "scratch one byte short": ((xp, op_, wp, need - 1, 1, 2, 13, 11, 70, 5), -4),
    }
    for name, (args, status) in refused.items():
        assert lib.rx_label_dilate(*args, sp) == status, name
        assert b"rx_label_dilate" in lib.rx_last_error(), name
    with pytest.raises(RxError, match="rx_label_dilate.*status -1"):
        E.label_dilate(x, 9)
    with pytest.raises(RxError):
        E.label_dilate(x.cpu(), 5)
    with pytest.raises(RxError):
        E.label_dilate(x.double(), 5)
    with pytest.raises(RxError):
        E.label_dilate(x, 5, out=out[:, :1])
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()) and same_01(x.cpu().numpy(), a)          # nothing was launched
    assert lib.rx_label_dilate(xp, op_, wp, need, 1, 2, 13, 11, 70, 5, sp) == 0      # and the good call runs
    torch.cuda.synchronize()
    assert same_01(out.cpu().numpy(), want)


def test_device_dilate_touches_the_named_targets_only():
    from mt3d_amd.engine.lib import RxError
    shape, r = (2, 1, 12, 13, 64), 5
    a, want = case(shape, r)
    rng = np.random.default_rng(2)
    img, nrm = rng.standard_normal(shape).astype(np.float32), rng.standard_normal((2, 3, 12, 13, 64)).astype(np.float32)
    batch = {"image": torch.from_numpy(img).cuda(), "sheet": torch.from_numpy(a.copy()).cuda(), "normals": torch.from_numpy(nrm).cuda()}
    before = dict(batch)
    out = D.DeviceDilate(["sheet"], r)(batch)
    assert set(out) == set(before) and all(out[k] is before[k] for k in before)
    assert same_01(out["sheet"].cpu().numpy(), want)
    assert same_01(out["image"].cpu().numpy(), img) and same_01(out["normals"].cpu().numpy(), nrm)
    four = {"sheet": torch.from_numpy(a[:, 0].copy()).cuda()}          # (B, Z, Y, X)
    assert same_01(D.DeviceDilate(["sheet"], r)(four)["sheet"].cpu().numpy(), want[:, 0])
    with pytest.raises(RxError, match="sheet"):
        D.DeviceDilate(["sheet"], r)({"image": batch["image"], "sheet": batch["sheet"].cpu()})


# ---- through the dataset, the feeder and the trainer -----------------------------------------------------------------------------
def _write_volume(tmp):
    """a 48 x 56 x 160 volume with a wavy sheet about 3 voxels thick, an image and a normals array, as zarr_lite stores"""
    from mt3d_amd.dataloading import zarr_lite
    rng = np.random.default_rng(0)
    shape = (48, 56, 160)
    z, y, x = np.meshgrid(*[np.arange(n) for n in shape], indexing="ij")
    sheet = np.abs(((y + 6 * np.sin(x / 9.0) + 4 * np.cos(z / 7.0)) % 16) - 8) < 1.5
    img = (sheet * 140 + rng.integers(0, 80, size=shape)).astype(np.uint8)
    nrm = (rng.integers(1, 65535, size=shape + (3,)) * sheet[..., None]).astype(np.uint16)
    os.makedirs(tmp, exist_ok=True)
    paths = {k: os.path.join(tmp, f"{k}.zarr") for k in ("img", "sheet", "normals")}
    zarr_lite.write_array(paths["img"], img, (16, 32, 80), compressor="zlib")
    zarr_lite.write_array(paths["sheet"], (sheet * 255).astype(np.uint8), (16, 32, 80), compressor="zlib")
    zarr_lite.write_array(paths["normals"], nrm, (16, 32, 80, 3), compressor="zlib")
    return paths


def test_feeder_batches_are_the_host_dataset_items(tmp_path):
    from types import SimpleNamespace
    from torch.utils.data import DataLoader
    from mt3d_amd.dataloading.dataset import ZarrSegmentationDataset3D
    from mt3d_amd.dataloading.stages import DevicePipeline
    from mt3d_amd.train import DeviceFeeder
    paths = _write_volume(str(tmp_path))
    tasks = {"sheet": {"channels": 1}, "normals": {"channels": 3}}

    def dataset(**dataset_config):
        return ZarrSegmentationDataset3D(SimpleNamespace(
            model_name="m", tasks=tasks, train_patch_size=(16, 24, 72), min_labeled_ratio=0.05, min_bbox_percent=0.5, dilate_label=True,
            use_cache=False, cache_folder=str(tmp_path / "cache"), dataset_config=dict(augment=False, **dataset_config),
            volume_paths=[{"input": paths["img"], "sheet": paths["sheet"], "normals": paths["normals"], "ref_label": "sheet"}]))
    dev_ds = dataset(dilate={"where": "device", "radius": 5})
    assert dev_ds.device_dilate["keys"] == ["sheet"] and len(dev_ds) >= 4
    n = min(len(dev_ds), 6)
    try:
        import scipy.ndimage  # noqa: F401
        host_ds = dataset()
        want = [host_ds[i] for i in range(n)]
    except ImportError:          # no scipy on this machine: the statement of the device stage applied to the raw items
        want = []
        for i in range(n):
            it = dict(dev_ds[i])
            it["sheet"] = torch.from_numpy(D.dilate_numpy(it["sheet"].numpy(), 5))
            want.append(it)
    device = torch.device("cuda", torch.cuda.current_device())
    loader = DataLoader(torch.utils.data.Subset(dev_ds, list(range(n))), batch_size=2, shuffle=False, num_workers=0)
    stage = D.DeviceDilate(dev_ds.device_dilate["keys"], dev_ds.device_dilate["radius"])
    seen = 0
    for b, batch in enumerate(DeviceFeeder(loader, device, DevicePipeline(dilate=stage))):
        torch.cuda.synchronize()
        for j in range(batch["image"].shape[0]):
            w = want[2 * b + j]
            assert batch["sheet"].shape[1:] == (1, 16, 24, 72)
            for k in ("image", "sheet", "normals"):
                assert batch[k].is_cuda and same_01(batch[k][j].cpu().numpy(), w[k].numpy()), (b, j, k)
            assert float(batch["sheet"][j].sum()) > float((dev_ds[2 * b + j]["sheet"] > 0).sum())
            seen += 1
    assert seen == n


def _trainer_run(tmp):
    """two steps of BaseTrainer with dilate_label and dilate.where: device; every sheet target the loss saw is 0 / 1 and is
    `dilate_numpy` of a raw item"""
    import yaml
    from mt3d_amd.dataloading.dataset import ZarrSegmentationDataset3D
    from mt3d_amd.train import BaseTrainer
    paths = _write_volume(tmp)
    cfg = yaml.safe_load(open(CFG))
    cfg["tr_setup"].update(model_name="zarr_dilate", dilate_label=True, ckpt_out_base=os.path.join(tmp, "ckpt"),
                           tensorboard_log_dir=os.path.join(tmp, "tb"))
    cfg["tr_config"].update(max_epoch=1, max_steps_per_epoch=2, max_val_steps_per_epoch=1, patch_size=[32, 32, 32], compile=False)
    cfg["dataset_config"]["targets"]["normals"] = {"channels": 3, "activation": "none", "weight": 1, "loss_fn": "MaskedCosineLoss"}
    cfg["dataset_config"].update(synthetic=False, min_labeled_ratio=0.05, min_bbox_percent=0.5, use_cache=False,
                                 cache_folder=os.path.join(tmp, "cache"), augment=False, dilate={"where": "device", "radius": 5},
                                 volume_paths=[{"input": paths["img"], "sheet": paths["sheet"], "normals": paths["normals"],
                                                "ref_label": "sheet"}])
    p = os.path.join(tmp, "cfg.yaml")
    yaml.safe_dump(cfg, open(p, "w"))
    os.chdir(tmp)
    targets, losses = [], []

    class Rec(BaseTrainer):
        def _build_loss(self):
            fns = super()._build_loss()

            def wrap(name, fn):
                def f(pred, gt):
                    if name == "sheet":
                        targets.append(gt.detach().cpu().clone())
                    out = fn(pred, gt)
                    losses.append(out.detach())
                    return out
                return f
            return {k: wrap(k, v) for k, v in fns.items()}

    torch.manual_seed(1234)
    np.random.seed(1234)
    tr = Rec(p, verbose=False)
    ds = tr._configure_dataset()
    assert isinstance(ds, ZarrSegmentationDataset3D) and ds.device_dilate == {"radius": 5, "where": "device", "keys": ["sheet"]}
    dilated = [D.dilate_numpy(ds[i]["sheet"].numpy(), 5) for i in range(len(ds))]
    tr.train()
    torch.cuda.synchronize()
    assert tr.device_dilate is not None and tr.device_dilate.radius == 5 and tr.device_dilate.keys == ["sheet"]
    assert len(targets) == 3 and len(losses) == 6 and all(bool(torch.isfinite(l).all()) for l in losses)
    for t in targets:          # training batches (staged or not) and the validation batch
        for i in range(t.shape[0]):
            assert any(same_01(t[i].numpy(), d) for d in dilated)
    return len(targets)


def _child(tmp, feeder):
    env = dict(os.environ, RX_DEVICE_FEEDER="1" if feeder else "0")
    code = (f"import sys; sys.path[:0] = [{ROOT!r}, {os.path.join(ROOT, 'tests')!r}]; import test_dilate_gpu as t; "
            f"print('RESULT', t._trainer_run({str(tmp)!r}))")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "RESULT 3" in r.stdout


@pytest.mark.parametrize("feeder", [True, False])
def test_two_trainer_steps_with_the_device_stage(tmp_path, feeder):
    """a fresh child process for the environment switch: behind the feeder and with RX_DEVICE_FEEDER=0 (and for validation
    either way) the loss sees dilated labels"""
    _child(str(tmp_path / "run"), feeder)
