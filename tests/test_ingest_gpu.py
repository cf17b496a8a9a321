"""GPU: rx_ingest (csrc/rx_ingest.hip) against the numpy statement `ingest_numpy`, through `ops.ingest`, `DeviceIngest`, the
feeder and the trainer.  Every comparison is on the float32 bit patterns: no tolerance anywhere."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import mt3d_amd  # noqa: F401
from mt3d_amd.dataloading import ingest_device as I

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "tasks", "synthetic_sheet.yaml")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_ingest_cpu import same_bits  # noqa: E402


def oracle(a, rule):
    """`ingest_numpy` of every sample of a (B, Z, Y, X[, C]) array -> (B, C, Z, Y, X)"""
    return np.stack([I.ingest_numpy(s, rule) for s in a])


def draw(shape, dtype, seed):
    """every sample different, the extremes of the dtype at the ends of every sample; float32: finite values of both signs"""
    rng = np.random.default_rng(seed)
    if np.dtype(dtype) == np.float32:
        a = rng.standard_normal(shape).astype(np.float32)
    else:
        hi = np.iinfo(dtype).max
        a = rng.integers(0, hi, size=shape, endpoint=True).astype(dtype)
        flat = a.reshape(shape[0], -1)
        flat[:, 0], flat[:, -1] = hi, 0
    return a


def run(a, rule, **kw):
    from mt3d_amd.engine import ops as E
    got = E.ingest(torch.from_numpy(a).cuda(), rule, **kw)
    torch.cuda.synchronize()
    return got


def test_every_uint8_and_uint16_value_under_every_rule():
    u8 = np.arange(256, dtype=np.uint8).reshape(1, 4, 8, 8)
    u16 = np.arange(65536, dtype=np.uint16).reshape(1, 16, 64, 64)
    for a in (u8, u16):
        for rule in I.RULES:
            got = run(a, rule)
            assert got.shape == (1, 1) + a.shape[1:] and got.dtype == torch.float32
            assert same_bits(got.cpu().numpy(), oracle(a, rule)), (a.dtype, rule)
    # the same values channels-last, so that the LDS path converts every one of them as well
    for a in (u8.reshape(1, 4, 8, 4, 2), u16.reshape(1, 16, 64, 8, 8)):
        for rule in I.RULES:
            assert same_bits(run(a, rule).cpu().numpy(), oracle(a, rule)), (a.dtype, rule)


@pytest.mark.parametrize("dtype,shape", [(np.uint8, (3, 5, 7, 13)), (np.uint16, (3, 5, 7, 70)), (np.float32, (3, 5, 7, 13)),
                                         (np.uint8, (2, 9, 37, 130)), (np.uint8, (4, 1, 1, 3))])
def test_head_and_tail_are_per_sample(dtype, shape):
    """uint8 (5, 7, 13): a sample stride of 455 bytes, so samples 1 and 2 start off every 16-byte boundary; uint16 x = 70: a
    stride of 4900 bytes; more than one workgroup per sample; samples shorter than a vector"""
    a = draw(shape, dtype, 3)
    for rule in ("copy", I.ingest_rule("image", dtype), I.ingest_rule("normals", dtype)):
        assert same_bits(run(a, rule).cpu().numpy(), oracle(a, rule)), rule


def test_bases_off_the_16_byte_grid():
    """the input at 4 and at 1 bytes past a boundary (the second cannot line loads up with stores: the scalar path), the output
    at 4 bytes past one"""
    from mt3d_amd.engine import ops as E
    a = draw((2, 5, 7, 13), np.uint8, 5)
    want = oracle(a, "div255")
    for off in (4, 1, 7):
        buf = torch.zeros(a.size + 16, dtype=torch.uint8, device="cuda")
        x = buf[off:off + a.size].view(a.shape)
        x.copy_(torch.from_numpy(a))
        assert x.data_ptr() % 16 == off
        assert same_bits(E.ingest(x, "div255").cpu().numpy(), want), off
    obuf = torch.full((want.size + 4,), -7.0, device="cuda")
    out = obuf[1:1 + want.size].view(want.shape)
    assert out.data_ptr() % 16 == 4
    for shape in ((2, 5, 7, 13), (2, 5, 7, 13, 1)):
        obuf.fill_(-7.0)
        assert E.ingest(torch.from_numpy(a.reshape(shape)).cuda(), "div255", out=out) is out
        assert same_bits(out.cpu().numpy(), want) and float(obuf[0]) == -7.0 and float(obuf[-1]) == -7.0
    c3 = draw((2, 3, 5, 9, 3), np.uint16, 6)
    w3 = oracle(c3, "normal_u16")
    obuf = torch.full((w3.size + 4,), -7.0, device="cuda")
    out = obuf[3:3 + w3.size].view(w3.shape)
    E.ingest(torch.from_numpy(c3).cuda(), "normal_u16", out=out)
    assert same_bits(out.cpu().numpy(), w3) and float(obuf[:3].sum()) == -21.0 and float(obuf[-1]) == -7.0


@pytest.mark.parametrize("dtype,shape,rule", [(np.uint16, (2, 5, 7, 13, 3), "normal_u16"), (np.float32, (2, 4, 6, 70, 3), "normal_mul2"),
                                              (np.uint8, (1, 3, 5, 9, 1), "normal_mul2"), (np.uint16, (1, 3, 5, 9, 2), "normal_u16"),
                                              (np.float32, (1, 3, 5, 9, 8), "copy"), (np.uint8, (1, 3, 5, 9, 8), "div255"),
                                              (np.uint16, (2, 11, 13, 17, 3), "normal_u16"), (np.uint8, (2, 11, 13, 17, 3), "normal_mul2")])
def test_channels_last_planes_are_the_numpy_transpose(dtype, shape, rule):
    """the issue's shapes, and (11, 13, 17): 2431 voxels, three tiles of 1024 with a short last one, for 1- and 2-byte elements"""
    a = draw(shape, dtype, 7)
    got = run(a, rule).cpu().numpy()
    assert got.shape == (shape[0], shape[4]) + shape[1:4]
    assert same_bits(got, oracle(a, rule))
    scaled = oracle(a.reshape(shape[0], -1, 1, 1), rule).reshape(shape)          # the rule alone, layout untouched
    for c in range(shape[4]):
        assert same_bits(got[:, c], scaled[..., c]), c


def test_float32_copy_keeps_every_bit():
    bits = np.array([0x80000000, 0x7f800000, 0xff800000, 0x7fc00000, 0x7fc12345, 0xffc00001, 0x7f800001, 0xff923456, 0x00000001,
                     0x807fffff, 0x00400000, 0x3f800000, 0x00000000], dtype=np.uint32)
    a = np.resize(bits, 2 * 3 * 5 * 14).view(np.float32).reshape(2, 3, 5, 14)
    got = run(a, "copy").cpu().numpy()
    assert np.array_equal(got.view(np.uint32), a.view(np.uint32)[:, None])
    cl = a.reshape(2, 3, 5, 7, 2)
    got = run(cl, "copy").cpu().numpy()
    assert np.array_equal(got.view(np.uint32), cl.view(np.uint32).transpose(0, 4, 1, 2, 3))


def test_on_another_stream_and_through_a_non_contiguous_batch():
    from mt3d_amd.engine import ops as E
    a = draw((4, 5, 7, 13, 3), np.uint16, 9)
    want = oracle(a, "normal_u16")
    x = torch.from_numpy(a).cuda()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        got = E.ingest(x, "normal_u16")
    s.synchronize()
    assert same_bits(got.cpu().numpy(), want)
    view = x[::2]                                   # a non-contiguous batch slice: made contiguous for the kernel
    assert not view.is_contiguous()
    got = E.ingest(view, "normal_u16")
    assert got.shape == (2, 3, 5, 7, 13) and same_bits(got.cpu().numpy(), want[::2])
    assert np.array_equal(x.cpu().numpy(), a)       # the input is never written


def test_bad_arguments_are_refused_before_anything_is_launched():
    from mt3d_amd.engine import ops as E
    from mt3d_amd.engine.lib import RxError, load
    lib = load()
    sp = E.stream_ptr()
    a = draw((2, 5, 7, 13), np.uint16, 1)
    want = oracle(a, "div65535")
    x = torch.from_numpy(a).cuda()
    out = torch.full((2, 1, 5, 7, 13), -7.0, device="cuda")
    xp, op_ = x.data_ptr(), out.data_ptr()
    refused = {
        "null in": (None, 1, op_, 2, 5, 7, 13, 1, 2), "null out": (xp, 1, None, 2, 5, 7, 13, 1, 2),
        "in == out": (op_, 2, op_, 2, 5, 7, 13, 1, 0), "unknown dtype": (xp, 3, op_, 2, 5, 7, 13, 1, 2),
        "unknown rule": (xp, 1, op_, 2, 5, 7, 13, 1, 5), "negative rule": (xp, 1, op_, 2, 5, 7, 13, 1, -1),
        "batch 0": (xp, 1, op_, 0, 5, 7, 13, 1, 2), "z 0": (xp, 1, op_, 2, 0, 7, 13, 1, 2), "x -1": (xp, 1, op_, 2, 5, 7, -1, 1, 2),
        "c 0": (xp, 1, op_, 2, 5, 7, 13, 0, 2), "c 9": (xp, 1, op_, 2, 5, 7, 13, 9, 2),
        "a sample of 2^31 elements": (xp, 1, op_, 1, 2048, 1024, 1024, 1, 2),
        "a sample of 2^31 elements with its channels": (xp, 1, op_, 1, 1024, 1024, 1024, 2, 2),
        "uint16 at an odd address": (xp + 1, 1, op_, 2, 5, 7, 13, 1, 2), "float32 at 2 mod 4": (xp + 2, 2, op_, 1, 5, 7, 13, 1, 0),
        "out at 2 mod 4": (xp, 1, op_ + 2, 2, 5, 7, 13, 1, 2),
    }
    for name, args in refused.items():
        assert lib.rx_ingest(*args, sp) == -1, name
        assert lib.rx_last_error().startswith(b"rx_ingest:"), name
    with pytest.raises(RxError, match="rule"):
        E.ingest(x, "div256")
    with pytest.raises(RxError):
        E.ingest(x.cpu(), "div65535")
    for bad in (torch.zeros(x.shape, dtype=dt, device="cuda") for dt in (torch.int32, torch.float64, torch.int16)):
        with pytest.raises(RxError, match="dtype"):
            E.ingest(bad, "copy")
    with pytest.raises(RxError):
        E.ingest(x[0], "div65535")                                               # (Z, Y, X): no batch axis
    with pytest.raises(RxError, match="rx_ingest.*status -1"):
        E.ingest(torch.zeros(1, 2, 2, 2, 9, dtype=torch.uint8, device="cuda"), "copy")
    with pytest.raises(RxError, match="out"):
        E.ingest(x, "div65535", out=out[:, 0])
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()) and np.array_equal(x.cpu().numpy(), a)      # nothing was launched
    assert lib.rx_ingest(xp, 1, op_, 2, 5, 7, 13, 1, 2, sp) == 0                 # and the good call runs
    torch.cuda.synchronize()
    assert same_bits(out.cpu().numpy(), want)


def test_device_ingest_touches_the_keys_with_rules_only():
    from mt3d_amd.engine.lib import RxError
    img, nrm = draw((2, 5, 7, 13), np.uint8, 2), draw((2, 5, 7, 13, 3), np.uint16, 3)
    flat_n = draw((2, 5, 7, 13), np.uint16, 4)
    ink = np.random.default_rng(4).random((2, 1, 5, 7, 13), dtype=np.float32)
    batch = {"image": torch.from_numpy(img).cuda(), "normals": torch.from_numpy(nrm).cuda(), "ink": torch.from_numpy(ink).cuda()}
    before = dict(batch)
    out = I.DeviceIngest({"image": "div255", "normals": "normal_u16"})(batch)
    torch.cuda.synchronize()
    assert set(out) == set(before) and out["ink"] is before["ink"] and all(batch[k] is before[k] for k in before)
    assert same_bits(out["image"].cpu().numpy(), oracle(img, "div255")) and out["image"].shape == (2, 1, 5, 7, 13)
    assert same_bits(out["normals"].cpu().numpy(), oracle(nrm, "normal_u16")) and out["normals"].shape == (2, 3, 5, 7, 13)
    assert np.array_equal(batch["image"].cpu().numpy(), img) and same_bits(out["ink"].cpu().numpy(), ink)
    # a 3-D normals store stays (B, Z, Y, X), as the host items have it
    out = I.DeviceIngest({"normals": "normal_u16"})({"normals": torch.from_numpy(flat_n).cuda()})
    assert out["normals"].shape == (2, 5, 7, 13) and same_bits(out["normals"].cpu().numpy(), oracle(flat_n, "normal_u16")[:, 0])
    with pytest.raises(RxError, match="image"):
        I.DeviceIngest({"image": "div255"})({"image": batch["image"].cpu()})
    with pytest.raises(RxError, match="no rule"):
        I.DeviceIngest({"normals": "normal_u16"})(batch)
    with pytest.raises(RxError, match="sheet"):
        I.DeviceIngest({"image": "div255", "sheet": "div255"})({"image": batch["image"]})


# ---- through the dataset, the feeder and the trainer -----------------------------------------------------------------------------
def _write_volume(tmp):
    """a 40 x 40 x 48 volume with a wavy sheet, a uint8 image and channels-last uint16 normals, as zarr_lite stores"""
    from mt3d_amd.dataloading import zarr_lite
    rng = np.random.default_rng(0)
    shape = (40, 40, 48)
    z, y, x = np.meshgrid(*[np.arange(n) for n in shape], indexing="ij")
    sheet = np.abs(((y + 4 * np.sin(x / 7.0) + 3 * np.cos(z / 5.0)) % 10) - 5) < 2.0
    img = (sheet * 140 + rng.integers(0, 80, size=shape)).astype(np.uint8)
    nrm = (rng.integers(1, 65535, size=shape + (3,)) * sheet[..., None]).astype(np.uint16)
    os.makedirs(tmp, exist_ok=True)
    paths = {k: os.path.join(tmp, f"{k}.zarr") for k in ("img", "sheet", "normals")}
    zarr_lite.write_array(paths["img"], img, (16, 16, 16), compressor="zlib")
    zarr_lite.write_array(paths["sheet"], (sheet * 255).astype(np.uint8), (16, 16, 16), compressor="zlib")
    zarr_lite.write_array(paths["normals"], nrm, (16, 16, 16, 3), compressor="zlib")
    return paths


def test_feeder_batches_are_the_collated_host_items(tmp_path):
    from types import SimpleNamespace
    from torch.utils.data import DataLoader, default_collate
    from mt3d_amd.dataloading.dataset import ZarrSegmentationDataset3D
    from mt3d_amd.dataloading.stages import DevicePipeline
    from mt3d_amd.train import DeviceFeeder, PinnedRingCollate
    paths = _write_volume(str(tmp_path))
    tasks = {"sheet": {"channels": 1}, "normals": {"channels": 3}}

    def dataset(**dataset_config):
        return ZarrSegmentationDataset3D(SimpleNamespace(
            model_name="m", tasks=tasks, train_patch_size=(16, 16, 16), min_labeled_ratio=0.05, min_bbox_percent=0.5, dilate_label=False,
            use_cache=False, cache_folder=str(tmp_path / "cache"), dataset_config=dict(augment=False, **dataset_config),
            volume_paths=[{"input": paths["img"], "sheet": paths["sheet"], "normals": paths["normals"], "ref_label": "sheet"}]))
    host_ds, dev_ds = dataset(ingest={"where": "host"}), dataset(ingest={"where": "device"})
    assert dev_ds.device_ingest == {"image": "div255", "sheet": "div255", "normals": "normal_u16"}
    n = min(len(dev_ds), 6)
    assert n >= 4 and len(host_ds) == len(dev_ds)
    want = [default_collate([host_ds[i], host_ds[i + 1]]) for i in range(0, n - 1, 2)]
    device = torch.device("cuda", torch.cuda.current_device())
    stage = I.DeviceIngest(dev_ds.device_ingest)
    for collate in (None, PinnedRingCollate()):          # default_collate, and the trainer's pinned ring
        loader = DataLoader(torch.utils.data.Subset(dev_ds, list(range(2 * len(want)))), batch_size=2, shuffle=False, num_workers=0,
                            **({"collate_fn": collate} if collate is not None else {}))
        seen = 0
        for b, batch in enumerate(DeviceFeeder(loader, device, DevicePipeline(ingest=stage))):
            torch.cuda.synchronize()
            assert batch["image"].shape == (2, 1, 16, 16, 16) and batch["normals"].shape == (2, 3, 16, 16, 16)
            for k in ("image", "sheet", "normals"):
                assert batch[k].is_cuda and batch[k].dtype == torch.float32
                assert same_bits(batch[k].cpu().numpy(), want[b][k].numpy()), (b, k)
            seen += 1
        assert seen == len(want)


def _trainer_run(tmp, where):
    """two steps of BaseTrainer on a zarr store (and one validation step); returns the bits of every loss the run computed"""
    import yaml
    from mt3d_amd.dataloading.dataset import ZarrSegmentationDataset3D
    from mt3d_amd.train import BaseTrainer
    paths = _write_volume(tmp)
    cfg = yaml.safe_load(open(CFG))
    cfg["tr_setup"].update(model_name="zarr_ingest", dilate_label=False, ckpt_out_base=os.path.join(tmp, "ckpt"),
                           tensorboard_log_dir=os.path.join(tmp, "tb"))
    cfg["tr_config"].update(max_epoch=1, max_steps_per_epoch=2, max_val_steps_per_epoch=1, patch_size=[16, 16, 16], compile=False)
    cfg["dataset_config"]["targets"]["normals"] = {"channels": 3, "activation": "none", "weight": 1, "loss_fn": "MaskedCosineLoss"}
    cfg["dataset_config"].update(synthetic=False, min_labeled_ratio=0.05, min_bbox_percent=0.5, use_cache=False,
                                 cache_folder=os.path.join(tmp, "cache"), augment=False, ingest={"where": where},
                                 volume_paths=[{"input": paths["img"], "sheet": paths["sheet"], "normals": paths["normals"],
                                                "ref_label": "sheet"}])
    p = os.path.join(tmp, "cfg.yaml")
    yaml.safe_dump(cfg, open(p, "w"))
    os.chdir(tmp)
    losses, dtypes = [], []

    class Rec(BaseTrainer):
        def _build_loss(self):
            fns = super()._build_loss()

            def wrap(fn):
                def f(pred, gt):
                    dtypes.append(gt.dtype)
                    out = fn(pred, gt)
                    losses.append(out.detach())
                    return out
                return f
            return {k: wrap(v) for k, v in fns.items()}

    torch.manual_seed(1234)
    np.random.seed(1234)
    tr = Rec(p, verbose=False)
    ds = tr._configure_dataset()
    assert isinstance(ds, ZarrSegmentationDataset3D) and (ds.device_ingest is not None) == (where == "device")
    tr.train()
    torch.cuda.synchronize()
    assert (tr.device_ingest is not None) == (where == "device")
    if where == "device":
        assert tr.device_ingest.rules == {"image": "div255", "sheet": "div255", "normals": "normal_u16"}
    assert len(losses) == 6 and all(bool(torch.isfinite(l).all()) for l in losses) and all(d == torch.float32 for d in dtypes)
    return [int(np.float32(float(l)).view(np.uint32)) for l in losses]


def _child(tmp, feeder, where):
    env = dict(os.environ, RX_DEVICE_FEEDER="1" if feeder else "0")
    code = (f"import sys; sys.path[:0] = [{ROOT!r}, {os.path.join(ROOT, 'tests')!r}]; import test_ingest_gpu as t; "
            f"print('RESULT', t._trainer_run({str(tmp)!r}, {where!r}))")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    assert len(line) == 1, r.stdout[-2000:]
    return line[0]


@pytest.mark.parametrize("feeder", [True, False])
def test_two_trainer_steps_with_the_device_stage(tmp_path, feeder):
    """fresh child processes for the environment switch: behind the feeder and with RX_DEVICE_FEEDER=0 (and for validation
    either way) the losses are finite and have the bits of the `where: host` run -- same seeds, same inputs to the bit"""
    dev = _child(str(tmp_path / "dev"), feeder, "device")
    host = _child(str(tmp_path / "host"), feeder, "host")
    assert dev == host and dev.count(",") == 5
