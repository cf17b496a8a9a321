"""GPU: rx_affine_apply (csrc/rx_affine.hip), its wrappers and DeviceSpatial against `affine_numpy`, the numpy statement that
tests/test_spatial_cpu.py anchors to torch's grid_sample and to the signed permutations.  Every comparison is bit for bit on int32
views."""
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch

import mt3d_amd  # noqa: F401
from mt3d_amd.dataloading import geometry_device as G
from mt3d_amd.dataloading import spatial_device as S

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "tasks", "synthetic_sheet.yaml")

# bricks are 32 x 8 x 4 (x, y, z): partial bricks on every axis, x no multiple of a wave, more than one brick per axis
SHAPES = [(10, 10, 10), (6, 12, 20), (33, 17, 65), (32, 32, 32)]
# (interp, border, fill)
MODES = [("linear", "constant", 0.0), ("linear", "constant", 0.5), ("linear", "clamp", 0.0), ("nearest", "constant", 0.0)]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and bool((a.view(np.int32) == b.view(np.int32)).all())


def field(shape, seed):
    """float32 with about a third of the voxels exactly +0.0 (what a masked normals target looks like) and some denormals"""
    rng = np.random.default_rng(seed)
    a = rng.standard_normal(shape).astype(np.float32) * (rng.random(shape[-3:]) < 0.66).astype(np.float32)
    a[a == 0] = 0.0
    a.reshape(-1)[::97] = np.float32(1e-41)
    return a


def make_ops():
    """identity and signed permutations; 7, 30, 45 and 90 degrees about each axis and chained; the scale limits (at 2.0 most
    sources are outside: the guards); a composed draw"""
    ops = [S.AffineOp(), S.from_geom(G.rot90_op("x", 1)), S.from_geom(G.compose(G.flip_op(2), G.rot90_op("y", 3)))]
    ops += [S.rotation_op(ax, deg) for ax in "zyx" for deg in (7.0, 30.0, 45.0, 90.0)]
    ops += [S.compose(S.compose(S.rotation_op("z", 7.0), S.rotation_op("y", -30.0)), S.rotation_op("x", 45.0)),
            S.compose(S.rotation_op("x", 90.0), S.rotation_op("z", 30.0)), S.scale_op(0.5), S.scale_op(2.0),
            S.draw_affine(random.Random(11), {"axes": ("z", "y", "x"), "max_degrees": 30.0, "p": 1.0}, {"range": (0.8, 1.25), "p": 1.0})]
    return ops


OPS = make_ops()


def device_apply(x, ops, interp, border, fill=0.0, vector=False):
    from mt3d_amd.engine import ops as E
    out = E.affine_apply(torch.from_numpy(x).cuda(), E.affine_table(ops), interp, border, fill, vector)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def oracle(x, ops, interp, border, fill=0.0, vector=False):
    return np.stack([S.affine_numpy(op, x[i], interp, border, fill, vector) for i, op in enumerate(ops)])


@pytest.mark.parametrize("shape", SHAPES)
def test_every_op_mode_and_channel_count(shape):
    assert len(OPS) > 16          # one batch: the by-value table crosses a launch boundary
    for channels in (1, 2, 3):
        x = field((len(OPS), channels, *shape), channels)
        for interp, border, fill in MODES:
            got, want = device_apply(x, OPS, interp, border, fill), oracle(x, OPS, interp, border, fill)
            for i, op in enumerate(OPS):
                assert same_bits(got[i], want[i]), (shape, channels, interp, border, fill, i, op)
    x = field((len(OPS), 3, *shape), 7)
    for interp, border, fill in (MODES[0], MODES[2], MODES[3]):          # the vector rule, against the same tensor without it
        got, want = device_apply(x, OPS, interp, border, fill, True), oracle(x, OPS, interp, border, fill, True)
        for i, op in enumerate(OPS):
            assert same_bits(got[i], want[i]), (shape, "vector", interp, border, i, op)
        assert not same_bits(got, device_apply(x, OPS, interp, border, fill, False))
    if shape == (32, 32, 32):
        far = device_apply(x, [S.scale_op(2.0)] * len(OPS), "linear", "constant", 0.5)
        assert (far == 0.5).mean() > 0.8          # scale 2.0: most sources are outside


def test_a_batch_of_17():
    ops = [OPS[(5 * i) % len(OPS)] for i in range(17)]          # 16 samples ride in one launch: 17 = 16 + 1
    x = field((17, 3, 10, 10, 10), 5)
    for interp, border, fill, vector in (("linear", "constant", 0.0, False), ("nearest", "constant", 0.0, True)):
        got, want = device_apply(x, ops, interp, border, fill, vector), oracle(x, ops, interp, border, fill, vector)
        for i in range(17):
            assert same_bits(got[i], want[i]), (interp, vector, i, ops[i])


def test_signed_permutations_on_the_device_are_the_geometry_kernel():
    from mt3d_amd.engine import ops as E
    shape = (10, 10, 10)
    gops = [G.GeomOp(), G.flip_op(0), G.rot90_op("z", 1), G.rot90_op("y", 3), G.compose(G.flip_op(2), G.rot90_op("x", 1))]
    x = np.abs(field((len(gops), 2, *shape), 3)) + np.float32(0.5)          # no -0.0: a lerp with weight 0 would turn it into +0.0
    want = E.geom_apply(torch.from_numpy(x).cuda(), gops, False).cpu().numpy()
    for interp, border in (("linear", "constant"), ("nearest", "constant"), ("linear", "clamp")):
        assert same_bits(device_apply(x, [S.from_geom(g) for g in gops], interp, border), want)


def test_bad_arguments_are_refused_before_anything_is_launched():
    from mt3d_amd.engine import ops as E
    from mt3d_amd.engine.lib import RxError, load
    lib = load()
    x3 = torch.from_numpy(field((2, 3, 4, 8, 8), 0)).cuda()
    x2 = torch.from_numpy(field((2, 2, 4, 8, 8), 1)).cuda()
    out3, out2 = torch.full_like(x3, -7.0), torch.full_like(x2, -7.0)
    good = E.affine_table([S.AffineOp(), S.rotation_op("z", 30.0)])
    nan = good.copy()
    nan[1, 4] = np.nan
    inf = good.copy()
    inf[0, 12] = np.inf
    with pytest.raises(RxError, match="rx_affine_apply.*status -1"):          # in is out
        E.affine_apply(x3, good, "linear", "constant", out=x3)
    before = x3.clone()
    with pytest.raises(RxError, match="rx_affine_apply.*status -1"):          # vector with c = 2
        E.affine_apply(x2, good, "nearest", "constant", vector=True, out=out2)
    for bad in (nan, inf):
        with pytest.raises(RxError, match="rx_affine_apply.*status -1"):      # a matrix entry that is not finite
            E.affine_apply(x3, bad, "linear", "constant", out=out3)
    with pytest.raises(RxError):                                              # a CPU tensor
        E.affine_apply(x3.cpu(), good, "linear", "constant")
    with pytest.raises(RxError):
        E.affine_apply(x3.double(), good, "linear", "constant")
    with pytest.raises(RxError):
        E.affine_apply(x3, good, "cubic", "constant")
    with pytest.raises(RxError):
        E.affine_apply(x3, good[:1], "linear", "constant")

    def raw(inp, outp, batch, c, z, y, xx, table, interp, border, vector):
        return lib.rx_affine_apply(inp, outp, batch, c, z, y, xx, None if table is None else table.ctypes.data, interp, border, 0.0, vector,
                                   E.stream_ptr())
    xp, op_ = x3.data_ptr(), out3.data_ptr()
    refused = {
        "null in": (None, op_, 2, 3, 4, 8, 8, good, 0, 0, 0), "null out": (xp, None, 2, 3, 4, 8, 8, good, 0, 0, 0),
        "null table": (xp, op_, 2, 3, 4, 8, 8, None, 0, 0, 0), "batch 0": (xp, op_, 0, 3, 4, 8, 8, good, 0, 0, 0),
        "interp": (xp, op_, 2, 3, 4, 8, 8, good, 2, 0, 0), "border": (xp, op_, 2, 3, 4, 8, 8, good, 0, 2, 0),
        "extent beyond the index arithmetic": (xp, op_, 2, 3, 2048, 2048, 2048, good, 0, 0, 0),
        "z beyond a grid dimension": (xp, op_, 2, 3, 70000, 8, 8, good, 0, 0, 0),
        "too many channels": (xp, op_, 2, 5000, 4, 8, 8, good, 0, 0, 0),
    }
    for name, args in refused.items():
        assert raw(*args) == -1, name
        assert b"rx_affine_apply" in lib.rx_last_error(), name
    torch.cuda.synchronize()
    assert bool((out3 == -7.0).all()) and bool((out2 == -7.0).all()) and torch.equal(x3, before)          # nothing was launched
    got = E.affine_apply(x3, good, "linear", "constant", out=out3)          # and the good table runs, into `out`
    torch.cuda.synchronize()
    assert got is out3
    assert same_bits(out3.cpu().numpy(), oracle(x3.cpu().numpy(), [S.AffineOp(), S.rotation_op("z", 30.0)], "linear", "constant"))


def test_device_spatial():
    from mt3d_amd.engine.lib import RxError
    rot = {"axes": ("z", "y", "x"), "max_degrees": 30.0, "p": 0.7}
    sc = {"range": (0.8, 1.25), "p": 0.5}
    B, shape = 5, (12, 20, 33)
    sheet = (np.random.default_rng(0).random((B, *shape)) < 0.3).astype(np.float32)          # (B, Z, Y, X): viewed as one channel
    host = {"image": field((B, 1, *shape), 1), "sheet": sheet, "normals": field((B, 3, *shape), 2) * sheet[:, None]}
    x = {k: torch.from_numpy(v).cuda() for k, v in host.items()}
    for border, fill in (("constant", 0.0), ("clamp", 0.0), ("constant", 0.25)):
        a = S.DeviceSpatial(rotation=rot, scale=sc, image_border=border, image_fill=fill, seed=5)
        b = S.DeviceSpatial(rotation=rot, scale=sc, image_border=border, image_fill=fill, seed=5)
        ya, yb = a(x), b(x)
        torch.cuda.synchronize()
        assert a.last_ops == b.last_ops and len(a.last_ops) == B and not all(op.is_identity() for op in a.last_ops)
        assert all(torch.equal(ya[k], yb[k]) for k in x) and all(ya[k].shape == x[k].shape for k in x)
        assert same_bits(ya["image"].cpu().numpy(), oracle(host["image"], a.last_ops, "linear", border, fill))
        assert same_bits(ya["sheet"].cpu().numpy(), oracle(host["sheet"][:, None], a.last_ops, "nearest", "constant")[:, 0])
        assert same_bits(ya["normals"].cpu().numpy(), oracle(host["normals"], a.last_ops, "nearest", "constant", 0.0, True))
        assert set(np.unique(ya["sheet"].cpu().numpy())) <= {0.0, 1.0}          # a label stays binary ...
        off = ya["sheet"].cpu().numpy() == 0
        assert (ya["normals"].cpu().numpy()[np.broadcast_to(off[:, None], (B, 3, *shape))] == 0).all()      # ... normals zero off it
    assert S.DeviceSpatial(rotation=rot, scale=sc, seed=5, rank=0).draw() != S.DeviceSpatial(rotation=rot, scale=sc, seed=5, rank=1).draw()
    still = S.DeviceSpatial(rotation=dict(rot, p=0.0), scale=dict(sc, p=0.0), seed=5)
    y = still(x)
    assert all(y[k] is x[k] for k in x) and all(op.is_identity() for op in still.last_ops)
    given = S.DeviceSpatial(seed=1)
    y = given(x, ops=[S.scale_op(0.9)] * B)
    assert given.last_ops == [S.scale_op(0.9)] * B and y["image"] is not x["image"]
    with pytest.raises(RxError, match="device tensor"):
        given({"image": x["image"].cpu()})
    with pytest.raises(RxError, match="expected"):
        given({"image": x["image"][0, 0]})
    with pytest.raises(RxError, match="normal_keys"):
        given({"image": x["image"], "normals": x["normals"][:, :2]})


# ---- through the trainer -------------------------------------------------------------------------------------------------------
BLOCK = {"rotation": {"axes": ["z", "y", "x"], "max_degrees": 30, "p": 0.8}, "scale": {"range": [0.8, 1.25], "p": 0.5},
         "normal_keys": ["normals"], "image_border": "constant", "where": "device"}


def _trainer_run(tmp, variant):
    """one short epoch of BaseTrainer on synthetic patches with a sheet and a normals task; returns the bits of every loss.
    variant: "on" (the block), "nokey", "false" (spatial: false) or "never" (the block with both probabilities 0)"""
    import yaml
    from mt3d_amd.train import BaseTrainer
    os.makedirs(tmp, exist_ok=True)
    cfg = yaml.safe_load(open(CFG))
    cfg["tr_setup"].update(model_name="spatial", ckpt_out_base=os.path.join(tmp, "ckpt"), tensorboard_log_dir=os.path.join(tmp, "tb"))
    cfg["tr_config"].update(max_epoch=1, max_steps_per_epoch=3, max_val_steps_per_epoch=1, patch_size=[16, 16, 16], compile=False)
    cfg["dataset_config"]["targets"]["normals"] = {"channels": 3, "activation": "none", "weight": 1, "loss_fn": "MaskedCosineLoss"}
    if variant == "on":
        cfg["dataset_config"]["spatial"] = BLOCK
    elif variant == "false":
        cfg["dataset_config"]["spatial"] = False
    elif variant == "never":
        cfg["dataset_config"]["spatial"] = dict(BLOCK, rotation=dict(BLOCK["rotation"], p=0.0), scale=dict(BLOCK["scale"], p=0.0))
    p = os.path.join(tmp, "cfg.yaml")
    yaml.safe_dump(cfg, open(p, "w"))
    os.chdir(tmp)
    losses, calls = [], []
    real_call = S.DeviceSpatial.__call__

    def recording_call(self, batch, ops=None):
        out = real_call(self, batch, ops)
        calls.append((batch["image"].shape[0], sum(not op.is_identity() for op in self.last_ops), out["image"] is batch["image"]))
        return out

    class Rec(BaseTrainer):
        def _build_loss(self):
            fns = super()._build_loss()

            def wrap(fn):
                def f(pred, gt):
                    out = fn(pred, gt)
                    losses.append(out.detach())
                    return out
                return f
            return {k: wrap(v) for k, v in fns.items()}

    torch.manual_seed(1234)
    np.random.seed(1234)
    tr = Rec(p, verbose=False)
    S.DeviceSpatial.__call__ = recording_call
    try:
        tr.train()
    finally:
        S.DeviceSpatial.__call__ = real_call
    torch.cuda.synchronize()
    assert len(losses) == 2 * (3 + 1) and all(bool(torch.isfinite(l).all()) for l in losses)
    if variant in ("on", "never"):
        assert tr.device_spatial is not None and tr.device_spatial.last_ops is not None
        assert len(calls) >= 3 + 1          # every training batch (the feeder stages one ahead) and the validation batch
        if variant == "on":
            assert sum(c[1] for c in calls) > 0 and all(c[2] == (c[1] == 0) for c in calls)
        else:
            assert all(c[1] == 0 and c[2] for c in calls)
    else:
        assert tr.device_spatial is None and not calls
    return [int(np.float32(float(l)).view(np.uint32)) for l in losses]


def _child(tmp, variant, feeder=True):
    env = dict(os.environ, RX_DEVICE_FEEDER="1" if feeder else "0")
    code = (f"import sys; sys.path[:0] = [{ROOT!r}, {os.path.join(ROOT, 'tests')!r}]; import test_spatial_gpu as t; "
            f"print('RESULT', t._trainer_run({str(tmp)!r}, {variant!r}))")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    assert len(line) == 1, r.stdout[-2000:]
    return line[0]


@pytest.mark.parametrize("feeder", [True, False])
def test_one_trainer_epoch_with_the_block(tmp_path, feeder):
    """a fresh child process for the environment switch: behind the feeder and with RX_DEVICE_FEEDER=0 (and for validation either
    way) `trainer.device_spatial` draws for every batch and the losses are finite"""
    assert _child(str(tmp_path / "on"), "on", feeder).count(",") == 7


def test_trainer_with_the_block_absent_or_never_drawing_is_the_run_without_the_key(tmp_path):
    """same seeds: `spatial: false`, and the block with both probabilities 0 (every draw the identity, every batch handed back
    untouched), give the loss bits of a run without the key"""
    nokey = _child(str(tmp_path / "nokey"), "nokey")
    assert _child(str(tmp_path / "false"), "false") == nokey and nokey.count(",") == 7
    assert _child(str(tmp_path / "never"), "never") == nokey
