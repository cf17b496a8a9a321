"""GPU: rx_elastic_apply (csrc/rx_elastic.hip), its wrappers and DeviceElastic against `elastic_numpy`, the numpy statement that
tests/test_elastic_cpu.py anchors to a float64 B-spline.  Every comparison is bit for bit on int32 views, the vector rule's
square root and division included (hipcc rounds both correctly by default)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import mt3d_amd  # noqa: F401
from mt3d_amd.dataloading import elastic_device as M
from mt3d_amd.dataloading import spatial_device as S

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "tasks", "synthetic_sheet.yaml")

# bricks are 64 x 4 x 8 (x, y, z).  (B, C, Z, Y, X), spacing: one partial brick; an x tail past one 64-lane row, odd extents, a
# spacing per axis; whole bricks, two per row, several z walks
CASES = [((1, 1, 9, 10, 11), (8, 8, 8)), ((2, 3, 17, 33, 70), (8, 16, 32)), ((3, 4, 8, 64, 128), (16, 16, 16))]
GUARD = 64


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and bool((a.view(np.int32) == b.view(np.int32)).all())


def data(shape, seed):
    """float32 with about a third of the voxels exactly +0.0 (what a masked normals target looks like) and some denormals"""
    rng = np.random.default_rng(seed)
    a = rng.standard_normal(shape).astype(np.float32) * (rng.random(shape[-3:]) < 0.66).astype(np.float32)
    a[a == 0] = 0.0
    a.reshape(-1)[::97] = np.float32(1e-41)
    return a


def fields_for(shape, spacing, seed, amplitude=None):
    """one field per sample, nodes uniform in +- the largest magnitude the config allows for this spacing"""
    amplitude = min(spacing) / 6.0 * (1.0 - 1e-6) if amplitude is None else amplitude
    rng = np.random.default_rng(seed)
    g = M.grid_shape(shape[2:], spacing)
    return [M.ElasticField(rng.uniform(-amplitude, amplitude, (3,) + g), spacing) for _ in range(shape[0])]


def device_apply(x, fields, interp, border, fill=0.0, vector=False):
    """through `ops`, into a NaN-prefilled output that sits between guard elements; input and guards must come back unchanged"""
    from mt3d_amd.engine import ops as E
    xd = torch.from_numpy(x).cuda()
    keep = xd.clone()
    buf = torch.full((x.size + 2 * GUARD,), float("nan"), device="cuda")
    buf[:GUARD] = -7.0
    buf[-GUARD:] = -7.0
    out = buf[GUARD:-GUARD].view(x.shape)
    sp = fields[0].spacing
    got = E.elastic_apply(xd, E.elastic_nodes(fields), E.elastic_tables(x.shape[2:], sp), sp, interp, border, fill, vector, out=out)
    torch.cuda.synchronize()
    assert got is out and torch.equal(xd.view(torch.int32), keep.view(torch.int32))
    assert bool((buf[:GUARD] == -7.0).all()) and bool((buf[-GUARD:] == -7.0).all())
    return out.cpu().numpy()


def oracle(x, fields, interp, border, fill=0.0, vector=False):
    return np.stack([M.elastic_numpy(f, x[i], interp, border, fill, vector) for i, f in enumerate(fields)])


@pytest.mark.parametrize("shape,spacing", CASES)
def test_every_mode_bit_for_bit(shape, spacing):
    fields = fields_for(shape, spacing, 1)
    x = data(shape, 2)
    x3 = x if shape[1] == 3 else data((shape[0], 3, *shape[2:]), 3)
    for interp in ("linear", "nearest"):
        for border in ("constant", "clamp"):
            for fill in (0.0, 0.5):
                got, want = device_apply(x, fields, interp, border, fill), oracle(x, fields, interp, border, fill)
                assert not np.isnan(got).any()
                for i in range(shape[0]):
                    assert same_bits(got[i], want[i]), (shape, interp, border, fill, i)
                got, want = device_apply(x3, fields, interp, border, fill, True), oracle(x3, fields, interp, border, fill, True)
                for i in range(shape[0]):
                    assert same_bits(got[i], want[i]), (shape, "vector", interp, border, fill, i)
                assert not same_bits(got, oracle(x3, fields, interp, border, fill, False))


def test_huge_nodes_are_served_with_every_index_clamped():
    """the fold guard is the parser's, not the op's: nodes of +-1e6 put every source outside -- constant gives `fill` everywhere,
    clamp gives border voxels -- and the result is still the statement's, bit for bit"""
    shape, spacing = (2, 3, 17, 33, 70), (8, 16, 32)
    g = M.grid_shape(shape[2:], spacing)
    signs = np.array([[1e6, -1e6, 1e6], [-1e6, -1e6, 1e6]])          # one sign per sample and component: |D| = 1e6 everywhere
    fields = [M.ElasticField(np.broadcast_to(signs[i][:, None, None, None], (3,) + g), spacing) for i in range(2)]
    x = data(shape, 4) + np.float32(2.0)
    for interp in ("linear", "nearest"):
        got = device_apply(x, fields, interp, "constant", 0.5)
        assert (got == 0.5).all() and same_bits(got, oracle(x, fields, interp, "constant", 0.5))
        got = device_apply(x, fields, interp, "clamp")
        assert same_bits(got, oracle(x, fields, interp, "clamp"))
        border = np.zeros(shape[2:], dtype=bool)
        border[[0, -1]] = border[:, [0, -1]] = border[:, :, [0, -1]] = True
        assert np.isin(got[0, 0], x[0, 0][border]).all()
    got = device_apply(x, fields, "nearest", "clamp", 0.0, True)
    assert same_bits(got, oracle(x, fields, "nearest", "clamp", 0.0, True))


def test_bad_arguments_are_refused_before_anything_is_launched():
    from mt3d_amd.engine import ops as E
    from mt3d_amd.engine.lib import RxError, load
    lib = load()
    shape, sp = (2, 3, 9, 10, 11), (8, 8, 8)
    x3 = torch.from_numpy(data(shape, 0)).cuda()
    x4 = torch.from_numpy(data((2, 4, 9, 10, 11), 1)).cuda()
    out3, out4 = torch.full_like(x3, -7.0), torch.full_like(x4, -7.0)
    fields = fields_for(shape, sp, 0)
    nodes, tables = E.elastic_nodes(fields), E.elastic_tables(shape[2:], sp)
    assert E.elastic_tables(shape[2:], sp) is tables                               # cached per (shape, spacing, device)
    before = x3.clone()
    with pytest.raises(RxError):                                                    # a CPU tensor
        E.elastic_apply(x3.cpu(), nodes, tables, sp, "linear", "constant", out=out3)
    with pytest.raises(RxError):                                                    # a wrong dtype
        E.elastic_apply(x3.double(), nodes, tables, sp, "linear", "constant", out=out3)
    with pytest.raises(RxError, match="rx_elastic_apply.*status -1"):               # in is out
        E.elastic_apply(x3, nodes, tables, sp, "linear", "constant", out=x3)
    with pytest.raises(RxError, match="rx_elastic_apply.*status -1"):               # vector with C = 4
        E.elastic_apply(x4, nodes, tables, sp, "nearest", "constant", vector=True, out=out4)
    with pytest.raises(RxError):                                                    # spacing 4
        E.elastic_apply(x3, torch.zeros((2, 3, 6, 6, 6), device="cuda"), E.elastic_tables(shape[2:], (4, 4, 4)), (4, 4, 4), "linear",
                        "constant", out=out3)
    with pytest.raises(RxError, match="nodes"):                                     # a nodes tensor of the wrong shape
        E.elastic_apply(x3, nodes[:, :, :4], tables, sp, "linear", "constant", out=out3)
    with pytest.raises(RxError, match="nodes"):
        E.elastic_apply(x3, nodes[:1], tables, sp, "linear", "constant", out=out3)
    with pytest.raises(RxError, match="tables"):
        E.elastic_apply(x3, nodes, E.elastic_tables((9, 10, 12), sp), sp, "linear", "constant", out=out3)
    with pytest.raises(RxError):
        E.elastic_apply(x3, nodes, tables, sp, "cubic", "constant", out=out3)
    for bad in (np.nan, np.inf):                                                    # nodes that are not finite never reach the device
        n = fields[1].nodes.copy()
        n[2, 1, 1, 1] = bad
        with pytest.raises(RxError, match="not finite"):
            E.elastic_nodes([fields[0], M.ElasticField(n, sp)])
    with pytest.raises(RxError, match="one lattice"):                               # mismatched spacings
        E.elastic_nodes([fields[0], M.ElasticField(fields[1].nodes, (8, 8, 9))])

    rec = E._l.RxElasticTables(*[t.data_ptr() for ax in tables for t in ax])
    null = E._l.RxElasticTables(*[0 if i == 4 else t.data_ptr() for i, t in enumerate(t for ax in tables for t in ax)])
    from ctypes import byref

    def raw(inp, outp, batch, c, z, y, xx, nd, spacing, tab, interp, border, vector):
        return lib.rx_elastic_apply(inp, outp, batch, c, z, y, xx, nd, None if spacing is None else E.I3(*spacing),
                                    None if tab is None else byref(tab), interp, border, 0.0, vector, E.stream_ptr())
    xp, op_, np_ = x3.data_ptr(), out3.data_ptr(), nodes.data_ptr()
    refused = {
        "null in": (None, op_, 2, 3, 9, 10, 11, np_, sp, rec, 0, 0, 0), "null out": (xp, None, 2, 3, 9, 10, 11, np_, sp, rec, 0, 0, 0),
        "null nodes": (xp, op_, 2, 3, 9, 10, 11, None, sp, rec, 0, 0, 0), "null spacing": (xp, op_, 2, 3, 9, 10, 11, np_, None, rec, 0, 0, 0),
        "null tables": (xp, op_, 2, 3, 9, 10, 11, np_, sp, None, 0, 0, 0), "null table pointer": (xp, op_, 2, 3, 9, 10, 11, np_, sp, null, 0, 0, 0),
        "in == out": (xp, xp, 2, 3, 9, 10, 11, np_, sp, rec, 0, 0, 0), "batch 0": (xp, op_, 0, 3, 9, 10, 11, np_, sp, rec, 0, 0, 0),
        "interp": (xp, op_, 2, 3, 9, 10, 11, np_, sp, rec, 2, 0, 0), "border": (xp, op_, 2, 3, 9, 10, 11, np_, sp, rec, 0, 2, 0),
        "vector with c = 4": (xp, op_, 2, 4, 9, 10, 11, np_, sp, rec, 1, 0, 1), "spacing 7": (xp, op_, 2, 3, 9, 10, 11, np_, (8, 7, 8), rec, 0, 0, 0),
        "extent beyond the index arithmetic": (xp, op_, 2, 3, 2048, 2048, 2048, np_, sp, rec, 0, 0, 0),
        "z beyond a grid dimension": (xp, op_, 2, 3, 70000, 8, 8, np_, sp, rec, 0, 0, 0),
        "too many channels": (xp, op_, 2, 5000, 9, 10, 11, np_, sp, rec, 0, 0, 0),
        "batch beyond a grid dimension": (xp, op_, 70000, 3, 9, 10, 11, np_, sp, rec, 0, 0, 0),
    }
    for name, args in refused.items():
        assert raw(*args) == -1, name
        assert b"rx_elastic_apply" in lib.rx_last_error(), name
    torch.cuda.synchronize()
    assert bool((out3 == -7.0).all()) and bool((out4 == -7.0).all()) and torch.equal(x3, before)          # nothing was launched
    got = E.elastic_apply(x3, nodes, tables, sp, "linear", "constant", out=out3)          # and the good call runs, into `out`
    torch.cuda.synchronize()
    assert got is out3 and same_bits(out3.cpu().numpy(), oracle(x3.cpu().numpy(), fields, "linear", "constant"))


def _host_batch(B, shape):
    sheet = (np.random.default_rng(0).random((B, *shape)) < 0.3).astype(np.float32)          # (B, Z, Y, X): viewed as one channel
    return {"image": data((B, 1, *shape), 1), "sheet": sheet, "normals": data((B, 3, *shape), 2) * sheet[:, None]}


def test_device_elastic():
    from mt3d_amd.engine.lib import RxError
    B, shape = 5, (12, 20, 70)
    host = _host_batch(B, shape)
    x = {k: torch.from_numpy(v).cuda() for k, v in host.items()}
    kw = dict(spacing=(8, 8, 16), magnitude=(0.5, 1.3), p=0.7)
    for border, fill in (("constant", 0.0), ("clamp", 0.0), ("constant", 0.25)):
        a = M.DeviceElastic(image_border=border, image_fill=fill, seed=5, **kw)
        b = M.DeviceElastic(image_border=border, image_fill=fill, seed=5, **kw)
        ya, yb = a(x), b(x)
        torch.cuda.synchronize()
        assert a.last_fields == b.last_fields and len(a.last_fields) == B
        assert 0 < sum(f.is_identity() for f in a.last_fields) < B          # p = 0.7: a mixed batch, zero fields go through the kernel
        assert all(torch.equal(ya[k], yb[k]) for k in x) and all(ya[k].shape == x[k].shape for k in x)
        for i, f in enumerate(a.last_fields):          # apply_item_numpy per sample: image, label and normals together
            want = M.apply_item_numpy(f, {k: v[i] for k, v in host.items()}, ("normals",), border, fill)
            for k in x:
                assert same_bits(ya[k][i].cpu().numpy(), want[k]), (border, fill, i, k)
        assert set(np.unique(ya["sheet"].cpu().numpy())) <= {0.0, 1.0}          # a label stays binary ...
        off = ya["sheet"].cpu().numpy() == 0
        assert (ya["normals"].cpu().numpy()[np.broadcast_to(off[:, None], (B, 3, *shape))] == 0).all()      # ... normals zero off it
    assert M.DeviceElastic(seed=5, rank=0, **dict(kw, p=1.0)).draw(shape) != M.DeviceElastic(seed=5, rank=1, **dict(kw, p=1.0)).draw(shape)
    still = M.DeviceElastic(seed=5, **dict(kw, p=0.0))
    y = still(x)
    assert y is x and all(f.is_identity() for f in still.last_fields)          # all zero: the same object back
    given = M.DeviceElastic(seed=1, **kw)
    fields = fields_for((B, 1, *shape), (8, 8, 16), 3)
    y = given(x, fields=fields)
    torch.cuda.synchronize()
    assert given.last_fields == fields and y["image"] is not x["image"]
    assert same_bits(y["image"].cpu().numpy(), oracle(host["image"], fields, "linear", "constant"))
    with pytest.raises(RxError, match="device tensor"):
        given({"image": x["image"].cpu()})
    with pytest.raises(RxError, match="expected"):
        given({"image": x["image"][0, 0]})
    with pytest.raises(RxError, match="normal_keys"):
        given({"image": x["image"], "normals": x["normals"][:, :2]})


def test_spatial_then_elastic_is_the_numpy_chain():
    B, shape = 3, (12, 20, 33)
    host = _host_batch(B, shape)
    x = {k: torch.from_numpy(v).cuda() for k, v in host.items()}
    spa = S.DeviceSpatial(rotation={"axes": ("z", "y", "x"), "max_degrees": 30.0, "p": 1.0}, scale={"range": (0.8, 1.25), "p": 1.0}, seed=3)
    ela = M.DeviceElastic(spacing=8, magnitude=(1.0, 1.3), p=1.0, seed=4)
    y = ela(spa(x))
    torch.cuda.synchronize()
    for i in range(B):
        mid = S.apply_item_numpy(spa.last_ops[i], {k: v[i] for k, v in host.items()})
        want = M.apply_item_numpy(ela.last_fields[i], mid)
        for k in x:
            assert same_bits(y[k][i].cpu().numpy(), want[k]), (i, k)


# ---- through the trainer -------------------------------------------------------------------------------------------------------
BLOCK = {"spacing": 8, "magnitude": [0.5, 1.3], "p": 0.8, "normal_keys": ["normals"], "image_border": "constant", "where": "device"}


def _trainer_run(tmp, variant):
    """one short epoch of BaseTrainer on synthetic patches with a sheet and a normals task; returns the bits of every loss.
    variant: "on" (the block), "nokey", "false" (elastic: false) or "never" (the block with p: 0)"""
    import yaml
    from mt3d_amd.train import BaseTrainer
    os.makedirs(tmp, exist_ok=True)
    cfg = yaml.safe_load(open(CFG))
    cfg["tr_setup"].update(model_name="elastic", ckpt_out_base=os.path.join(tmp, "ckpt"), tensorboard_log_dir=os.path.join(tmp, "tb"))
    cfg["tr_config"].update(max_epoch=1, max_steps_per_epoch=3, max_val_steps_per_epoch=1, patch_size=[16, 16, 16], compile=False)
    cfg["dataset_config"]["targets"]["normals"] = {"channels": 3, "activation": "none", "weight": 1, "loss_fn": "MaskedCosineLoss"}
    if variant == "on":
        cfg["dataset_config"]["elastic"] = BLOCK
    elif variant == "false":
        cfg["dataset_config"]["elastic"] = False
    elif variant == "never":
        cfg["dataset_config"]["elastic"] = dict(BLOCK, p=0.0)
    p = os.path.join(tmp, "cfg.yaml")
    yaml.safe_dump(cfg, open(p, "w"))
    os.chdir(tmp)
    losses, calls = [], []
    real_call = M.DeviceElastic.__call__

    def recording_call(self, batch, fields=None):
        out = real_call(self, batch, fields)
        calls.append((batch["image"].shape[0], sum(not f.is_identity() for f in self.last_fields), out["image"] is batch["image"]))
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
    M.DeviceElastic.__call__ = recording_call
    try:
        tr.train()
    finally:
        M.DeviceElastic.__call__ = real_call
    torch.cuda.synchronize()
    assert len(losses) == 2 * (3 + 1) and all(bool(torch.isfinite(l).all()) for l in losses)
    if variant in ("on", "never"):
        assert tr.device_elastic is not None and tr.device_elastic.last_fields is not None
        assert len(calls) >= 3 + 1          # every training batch (the feeder stages one ahead) and the validation batch
        if variant == "on":
            assert sum(c[1] for c in calls) > 0 and all(c[2] == (c[1] == 0) for c in calls)
        else:
            assert all(c[1] == 0 and c[2] for c in calls)
    else:
        assert tr.device_elastic is None and not calls
    return [int(np.float32(float(l)).view(np.uint32)) for l in losses]


def _child(tmp, variant, feeder=True):
    env = dict(os.environ, RX_DEVICE_FEEDER="1" if feeder else "0")
    code = (f"import sys; sys.path[:0] = [{ROOT!r}, {os.path.join(ROOT, 'tests')!r}]; import test_elastic_gpu as t; "
            f"print('RESULT', t._trainer_run({str(tmp)!r}, {variant!r}))")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    assert len(line) == 1, r.stdout[-2000:]
    return line[0]


@pytest.mark.parametrize("feeder", [True, False])
def test_one_trainer_epoch_with_the_block(tmp_path, feeder):
    """a fresh child process for the environment switch: behind the feeder and with RX_DEVICE_FEEDER=0 (and for validation either
    way) `trainer.device_elastic` draws for every batch, the draws are not all zero and the losses are finite"""
    assert _child(str(tmp_path / "on"), "on", feeder).count(",") == 7


def test_trainer_with_the_block_absent_or_never_drawing_is_the_run_without_the_key(tmp_path):
    """same seeds: `elastic: false`, and the block with p: 0 (every field zero, every batch handed back untouched), give the loss
    bits of a run without the key"""
    nokey = _child(str(tmp_path / "nokey"), "nokey")
    assert _child(str(tmp_path / "false"), "false") == nokey and nokey.count(",") == 7
    assert _child(str(tmp_path / "never"), "never") == nokey
