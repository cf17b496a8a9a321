"""GPU: rx_geom_apply (csrc/rx_geometry.hip) and DeviceGeometry against `apply_op_numpy`, the numpy statement that
tests/test_geometry_cpu.py pins to the reference's own classes.  Every comparison is bit for bit (int32 views: -0.0 counts)."""
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import mt3d_amd  # noqa: F401
from mt3d_amd.dataloading import geometry_device as G

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "tasks", "synthetic_sheet.yaml")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_geometry_cpu import KEYS, load_cases, same_bits  # noqa: E402


def field(shape, seed):
    """float32 with about half the voxels exactly +0.0 (what a masked normals target looks like)"""
    rng = np.random.default_rng(seed)
    a = rng.standard_normal(shape).astype(np.float32) * (rng.random(shape[-3:]) < 0.5).astype(np.float32)
    a[a == 0] = 0.0
    return a


def device_apply(x, ops, vector):
    from mt3d_amd.engine import ops as E
    out = E.geom_apply(torch.from_numpy(x).cuda(), ops, vector)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def oracle(x, ops, vector):
    return np.stack([G.apply_op_numpy(op, x[i], vector) for i, op in enumerate(ops)])


def component_rules():
    """the component rule of each fixture chain, keyed by its signed axis permutation (several chains may share one: keep all)"""
    rules = {}
    for c in load_cases():
        rules.setdefault((c.op.src_axis, c.op.flip), set()).add((c.op.ch_src, c.op.ch_neg))
    return rules


def all_ops():
    rules = component_rules()
    assert len(rules) == 48
    ops = []
    for src in itertools.permutations(range(3)):
        for flip in itertools.product((0, 1), repeat=3):
            for ch, neg in sorted(rules[(src, flip)]):
                ops.append(G.GeomOp(src, flip, ch, neg))
    assert len({(o.src_axis, o.flip) for o in ops}) == 48
    return ops


@pytest.mark.parametrize("shape", [(10, 10, 10), (32, 32, 32), (6, 12, 12), (12, 12, 6)])
def test_every_signed_axis_permutation(shape):
    ops = [op for op in all_ops() if op.preserves(shape)]
    assert len({(o.src_axis, o.flip) for o in ops}) == (48 if shape[0] == shape[1] == shape[2] else 16)
    for channels, vector in ((1, False), (3, True), (3, False)):
        x = field((len(ops), channels, *shape), 3 + channels)
        got = device_apply(x, ops, vector)
        want = oracle(x, ops, vector)
        for i, op in enumerate(ops):
            assert same_bits(got[i], want[i]), (shape, channels, vector, op)
    if shape == (32, 32, 32):
        v = device_apply(field((len(ops), 3, *shape), 9), ops, True)
        assert (np.signbit(v) & (v == 0)).any()          # a negated zero is -0.0


def test_a_batch_of_different_ops_and_a_batch_larger_than_one_launch():
    ops = all_ops()
    rows = [o for o in ops if o.src_axis[2] == 2 and not o.is_identity()]
    tiles = [o for o in ops if o.src_axis[2] != 2]
    five = [G.GeomOp.identity(), rows[1], tiles[0], rows[-1], tiles[-1]]
    assert len(set(five)) == 5
    for shape in [(12, 12, 12), (20, 20, 20)]:
        for channels, vector in ((3, True), (2, False)):
            x = field((5, channels, *shape), 1)
            assert same_bits(device_apply(x, five, vector), oracle(x, five, vector))
    many = [ops[(7 * i) % len(ops)] for i in range(37)]          # 16 samples ride in one launch: 37 = 16 + 16 + 5
    x = field((37, 3, 8, 8, 8), 2)
    got = device_apply(x, many, True)
    want = oracle(x, many, True)
    for i in range(37):
        assert same_bits(got[i], want[i]), (i, many[i])


def test_buffers_off_the_16_byte_grid_take_the_scalar_path():
    """x % 4 == 0 but `in` and / or `out` 4 bytes off a 16-byte boundary (a view into a larger buffer, through the raw ABI):
    the 16-byte loads and stores must not be used"""
    from mt3d_amd.engine import ops as E
    from mt3d_amd.engine.lib import load
    ops = all_ops()
    rows = [o for o in ops if o.src_axis[2] == 2]
    tiles = [o for o in ops if o.src_axis[2] != 2]
    pick = [rows[0], rows[3], rows[-1], tiles[2], G.compose(G.flip_op(2), G.flip_op(0))]
    shape = (len(pick), 3, 8, 8, 8)
    x = field(shape, 6)
    n = x.size
    table = E.geom_table(pick)
    want = oracle(x, pick, True)
    for off_in, off_out in ((1, 0), (0, 1), (1, 1), (2, 3)):
        src = torch.zeros(n + 4, dtype=torch.float32, device="cuda")
        dst = torch.full((n + 4,), -7.0, dtype=torch.float32, device="cuda")
        src[off_in:off_in + n] = torch.from_numpy(x).cuda().reshape(-1)
        assert src.data_ptr() % 16 == 0 and dst.data_ptr() % 16 == 0
        rc = load().rx_geom_apply(src.data_ptr() + 4 * off_in, dst.data_ptr() + 4 * off_out, *shape, table.ctypes.data, 1, E.stream_ptr())
        torch.cuda.synchronize()
        assert rc == 0
        got = dst.cpu().numpy()
        assert same_bits(got[off_out:off_out + n].reshape(shape), want), (off_in, off_out)
        assert (got[:off_out] == -7.0).all() and (got[off_out + n:] == -7.0).all()          # nothing outside the tensor


def test_full_size_vector_batch():
    a = G.compose(G.compose(G.flip_op(0), G.flip_op(2)), G.rot90_op("y", 1))      # x moves
    b = G.compose(G.flip_op(1), G.compose(G.rot90_op("x", 3), G.flip_op(2)))       # x stays innermost, flipped
    assert a.src_axis[2] != 2 and b.src_axis[2] == 2
    x = field((2, 3, 128, 128, 128), 4)
    got = device_apply(x, [a, b], True)
    for i, op in enumerate((a, b)):
        assert same_bits(got[i], G.apply_op_numpy(op, x[i], True)), op


def test_fixture_cases_through_device_geometry():
    geo = G.DeviceGeometry(flip={"p": 0.5}, rot90={"p": 0.5}, seed=1)
    cases = load_cases()
    for shape in ((6, 6, 6), (4, 6, 6)):
        group = [c for c in cases if c.shape == shape]
        batch = {"image": np.stack([c.inputs["image"] for c in group]),            # (B, Z, Y, X): viewed as one channel
                 "sheet": np.stack([c.inputs["sheet"] for c in group]), "normals": np.stack([c.inputs["normals"] for c in group])}
        out = geo({k: torch.from_numpy(v).cuda() for k, v in batch.items()}, ops=[c.op for c in group])
        torch.cuda.synchronize()
        assert geo.last_ops == [c.op for c in group]
        for k in KEYS:
            got = out[k].cpu().numpy()
            assert got.shape == batch[k].shape
            for i, c in enumerate(group):
                assert same_bits(got[i], c.outputs[k]), (c.i, k)
    # drawn ops: repeatable, and an all-identity batch is handed back as it came
    x = {"image": torch.from_numpy(field((4, 1, 8, 8, 8), 0)).cuda(), "normals": torch.from_numpy(field((4, 3, 8, 8, 8), 1)).cuda()}
    a = G.DeviceGeometry(flip={"p": 0.5}, rot90={"p": 0.5}, seed=5)
    b = G.DeviceGeometry(flip={"p": 0.5}, rot90={"p": 0.5}, seed=5)
    ya, yb = a(x), b(x)
    assert a.last_ops == b.last_ops and all(torch.equal(ya[k], yb[k]) for k in x)
    for k in x:
        assert same_bits(ya[k].cpu().numpy(), oracle(x[k].cpu().numpy(), a.last_ops, k == "normals"))
    still = G.DeviceGeometry(flip={"p": 0.0}, seed=5)(x)
    assert all(still[k] is x[k] for k in x)
    with pytest.raises(ValueError, match="would change the shape"):
        flat = {"image": torch.zeros(1, 1, 4, 8, 8, device="cuda")}
        G.DeviceGeometry(seed=1)(flat, ops=[G.rot90_op("x", 1)])


def test_bad_arguments_are_refused_before_anything_is_launched():
    from mt3d_amd.engine import ops as E
    from mt3d_amd.engine.lib import RxError, load
    lib = load()
    sp = E.stream_ptr()
    x = torch.from_numpy(field((2, 3, 4, 8, 8), 0)).cuda()
    out = torch.full_like(x, -7.0)
    good = E.geom_table([G.GeomOp.identity(), G.rot90_op("z", 1)])

    def call(inp, outp, batch, c, z, y, xx, table, vector):
        return lib.rx_geom_apply(inp, outp, batch, c, z, y, xx, None if table is None else table.ctypes.data, vector, sp)

    def bad_row(**kw):
        t = good.copy()
        for k, v in kw.items():
            lo = {"src_axis": 0, "flip": 3, "ch_src": 6, "ch_neg": 9}[k]
            t[1, lo:lo + 3] = v
        return t
    xp, op_ = x.data_ptr(), out.data_ptr()
    refused = {
        "null in": (None, op_, 2, 3, 4, 8, 8, good, 1),
        "null out": (xp, None, 2, 3, 4, 8, 8, good, 1),
        "null table": (xp, op_, 2, 3, 4, 8, 8, None, 1),
        "in place": (xp, xp, 2, 3, 4, 8, 8, good, 1),
        "batch 0": (xp, op_, 0, 3, 4, 8, 8, good, 1),
        "src_axis repeats": (xp, op_, 2, 3, 4, 8, 8, bad_row(src_axis=(0, 2, 2)), 1),
        "src_axis out of range": (xp, op_, 2, 3, 4, 8, 8, bad_row(src_axis=(0, 1, 3)), 1),
        "changes the shape": (xp, op_, 2, 3, 4, 8, 8, bad_row(src_axis=(1, 0, 2)), 1),
        "ch_src repeats": (xp, op_, 2, 3, 4, 8, 8, bad_row(ch_src=(1, 1, 2)), 1),
        "ch_src negative": (xp, op_, 2, 3, 4, 8, 8, bad_row(ch_src=(-1, 1, 2)), 1),
        "vector with c != 3": (xp, op_, 3, 2, 4, 8, 8, np.concatenate([good, good[:1]]), 1),
        "extent beyond the index arithmetic": (xp, op_, 2, 3, 2048, 2048, 2048, good, 1),
        "z beyond a grid dimension": (xp, op_, 2, 3, 70000, 8, 8, good, 0),
        "too many channels": (xp, op_, 2, 5000, 4, 8, 8, good, 0),
    }
    for name, args in refused.items():
        assert call(*args) == -1, name
        assert b"rx_geom_apply" in lib.rx_last_error(), name
    with pytest.raises(RxError, match="rx_geom_apply.*status -1"):
        E.geom_apply(x, bad_row(src_axis=(1, 0, 2)), True)
    with pytest.raises(RxError):
        E.geom_apply(x.cpu(), good, True)
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())          # nothing was launched
    assert call(xp, op_, 2, 3, 4, 8, 8, good, 1) == 0          # and the good table runs
    torch.cuda.synchronize()
    assert same_bits(out.cpu().numpy(), oracle(x.cpu().numpy(), [G.GeomOp.identity(), G.rot90_op("z", 1)], True))


# ---- through the trainer -------------------------------------------------------------------------------------------------------
def _trainer_run(tmp, geometric=True):
    """two epochs of BaseTrainer on a small zarr_lite volume with a sheet and a normals task; returns the ops drawn for the
    training batches and checks that every batch the model and the losses saw is `apply_op_numpy(op, raw item)`"""
    import yaml
    from mt3d_amd.dataloading import zarr_lite
    from mt3d_amd.dataloading.dataset import ZarrSegmentationDataset3D
    from mt3d_amd.train import BaseTrainer, DeviceFeeder
    rng = np.random.default_rng(0)
    Dm = 64
    z, y, x = np.meshgrid(np.arange(Dm), np.arange(Dm), np.arange(Dm), indexing="ij")
    sheet = (np.abs(((y + 6 * np.sin(x / 9.0) + 4 * np.cos(z / 7.0)) % 16) - 8) < 2.5)
    img = (sheet * 140 + rng.integers(0, 80, size=sheet.shape)).astype(np.uint8)
    nrm = (rng.integers(1, 65535, size=(Dm, Dm, Dm, 3)) * sheet[..., None]).astype(np.uint16)
    os.makedirs(tmp, exist_ok=True)
    zarr_lite.write_array(os.path.join(tmp, "img.zarr"), img, (32, 32, 32), compressor="zlib")
    zarr_lite.write_array(os.path.join(tmp, "sheet.zarr"), (sheet * 255).astype(np.uint8), (32, 32, 32), compressor="zlib")
    zarr_lite.write_array(os.path.join(tmp, "normals.zarr"), nrm, (32, 32, 32, 3), compressor="zlib")
    cfg = yaml.safe_load(open(CFG))
    cfg["tr_setup"].update(model_name="zarr_geom", ckpt_out_base=os.path.join(tmp, "ckpt"), tensorboard_log_dir=os.path.join(tmp, "tb"))
    cfg["tr_config"].update(max_epoch=2, max_steps_per_epoch=6, max_val_steps_per_epoch=2, patch_size=[32, 32, 32], compile=False)
    cfg["dataset_config"]["targets"]["normals"] = {"channels": 3, "activation": "none", "weight": 1, "loss_fn": "MaskedCosineLoss"}
    cfg["dataset_config"].update(synthetic=False, min_labeled_ratio=0.05, min_bbox_percent=0.5, use_cache=False,
                                 cache_folder=os.path.join(tmp, "cache"), augment=False,
                                 volume_paths=[{"input": os.path.join(tmp, "img.zarr"), "sheet": os.path.join(tmp, "sheet.zarr"),
                                                "normals": os.path.join(tmp, "normals.zarr"), "ref_label": "sheet"}])
    if geometric:
        cfg["dataset_config"]["geometric"] = {"flip": {"p": 0.5, "p_transform": 1.0}, "rot90": {"axes": ["x", "y", "z"], "p": 0.5},
                                              "normal_keys": ["normals"], "where": "device"}
    p = os.path.join(tmp, "cfg.yaml")
    yaml.safe_dump(cfg, open(p, "w"))
    os.chdir(tmp)
    seen, targets, drawn = [], {"sheet": [], "normals": []}, []

    real_call = G.DeviceGeometry.__call__

    def recording_call(self, batch, ops=None):
        out = real_call(self, batch, ops)
        drawn.append(list(self.last_ops))
        return out

    class Rec(BaseTrainer):
        def _build_model(self):
            model = super()._build_model()
            model.register_forward_pre_hook(lambda m, args: seen.append(args[0].detach().float().cpu().clone()))
            return model

        def _build_loss(self):
            fns = super()._build_loss()

            def wrap(name, fn):
                def f(pred, gt):
                    targets[name].append(gt.detach().cpu().clone())
                    return fn(pred, gt)
                return f
            return {k: wrap(k, v) for k, v in fns.items()}

    torch.manual_seed(1234)
    np.random.seed(1234)
    tr = Rec(p, verbose=False)
    ds = tr._configure_dataset()
    assert isinstance(ds, ZarrSegmentationDataset3D) and (ds.geometric is not None) == geometric
    raw = [ds[i] for i in range(len(ds))]
    G.DeviceGeometry.__call__ = recording_call
    try:
        tr.train()
    finally:
        G.DeviceGeometry.__call__ = real_call
    torch.cuda.synchronize()
    steps = len(seen)
    assert steps == 2 * (6 + 2) and len(targets["sheet"]) == steps and len(targets["normals"]) == steps
    if not geometric:
        assert tr.device_geometry is None and not drawn
        for b in range(steps):          # the parent's batches: raw items, bit for bit
            for i in range(seen[b].shape[0]):
                assert any(torch.equal(seen[b][i], r["image"]) and torch.equal(targets["sheet"][b][i], r["sheet"])
                           and same_bits(targets["normals"][b][i].numpy(), r["normals"].numpy()) for r in raw)
        return []
    feeder = os.environ.get("RX_DEVICE_FEEDER", "1") != "0"
    # with the feeder one batch is staged (and drawn for) ahead of the step that consumes it; batches cut off by
    # max_steps_per_epoch are drawn for and never seen.  Match every seen batch to a draw by its content instead of its position.
    assert len(drawn) >= steps
    flat_ops = [op for ops in drawn for op in ops]
    assert len({op for op in flat_ops}) > 4 and any(op.src_axis[2] != 2 for op in flat_ops)
    matched = mixed = 0
    for b in range(steps):
        hit = False
        for ops in drawn:
            if len(ops) != seen[b].shape[0]:
                continue
            ok = True
            for i, op in enumerate(ops):
                ok = ok and any(same_bits(seen[b][i].numpy(), G.apply_op_numpy(op, r["image"].numpy()))
                                and same_bits(targets["sheet"][b][i].numpy(), G.apply_op_numpy(op, r["sheet"].numpy()))
                                and same_bits(targets["normals"][b][i].numpy(), G.apply_op_numpy(op, r["normals"].numpy(), True))
                                for r in raw)
            if ok:
                hit = True
                mixed += len(set(ops)) > 1          # two samples of one batch under different ops: the sample-to-record pairing
                break
        assert hit, f"batch {b}: no drawn op set explains (image, sheet, normals) of every item"
        matched += 1
    assert mixed > 0, "no batch carried two different ops"
    print(f"trainer (feeder={feeder}): {matched} batches, {mixed} with different ops per sample, explained by {len(drawn)} draws, {len(set(flat_ops))} distinct ops")
    return [op.row() for op in flat_ops]


def _child(tmp, geometric, feeder):
    env = dict(os.environ, RX_DEVICE_FEEDER="1" if feeder else "0")
    code = (f"import sys; sys.path[:0] = [{ROOT!r}, {os.path.join(ROOT, 'tests')!r}]; import test_geometry_gpu as t; "
            f"print('RESULT', t._trainer_run({str(tmp)!r}, {geometric!r}))")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("RESULT")]
    assert line
    return line[-1]


def test_trainer_behind_the_feeder_same_seed_same_ops(tmp_path):
    """fresh child processes (a process that has trained keeps its device and generator state): two runs with the same seed draw
    the same ops, and every batch is the op of its sample applied to the raw items"""
    a = _child(tmp_path / "a", True, True)
    b = _child(tmp_path / "b", True, True)
    assert a == b and len(a) > 100


def test_trainer_without_the_feeder(tmp_path):
    _child(tmp_path / "a", True, False)


def test_trainer_with_the_key_absent_feeds_the_raw_items(tmp_path):
    assert _child(tmp_path / "a", False, True) == "RESULT []"
