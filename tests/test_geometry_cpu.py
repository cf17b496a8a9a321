"""CPU: flips and 90-degree rotations with the normals component rule (dataloading/geometry_device.py, the host classes in
training/transforms/geometric/geometry.py) against tests/golden/geometry.npz -- recorded from the reference's own classes by
scripts/make_geometry_fixture.py -- and, where the reference tree is present, against those classes live.  Every comparison is on
the int32 view of the float32 arrays: bit for bit, the sign of zero included."""
import importlib.util
import itertools
import json
import os
import random
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import mt3d_amd  # noqa: F401
from mt3d_amd.dataloading import geometry_device as G
from mt3d_amd.dataloading import zarr_lite
from mt3d_amd.training.transforms.geometric.geometry import RandomFlipWithNormals, RandomRotate90WithNormals

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "geometry.npz")
REF = os.path.join(os.environ.get("RX_REFERENCE_ROOT", "/root/reference"), "training", "transforms", "geometric", "geometry.py")
KEYS = ("image", "sheet", "normals")


def bits(a):
    a = np.ascontiguousarray(a)
    assert a.dtype == np.float32
    return a.view(np.int32)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def load_cases():
    z = np.load(FIXTURE)
    cases = []
    for i in range(len(z["seeds"])):
        shape = tuple(int(v) for v in z["shapes"][i])
        tag = "x".join(map(str, shape))
        cases.append(SimpleNamespace(
            i=i, shape=shape, seed=int(z["seeds"][i]), chain=json.loads(str(z["chains"][i])), op=G.GeomOp.from_row(z["ops"][i]),
            inputs={k: z[f"in_{tag}_{k}"] for k in KEYS},
            outputs={k: z[f"c{i:03d}_{k}"].astype(np.float32) for k in KEYS}))
    return cases


def ours(chain, rng):
    cls = {"flip": RandomFlipWithNormals, "rot90": RandomRotate90WithNormals}
    return [cls[name](rng=rng, **{k: (tuple(v) if k == "axes" else v) for k, v in kw.items()}) for name, kw in chain]


def draw_chain(chain, rng):
    op = G.GeomOp.identity()
    for name, kw in chain:
        kw = {k: (tuple(v) if k == "axes" else v) for k, v in kw.items()}
        op = G.compose(op, G.draw_flip(rng, **kw) if name == "flip" else G.draw_rot90(rng, **kw))
    return op


def test_fixture_shape():
    cases = load_cases()
    assert len(cases) == 138 and os.path.getsize(FIXTURE) < 256 * 1024
    assert sum(c.shape == (4, 6, 6) for c in cases) == 6
    nrm = cases[0].inputs["normals"]
    assert 0.3 < (nrm == 0).mean() < 0.7 and not np.signbit(nrm[nrm == 0]).any()
    assert any((np.signbit(c.outputs["normals"]) & (c.outputs["normals"] == 0)).any() for c in cases)      # -0.0 is in play


def test_host_classes_and_composed_draws_reproduce_every_fixture_case():
    for c in load_cases():
        # the host classes, fed by a private generator in the state `random.seed(seed)` leaves the module in
        d = {k: v.copy() for k, v in c.inputs.items()}
        for t in ours(c.chain, random.Random(c.seed)):
            d = t(d)
        for k in KEYS:
            assert same_bits(d[k], c.outputs[k]), (c.i, k, "host classes")
        # one composed op: the draws alone, then the statement of the kernel
        op = draw_chain(c.chain, random.Random(c.seed))
        assert op == c.op, (c.i, op, c.op)
        assert c.op.preserves(c.shape)
        for k in KEYS:
            assert same_bits(G.apply_op_numpy(c.op, c.inputs[k], k == "normals"), c.outputs[k]), (c.i, k, "apply_op_numpy")


@pytest.mark.skipif(not os.path.exists(REF), reason="the reference tree is not on this machine")
def test_live_reference_same_arrays_and_same_generator_consumption():
    spec = importlib.util.spec_from_file_location("ref_geometry_live", REF)
    ref = importlib.util.module_from_spec(spec)
    import sys
    old = sys.dont_write_bytecode
    sys.dont_write_bytecode = True
    try:
        spec.loader.exec_module(ref)
    finally:
        sys.dont_write_bytecode = old
    data_rng = np.random.default_rng(5)
    shape = (6, 6, 6)
    data = {"image": data_rng.random(shape, dtype=np.float32), "sheet": data_rng.random((1, *shape), dtype=np.float32),
            "normals": (data_rng.standard_normal((3, *shape)).astype(np.float32)
                        * (data_rng.random(shape) < 0.5).astype(np.float32)[None])}
    data["normals"][data["normals"] == 0] = 0.0
    moved = 0
    for seed in range(200):
        kw_f = {"p": 0.5, "p_transform": (1.0, 0.7)[seed % 2]}
        kw_r = {"axes": (("x", "y", "z"), ("z",), ("y", "x"))[seed % 3], "p": 0.6, "p_transform": (1.0, 0.8)[seed % 2]}
        random.seed(seed)
        want = {k: v.copy() for k, v in data.items()}
        for t in (ref.RandomFlipWithNormals(**kw_f), ref.RandomRotate90WithNormals(**kw_r)):
            want = t(want)
        state = random.getstate()
        rng = random.Random(seed)
        got = {k: v.copy() for k, v in data.items()}
        for t in (RandomFlipWithNormals(rng=rng, **kw_f), RandomRotate90WithNormals(rng=rng, **kw_r)):
            got = t(got)
        assert rng.getstate() == state, seed          # the same number of generator calls
        for k in KEYS:
            assert same_bits(np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])), (seed, k)
        moved += not same_bits(got["image"], data["image"])
    assert moved > 100


def test_default_generator_is_the_random_module():
    random.seed(3)
    a = RandomFlipWithNormals()({"image": np.arange(27, dtype=np.float32).reshape(3, 3, 3)})
    b = RandomFlipWithNormals(rng=random.Random(3))({"image": np.arange(27, dtype=np.float32).reshape(3, 3, 3)})
    assert same_bits(a["image"], b["image"])


def all_axis_ops():
    return [G.GeomOp(src, flip) for src in itertools.permutations(range(3)) for flip in itertools.product((0, 1), repeat=3)]


def test_group_sanity():
    cases = load_cases()
    assert len({(c.op.src_axis, c.op.flip) for c in cases[:80]}) == 32          # one flip + one rotation
    assert len({(c.op.src_axis, c.op.flip) for c in cases}) == 48               # every signed axis permutation
    assert len(set(all_axis_ops())) == 48
    ops = sorted({c.op for c in cases}, key=lambda o: o.row())
    rng = random.Random(0)
    ident = G.GeomOp.identity()
    for _ in range(300):
        a, b, c = (rng.choice(ops) for _ in range(3))
        assert G.compose(G.compose(a, b), c) == G.compose(a, G.compose(b, c))
    data = np.random.default_rng(1)
    vol = data.standard_normal((3, 5, 5, 5)).astype(np.float32) * (data.random((5, 5, 5)) < 0.5).astype(np.float32)[None]
    for op in ops:
        inv = op.inverse()
        assert G.compose(op, inv) == ident and G.compose(inv, op) == ident
        for is_normal in (False, True):
            there = G.apply_op_numpy(op, vol, is_normal)
            assert same_bits(G.apply_op_numpy(inv, there, is_normal), vol)
            # compose is "a then b"
            other = ops[(ops.index(op) * 7 + 3) % len(ops)]
            assert same_bits(G.apply_op_numpy(other, there, is_normal), G.apply_op_numpy(G.compose(op, other), vol, is_normal))
    # `preserves` against the shape numpy returns
    for shape in [(4, 6, 6), (6, 4, 6), (6, 6, 4), (3, 4, 5), (5, 5, 5)]:
        x = np.zeros(shape, np.float32)
        for op in all_axis_ops():
            assert op.preserves(shape) == (G.apply_op_numpy(op, x).shape == shape), (shape, op)
    # the op of a rotation is numpy's rot90
    idx = np.arange(4 * 5 * 6, dtype=np.float32).reshape(4, 5, 6)
    for axis, k in itertools.product("xyz", (1, 2, 3)):
        assert np.array_equal(G.apply_op_numpy(G.rot90_op(axis, k), idx), np.rot90(idx, k, axes=G.PLANE[axis]))
    assert G.allowed_rot90_axes((4, 6, 6)) == ("z",) and G.allowed_rot90_axes((6, 6, 6)) == ("x", "y", "z")
    assert G.allowed_rot90_axes((4, 5, 6)) == ()


# ---- configuration ---------------------------------------------------------------------------------------------------------------
TASKS = {"sheet": {"channels": 1}, "normals": {"channels": 3}}


def test_config_rejections_name_the_offending_key():
    def parse(g, patch=(8, 8, 8), tasks=TASKS):
        return G.parse_geometric({"geometric": g}, patch, tasks)
    assert G.parse_geometric({}, (8, 8, 8), TASKS) is None and parse(False) is None and parse(None) is None
    ok = parse({"flip": {"p": 0.5}, "rot90": {"axes": ["x", "z"], "p": 0.25}, "normal_keys": ["normals"], "where": "device"})
    assert ok == {"flip": {"p": 0.5}, "rot90": {"axes": ("x", "z"), "p": 0.25}, "normal_keys": ("normals",), "where": "device"}
    assert parse({"flip": {}})["rot90"] is None and parse({"rot90": {}})["rot90"]["axes"] == ("x", "y", "z")
    assert parse({"rot90": {"axes": ["z"]}}, patch=(4, 8, 8))["rot90"]["axes"] == ("z",)
    with pytest.raises(ValueError, match=r"rot90\.axes.*\['x', 'y'\].*allows: \['z'\]"):
        parse({"rot90": {"axes": ["x", "y", "z"]}}, patch=(4, 8, 8))
    with pytest.raises(ValueError, match=r"rot90\.axes"):
        parse({"rot90": {"axes": ["w"]}})
    with pytest.raises(ValueError, match="3-D patch"):
        parse({"flip": {}}, patch=(8, 8))
    with pytest.raises(ValueError, match=r"normal_keys.*'normals'.*channels = 2"):
        parse({"flip": {}}, tasks={"normals": {"channels": 2}})
    with pytest.raises(ValueError, match=r"geometric: unknown key\(s\) \['rotate'\]"):
        parse({"rotate": {}})
    with pytest.raises(ValueError, match=r"geometric\.flip: unknown key\(s\) \['axes'\]"):
        parse({"flip": {"axes": ["x"]}})
    with pytest.raises(ValueError, match=r"geometric\.rot90: unknown key\(s\) \['k'\]"):
        parse({"rot90": {"k": 2}})
    with pytest.raises(ValueError, match=r"geometric\.where"):
        parse({"flip": {}, "where": "gpu"})
    with pytest.raises(ValueError, match=r"geometric\.flip\.p:"):
        parse({"flip": {"p": 1.5}})


def _index_volume(tmp_path, D=24):
    """image and sheet hold the SAME index volume (as uint16 codes), normals three distinguishable components"""
    idx = (np.arange(D ** 3, dtype=np.int64) % 60000 + 1).astype(np.uint16).reshape(D, D, D)
    nrm = np.stack([idx // 3, idx // 3 + 20000, idx // 3 + 40000], axis=-1).astype(np.uint16)
    paths = {}
    for name, arr, ch in [("img", idx, (16, 16, 16)), ("sheet", idx, (16, 16, 16)), ("normals", nrm, (16, 16, 16, 3))]:
        paths[name] = str(tmp_path / f"{name}.zarr")
        zarr_lite.write_array(paths[name], arr, ch, compressor="zlib")
    return paths


def _mgr(tmp_path, paths, dataset_config):
    return SimpleNamespace(model_name="g", tasks=TASKS, train_patch_size=(12, 12, 12), min_labeled_ratio=0.1, min_bbox_percent=0.5,
                           dilate_label=False, use_cache=False, cache_folder=str(tmp_path / "cache"), dataset_config=dataset_config,
                           volume_paths=[{"input": paths["img"], "sheet": paths["sheet"], "normals": paths["normals"],
                                          "ref_label": "sheet"}])


def test_zarr_dataset_host_geometry_moves_image_and_targets_together(tmp_path):
    from mt3d_amd.dataloading.dataset import SyntheticPatchDataset, ZarrSegmentationDataset3D
    paths = _index_volume(tmp_path)
    plain = ZarrSegmentationDataset3D(_mgr(tmp_path, paths, {"augment": False}))
    assert plain.geometric is None and plain._host_geometry == [] and len(plain) > 0
    geo_cfg = {"flip": {"p": 0.5}, "rot90": {"p": 0.7}, "normal_keys": ["normals"], "where": "host"}
    host = ZarrSegmentationDataset3D(_mgr(tmp_path, paths, {"augment": False, "geometric": geo_cfg}))
    dev = ZarrSegmentationDataset3D(_mgr(tmp_path, paths, {"augment": False, "geometric": dict(geo_cfg, where="device")}))
    assert host.geometric["where"] == "host" and len(host._host_geometry) == 2
    assert dev.geometric["where"] == "device" and dev._host_geometry == []
    moved = 0
    random.seed(7)
    for n in range(24):
        i = n % len(plain)
        raw, got, untouched = plain[i], host[i], dev[i]
        for k in raw:          # key absent / where: device -> the items of the parent, bit for bit
            assert torch.equal(raw[k], untouched[k]) and raw[k].dtype == untouched[k].dtype
        ops = [t.last_op for t in host._host_geometry]
        op = G.compose(ops[0], ops[1])
        assert got["image"].shape == raw["image"].shape and got["image"].is_contiguous()
        for k in ("image", "sheet", "normals"):
            assert same_bits(got[k].numpy(), G.apply_op_numpy(op, raw[k].numpy(), k == "normals")), (n, k)
        assert torch.equal(got["image"], got["sheet"]) and torch.equal(raw["image"], raw["sheet"])
        moved += not op.is_identity()          # (image and sheet hold the same index volume: they moved to the same place)
    assert moved > 8
    with pytest.raises(ValueError, match=r"rot90\.axes"):
        m = _mgr(tmp_path, paths, {"augment": False, "geometric": {"rot90": {}}})
        m.train_patch_size = (8, 12, 12)
        ZarrSegmentationDataset3D(m)
    with pytest.raises(ValueError, match=r"normal_keys"):
        ZarrSegmentationDataset3D(_mgr(tmp_path, paths, {"augment": False, "geometric": {"flip": {}, "normal_keys": ["sheet", "normals"]}}))
    smgr = SimpleNamespace(train_patch_size=(8, 8, 8), in_channels=1, tasks=TASKS, dataset_config={"geometric": {"flip": {}}})
    assert SyntheticPatchDataset(smgr).geometric["where"] == "device"
    smgr.dataset_config = {"geometric": {"flip": {}, "where": "host"}}
    with pytest.raises(ValueError, match=r"geometric\.where"):
        SyntheticPatchDataset(smgr)
    smgr.dataset_config = {}
    assert SyntheticPatchDataset(smgr).geometric is None


def test_device_geometry_draws_without_a_device():
    """the draws are host state: seeded -> repeatable, ranks differ; CPU tensors are refused"""
    from mt3d_amd.engine.lib import RxError
    kw = dict(flip={"p": 0.5}, rot90={"p": 0.5}, seed=9)
    a, b, c = G.DeviceGeometry(**kw), G.DeviceGeometry(**kw), G.DeviceGeometry(rank=1, **kw)
    da, db, dc = ([g.draw() for _ in range(40)] for g in (a, b, c))
    assert da == db and da != dc and len(set(da)) > 10
    with pytest.raises(RxError, match="device tensor"):
        a({"image": torch.zeros(1, 1, 4, 4, 4)})
    with pytest.raises(ValueError, match=r"DeviceGeometry\.rot90: unknown key"):
        G.DeviceGeometry(rot90={"k": 1})
    from mt3d_amd.engine import ops
    with pytest.raises(RxError, match="device tensor"):
        ops.geom_apply(torch.zeros(1, 1, 4, 4, 4), [G.GeomOp.identity()], False)


def test_record_check_and_lowering_host_program(tmp_path):
    """csrc/rx_geom_core.h is what rx_geom_apply, rx_sw_gather_geom and rx_sw_accumulate_geom check and lower a record with.  A
    stand-alone C++ program (csrc/tools/geom_core_check.cpp) runs it over all 48 (src_axis, flip) records and three shapes against the
    definition in include/rxunet.h, voxel by voxel, and over the malformed kinds, compiled with -fsanitize=address,undefined."""
    import subprocess
    csrc = os.path.join(ROOT, "multi-task-3d-resencoder-unet_amd", "csrc")
    exe = str(tmp_path / "geom_core_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(csrc, "tools", "geom_core_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and not r.stderr, r.stdout[-1000:] + r.stderr[-3000:]
    shapes = [(4, 4, 4), (3, 5, 5), (3, 4, 5)]
    keep = [sum(op.preserves(s) for op in all_axis_ops()) for s in shapes]
    assert keep == [48, 16, 8] and r.stdout.strip() == "accepted 48 16 8 of 48, 0 expectations failed"


def test_rx_geom_apply_is_declared_and_exported():
    import ctypes
    import __graft_entry__
    __graft_entry__.build()
    from mt3d_amd.engine import lib
    hdr = open(os.path.join(ROOT, "include", "rxunet.h")).read()
    assert re.search(r"\bint\s+rx_geom_apply\s*\(", hdr) and "rx_geom_sample;" in hdr
    assert hasattr(ctypes.CDLL(lib.LIB_PATH), "rx_geom_apply") and "rx_geom_apply" in lib.exported_symbols()
    assert lib.load().rx_abi_version() == 1
    # host-side validation needs no device: a null table is refused with the entry point named
    assert lib.load().rx_geom_apply(None, None, 1, 1, 4, 4, 4, None, 0, None) == -1
    assert b"rx_geom_apply" in lib.load().rx_last_error()
