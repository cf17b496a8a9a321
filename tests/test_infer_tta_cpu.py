"""Test-time augmentation of streaming inference, CPU side: the view enumeration (`tta_views`), a numpy statement of the semantics
driven by toy "networks" (an exactly equivariant one and one that is not), the schedule with views, the config keys and the
refusals `StreamingInferer` makes at construction."""
import itertools

import numpy as np
import pytest

import mt3d_amd  # noqa: F401
from mt3d_amd import inference as inf
from mt3d_amd.dataloading.geometry_device import GeomOp, allowed_rot90_axes, apply_op_numpy, compose, flip_op, rot90_op

TASKS = {"sheet": {"channels": 1, "activation": "sigmoid"}, "normals": {"channels": 3, "activation": "none"}}
COUNTS = [("zyx", "", 8), ("zyx", "z", 16), ("zyx", "zyx", 48), ("yx", "z", 8), ("", "z", 4), ("", "zyx", 24)]


def _spec(flips, rots):
    s = {}
    if flips:
        s["flip"] = list(flips)
    if rots:
        s["rot90"] = list(rots)
    return s


# ---- tta_views ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flips,rots,n", COUNTS)
def test_view_counts_identity_first_no_duplicates(flips, rots, n):
    views = inf.tta_views(_spec(flips, rots), (16, 16, 16), TASKS)
    assert isinstance(views, tuple) and len(views) == n
    assert views[0] == GeomOp() and len(set(views)) == n
    for op in views:
        assert isinstance(op, GeomOp) and op.preserves((16, 16, 16))
        assert compose(op, op.inverse()) == GeomOp() and compose(op.inverse(), op) == GeomOp()


def test_view_order_is_flip_major_binary_counting_then_rotation_chains():
    views = inf.tta_views({"flip": ["x", "z"], "rot90": ["z"]}, (8, 8, 8))
    fx, fz = flip_op(2), flip_op(0)
    combos = [GeomOp(), fx, fz, compose(fx, fz)]            # bit 0 is the first listed axis
    want = [compose(f, rot90_op("z", k) if k else GeomOp()) for f in combos for k in range(4)]
    assert list(views) == list(dict.fromkeys(want))
    # two rotation axes: the first listed is the outer loop, and the chain applies them in the listed order
    views = inf.tta_views({"rot90": ["z", "y"]}, (8, 8, 8))
    want = [compose(rot90_op("z", a) if a else GeomOp(), rot90_op("y", b) if b else GeomOp()) for a in range(4) for b in range(4)]
    assert list(views) == list(dict.fromkeys(want))


def test_off_shorthand_and_anisotropic_patches():
    for off in (None, False):
        assert inf.tta_views(off, (16, 24, 32), TASKS) == (GeomOp(),)
    flip = inf.tta_views("flip", (16, 24, 32), TASKS)
    assert len(flip) == 8 and flip == inf.tta_views({"flip": ["z", "y", "x"]}, (16, 24, 32), TASKS)
    assert all(op.preserves((16, 24, 32)) for op in flip)
    with pytest.raises(ValueError, match="tta.rot90") as e:
        inf.tta_views({"rot90": ["z"]}, (16, 24, 32), TASKS)
    assert str(list(allowed_rot90_axes((16, 24, 32)))) in str(e.value)
    with pytest.raises(ValueError, match="tta.rot90") as e:
        inf.tta_views({"flip": ["z"], "rot90": ["z", "x"]}, (16, 24, 24), TASKS)      # only a turn about z moves a square plane
    assert str(list(allowed_rot90_axes((16, 24, 24)))) in str(e.value) and "'x'" in str(e.value)
    assert len(inf.tta_views({"rot90": ["z"]}, (16, 24, 24), TASKS)) == 4


def test_refusals_name_the_key():
    with pytest.raises(ValueError, match="mirror"):
        inf.tta_views({"flip": ["z"], "mirror": ["x"]}, (16, 16, 16), TASKS)
    with pytest.raises(ValueError, match="tta.flip"):
        inf.tta_views({"flip": ["w"]}, (16, 16, 16), TASKS)
    with pytest.raises(ValueError, match="tta"):
        inf.tta_views("rot", (16, 16, 16), TASKS)
    one = {"normals": {"channels": 1, "activation": "none"}}
    with pytest.raises(ValueError, match="normals"):
        inf.tta_views("flip", (16, 16, 16), one, normal_keys=("normals",))
    assert inf.default_normal_keys(one) == ()                  # by default a 1-channel `normals` task is no vector field
    assert inf.default_normal_keys(TASKS) == ("normals",)
    with pytest.raises(ValueError, match="sheet"):
        inf.tta_views("flip", (16, 16, 16), TASKS, normal_keys=("sheet",))
    with pytest.raises(ValueError, match="view 1"):
        inf.tta_views([GeomOp(), rot90_op("z", 1)], (16, 16, 24), TASKS)             # would change the patch shape
    # more than 48 distinct records: spatial ops with component rules that do not belong to them
    many = [GeomOp(v.src_axis, v.flip, (0, 1, 2), n) for v in inf.tta_views(_spec("zyx", "zyx"), (8, 8, 8))[:25]
            for n in ((0, 0, 0), (1, 0, 0))]
    with pytest.raises(ValueError, match="48"):
        inf.tta_views(many, (8, 8, 8), TASKS)


def test_explicit_ops_are_deduplicated_and_need_no_identity():
    a, b = flip_op(2), rot90_op("z", 1)
    views = inf.tta_views([a, b, a, compose(a, a), b], (16, 16, 16), TASKS)
    assert views == (a, b, GeomOp())
    assert inf.tta_views([GeomOp()], (16, 16, 16)) == (GeomOp(),)


# ---- the semantics, in numpy ------------------------------------------------------------------------------------------------------
def tta_blend_numpy(vol, patch, overlap, views, weight, predict, normal_keys):
    """`vol` (C, Z, Y, X) float32, already scaled; `predict(x)` -> {task: activated (c, pz, py, px) prediction of the patch x}.
    Position-major, view-minor; the weight is indexed by the destination voxel.  Returns ({task: sum}, wsum)."""
    pz, py, px = patch
    sums, wsum = None, np.zeros(vol.shape[1:], np.float32)
    for z, y, x in inf.all_positions(vol.shape[1:], patch, overlap):
        box = np.s_[z:z + pz, y:y + py, x:x + px]
        for g in views:
            pred = predict(apply_op_numpy(g, vol[(slice(None),) + box]))
            if sums is None:
                sums = {n: np.zeros((p.shape[0],) + vol.shape[1:], np.float32) for n, p in pred.items()}
            for n, p in pred.items():
                q = apply_op_numpy(g.inverse(), p.astype(np.float32), is_normal=n in normal_keys)
                sums[n][(slice(None),) + box] += weight[None] * q
            wsum[box] += weight
    return sums, wsum


def _grad(x):
    """central differences with wrap-around, components (x, y, z): a vector field that turns and mirrors with its volume"""
    v = x[0].astype(np.float32)
    return np.stack([np.roll(v, -1, a) - np.roll(v, 1, a) for a in (2, 1, 0)])


def _equivariant(x):
    return {"sheet": (x * np.float32(0.5) + np.float32(0.25)).astype(np.float32), "normals": _grad(x)}


def _make_biased(patch, seed=5):
    rng = np.random.default_rng(seed)
    a, b = rng.normal(size=patch).astype(np.float32), rng.normal(size=patch).astype(np.float32)
    zi = np.arange(patch[0], dtype=np.float32)[:, None, None] / patch[0]

    def predict(x):      # a fixed per-voxel affine map plus the local z index: it knows where it is in the patch
        s = (x * a + b + zi).astype(np.float32)
        return {"sheet": s, "normals": (_grad(x) + np.stack([a, b, zi + 0 * a])).astype(np.float32)}
    return predict


def _blend(sums, wsum):
    n = sums["normals"]
    return sums["sheet"][0] / wsum, n / (np.sqrt((n * n).sum(0)) + np.float32(1e-8))


@pytest.mark.parametrize("blend", ["uniform", "gaussian"])
@pytest.mark.parametrize("flips,rots", [("zyx", ""), ("zyx", "zyx")])
def test_numpy_semantics_equivariant_equals_single_view_and_biased_differs(blend, flips, rots):
    patch, shape = (8, 8, 8), (20, 18, 22)
    rng = np.random.default_rng(3)
    vol = rng.random(size=(1,) + shape).astype(np.float32)
    w = inf.gaussian_importance_map(patch) if blend == "gaussian" else np.ones(patch, np.float32)
    views = inf.tta_views(_spec(flips, rots), patch, TASKS)
    nk = ("normals",)
    one_s, one_w = tta_blend_numpy(vol, patch, 0.5, (GeomOp(),), w, _equivariant, nk)
    all_s, all_w = tta_blend_numpy(vol, patch, 0.5, views, w, _equivariant, nk)
    # every view of an equivariant function, moved back with the component and sign rule, is the single view: the sums are
    # V x it up to fp32 summation.  A voxel adds at most T = V x (patches on it) terms one after the other; each addition rounds
    # by at most 2^-24 of the running sum, which stays below the largest |sum| M -- so T * 2^-24 * M per side, 2^-23 for both
    V = len(views)
    cnt = np.zeros(shape, np.float32)
    for z, y, x in inf.all_positions(shape, patch, 0.5):
        cnt[z:z + 8, y:y + 8, x:x + 8] += 1
    T = V * float(cnt.max())
    assert np.abs(all_w - V * one_w).max() <= T * 2.0 ** -23 * float(V * one_w.max())
    for n in one_s:
        M = float(np.abs(V * one_s[n]).max())
        assert np.abs(all_s[n] - V * one_s[n]).max() <= T * 2.0 ** -23 * M, n
    got, want = all_s["sheet"][0] / all_w, one_s["sheet"][0] / one_w              # averages of values in [0.25, 0.75]
    assert np.abs(got - want).max() <= 4 * T * 2.0 ** -23
    # undoing the views WITHOUT the component rule is not the single view: the normals rule is what makes the blend right
    bad_s, _ = tta_blend_numpy(vol, patch, 0.5, views, w, _equivariant, ())
    assert np.abs(bad_s["normals"] - V * one_s["normals"]).max() > 0.1
    # a function that knows where it is in the patch sees the views: the blend changes, for both tasks
    biased = _make_biased(patch)
    b1_s, b1_w = tta_blend_numpy(vol, patch, 0.5, (GeomOp(),), w, biased, nk)
    bv_s, bv_w = tta_blend_numpy(vol, patch, 0.5, views, w, biased, nk)
    for got, want in zip(_blend(bv_s, bv_w), _blend(b1_s, b1_w)):
        assert np.abs(got - want).max() > 0.05


# ---- the schedule with views --------------------------------------------------------------------------------------------------------
CASES = [((40, 36, 44), (16, 16, 16), 0.5, 2), ((37, 20, 24), (16, 8, 8), 0.25, 3), ((16, 16, 16), (16, 16, 16), 0.5, 2),
         ((100, 24, 24), (32, 16, 16), 0.75, 4), ((65, 17, 19), (8, 8, 8), 0.0, 1), ((129, 16, 16), (64, 16, 16), 0.5, 2)]


@pytest.mark.parametrize("shape,patch,overlap,bs", CASES)
@pytest.mark.parametrize("V", [1, 3, 8])
def test_schedule_with_views(shape, patch, overlap, bs, V):
    base = inf.stream_schedule(shape, patch, overlap, bs, cin=2, in_itemsize=2, acc_channels=4, out_bytes_per_voxel=23)
    s = inf.stream_schedule(shape, patch, overlap, bs, cin=2, in_itemsize=2, acc_channels=4, out_bytes_per_voxel=23, n_views=V)
    pos = inf.all_positions(shape, patch, overlap)
    ran = []
    for st in s["steps"]:
        assert len(st["views"]) == len(st["batches"])
        for (chunk, valid), vidx in zip(st["batches"], st["views"]):
            assert len(chunk) == len(vidx) == s["batch"] and 1 <= valid <= s["batch"]
            assert all(0 <= v < V for v in vidx) and all(p[0] == st["z"] for p in chunk)
            assert all((p, v) == (chunk[valid - 1], vidx[valid - 1]) for p, v in zip(chunk[valid:], vidx[valid:]))
            ran += list(zip(chunk[:valid], vidx[:valid]))
    assert ran == [(p, v) for p in pos for v in range(V)]         # each pair once, position-major and view-minor
    for k in ("positions", "batch", "ring", "max_finalize_rows", "accumulator_bytes", "input_bytes", "staging_bytes", "patch_bytes",
              "device_bytes"):
        assert s[k] == base[k], k
    assert len(s["steps"]) == len(base["steps"])
    for a, b in zip(s["steps"], base["steps"]):
        for k in ("z", "load", "finalize", "write"):
            assert a[k] == b[k], k
    if V == 1:      # the call without the argument, apart from the added key
        assert all(st["views"] == [(0,) * s["batch"]] * len(st["batches"]) for st in s["steps"])
        assert s == base
        for st in s["steps"]:
            assert set(st) == {"z", "load", "batches", "views", "finalize", "write"}
    with pytest.raises(ValueError):
        inf.stream_schedule(shape, patch, overlap, bs, n_views=0)


# ---- config and construction ----------------------------------------------------------------------------------------------------
def _cfg(tmp_path, ic, targets=None):
    import yaml
    cfg = {"tr_setup": {}, "tr_config": {"patch_size": [16, 16, 16]}, "model_config": {},
           "dataset_config": {"targets": targets or {"sheet": {"channels": 1, "activation": "sigmoid"}}}, "inference_config": ic}
    p = tmp_path / "cfg.yaml"
    p.write_text(yaml.safe_dump(cfg))
    return str(p)


def test_config_keys(tmp_path):
    from mt3d_amd.configuration.config_manager import ConfigManager
    m = ConfigManager(_cfg(tmp_path, {}), verbose=False)
    assert m.infer_tta is None and m.infer_tta_normal_keys is None
    m = ConfigManager(_cfg(tmp_path, {"tta": "flip", "tta_normal_keys": ["normals", "n2"]}), verbose=False)
    assert m.infer_tta == "flip" and m.infer_tta_normal_keys == ("normals", "n2")
    spec = {"flip": ["z", "y", "x"], "rot90": ["z"]}
    m = ConfigManager(_cfg(tmp_path, {"tta": spec, "tta_normal_keys": "normals"}, TASKS), verbose=False)
    assert m.infer_tta == spec and m.infer_tta_normal_keys == ("normals",)
    r = inf.StreamingInferer(None, m.infer_targets, m.infer_patch_size, tta=m.infer_tta, normal_keys=m.infer_tta_normal_keys)
    assert len(r.views) == 16 and r.normal_keys == ("normals",)


def test_streaming_inferer_views_and_refusals_at_construction():
    def make(**k):
        return inf.StreamingInferer(None, TASKS, k.pop("patch", (16, 16, 16)), **k)
    r = make()
    assert r.views == (GeomOp(),) and not r.tta and r.normal_keys == ("normals",)
    assert not make(tta=False).tta and make(tta=[GeomOp()]).tta
    r = make(tta="flip")
    assert r.tta and len(r.views) == 8
    # the schedule carries the views; the device bytes do not change
    s0, s8 = make().schedule((40, 36, 44)), r.schedule((40, 36, 44))
    assert s8["device_bytes"] == s0["device_bytes"]
    assert sum(v for st in s8["steps"] for _, v in st["batches"]) == 8 * len(s0["positions"])
    for bad in ({"rot90": ["z"], "patch": (16, 16, 24)}, {"tta": {"flips": ["z"]}}, {"tta": "all"}, {"tta": [rot90_op("y", 1)], "patch": (8, 16, 16)},
                {"tta": "flip", "normal_keys": ("sheet",)}, {"tta": 3}):
        if "rot90" in bad:
            bad = {"tta": {"rot90": bad["rot90"]}, "patch": bad["patch"]}
        with pytest.raises(ValueError):
            make(**bad)
    for blend, rots in itertools.product(("uniform", "gaussian"), ("z", "zyx")):
        assert len(make(tta={"flip": ["z", "y", "x"], "rot90": list(rots)}, blend=blend).views) == (16 if rots == "z" else 48)
